// Compiled autograd binding of the fused fake-quant layer ops: torch::autograd::Function nodes in C++ over the SAME
// C ABI (include/mhaq_fq.h -> libmhaq_fq.so, resolved with dlopen / dlsym from the path the Python side hands over).
//
// Why: the reference's ops are Python torch.autograd.Functions invoked once per layer
//     /root/reference/src/quantization/gdnsq/gdnsq.py:13-23        (QNoise / QN* Functions)
//     /root/reference/src/quantization/gdnsq/layers/gdnsq_act.py:39-55      (NoisyAct.forward)
//     /root/reference/src/quantization/gdnsq/layers/gdnsq_conv2d.py:71-100  (NoisyConv2d.forward)
// and a Python Function over ctypes costs ~24 us per forward and ~60 us per backward op of host time (Python frames,
// ctypes argument conversion, the GIL hand-over to the autograd thread) -- the whole run time of the small
// configurations (ResNet-20 at batch 128, RFDN at 24x24), whose kernels take 2-10 us.  Here the forward is one
// pybind11 call and the backward never takes the GIL: the autograd engine calls straight into apply(), which
// allocates the outputs through the torch caching allocator and launches on the current HIP stream.
//
// This file holds NO arithmetic: every number is produced by the kernels behind the C ABI; results are bit-identical
// to the ctypes path (same entry points, same arguments).  Host-only C++ (no device code); torch is plumbing
// (device memory, streams, the autograd graph).
#include <torch/extension.h>
#include <torch/version.h>
#include <torch/csrc/autograd/custom_function.h>

#include <c10/hip/HIPCachingAllocator.h>
#include <c10/hip/HIPGraphsC10Utils.h>
#include <c10/hip/HIPStream.h>
#include <c10/core/DeviceGuard.h>
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/mhaq_fq.h"

namespace py = pybind11;
using at::Tensor;
using torch::autograd::AutogradContext;
using torch::autograd::variable_list;

namespace {

// ------------------------------------------------------------------------------------------------ the C ABI
#define MHAQ_API(X)                                                                                                   \
  X(mhaq_fq_abi_version) X(mhaq_fq_error_string) X(mhaq_fq_act_fwd) X(mhaq_fq_act_bwd_workspace_bytes)                \
  X(mhaq_fq_act_bwd) X(mhaq_fq_act_bwd_partials) X(mhaq_fq_act_bwd_finalize_multi) X(mhaq_fq_wlayer_fwd)              \
  X(mhaq_fq_wlayer_bwd) X(mhaq_fq_pc_aewgs_stats) X(mhaq_fq_wlayer_fwd_multi) X(mhaq_fq_wlayer_bwd_group)             \
  X(mhaq_fq_wlayer_aewgs_stats_group) X(mhaq_fq_wlayer_pt_fwd) X(mhaq_fq_wlayer_pt_bwd)                               \
  X(mhaq_fq_potential_loss_fwd) X(mhaq_fq_potential_loss_bwd) X(mhaq_fq_wlayer_ptl_workspace_bytes)                   \
  X(mhaq_fq_wlayer_ptl_fwd) X(mhaq_fq_wlayer_ptl_bwd) X(mhaq_fq_pt_aewgs_colstats_workspace_bytes)                     \
  X(mhaq_fq_pt_aewgs_colstats) X(mhaq_fq_act_fwd_x16) X(mhaq_fq_act_bwd_x16) X(mhaq_fq_act_bwd_partials_x16)                    \
  X(mhaq_fq_act_relu_fwd) X(mhaq_fq_act_relu_bwd) X(mhaq_fq_act_relu_bwd_partials)                                    \
  X(mhaq_fq_act_relu_fwd_x16) X(mhaq_fq_act_relu_bwd_x16) X(mhaq_fq_act_relu_bwd_partials_x16)                        \
  X(mhaq_fq_bn_bwd_workspace_bytes) X(mhaq_fq_bn_bwd) X(mhaq_fq_maxpool3s2_fwd)                                       \
  X(mhaq_fq_bn_pool_bwd_workspace_bytes) X(mhaq_fq_bn_pool_bwd) X(mhaq_fq_bn_bwd_x16_workspace_bytes)                 \
  X(mhaq_fq_bn_bwd_x16) X(mhaq_fq_bn_fwd_workspace_bytes) X(mhaq_fq_bn_fwd)                                         \
  X(mhaq_fq_bn_fwd_x16_workspace_bytes) X(mhaq_fq_bn_fwd_x16)                                                       \
  X(mhaq_fq_bn_pool_bwd_x16_workspace_bytes) X(mhaq_fq_bn_pool_bwd_x16) X(mhaq_fq_bn_norm_pool3s2_fwd_x16)          \
  X(mhaq_fq_bn_infer_consts) X(mhaq_fq_bn_infer_act) X(mhaq_fq_bn_relu_pool3s2)                                     \
  X(mhaq_fq_bn_infer_act_x16) X(mhaq_fq_bn_relu_pool3s2_x16)                                                        \
  X(mhaq_fq_radam_chunk_elements) X(mhaq_fq_radam_step)                                                          \
  X(mhaq_fq_distill_loss_workspace_bytes) X(mhaq_fq_distill_loss_fwd) X(mhaq_fq_distill_loss_bwd)             \
  X(mhaq_fq_cls_head_workspace_bytes) X(mhaq_fq_cls_head_fwd)

struct Api {
#define X(n) decltype(&::n) n = nullptr;
  MHAQ_API(X)
#undef X
  void* handle = nullptr;
  std::string path;
};
Api A;

struct MhaqError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

void bind_library(const std::string& path) {
  if (A.handle && A.path == path) return;
  void* h = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
  if (!h) throw MhaqError("cannot load " + path + ": " + dlerror() + " (there is no CPU fallback)");
  Api a;
#define X(n)                                                                        \
  a.n = reinterpret_cast<decltype(a.n)>(dlsym(h, #n));                              \
  if (!a.n) throw MhaqError(std::string(#n) + " is not exported by " + path);
  MHAQ_API(X)
#undef X
  if (a.mhaq_fq_abi_version() != MHAQ_FQ_ABI_VERSION) throw MhaqError("libmhaq_fq.so ABI version mismatch");
  a.handle = h;
  a.path = path;
  A = a;
}

inline void need_lib() {
  if (!A.handle) throw MhaqError("the C-ABI library is not bound (mhaq_amd._ext.bind)");
}

inline void check(int rc, const char* what) {
  if (rc != 0)
    throw MhaqError(std::string(what) + " failed: " + A.mhaq_fq_error_string(rc) + " (code " + std::to_string(rc) + ")");
}

inline void* cur_stream(const Tensor& t) {
  return (void*)c10::hip::getCurrentHIPStream(t.device().index()).stream();
}

inline bool capturing() {
  return c10::hip::currentStreamCaptureStatusMayInitCtx() != c10::hip::CaptureStatus::None;
}

// The C ABI launches on the stream it is handed and expects the calling thread's CURRENT device to be that stream's (and the
// pointers') device -- include/mhaq_fq.h, "Devices".  torch ops work on a tensor's device whatever the current one is (the
// reference is plain torch ops: a model moved to cuda:1 in a process whose current device is cuda:0 just works), so every
// forward entry point below switches to its input's device for its own duration.  (Backward nodes run on the autograd
// engine's thread of their device, which has made it current.)  ~50 ns when the device already is the current one.
#define MHAQ_ON_DEVICE_OF(t) const c10::OptionalDeviceGuard mhaq_device_guard_(at::device_of(t))

inline const float* fptr(const Tensor& t) { return static_cast<const float*>(t.const_data_ptr()); }
inline float* fptr_mut(const Tensor& t) { return static_cast<float*>(t.mutable_data_ptr()); }
inline const float* fptr_or_null(const Tensor& t) { return t.defined() ? fptr(t) : nullptr; }

// element type of a 16-bit activation for the *_x16 entry points; 0 = float32 (the fp32 entry points)
inline int act_dtype(const Tensor& x) {
  switch (x.scalar_type()) {
    case at::kBFloat16: return MHAQ_FQ_DT_BF16;
    case at::kHalf: return MHAQ_FQ_DT_F16;
    default: return 0;
  }
}

// the upstream gradient in the memory order of x (the kernels walk both as flat streams)
inline Tensor like_layout(const Tensor& g, const Tensor& x) {
  if (g.sizes() == x.sizes() && g.strides() == x.strides()) return g;
  Tensor out = at::empty_like(x);
  out.copy_(g);
  return out;
}

// ------------------------------------------------------------------------------------------------ host timers
// Where does the host time of a node go?  Cheap enough to stay compiled in (steady_clock::now() is ~25 ns); read and
// reset with host_timers() (tools/host_profile.py).  Relaxed atomics: the backward nodes run on the autograd thread.
enum { T_ACT_FWD, T_ACT_FWD_LAUNCH, T_ACT_BWD, T_ACT_BWD_SAVED, T_ACT_BWD_ALLOC, T_ACT_BWD_HUB, T_ACT_BWD_LAUNCH, T_HUB_BWD,
       T_N };
const char* kTimerNames[T_N] = {"act_fwd", "act_fwd_launch", "act_bwd", "act_bwd_saved", "act_bwd_alloc", "act_bwd_hub",
                                "act_bwd_launch", "hub_bwd"};
std::atomic<int64_t> g_tns[T_N];
std::atomic<int64_t> g_tcnt[T_N];
inline int64_t now_ns() {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
inline void tick(int which, int64_t t0, int64_t t1) {
  g_tns[which].fetch_add(t1 - t0, std::memory_order_relaxed);
  g_tcnt[which].fetch_add(1, std::memory_order_relaxed);
}

// ------------------------------------------------------------------------------------------------ sign streams
// (seed, offset) source of the in-kernel Philox sign stream (gdnsq.py:54 randint_like; SURVEY.md section 8e: ranks
// draw different streams, every backward call gets a fresh offset).  One owner for the Python ops (ctypes) and the
// nodes below: mhaq_amd.ops.rng is a facade over this object.
struct Rng {
  std::mutex mu;
  bool seeded = false;
  uint64_t seed = 0, count = 0;
  Tensor base;   // nullable one-element int64 device tensor the kernels add to their host offset (hipGraph replays)
};
Rng& R = *new Rng();     // never destroyed (it may hold a device tensor): see the registries below

constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;

struct Draw {
  uint64_t seed = 0, offset = 0;
  const uint64_t* offset_dev = nullptr;
};

// what ops._signs does for a backward call: none for explicit signs / LSQ, else the next offset of the rank's stream
Draw draw_signs(bool has_r_sign, int64_t method, int64_t rank, const Tensor& like) {
  Draw d;
  if (has_r_sign || method == MHAQ_FQ_LSQ) return d;
  std::lock_guard<std::mutex> g(R.mu);
  if (!R.seeded) throw MhaqError("sign stream used before it was seeded (mhaq_amd.ops.manual_seed)");
  d.seed = R.seed ^ ((uint64_t)rank * kGolden);
  d.offset = ++R.count;
  if (R.base.defined() && R.base.device() == like.device())
    d.offset_dev = static_cast<const uint64_t*>(R.base.const_data_ptr());
  return d;
}

// ------------------------------------------------------------------------------------------------ handles and tables
// Hubs and plans are handed to Python as integer ids.  A registry is never destroyed (heap-allocated, see its two
// instances): a static map would free device tensors and HIP events from a static destructor, after the HIP runtime and
// the interpreter are gone.
template <class T>
struct Registry {
  const char* const what;
  std::mutex mu;
  std::unordered_map<int64_t, std::shared_ptr<T>> items;
  int64_t next = 1;
  explicit Registry(const char* w) : what(w) {}

  std::shared_ptr<T> get(int64_t id) {
    std::lock_guard<std::mutex> g(mu);
    auto it = items.find(id);
    if (it == items.end()) throw MhaqError(std::string(what) + " " + std::to_string(id) + " no longer exists");
    return it->second;
  }
  int64_t add(std::shared_ptr<T> item) { std::lock_guard<std::mutex> g(mu); items[next] = std::move(item); return next++; }
  void erase(int64_t id) { std::lock_guard<std::mutex> g(mu); items.erase(id); }
};

// pinned staging + async copy on the current stream; the caching host allocator keeps `host` until the copy has run
std::pair<Tensor, Tensor> upload(const void* bytes, size_t nbytes, const Tensor& like) {
  Tensor host = at::empty({(int64_t)nbytes}, at::TensorOptions().dtype(at::kByte).pinned_memory(true));
  std::memcpy(host.mutable_data_ptr(), bytes, nbytes);
  Tensor dev = host.to(like.device(), /*non_blocking=*/true);
  return {dev, host};
}

// Device descriptor tables keyed by the pointers they hold, allocated and uploaded on a miss.  A table handed out WHILE
// A CAPTURE WAS ACTIVE is held until release_captured() -- a captured hipGraph has baked its address into its launches;
// eager tables live in a small LRU (a table the stream still reads stays valid: the allocator orders reuse).  Not
// thread-safe: the owner's mutex guards it.
// (Two mechanisms on purpose: the keys here repeat step after step, so a miss may allocate.  TablePool below serves keys
// that change every step -- its entries are allocated up front and refilled in place behind an event.)
struct TableCache {
  struct Entry { Tensor dev, host; bool captured = false; uint64_t stamp = 0; };
  std::map<std::vector<int64_t>, Entry> entries;
  uint64_t clock = 0;

  // `make_descs()` -> std::vector of descriptors: the bytes to upload, built only on a miss
  template <class MakeDescs>
  Tensor get(const std::vector<int64_t>& key, size_t eager_capacity, const Tensor& like, MakeDescs make_descs) {
    const bool cap = capturing();
    auto it = entries.find(key);
    if (it == entries.end()) {
      const auto descs = make_descs();
      auto up = upload(descs.data(), descs.size() * sizeof(descs[0]), like);
      if (!cap) {
        size_t eager = entries.size() - captured();
        while (eager >= eager_capacity) {
          auto victim = entries.end();
          for (auto jt = entries.begin(); jt != entries.end(); ++jt)
            if (!jt->second.captured && (victim == entries.end() || jt->second.stamp < victim->second.stamp)) victim = jt;
          entries.erase(victim);
          --eager;
        }
      }
      it = entries.emplace(key, Entry{up.first, up.second, cap, 0}).first;
    }
    it->second.captured = it->second.captured || cap;
    it->second.stamp = ++clock;
    return it->second.dev;
  }

  void release_captured() {
    for (auto it = entries.begin(); it != entries.end();) it = it->second.captured ? entries.erase(it) : std::next(it);
  }
  size_t captured() const {
    return std::count_if(entries.begin(), entries.end(), [](auto& kv) { return kv.second.captured; });
  }
};

// ------------------------------------------------------------------------------------------------ activation hub
// One finalize launch for every NoisyAct quantizer of a backward pass (mhaq_amd/act_hub.py describes the scheme).
// Its workspaces follow the lifetime rule of its descriptor tables (TableCache): one handed out WHILE A CAPTURE WAS ACTIVE
// is held until release_captured() (outgrown: in `retired`); an outgrown eager workspace is simply dropped (the allocator
// orders its reuse behind the kernels that read it).
struct Hub {
  struct Pending { int64_t slot, nparts; Tensor ws; };
  std::mutex mu;
  int64_t n = 0;
  std::vector<Tensor> ws;
  std::vector<char> ws_captured;
  std::vector<Pending> pending;
  TableCache tables;
  std::vector<Tensor> retired;
  std::vector<std::vector<int64_t>> shapes;   // parameter shapes of this step's begin()
  std::unordered_map<int, Tensor> placeholders;
  Tensor last_table;
  static constexpr size_t kEagerTables = 4;

  Tensor workspace(int64_t slot, int64_t nbytes, const Tensor& like) {
    Tensor& w = ws.at(slot);
    const bool cap = capturing();
    if (!w.defined() || w.numel() < nbytes || w.device() != like.device()) {
      if (w.defined() && ws_captured[slot]) retired.push_back(w);
      w = at::empty({nbytes}, like.options().dtype(at::kByte));
      ws_captured[slot] = 0;
    }
    if (cap) ws_captured[slot] = 1;
    return w;
  }

  Tensor placeholder(const Tensor& like) {
    Tensor& p = placeholders[like.device().index()];
    if (!p.defined()) p = at::zeros({1}, like.options());
    return p;
  }

  void release_captured() {
    std::lock_guard<std::mutex> g(mu);
    retired.clear();
    std::fill(ws_captured.begin(), ws_captured.end(), 0);
    tables.release_captured();
  }
};

Registry<Hub>& g_hubs = *new Registry<Hub>("ActGradHub");

int64_t hub_create(int64_t n) {
  auto h = std::make_shared<Hub>();
  h->n = n;
  h->ws.resize(n);
  h->ws_captured.assign(n, 0);
  return g_hubs.add(std::move(h));
}

class HubFn : public torch::autograd::Function<HubFn> {
 public:
  static variable_list forward(AutogradContext* ctx, int64_t hub_id, at::TensorList params) {
    ctx->saved_data["hub"] = hub_id;
    ctx->set_materialize_grads(false);
    auto hub = g_hubs.get(hub_id);
    std::lock_guard<std::mutex> g(hub->mu);
    hub->pending.clear();
    hub->shapes.clear();
    variable_list out;
    out.reserve(params.size());
    for (const auto& p : params) {
      hub->shapes.emplace_back(p.sizes().vec());
      out.push_back(p.view_as(p));          // aliases: the kernels read the parameters in place
    }
    return out;
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    struct Scope { int64_t t0 = now_ns(); ~Scope() { tick(T_HUB_BWD, t0, now_ns()); } } scope;
    auto hub = g_hubs.get(ctx->saved_data["hub"].toInt());
    std::lock_guard<std::mutex> g(hub->mu);
    variable_list out(1 + grads.size());
    std::vector<Hub::Pending> pending;
    pending.swap(hub->pending);
    if (pending.empty()) return out;
    const Tensor& like = pending[0].ws;
    std::vector<int64_t> key;
    key.reserve(3 * pending.size());
    for (auto& p : pending) {
      key.push_back(p.slot);
      key.push_back(p.nparts);
      key.push_back((int64_t)(uintptr_t)p.ws.const_data_ptr());
    }
    hub->last_table = hub->tables.get(key, Hub::kEagerTables, like, [&] {
      std::vector<mhaq_act_finalize_desc> descs(pending.size());
      for (size_t j = 0; j < pending.size(); ++j)
        descs[j] = mhaq_act_finalize_desc{static_cast<const float*>(pending[j].ws.const_data_ptr()), pending[j].nparts};
      return descs;
    });
    Tensor slab = at::empty({(int64_t)pending.size(), 3}, like.options().dtype(at::kFloat));
    check(A.mhaq_fq_act_bwd_finalize_multi(static_cast<const mhaq_act_finalize_desc*>(hub->last_table.const_data_ptr()),
                                           (int)pending.size(), fptr_mut(slab), cur_stream(slab)),
          "mhaq_fq_act_bwd_finalize_multi");
    // one unbind makes all 3n one-element views (0.15 us each; select + narrow + view per gradient cost 1.2 us)
    const std::vector<Tensor> pieces = slab.view({(int64_t)pending.size() * 3, 1}).unbind(0);
    for (size_t j = 0; j < pending.size(); ++j) {
      const int64_t s = pending[j].slot;
      for (int c = 0; c < 3; ++c) {
        const size_t k = (size_t)(3 * s + c);
        if (k < grads.size() && grads[k].defined()) {    // autograd asked for it (requires_grad + reached)
          const auto& shp = hub->shapes.at(k);
          const Tensor& piece = pieces[3 * j + c];
          out[1 + k] = (shp.size() == 1 && shp[0] == 1) ? piece : piece.view(shp);
        }
      }
    }
    return out;
  }
};

// (the parameters go in as an at::TensorList: Function<T>::apply only unpacks that list type into autograd inputs)
variable_list hub_begin(int64_t hub_id, const variable_list& params) { need_lib(); return HubFn::apply(hub_id, at::TensorList(params)); }      // (no launch: aliases only)

// ------------------------------------------------------------------------------------------------ shared node pieces
// save_for_backward of `tensors` plus the explicit sign tensor when there is one (then the LAST saved tensor)
void save_with_sign(AutogradContext* ctx, variable_list tensors, const std::optional<Tensor>& r_sign) {
  if (r_sign.has_value() && r_sign->defined()) tensors.push_back(*r_sign);
  ctx->save_for_backward(std::move(tensors));
}

// ... and what the three weight nodes keep besides
void weight_save_ctx(AutogradContext* ctx, variable_list tensors, const std::optional<Tensor>& r_sign, int64_t method,
                     int64_t rank, const Tensor& log_s) {
  save_with_sign(ctx, std::move(tensors), r_sign);
  ctx->saved_data["method"] = method;
  ctx->saved_data["rank"] = rank;
  ctx->saved_data["ls_shape"] = log_s.sizes().vec();
  ctx->set_materialize_grads(false);
}

// the explicit signs saved behind `k` tensors, or null (then draw_signs decides)
inline const int8_t* saved_sign(const variable_list& saved, size_t k) {
  return saved.size() > k ? static_cast<const int8_t*>(saved[k].const_data_ptr()) : nullptr;
}

// the scale gradient in the shape of the log_wght_s the weight node saved as "ls_shape"
inline Tensor ls_view(AutogradContext* ctx, const Tensor& gls) {
  return gls.view(ctx->saved_data["ls_shape"].toIntVector());
}

void check_act_params(const char* who, const Tensor& log_s, const Tensor& log_q, const Tensor& b) {
  TORCH_CHECK(log_s.numel() == 1 && log_q.numel() == 1 && b.numel() == 1 && log_s.is_cuda() && log_q.is_cuda() &&
                  b.is_cuda() && log_s.scalar_type() == at::kFloat && log_q.scalar_type() == at::kFloat &&
                  b.scalar_type() == at::kFloat,
              who, ": log_act_s / log_act_q / act_b must be one-element float32 device tensors");
}

// what both activation nodes leave for act_backward: ints = {method, hub, slot, rank, ...node's own}
void act_save_ctx(AutogradContext* ctx, std::vector<int64_t> ints, const Tensor& log_s, const Tensor& log_q,
                  const Tensor& b, const Tensor& params) {
  if (ints[1] <= 0)            // the hub path hands out placeholders: no shapes needed
    ctx->saved_data["shapes"] = std::vector<std::vector<int64_t>>{log_s.sizes().vec(), log_q.sizes().vec(), b.sizes().vec()};
  ctx->saved_data["i"] = std::move(ints);       // one map entry instead of four
  ctx->mark_non_differentiable({params});
}

// One activation backward launch as the node's callable sees it.  hub: the *_partials entry point, which leaves the
// partial rows in ws for the hub's finalize and their count in *nparts; else the full backward, which finishes the three
// parameter gradients into gr[3].
struct ActBwdLaunch {
  const Tensor &x, &g, &ga, &gx, &params;    // ga: undefined unless the node passed one
  int64_t n; int method; const Draw& d;
  void* ws; size_t nb; bool hub; float* gr; int32_t* nparts; void* stream;
};
struct ActGrads { Tensor gx, gp[3]; };      // gp: dL/dlog_act_s, dL/dlog_act_q, dL/dact_b

// The backward of ActLayerFn and ActReluFn behind their own input checks: x = saved[0], params = saved[1], ic = the
// node's saved integers, gy / ga the incoming gradients as autograd handed them over (gy undefined: a y nobody used, the
// quantizer's parameters get zeros), need0 = needs_input_grad index of log_act_s.  One sign-stream draw
// (draw_signs: none for explicit signs / LSQ), taken before the hub's lock; `launch(const ActBwdLaunch&)` runs the node's
// entry point.  With a hub the parameter gradients are its placeholder (HubFn::backward delivers the real ones).
// t0 / t1: the node's clock at its start and after it has read its saved state (T_ACT_BWD_SAVED).
template <class Launch>
ActGrads act_backward(AutogradContext* ctx, int64_t t0, int64_t t1, const variable_list& saved,
                      const std::vector<int64_t>& ic, const Tensor& gy, const Tensor& ga_in, bool has_r, size_t need0,
                      Launch launch) {
  const Tensor& x = saved[0];
  const Tensor& params = saved[1];
  const int64_t method = ic[0], hub_id = ic[1], slot = ic[2], rank = ic[3];
  Tensor g = gy.defined() ? like_layout(gy, x) : at::zeros_like(x);
  Tensor ga = ga_in.defined() ? like_layout(ga_in, x) : Tensor();
  ActGrads out;
  out.gx = at::empty_like(x);
  const int64_t t2 = now_ns();
  tick(T_ACT_BWD_SAVED, t0, t1);
  tick(T_ACT_BWD_ALLOC, t1, t2);
  const int64_t n = x.numel();
  const size_t nb = A.mhaq_fq_act_bwd_workspace_bytes(n);
  const Draw d = draw_signs(has_r, method, rank, x);
  if (hub_id > 0) {
    auto hub = g_hubs.get(hub_id);
    std::lock_guard<std::mutex> lk(hub->mu);
    Tensor ws = hub->workspace(slot, (int64_t)nb, x);
    int32_t nparts = 0;
    const int64_t t3 = now_ns();
    launch(ActBwdLaunch{x, g, ga, out.gx, params, n, (int)method, d, ws.mutable_data_ptr(), nb, true, nullptr, &nparts,
                        cur_stream(x)});
    // a y nobody used gives its quantizer NO gradient (0 * NaN of a non-finite input is not one): empty rows
    if (!gy.defined()) ws.narrow(0, 0, 3 * (int64_t)nparts * (int64_t)sizeof(float)).zero_();
    const int64_t t4 = now_ns();
    hub->pending.push_back(Hub::Pending{slot, nparts, ws});
    const Tensor ph = hub->placeholder(params);     // float32 like the parameters (x may be 16-bit)
    for (int c = 0; c < 3; ++c)
      if (ctx->needs_input_grad(need0 + c)) out.gp[c] = ph;
    tick(T_ACT_BWD_HUB, t2, t3);
    tick(T_ACT_BWD_LAUNCH, t3, t4);
    tick(T_ACT_BWD, t0, now_ns());
    return out;
  }
  Tensor gr = at::empty({3}, x.options().dtype(at::kFloat));
  Tensor ws = at::empty({(int64_t)nb}, x.options().dtype(at::kByte));
  launch(ActBwdLaunch{x, g, ga, out.gx, params, n, (int)method, d, ws.mutable_data_ptr(), nb, false, fptr_mut(gr), nullptr,
                      cur_stream(x)});
  if (!gy.defined()) gr.zero_();             // (as above: an unused y gives no parameter gradient)
  const auto shapes = ctx->saved_data["shapes"].to<std::vector<std::vector<int64_t>>>();
  for (int c = 0; c < 3; ++c)
    if (ctx->needs_input_grad(need0 + c)) out.gp[c] = gr.narrow(0, c, 1).view(shapes[c]);
  return out;
}

// ------------------------------------------------------------------------------------------------ NoisyAct layer op
// NoisyAct.forward from its learnable parameters (gdnsq_act.py:39-55): returns (y, params[5] = {s, zp, lo, hi, qr}).
// x float32, or bf16 / fp16 (autocast; mhaq_amd/ops.py decides when): y and gx then have x's dtype, params and the
// parameter gradients stay float32 (include/mhaq_fq.h, "16-bit activations").
class ActLayerFn : public torch::autograd::Function<ActLayerFn> {
 public:
  static variable_list forward(AutogradContext* ctx, const Tensor& x, const Tensor& log_s, const Tensor& log_q,
                               const Tensor& b, int64_t method, const std::optional<Tensor>& r_sign, int64_t hub_id,
                               int64_t slot, int64_t rank) {
    Tensor y = at::empty_like(x);
    Tensor params = at::empty({5}, x.options().dtype(at::kFloat));
    const int64_t tl0 = now_ns();
    if (const int dt = act_dtype(x))
      check(A.mhaq_fq_act_fwd_x16(x.const_data_ptr(), y.mutable_data_ptr(), x.numel(), dt, fptr(log_s), fptr(log_q),
                                  fptr(b), fptr_mut(params), nullptr, nullptr, nullptr, 0, cur_stream(x)),
            "mhaq_fq_act_fwd_x16");
    else
      check(A.mhaq_fq_act_fwd(fptr(x), fptr_mut(y), x.numel(), fptr(log_s), fptr(log_q), fptr(b), fptr_mut(params),
                              nullptr, nullptr, nullptr, 0, cur_stream(x)),
            "mhaq_fq_act_fwd");
    tick(T_ACT_FWD_LAUNCH, tl0, now_ns());
    save_with_sign(ctx, {x, params}, r_sign);
    act_save_ctx(ctx, {method, hub_id, slot, rank}, log_s, log_q, b, params);
    return {y, params};
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const int64_t t0 = now_ns();
    auto saved = ctx->get_saved_variables();
    const std::vector<int64_t> ic = ctx->saved_data["i"].toIntVector();
    const int64_t t1 = now_ns();
    const Tensor& x = saved[0];
    // autograd hands the gradient over in y's dtype (= x's); a 16-bit kernel must not read a float32 stream as 16-bit
    TORCH_CHECK(grads[0].scalar_type() == x.scalar_type(), "act_layer backward: the gradient is ",
                grads[0].scalar_type(), ", the input ", x.scalar_type());
    const int dt = act_dtype(x);
    const int8_t* r = saved_sign(saved, 2);
    ActGrads res = act_backward(ctx, t0, t1, saved, ic, grads[0], Tensor(), /*has_r=*/saved.size() > 2, /*need0=*/1,
                               [&](const ActBwdLaunch& a) {
      const void *xp = a.x.const_data_ptr(), *gp = a.g.const_data_ptr();
      void* gxp = a.gx.mutable_data_ptr();
      const float* pp = fptr(a.params);
      if (a.hub && dt)
        check(A.mhaq_fq_act_bwd_partials_x16(xp, gp, gxp, a.n, dt, pp, a.method, r, a.d.seed, a.d.offset, a.d.offset_dev,
                                             a.ws, a.nb, a.nparts, a.stream),
              "mhaq_fq_act_bwd_partials_x16");
      else if (a.hub)
        check(A.mhaq_fq_act_bwd_partials(fptr(a.x), fptr(a.g), fptr_mut(a.gx), a.n, pp, a.method, r, a.d.seed, a.d.offset,
                                         a.d.offset_dev, a.ws, a.nb, a.nparts, a.stream),
              "mhaq_fq_act_bwd_partials");
      else if (dt)
        check(A.mhaq_fq_act_bwd_x16(xp, gp, gxp, a.n, dt, pp, a.method, r, a.d.seed, a.d.offset, a.d.offset_dev, a.gr, a.ws,
                                    a.nb, a.stream),
              "mhaq_fq_act_bwd_x16");
      else
        check(A.mhaq_fq_act_bwd(fptr(a.x), fptr(a.g), fptr_mut(a.gx), a.n, pp, a.method, r, a.d.seed, a.d.offset,
                                a.d.offset_dev, a.gr, a.ws, a.nb, a.stream),
              "mhaq_fq_act_bwd");
    });
    variable_list out(9);
    if (ctx->needs_input_grad(0)) out[0] = std::move(res.gx);
    for (int c = 0; c < 3; ++c) out[1 + c] = std::move(res.gp[c]);
    return out;
  }
};

// (y, params, s = params[0:1], hi = params[3:4]): the two views are what NoisyAct publishes on its Quantizer
std::tuple<Tensor, Tensor, Tensor, Tensor> act_layer(const Tensor& x_in, const Tensor& log_s, const Tensor& log_q,
                                                     const Tensor& b, int64_t method,
                                                     const std::optional<Tensor>& r_sign, int64_t hub_id, int64_t slot,
                                                     int64_t rank) {
  need_lib();
  MHAQ_ON_DEVICE_OF(x_in);
  TORCH_CHECK(x_in.is_cuda() && (x_in.scalar_type() == at::kFloat || act_dtype(x_in) != 0),
              "act_layer: x must be a float32, bfloat16 or float16 device tensor");
  check_act_params("act_layer", log_s, log_q, b);
  const int64_t t0 = now_ns();
  const Tensor x = x_in.is_non_overlapping_and_dense() ? x_in : x_in.contiguous();
  auto out = ActLayerFn::apply(x, log_s, log_q, b, method, r_sign, hub_id, slot, rank);
  const Tensor& params = out[1];
  std::tuple<Tensor, Tensor, Tensor, Tensor> res{out[0], params, params.narrow(0, 0, 1), params.narrow(0, 3, 1)};
  tick(T_ACT_FWD, t0, now_ns());
  return res;
}

// ------------------------------------------------------------------------------------------------ ReLU + NoisyAct
// The NoisyAct behind a ReLU, with the ReLU (and the residual add in front of it) inside the quantizer's launches
// (mhaq_fq_act_relu_fwd / _bwd, mhaq_amd/fused_blocks.py): a = relu(z [+ addend]), y = fake_quant(a).  Outputs (y, params)
// or, when a has another consumer (the residual branch), (y, params, a).  The backward receives dL/dy and dL/da together
// and returns ONE gradient, which both z and addend take -- where the separate nodes ran autograd's accumulation of the
// two gradients of a, threshold_backward and the quantizer's backward.  One sign-stream offset per backward, partials
// registered with the hub: exactly as ActLayerFn.
// z (and addend) float32, or bf16 / fp16 under autocast (mhaq_fq_act_relu_*_x16; mhaq_amd/layers.py decides when): y, a and
// the gradient then have z's dtype and the bits of the separate 16-bit launches, params and the parameter gradients stay
// float32 (include/mhaq_fq.h).
class ActReluFn : public torch::autograd::Function<ActReluFn> {
 public:
  static variable_list forward(AutogradContext* ctx, const Tensor& z, const std::optional<Tensor>& addend,
                               const Tensor& log_s, const Tensor& log_q, const Tensor& b, int64_t method, bool want_act,
                               int64_t hub_id, int64_t slot, int64_t rank) {
    const bool has_add = addend.has_value() && addend->defined();
    Tensor y = at::empty_like(z);
    Tensor a = want_act ? at::empty_like(z) : Tensor();
    Tensor params = at::empty({5}, z.options().dtype(at::kFloat));
    const int64_t tl0 = now_ns();
    if (const int dt = act_dtype(z))
      check(A.mhaq_fq_act_relu_fwd_x16(z.const_data_ptr(), has_add ? addend->const_data_ptr() : nullptr,
                                       y.mutable_data_ptr(), want_act ? a.mutable_data_ptr() : nullptr, z.numel(), dt,
                                       fptr(log_s), fptr(log_q), fptr(b), fptr_mut(params), cur_stream(z)),
            "mhaq_fq_act_relu_fwd_x16");
    else
      check(A.mhaq_fq_act_relu_fwd(fptr(z), has_add ? fptr(*addend) : nullptr, fptr_mut(y),
                                   want_act ? fptr_mut(a) : nullptr, z.numel(), fptr(log_s), fptr(log_q), fptr(b),
                                   fptr_mut(params), cur_stream(z)),
            "mhaq_fq_act_relu_fwd");
    tick(T_ACT_FWD_LAUNCH, tl0, now_ns());
    // relu is idempotent: the backward recomputes a from the ReLU's input (mid-block) or from a itself
    ctx->save_for_backward({want_act ? a : z, params});
    act_save_ctx(ctx, {method, hub_id, slot, rank, (int64_t)want_act, (int64_t)has_add}, log_s, log_q, b, params);
    ctx->set_materialize_grads(false);
    if (want_act) return {y, params, a};
    return {y, params};
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const int64_t t0 = now_ns();
    auto saved = ctx->get_saved_variables();
    const std::vector<int64_t> ic = ctx->saved_data["i"].toIntVector();
    variable_list out(10);
    const bool g_y_def = grads[0].defined(), g_a_def = ic[4] /*want_act*/ != 0 && grads.size() > 2 && grads[2].defined();
    if (!g_y_def && !g_a_def) return out;
    const int64_t t1 = now_ns();
    // autograd hands the gradients over in y's and a's dtype (= z's); a 16-bit kernel must not read a float32 stream as 16-bit
    const Tensor& zs = saved[0];
    TORCH_CHECK((!g_y_def || grads[0].scalar_type() == zs.scalar_type()) &&
                    (!g_a_def || grads[2].scalar_type() == zs.scalar_type()),
                "act_relu_layer backward: a gradient does not have the input's dtype ", zs.scalar_type());
    const int dt = act_dtype(zs);
    // (needs_input_grad counts the tensor inputs that were present: an absent addend takes no slot)
    const size_t e = ic[5] != 0 ? 1 : 0;
    ActGrads res = act_backward(ctx, t0, t1, saved, ic, grads[0], g_a_def ? grads[2] : Tensor(), /*has_r=*/false,
                                /*need0=*/1 + e,
                               [dt](const ActBwdLaunch& a) {
      const void* gap = a.ga.defined() ? a.ga.const_data_ptr() : nullptr;
      if (a.hub && dt)
        check(A.mhaq_fq_act_relu_bwd_partials_x16(a.x.const_data_ptr(), a.g.const_data_ptr(), gap, a.gx.mutable_data_ptr(),
                                                  a.n, dt, fptr(a.params), a.method, a.d.seed, a.d.offset, a.d.offset_dev,
                                                  a.ws, a.nb, a.nparts, a.stream),
              "mhaq_fq_act_relu_bwd_partials_x16");
      else if (dt)
        check(A.mhaq_fq_act_relu_bwd_x16(a.x.const_data_ptr(), a.g.const_data_ptr(), gap, a.gx.mutable_data_ptr(), a.n, dt,
                                         fptr(a.params), a.method, a.d.seed, a.d.offset, a.d.offset_dev, a.gr, a.ws, a.nb,
                                         a.stream),
              "mhaq_fq_act_relu_bwd_x16");
      else if (a.hub)
        check(A.mhaq_fq_act_relu_bwd_partials(fptr(a.x), fptr(a.g), fptr_or_null(a.ga), fptr_mut(a.gx), a.n, fptr(a.params),
                                              a.method, a.d.seed, a.d.offset, a.d.offset_dev, a.ws, a.nb, a.nparts,
                                              a.stream),
              "mhaq_fq_act_relu_bwd_partials");
      else
        check(A.mhaq_fq_act_relu_bwd(fptr(a.x), fptr(a.g), fptr_or_null(a.ga), fptr_mut(a.gx), a.n, fptr(a.params), a.method,
                                     a.d.seed, a.d.offset, a.d.offset_dev, a.gr, a.ws, a.nb, a.stream),
              "mhaq_fq_act_relu_bwd");
    });
    if (e && ctx->needs_input_grad(1)) out[1] = res.gx;    // z and addend take the one gradient
    if (ctx->needs_input_grad(0)) out[0] = std::move(res.gx);
    for (int c = 0; c < 3; ++c) out[2 + c] = std::move(res.gp[c]);
    return out;
  }
};

// (y, a or None, params, s = params[0:1], hi = params[3:4])
std::tuple<Tensor, std::optional<Tensor>, Tensor, Tensor, Tensor> act_relu_layer(
    const Tensor& z, const std::optional<Tensor>& addend, const Tensor& log_s, const Tensor& log_q, const Tensor& b,
    int64_t method, bool want_act, int64_t hub_id, int64_t slot, int64_t rank) {
  need_lib();
  MHAQ_ON_DEVICE_OF(z);
  TORCH_CHECK(z.is_cuda() && (z.scalar_type() == at::kFloat || act_dtype(z) != 0) && z.is_non_overlapping_and_dense(),
              "act_relu_layer: z must be a dense float32, bfloat16 or float16 device tensor");
  const bool has_add = addend.has_value() && addend->defined();
  TORCH_CHECK(!has_add || (addend->device() == z.device() && addend->scalar_type() == z.scalar_type() &&
                           addend->sizes() == z.sizes() && addend->strides() == z.strides()),
              "act_relu_layer: addend must have z's device, dtype, shape and strides");
  TORCH_CHECK(!has_add || want_act, "act_relu_layer: with an addend the ReLU output is an output of the op (want_act)");
  TORCH_CHECK(method == MHAQ_FQ_STE || method == MHAQ_FQ_LSQ || method == MHAQ_FQ_EWGS,
              "act_relu_layer: STE, LSQ or EWGS");
  check_act_params("act_relu_layer", log_s, log_q, b);
  const int64_t t0 = now_ns();
  auto out = ActReluFn::apply(z, addend, log_s, log_q, b, method, want_act, hub_id, slot, rank);
  const Tensor& params = out[1];
  std::tuple<Tensor, std::optional<Tensor>, Tensor, Tensor, Tensor> res{
      out[0], want_act ? std::optional<Tensor>(out[2]) : std::nullopt, params, params.narrow(0, 0, 1),
      params.narrow(0, 3, 1)};
  tick(T_ACT_FWD, t0, now_ns());
  return res;
}

// ------------------------------------------------------------------------------------------------ BatchNorm backward
// Training-mode BatchNorm whose FORWARD is the framework's own -- at::_batch_norm_impl_index, what F.batch_norm calls:
// same dispatch, same kernels, same bits in y, the saved statistics and the running statistics -- and whose BACKWARD
// runs mhaq_fq_bn_bwd on a dense float32 channels_last tensor with C % 4 == 0.  Everything else takes
// at::_batch_norm_impl_index_backward with the saved implementation index and reserve: the backward autograd itself
// would have run.  The gradients of the HIP path differ from it by summation order only.  Once-differentiable.
// A bf16 / fp16 x (the convolution's output under autocast) takes mhaq_fq_bn_bwd_x16 where the caller enabled that route for
// the call (`x16`): C % 8 == 0, fp32 weight and statistics, and a dy of x's dtype; its dx is the fp32 arithmetic rounded once.
inline bool aligned16(const Tensor& t) { return (reinterpret_cast<uintptr_t>(t.const_data_ptr()) & 15) == 0; }

// What every HIP route asks: x a non-empty dense channels_last device tensor of fp32, bf16 or fp16, 16-byte aligned, C a multiple
// of the channels in a lane's 16 bytes (4, 8 for 16-bit elements); the statistics (absent before the forward has produced them)
// and the optional weight fp32, contiguous and of length C.  The 16-bit route adds "dy has x's dtype and sizes", the pooled
// node "n * h * w < 2^31 and a weight" (and, for a 16-bit x, the HIP forward's eligibility), at their call sites.
inline bool bn_hip_eligible(const Tensor& x, const Tensor& w, const Tensor* mean = nullptr, const Tensor* invstd = nullptr) {
  if (!x.is_cuda() || (x.scalar_type() != at::kFloat && act_dtype(x) == 0) || x.dim() != 4 || x.numel() == 0) return false;
  if (!x.is_contiguous(at::MemoryFormat::ChannelsLast) || (x.size(1) & (act_dtype(x) ? 7 : 3)) || !aligned16(x)) return false;
  auto stat_ok = [&](const Tensor& t) {
    return t.defined() && t.is_cuda() && t.scalar_type() == at::kFloat && t.is_contiguous() && t.numel() == x.size(1);
  };
  return (!mean || stat_ok(*mean)) && (!invstd || stat_ok(*invstd)) && (!w.defined() || stat_ok(w));
}

std::atomic<int64_t> g_bn_hip_backwards{0};   // backwards that took mhaq_fq_bn_bwd (tests: the fallback is never silent)
std::atomic<int64_t> g_bn_hip_backwards_x16{0};   // ... that took mhaq_fq_bn_bwd_x16
std::atomic<int64_t> g_bn_pool_hip_backwards{0};   // ... that took mhaq_fq_bn_pool_bwd
std::atomic<int64_t> g_bn_pool_hip_backwards_x16{0};   // ... that took mhaq_fq_bn_pool_bwd_x16
std::atomic<int64_t> g_bn_pool_hip_forwards_x16{0};   // forwards of the 16-bit pooled node (mhaq_fq_bn_norm_pool3s2_fwd_x16)

// ... and the opt-in HIP FORWARD (mhaq_fq_bn_fwd; `hip_forward` of bn_train / bn_pool_train): taken where bn_hip_eligible
// holds for an fp32 x with N * H * W >= 2, the bias is eligible like the weight, and the running statistics are both absent or
// both fp32 contiguous device tensors of length C.  Anything else is the framework's forward, as without the flag.
// A 16-bit x takes mhaq_fq_bn_fwd_x16 under the same conditions (C % 8 == 0 by bn_hip_eligible) where bn_train's caller set
// `hip_forward_x16` next to `x16`: the 16-bit backward is the only backward such a node has.
std::atomic<int64_t> g_bn_hip_forwards{0};   // forwards of both nodes that took mhaq_fq_bn_fwd
std::atomic<int64_t> g_bn_hip_forwards_x16{0};   // forwards of bn_train that took mhaq_fq_bn_fwd_x16

inline Tensor opt_tensor(const std::optional<Tensor>& t) { return t.has_value() ? *t : Tensor(); }

// x16: the eligibility of a 16-bit x (mhaq_fq_bn_fwd_x16) instead of an fp32 one
inline bool bn_hip_forward_eligible(const Tensor& x, const Tensor& w, const Tensor& b, const Tensor& rm, const Tensor& rv,
                                    bool x16 = false) {
  if (rm.defined() != rv.defined()) return false;
  return bn_hip_eligible(x, w) && (x16 ? act_dtype(x) != 0 : x.scalar_type() == at::kFloat) && x.numel() / x.size(1) >= 2 &&
         bn_hip_eligible(x, b, rm.defined() ? &rm : nullptr, rv.defined() ? &rv : nullptr);
}

// One HIP BatchNorm forward of an eligible x: {y, mean, invstd}; the running statistics are updated in place, with their
// version counters bumped as the framework's in-place update bumps them.  The entry point follows from x's dtype; the
// statistics are fp32 either way.  with_y = false (the 16-bit pooled node): the statistics alone, y stays undefined and the
// third launch is skipped (y == NULL); that call belongs to the pooled node's counter, not to bn_hip_forwards_x16.
std::array<Tensor, 3> bn_hip_forward(const Tensor& x, const Tensor& w, const Tensor& b, const Tensor& rm, const Tensor& rv,
                                     double momentum, double eps, bool with_y = true) {
  need_lib();
  const int64_t c = x.size(1), m = x.numel() / c;
  Tensor y = with_y ? at::empty_like(x) : Tensor();
  const int dt = act_dtype(x);
  TORCH_CHECK(with_y || dt, "bn_hip_forward: the statistics-only form is the 16-bit pooled node's");
  Tensor mean = at::empty({c}, x.options().dtype(at::kFloat)), invstd = at::empty({c}, x.options().dtype(at::kFloat));
  const size_t nb = dt ? A.mhaq_fq_bn_fwd_x16_workspace_bytes(m, c) : A.mhaq_fq_bn_fwd_workspace_bytes(m, c);
  Tensor ws = at::empty({(int64_t)nb}, x.options().dtype(at::kByte));
  float *rmp = rm.defined() ? fptr_mut(rm) : nullptr, *rvp = rv.defined() ? fptr_mut(rv) : nullptr;
  if (dt) {
    check(A.mhaq_fq_bn_fwd_x16(x.const_data_ptr(), fptr_or_null(w), fptr_or_null(b), with_y ? y.mutable_data_ptr() : nullptr,
                               fptr_mut(mean), fptr_mut(invstd), rmp, rvp, momentum, eps, m, c, dt, ws.mutable_data_ptr(), nb,
                               cur_stream(x)),
          "mhaq_fq_bn_fwd_x16");
    if (with_y) g_bn_hip_forwards_x16.fetch_add(1, std::memory_order_relaxed);
  } else {
    check(A.mhaq_fq_bn_fwd(fptr(x), fptr_or_null(w), fptr_or_null(b), fptr_mut(y), fptr_mut(mean), fptr_mut(invstd), rmp, rvp,
                           momentum, eps, m, c, ws.mutable_data_ptr(), nb, cur_stream(x)),
          "mhaq_fq_bn_fwd");
    g_bn_hip_forwards.fetch_add(1, std::memory_order_relaxed);
  }
  if (rm.defined()) {
    torch::autograd::impl::bump_version(rm);
    torch::autograd::impl::bump_version(rv);
  }
  return {y, mean, invstd};
}

// One HIP BatchNorm backward of an eligible x: {dx, dweight, dbias} in the first three of `slots` outputs, undefined where the
// mask says so.  The gradient comes as dy in x's layout or, with `code`, as the pooled gradient in the layout of its argmax
// codes (of x's dtype either way); the entry point follows from that and from x's dtype: four cases.
variable_list bn_hip_backward(size_t slots, const Tensor& x, const Tensor& grad, const Tensor& code, const Tensor& w,
                              const Tensor& mean, const Tensor& invstd, const std::array<bool, 3>& mask) {
  need_lib();
  const int64_t n = x.size(0), c = x.size(1), h = x.size(2), wd = x.size(3), m = x.numel() / c;
  const int dt = act_dtype(x);
  Tensor dx = mask[0] ? at::empty_like(x) : Tensor();
  Tensor dw = mask[1] ? at::empty_like(w) : Tensor();
  Tensor db = mask[2] ? at::empty({c}, mean.options()) : Tensor();
  const size_t nb = code.defined() ? (dt ? A.mhaq_fq_bn_pool_bwd_x16_workspace_bytes(n, h, wd, c)
                                         : A.mhaq_fq_bn_pool_bwd_workspace_bytes(n, h, wd, c))
                                   : dt ? A.mhaq_fq_bn_bwd_x16_workspace_bytes(m, c) : A.mhaq_fq_bn_bwd_workspace_bytes(m, c);
  Tensor ws = at::empty({(int64_t)nb}, x.options().dtype(at::kByte));
  void* dxp = mask[0] ? dx.mutable_data_ptr() : nullptr;
  float *dwp = mask[1] ? fptr_mut(dw) : nullptr, *dbp = mask[2] ? fptr_mut(db) : nullptr;
  if (code.defined() && dt) {
    check(A.mhaq_fq_bn_pool_bwd_x16(x.const_data_ptr(), grad.const_data_ptr(), static_cast<const uint8_t*>(code.const_data_ptr()),
                                    fptr(mean), fptr(invstd), fptr_or_null(w), dxp, dwp, dbp, n, h, wd, c, dt,
                                    ws.mutable_data_ptr(), nb, cur_stream(x)),
          "mhaq_fq_bn_pool_bwd_x16");
    g_bn_pool_hip_backwards_x16.fetch_add(1, std::memory_order_relaxed);
  } else if (code.defined()) {
    check(A.mhaq_fq_bn_pool_bwd(fptr(x), fptr(grad), static_cast<const uint8_t*>(code.const_data_ptr()), fptr(mean),
                                fptr(invstd), fptr_or_null(w), static_cast<float*>(dxp), dwp, dbp, n, h, wd, c,
                                ws.mutable_data_ptr(), nb, cur_stream(x)),
          "mhaq_fq_bn_pool_bwd");
    g_bn_pool_hip_backwards.fetch_add(1, std::memory_order_relaxed);
  } else if (dt) {
    check(A.mhaq_fq_bn_bwd_x16(x.const_data_ptr(), grad.const_data_ptr(), fptr(mean), fptr(invstd), fptr_or_null(w), dxp, dwp,
                               dbp, m, c, dt, ws.mutable_data_ptr(), nb, cur_stream(x)),
          "mhaq_fq_bn_bwd_x16");
    g_bn_hip_backwards_x16.fetch_add(1, std::memory_order_relaxed);
  } else {
    check(A.mhaq_fq_bn_bwd(fptr(x), fptr(grad), fptr(mean), fptr(invstd), fptr_or_null(w), static_cast<float*>(dxp), dwp, dbp,
                           m, c, ws.mutable_data_ptr(), nb, cur_stream(x)),
          "mhaq_fq_bn_bwd");
    g_bn_hip_backwards.fetch_add(1, std::memory_order_relaxed);
  }
  variable_list out(slots);
  out[0] = dx;
  out[1] = dw;
  out[2] = db;
  return out;
}

class BatchNormTrainFn : public torch::autograd::Function<BatchNormTrainFn> {
 public:
  static Tensor forward(AutogradContext* ctx, const Tensor& x, const std::optional<Tensor>& w,
                        const std::optional<Tensor>& b, const std::optional<Tensor>& running_mean,
                        const std::optional<Tensor>& running_var, double momentum, double eps, bool cudnn_enabled,
                        bool x16, bool hip_forward, bool hip_forward_x16) {
    const bool has_w = w.has_value() && w->defined();
    ctx->saved_data["hip_fwd"] = false;
    // a 16-bit x: only with the 16-bit backward enabled next to it (`x16`), the one backward such a node can take
    const bool fwd16 = act_dtype(x) != 0;
    if ((fwd16 ? hip_forward_x16 && x16 : hip_forward) &&
        bn_hip_forward_eligible(x, opt_tensor(w), opt_tensor(b), opt_tensor(running_mean), opt_tensor(running_var), fwd16)) {
      // the HIP forward: no reserve, no implementation index; such a node is eligible for the HIP backward by construction
      // (autograd hands a dy of y's dtype and sizes)
      auto out = bn_hip_forward(x, opt_tensor(w), opt_tensor(b), opt_tensor(running_mean), opt_tensor(running_var), momentum,
                                eps);
      ctx->save_for_backward({x, has_w ? *w : Tensor(), out[1], out[2], Tensor()});
      ctx->saved_data["hip_fwd"] = true;
      ctx->saved_data["x16"] = fwd16;
      ctx->set_materialize_grads(false);
      return out[0];
    }
    auto out = at::_batch_norm_impl_index(x, w, b, running_mean, running_var, /*training=*/true, momentum, eps,
                                          cudnn_enabled);
    ctx->save_for_backward({x, has_w ? *w : Tensor(), std::get<1>(out), std::get<2>(out), std::get<3>(out)});
    ctx->saved_data["impl"] = std::get<4>(out);
    ctx->saved_data["eps"] = eps;
    ctx->saved_data["x16"] = x16;
    // read by no training-mode backward; handed on as the framework's own node does, without its version check
    if (running_mean.has_value() && running_mean->defined()) ctx->saved_data["rm"] = *running_mean;
    if (running_var.has_value() && running_var->defined()) ctx->saved_data["rv"] = *running_var;
    ctx->set_materialize_grads(false);
    return std::get<0>(out);
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    variable_list out(11);
    if (!grads[0].defined()) return out;
    TORCH_CHECK(!(at::GradMode::is_enabled() && grads[0].requires_grad()),
                "bn_train: the node is once-differentiable (no double backward)");
    at::NoGradGuard no_grad;
    auto saved = ctx->get_saved_variables();
    const Tensor &x = saved[0], &w = saved[1], &mean = saved[2], &invstd = saved[3], &reserve = saved[4];
    const std::array<bool, 3> mask = {ctx->needs_input_grad(0), w.defined() && ctx->needs_input_grad(1),
                                      ctx->needs_input_grad(2)};
    // the route: 16-bit where the caller enabled it and dy has x's dtype and sizes, else fp32, else the framework's own backward
    const bool hip = bn_hip_eligible(x, w, &mean, &invstd);
    if (hip && act_dtype(x) != 0 && ctx->saved_data["x16"].toBool() && grads[0].scalar_type() == x.scalar_type() &&
        grads[0].sizes() == x.sizes()) {
      const Tensor dy = like_layout(grads[0], x);
      if (dy.is_cuda()) return bn_hip_backward(11, x, dy, Tensor(), w, mean, invstd, mask);
    }
    if (hip && x.scalar_type() == at::kFloat) {
      const Tensor dy = like_layout(grads[0].scalar_type() == at::kFloat ? grads[0] : grads[0].to(at::kFloat), x);
      return bn_hip_backward(11, x, dy, Tensor(), w, mean, invstd, mask);
    }
    TORCH_CHECK(!ctx->saved_data["hip_fwd"].toBool(), "bn_train: a node whose forward was mhaq_fq_bn_fwd / mhaq_fq_bn_fwd_x16 "
                "has no framework backward to fall back to");
    auto opt = [](const Tensor& t) { return t.defined() ? std::optional<Tensor>(t) : std::nullopt; };
    auto get = [&](const char* k) {
      return ctx->saved_data.count(k) ? std::optional<Tensor>(ctx->saved_data[k].toTensor()) : std::nullopt;
    };
    auto g = at::_batch_norm_impl_index_backward(ctx->saved_data["impl"].toInt(), x, grads[0], opt(w), get("rm"), get("rv"),
                                                 opt(mean), opt(invstd), /*train=*/true, ctx->saved_data["eps"].toDouble(),
                                                 mask, reserve);
    if (mask[0]) out[0] = std::get<0>(g);
    if (mask[1]) out[1] = std::get<1>(g);
    if (mask[2]) out[2] = std::get<2>(g);
    return out;
  }
};

Tensor bn_train(const Tensor& x, const std::optional<Tensor>& w, const std::optional<Tensor>& b,
                const std::optional<Tensor>& running_mean, const std::optional<Tensor>& running_var, double momentum,
                double eps, bool cudnn_enabled, bool x16, bool hip_forward, bool hip_forward_x16) {
  TORCH_CHECK(w.has_value() && w->defined() && b.has_value() && b->defined(),
              "bn_train: an affine BatchNorm (weight and bias) is required");
  MHAQ_ON_DEVICE_OF(x);
  return BatchNormTrainFn::apply(x, w, b, running_mean, running_var, momentum, eps, cudnn_enabled, x16, hip_forward,
                                 hip_forward_x16);
}

// ------------------------------------------------------------------------------------------------ BatchNorm + stem pool
// max_pool2d(bn_train(x, ..), 3, 2, 1) as ONE node (the ResNet stem, mhaq_amd/fused_blocks.py).  Forward: the framework's
// BatchNorm forward as above (mhaq_fq_bn_fwd with `hip_forward`, where eligible), then mhaq_fq_maxpool3s2_fwd, which leaves
// the pooled tensor and a 1-byte argmax code per output; the BatchNorm output dies with the forward, and neither it nor int64 indices are kept for the backward.
// Backward: mhaq_fq_bn_pool_bwd, the BatchNorm backward that gathers its dy from the pooled gradient and the codes instead
// of reading a materialized one.  Output, running statistics and the three gradients are the bits of the two nodes run one
// after the other.  Taken under BatchNormTrainFn's own conditions (and n * h * w < 2^31); outside them bn_pool_train IS
// that composition.
// The 16-bit form (`pool_x16` next to `x16`; a bf16 / fp16 x under autocast) never calls the framework's 16-bit BatchNorm forward:
// mhaq_fq_bn_fwd_x16 with y == NULL leaves the statistics (and updates the running ones) in two launches, and
// mhaq_fq_bn_norm_pool3s2_fwd_x16 writes the pooled tensor and the codes from x and those statistics in a third: neither the
// BatchNorm output nor int64 indices exist at any time.  Backward: mhaq_fq_bn_pool_bwd_x16 on a pooled gradient of x's dtype.
// Its outputs, statistics and gradients are the bits of max_pool2d(bn_train(x, .., x16, hip_forward_x16 = true)).  Taken where
// that 16-bit HIP forward would apply (bn_hip_forward_eligible) and n * h * w < 2^31; a 16-bit x outside that is
// max_pool2d(bn_train(x, ..)) with the caller's x16 and hip_forward_x16.
class BatchNormPoolTrainFn : public torch::autograd::Function<BatchNormPoolTrainFn> {
 public:
  static Tensor forward(AutogradContext* ctx, const Tensor& x, const Tensor& w, const Tensor& b,
                        const std::optional<Tensor>& running_mean, const std::optional<Tensor>& running_var,
                        double momentum, double eps, bool cudnn_enabled, bool hip_forward, bool pool_x16) {
    // hip_forward, pool_x16: bn_pool_train has checked bn_hip_forward_eligible before this node was entered
    const int64_t n = x.size(0), c = x.size(1), h = x.size(2), wd = x.size(3);
    if (pool_x16) {
      // a 16-bit x: the statistics from mhaq_fq_bn_fwd_x16 without a y (two launches; the running statistics are updated), then
      // normalisation and pool in one launch.  The framework's 16-bit BatchNorm forward is not called on this path.
      auto out = bn_hip_forward(x, w, b, opt_tensor(running_mean), opt_tensor(running_var), momentum, eps, /*with_y=*/false);
      const Tensor &mean = out[1], &invstd = out[2];
      Tensor p = at::empty({n, c, (h - 1) / 2 + 1, (wd - 1) / 2 + 1}, x.options().memory_format(at::MemoryFormat::ChannelsLast));
      Tensor code = at::empty_like(p, p.options().dtype(at::kByte));      // p's strides: NHWC, one byte per element
      check(A.mhaq_fq_bn_norm_pool3s2_fwd_x16(x.const_data_ptr(), fptr(mean), fptr(invstd), fptr(w), fptr(b), p.mutable_data_ptr(),
                                              static_cast<uint8_t*>(code.mutable_data_ptr()), n, h, wd, c, act_dtype(x),
                                              cur_stream(x)),
            "mhaq_fq_bn_norm_pool3s2_fwd_x16");
      g_bn_pool_hip_forwards_x16.fetch_add(1, std::memory_order_relaxed);
      ctx->save_for_backward({x, w, mean, invstd, code});
      ctx->set_materialize_grads(false);
      return p;
    }
    Tensor t, mean, invstd;
    if (hip_forward) {
      auto out = bn_hip_forward(x, w, b, opt_tensor(running_mean), opt_tensor(running_var), momentum, eps);
      t = out[0], mean = out[1], invstd = out[2];
    } else {
      auto out = at::_batch_norm_impl_index(x, w, b, running_mean, running_var, /*training=*/true, momentum, eps,
                                            cudnn_enabled);
      mean = std::get<1>(out), invstd = std::get<2>(out);
      t = std::get<0>(out).contiguous(at::MemoryFormat::ChannelsLast);
    }
    TORCH_CHECK(bn_hip_eligible(x, w, &mean, &invstd), "bn_pool_train: the BatchNorm forward left statistics the HIP "
                "backward cannot read (there is no fallback behind this point)");
    Tensor p = at::empty({n, c, (h - 1) / 2 + 1, (wd - 1) / 2 + 1}, x.options().memory_format(at::MemoryFormat::ChannelsLast));
    Tensor code = at::empty_like(p, p.options().dtype(at::kByte));
    check(A.mhaq_fq_maxpool3s2_fwd(fptr(t), fptr_mut(p), static_cast<uint8_t*>(code.mutable_data_ptr()), n, h, wd, c,
                                   cur_stream(x)),
          "mhaq_fq_maxpool3s2_fwd");
    ctx->save_for_backward({x, w, mean, invstd, code});
    ctx->set_materialize_grads(false);
    return p;
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    variable_list out(10);
    if (!grads[0].defined()) return out;
    TORCH_CHECK(!(at::GradMode::is_enabled() && grads[0].requires_grad()),
                "bn_pool_train: the node is once-differentiable (no double backward)");
    at::NoGradGuard no_grad;
    auto saved = ctx->get_saved_variables();
    const Tensor &x = saved[0], &w = saved[1], &mean = saved[2], &invstd = saved[3], &code = saved[4];
    const std::array<bool, 3> mask = {ctx->needs_input_grad(0), ctx->needs_input_grad(1), ctx->needs_input_grad(2)};
    // the pooled gradient in x's dtype (fp32, or the 16-bit node's) and the memory order of the pooled tensor (= the codes')
    const auto gt = x.scalar_type();
    Tensor g = grads[0].scalar_type() == gt ? grads[0] : grads[0].to(gt);
    if (g.sizes() != code.sizes() || g.strides() != code.strides()) {
      Tensor dense = at::empty_like(code, code.options().dtype(gt));
      dense.copy_(g);
      g = dense;
    }
    return bn_hip_backward(10, x, g, code, w, mean, invstd, mask);
  }
};

Tensor bn_pool_train(const Tensor& x, const std::optional<Tensor>& w, const std::optional<Tensor>& b,
                     const std::optional<Tensor>& running_mean, const std::optional<Tensor>& running_var, double momentum,
                     double eps, bool cudnn_enabled, bool hip_forward, bool x16, bool pool_x16, bool hip_forward_x16) {
  TORCH_CHECK(w.has_value() && w->defined() && b.has_value() && b->defined(),
              "bn_pool_train: an affine BatchNorm (weight and bias) is required");
  MHAQ_ON_DEVICE_OF(x);
  if (act_dtype(x) != 0) {
    // A 16-bit x.  x16, hip_forward_x16: the flags of the unpooled node (bn_train).  The pooled node, with x16 and pool_x16: where
    // the 16-bit HIP forward applies (its statistics are that forward's) and the pool kernels' 32-bit pixel arithmetic holds.
    // Anything else is the unpooled node under its own flags and the framework's pool: what ran before pool_x16 existed.
    if (x16 && pool_x16 &&
        bn_hip_forward_eligible(x, *w, *b, opt_tensor(running_mean), opt_tensor(running_var), /*x16=*/true) &&
        x.numel() / x.size(1) < (1ll << 31)) {
      need_lib();
      return BatchNormPoolTrainFn::apply(x, *w, *b, running_mean, running_var, momentum, eps, cudnn_enabled,
                                         /*hip_forward=*/false, /*pool_x16=*/true);
    }
    return at::max_pool2d(BatchNormTrainFn::apply(x, w, b, running_mean, running_var, momentum, eps, cudnn_enabled, x16,
                                                  /*hip_forward=*/false, hip_forward_x16),
                          {3, 3}, {2, 2}, {1, 1});
  }
  // the HIP forward's eligibility is settled here, before either node runs: nothing a fallback needs is dropped later
  const bool hipf = hip_forward && bn_hip_forward_eligible(x, *w, *b, opt_tensor(running_mean), opt_tensor(running_var));
  // the fused node: fp32, with the 32-bit pixel arithmetic of its kernels (n * h * w < 2^31)
  if (!(bn_hip_eligible(x, *w) && x.scalar_type() == at::kFloat && x.numel() / x.size(1) < (1ll << 31)))
    return at::max_pool2d(BatchNormTrainFn::apply(x, w, b, running_mean, running_var, momentum, eps, cudnn_enabled,
                                                  /*x16=*/false, hipf, /*hip_forward_x16=*/false),
                          {3, 3}, {2, 2}, {1, 1});
  need_lib();
  return BatchNormPoolTrainFn::apply(x, *w, *b, running_mean, running_var, momentum, eps, cudnn_enabled, hipf,
                                     /*pool_x16=*/false);
}

// ------------------------------------------------------------------------------------------------ the frozen teacher
// Eval-mode BatchNorm with its ReLU, residual add and stem pool in one launch per place (mhaq_amd/frozen_blocks.py;
// mhaq_fq_bn_infer_*).  Plain functions, not nodes: the teacher runs without grad.  The caller has settled that the place may
// be fused; what arrives here and does not fit the kernels is an error, never a quiet framework path.  Outputs come from the
// caching allocator, the launch goes to the current stream of the input's device: no host synchronisation, capture-safe.
std::atomic<int64_t> g_teacher_fused_calls{0};   // launches of mhaq_fq_bn_infer_act and mhaq_fq_bn_relu_pool3s2 so far, fp32 and 16-bit
std::atomic<int64_t> g_teacher_fused_x16_calls{0};   // ... of them, the 16-bit ones (mhaq_fq_bn_infer_act_x16 / _relu_pool3s2_x16)

// x16: the caller takes bf16 / fp16 inputs too (C % 8 == 0); without it a 16-bit input is refused like any other non-fp32 one
inline void check_frozen_input(const Tensor& x, const Tensor& consts, const char* what, bool x16 = false) {
  TORCH_CHECK(bn_hip_eligible(x, Tensor()) && (x.scalar_type() == at::kFloat || x16), what,
              x16 ? ": x must be a non-empty dense channels_last device tensor, float32 with C % 4 == 0 or bfloat16 / float16 "
                    "with C % 8 == 0"
                  : ": x must be a non-empty dense channels_last float32 device tensor with C % 4 == 0");
  TORCH_CHECK(consts.defined() && consts.is_cuda() && consts.device() == x.device() && consts.scalar_type() == at::kFloat &&
                  consts.is_contiguous() && consts.numel() == 3 * x.size(1) && aligned16(consts),
              what, ": the constants must be a contiguous float32 [3, C] slab on x's device");
}

void bn_infer_consts(const Tensor& running_mean, const Tensor& running_var, const std::optional<Tensor>& weight,
                     const std::optional<Tensor>& bias, double eps, const Tensor& consts) {
  need_lib();
  const int64_t c = running_mean.numel();
  const Tensor w = opt_tensor(weight), b = opt_tensor(bias);
  auto vec_ok = [&](const Tensor& t) {
    return t.is_cuda() && t.device() == consts.device() && t.scalar_type() == at::kFloat && t.is_contiguous() && t.numel() == c;
  };
  TORCH_CHECK(consts.defined() && consts.is_cuda() && consts.scalar_type() == at::kFloat && consts.is_contiguous() &&
                  consts.numel() == 3 * c && vec_ok(running_mean) && vec_ok(running_var) && (!w.defined() || vec_ok(w)) &&
                  (!b.defined() || vec_ok(b)),
              "bn_infer_consts: contiguous float32 vectors of one length C on the device of a [3, C] slab are required");
  MHAQ_ON_DEVICE_OF(consts);
  check(A.mhaq_fq_bn_infer_consts(fptr(running_mean), fptr(running_var), fptr_or_null(w), fptr_or_null(b), eps, c,
                                  fptr_mut(consts), cur_stream(consts)),
        "mhaq_fq_bn_infer_consts");
}

// x16 (here and in bn_relu_pool): a bf16 / fp16 x takes the *_x16 entry point; an fp32 x takes the fp32 one either way.
Tensor bn_infer_act(const Tensor& x, const Tensor& consts, int64_t mode, const std::optional<Tensor>& x2,
                    const std::optional<Tensor>& consts2, const std::optional<Tensor>& residual, bool x16) {
  need_lib();
  check_frozen_input(x, consts, "bn_infer_act", x16);
  const Tensor b = opt_tensor(x2), k2 = opt_tensor(consts2), r = opt_tensor(residual);
  for (const Tensor* t : {&b, &r})
    TORCH_CHECK(!t->defined() || (t->is_cuda() && t->device() == x.device() && t->scalar_type() == x.scalar_type() &&
                                  t->sizes() == x.sizes() && t->strides() == x.strides() && aligned16(*t)),
                "bn_infer_act: the second input and the residual must have x's dtype, device, sizes and strides");
  if (b.defined()) check_frozen_input(b, k2, "bn_infer_act (second input)", x16);
  MHAQ_ON_DEVICE_OF(x);
  const int64_t c = x.size(1), m = x.numel() / c;
  const int dt = act_dtype(x);
  Tensor y = at::empty_like(x);
  if (dt) {
    auto vptr = [](const Tensor& t) { return t.defined() ? t.const_data_ptr() : nullptr; };
    check(A.mhaq_fq_bn_infer_act_x16(x.const_data_ptr(), fptr(consts), vptr(b), fptr_or_null(k2), vptr(r), y.mutable_data_ptr(),
                                     m, c, (int)mode, dt, cur_stream(x)),
          "mhaq_fq_bn_infer_act_x16");
    g_teacher_fused_x16_calls.fetch_add(1, std::memory_order_relaxed);
  } else {
    check(A.mhaq_fq_bn_infer_act(fptr(x), fptr(consts), fptr_or_null(b), fptr_or_null(k2), fptr_or_null(r), fptr_mut(y), m, c,
                                 (int)mode, cur_stream(x)),
          "mhaq_fq_bn_infer_act");
  }
  g_teacher_fused_calls.fetch_add(1, std::memory_order_relaxed);
  return y;
}

Tensor bn_relu_pool(const Tensor& x, const Tensor& consts, bool x16) {
  need_lib();
  check_frozen_input(x, consts, "bn_relu_pool", x16);
  MHAQ_ON_DEVICE_OF(x);
  const int64_t n = x.size(0), c = x.size(1), h = x.size(2), wd = x.size(3);
  const int dt = act_dtype(x);
  Tensor p = at::empty({n, c, (h - 1) / 2 + 1, (wd - 1) / 2 + 1}, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  if (dt) {
    check(A.mhaq_fq_bn_relu_pool3s2_x16(x.const_data_ptr(), fptr(consts), p.mutable_data_ptr(), n, h, wd, c, dt, cur_stream(x)),
          "mhaq_fq_bn_relu_pool3s2_x16");
    g_teacher_fused_x16_calls.fetch_add(1, std::memory_order_relaxed);
  } else {
    check(A.mhaq_fq_bn_relu_pool3s2(fptr(x), fptr(consts), fptr_mut(p), n, h, wd, c, cur_stream(x)), "mhaq_fq_bn_relu_pool3s2");
  }
  g_teacher_fused_calls.fetch_add(1, std::memory_order_relaxed);
  return p;
}

// ------------------------------------------------------------------------------------------------ weight layer ops
struct Pre {   // this step's forward of the layer out of the model-wide launch (multi.py, forward-only mode)
  bool has = false;
  Tensor wq, s, zp, mx, lwq;
};

// set from Python: the packed AEWGS statistics exchange (takes the GIL).  A raw, never-released reference: static
// destructors run after the interpreter is gone.
PyObject* g_allreduce_avg = nullptr;
std::atomic<bool> g_dist_active{false};

void allreduce_avg(const Tensor& t) {
  py::gil_scoped_acquire gil;
  if (!g_allreduce_avg) throw MhaqError("AEWGS statistics exchange requested but no all-reduce is installed");
  py::reinterpret_borrow<py::object>(g_allreduce_avg)(t);
}

// Per-channel NoisyConv2d weight path from log_wght_s plus the layer's regulariser input lwq = log2(max - min + s)
// (gdnsq_conv2d.py:71-98, model_helper.py:24-44): returns (wq, zp, s, lwq).
class WeightLayerFn : public torch::autograd::Function<WeightLayerFn> {
 public:
  static variable_list forward(AutogradContext* ctx, const Tensor& w, const Tensor& log_s, int64_t method,
                               const std::optional<Tensor>& r_sign, bool zp_grad, const Pre& pre, int64_t rank,
                               bool distributed) {
    const int64_t co = w.size(0), row = co ? w.numel() / co : 0;
    Tensor wq, s, zp, mx, lwq;
    if (pre.has) {
      wq = pre.wq; s = pre.s; zp = pre.zp; mx = pre.mx; lwq = pre.lwq;
    } else {
      wq = at::empty_like(w);
      Tensor aux = at::empty({4, co}, w.options());
      s = aux.select(0, 0); zp = aux.select(0, 1); mx = aux.select(0, 2); lwq = aux.select(0, 3);
      check(A.mhaq_fq_wlayer_fwd(fptr(w), fptr_mut(wq), fptr(log_s), co, row, fptr_mut(s), fptr_mut(zp), fptr_mut(mx),
                                 fptr_mut(lwq), cur_stream(w)),
            "mhaq_fq_wlayer_fwd");
    }
    weight_save_ctx(ctx, {w, s, zp, mx}, r_sign, method, rank, log_s);
    ctx->saved_data["dist"] = distributed;
    // zp_grad = the quantized-bias mode (gdnsq_conv2d.py:86-94): the bias quantizer reuses this layer's s and zp and
    // sends gradient into both, so both stay differentiable outputs
    if (!zp_grad) ctx->mark_non_differentiable({s, zp});
    return {wq, zp, s, lwq};
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    auto saved = ctx->get_saved_variables();
    const Tensor &w = saved[0], &s = saved[1], &zp = saved[2], &mx = saved[3];
    const bool has_r = saved.size() > 4;
    const int64_t method = ctx->saved_data["method"].toInt();
    Tensor G = grads[0].defined() ? like_layout(grads[0], w) : at::zeros_like(w);
    Tensor gzp_extra = grads[1].defined() ? grads[1].contiguous() : Tensor();
    Tensor g_lwq = grads[3].defined() ? grads[3].contiguous() : Tensor();
    const int64_t co = w.size(0), row = co ? w.numel() / co : 0;
    Tensor stats;
    if (method == MHAQ_FQ_AEWGS && ctx->saved_data["dist"].toBool()) {
      stats = at::empty({3, co}, w.options());
      check(A.mhaq_fq_pc_aewgs_stats(fptr(w), fptr(G), fptr(s), fptr(zp), co, row, fptr_mut(stats), cur_stream(w)),
            "mhaq_fq_pc_aewgs_stats");
      allreduce_avg(stats);          // gdnsq.py:126-129, one packed message
    }
    Tensor gw = at::empty_like(w);
    Tensor gls = at::empty({co}, w.options());
    const Draw d = draw_signs(has_r, method, ctx->saved_data["rank"].toInt(), w);
    check(A.mhaq_fq_wlayer_bwd(fptr(w), fptr(G), fptr_mut(gw), fptr_mut(gls), fptr(s), fptr(zp), fptr(mx),
                               fptr_or_null(g_lwq), co, row, (int)method, fptr_or_null(stats), fptr_or_null(gzp_extra),
                               saved_sign(saved, 4), d.seed, d.offset, d.offset_dev, cur_stream(w)),
          "mhaq_fq_wlayer_bwd");
    if (grads[2].defined())     // gradient reaching s from the quantized bias: exp2 backward, grad * s * ln2
      gls = gls + at::mul(at::mul(grads[2].reshape({co}), s), 0.69314718055994531);
    variable_list out(8);
    out[0] = gw;
    out[1] = ls_view(ctx, gls);
    return out;
  }
};

// returns (wq, zp [co,1,..], s [co,1,..], lwq [co])
std::tuple<Tensor, Tensor, Tensor, Tensor> weight_layer(const Tensor& w_in, const Tensor& log_s_in, int64_t method,
                                                        const std::optional<Tensor>& r_sign, bool zp_grad,
                                                        const std::optional<std::vector<Tensor>>& pre, int64_t rank) {
  need_lib();
  MHAQ_ON_DEVICE_OF(w_in);
  TORCH_CHECK(w_in.is_cuda() && w_in.scalar_type() == at::kFloat && log_s_in.is_cuda() &&
                  log_s_in.scalar_type() == at::kFloat,
              "weight_layer: weight and log_wght_s must be float32 device tensors");
  TORCH_CHECK(w_in.dim() >= 1 && log_s_in.numel() == w_in.size(0), "per-channel log scale must have ", w_in.size(0),
              " elements, got ", log_s_in.sizes());
  const Tensor w = w_in.is_non_overlapping_and_dense() ? w_in : w_in.contiguous();
  const Tensor log_s = log_s_in.is_contiguous() ? log_s_in : log_s_in.contiguous();
  Pre p;
  if (pre.has_value()) {
    TORCH_CHECK(pre->size() >= 5, "weight_layer: pre = (wq, s, zp, mx, lwq[, s and zp in the published shape])");
    p.has = true;
    p.wq = (*pre)[0]; p.s = (*pre)[1]; p.zp = (*pre)[2]; p.mx = (*pre)[3]; p.lwq = (*pre)[4];
  }
  auto out = WeightLayerFn::apply(w, log_s, method, r_sign, zp_grad, p, rank, g_dist_active.load());
  std::vector<int64_t> shp(w.dim(), 1);
  shp[0] = w.size(0);
  return {out[0], out[1].view(shp), out[2].view(shp), out[3]};
}

// what weight_layer_pt / _ptl return from their node's (wq, aux = {s, zp, ..}, lwq): (wq, zp 0-dim, s [1], lwq [1])
std::tuple<Tensor, Tensor, Tensor, Tensor> pt_result(const variable_list& out) {
  const Tensor& aux = out[1];
  return {out[0], aux.select(0, 1), aux.narrow(0, 0, 1), out[2]};
}

// PER_TENSOR weight layer small enough for one workgroup (every CIFAR ResNet-20 / RFDN layer): one launch per
// direction from log_wght_s, regulariser input included.  Returns (wq, aux[4] = {s, zp, max, lwq}, lwq[1]).
class WeightLayerPTFn : public torch::autograd::Function<WeightLayerPTFn> {
 public:
  static variable_list forward(AutogradContext* ctx, const Tensor& w, const Tensor& log_s, int64_t method,
                               const std::optional<Tensor>& r_sign, int64_t rank) {
    Tensor wq = at::empty_like(w);
    Tensor aux = at::empty({4}, w.options());
    check(A.mhaq_fq_wlayer_pt_fwd(fptr(w), fptr_mut(wq), fptr(log_s), w.numel(), fptr_mut(aux), cur_stream(w)),
          "mhaq_fq_wlayer_pt_fwd");
    Tensor lwq = aux.narrow(0, 3, 1).clone();
    weight_save_ctx(ctx, {w, aux}, r_sign, method, rank, log_s);
    ctx->mark_non_differentiable({aux});
    return {wq, aux, lwq};
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    auto saved = ctx->get_saved_variables();
    const Tensor &w = saved[0], &aux = saved[1];
    const bool has_r = saved.size() > 2;
    const int64_t method = ctx->saved_data["method"].toInt();
    Tensor G = grads[0].defined() ? grads[0].contiguous() : at::zeros_like(w);
    Tensor g_lwq = grads[2].defined() ? grads[2].contiguous() : Tensor();
    Tensor gw = at::empty_like(w);
    Tensor gls = at::empty({1}, w.options());
    const Draw d = draw_signs(has_r, method, ctx->saved_data["rank"].toInt(), w);
    check(A.mhaq_fq_wlayer_pt_bwd(fptr(w), fptr(G), fptr_mut(gw), fptr_mut(gls), fptr(aux), fptr_or_null(g_lwq), w.numel(),
                                  (int)method, saved_sign(saved, 2), d.seed, d.offset, d.offset_dev, cur_stream(w)),
          "mhaq_fq_wlayer_pt_bwd");
    variable_list out(5);
    out[0] = gw;
    out[1] = ls_view(ctx, gls);
    return out;
  }
};

// returns (wq, zp 0-dim, s [1], lwq [1])
std::tuple<Tensor, Tensor, Tensor, Tensor> weight_layer_pt(const Tensor& w_in, const Tensor& log_s, int64_t method,
                                                           const std::optional<Tensor>& r_sign, int64_t rank) {
  need_lib();
  MHAQ_ON_DEVICE_OF(w_in);
  TORCH_CHECK(w_in.is_cuda() && w_in.scalar_type() == at::kFloat && log_s.is_cuda() &&
                  log_s.scalar_type() == at::kFloat && log_s.numel() == 1,
              "weight_layer_pt: weight and a one-element log_wght_s must be float32 device tensors");
  const Tensor w = w_in.contiguous();
  auto out = WeightLayerPTFn::apply(w, log_s, method, r_sign, rank);
  return pt_result(out);
}

// PER_TENSOR weight layer of any size (and every PER_TENSOR AEWGS layer): streaming launches, regulariser input and its
// amin / amax backward included (mhaq_fq_wlayer_ptl_fwd / _bwd).  Returns (wq, aux[7], lwq[1]).
class WeightLayerPTLFn : public torch::autograd::Function<WeightLayerPTLFn> {
 public:
  static variable_list forward(AutogradContext* ctx, const Tensor& w, const Tensor& log_s, int64_t method,
                               const std::optional<Tensor>& r_sign, int64_t rank, bool distributed) {
    Tensor wq = at::empty_like(w);
    Tensor aux = at::empty({7}, w.options());
    const size_t nb = A.mhaq_fq_wlayer_ptl_workspace_bytes(w.numel());
    Tensor ws = at::empty({(int64_t)nb}, w.options().dtype(at::kByte));
    check(A.mhaq_fq_wlayer_ptl_fwd(fptr(w), fptr_mut(wq), fptr(log_s), w.numel(), fptr_mut(aux), ws.mutable_data_ptr(), nb,
                                   cur_stream(w)),
          "mhaq_fq_wlayer_ptl_fwd");
    Tensor lwq = aux.narrow(0, 3, 1).clone();
    weight_save_ctx(ctx, {w, aux}, r_sign, method, rank, log_s);
    ctx->saved_data["dist"] = distributed;
    ctx->mark_non_differentiable({aux});
    return {wq, aux, lwq};
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    auto saved = ctx->get_saved_variables();
    const Tensor &w = saved[0], &aux = saved[1];
    const bool has_r = saved.size() > 2;
    const int64_t method = ctx->saved_data["method"].toInt();
    Tensor G = grads[0].defined() ? like_layout(grads[0], w) : at::zeros_like(w);
    Tensor g_lwq = grads[2].defined() ? grads[2].contiguous() : Tensor();
    const int64_t n = w.numel();
    void* stream = cur_stream(w);
    Tensor stats;
    int64_t period = 0;
    if (method == MHAQ_FQ_AEWGS) {
      // statistics of a [1]-shaped scale: means over dim 0 per position (gdnsq.py:150-152), then the all-reduce of
      // gdnsq.py:126-129 as ONE packed [3, period] message
      const int64_t co = w.size(0);
      period = n / co;
      stats = at::empty({3, period}, w.options());
      const size_t sb = A.mhaq_fq_pt_aewgs_colstats_workspace_bytes(co, period);
      Tensor sws = sb ? at::empty({(int64_t)sb}, w.options().dtype(at::kByte)) : Tensor();
      check(A.mhaq_fq_pt_aewgs_colstats(fptr(w), fptr(G), co, period, fptr(aux), fptr(aux) + 1, nullptr, nullptr,
                                        fptr_mut(stats), sb ? sws.mutable_data_ptr() : nullptr, sb, stream),
            "mhaq_fq_pt_aewgs_colstats");
      if (ctx->saved_data["dist"].toBool()) allreduce_avg(stats);
    }
    Tensor gw = at::empty_like(w);
    Tensor gls = at::empty({1}, w.options());
    const size_t nb = A.mhaq_fq_wlayer_ptl_workspace_bytes(n);
    Tensor ws = at::empty({(int64_t)nb}, w.options().dtype(at::kByte));
    const Draw d = draw_signs(has_r, method, ctx->saved_data["rank"].toInt(), w);
    check(A.mhaq_fq_wlayer_ptl_bwd(fptr(w), fptr(G), fptr_mut(gw), fptr_mut(gls), fptr(aux), fptr_or_null(g_lwq), n,
                                   (int)method, fptr_or_null(stats), period, saved_sign(saved, 2), d.seed, d.offset,
                                   d.offset_dev, ws.mutable_data_ptr(), nb, stream),
          "mhaq_fq_wlayer_ptl_bwd");
    variable_list out(6);
    out[0] = gw;
    out[1] = ls_view(ctx, gls);
    return out;
  }
};

// returns (wq, zp 0-dim, s [1], lwq [1])
std::tuple<Tensor, Tensor, Tensor, Tensor> weight_layer_ptl(const Tensor& w_in, const Tensor& log_s, int64_t method,
                                                            const std::optional<Tensor>& r_sign, int64_t rank) {
  need_lib();
  MHAQ_ON_DEVICE_OF(w_in);
  TORCH_CHECK(w_in.is_cuda() && w_in.scalar_type() == at::kFloat && log_s.is_cuda() &&
                  log_s.scalar_type() == at::kFloat && log_s.numel() == 1 && w_in.numel() > 0 && w_in.dim() >= 1,
              "weight_layer_ptl: a non-empty weight and a one-element log_wght_s must be float32 device tensors");
  // any dense layout with dim 0 outermost (contiguous, channels_last): the quantizer is elementwise and the AEWGS
  // statistics are per physical position within a dim-0 slice
  const Tensor w = w_in.is_non_overlapping_and_dense() ? w_in : w_in.contiguous();
  auto out = WeightLayerPTLFn::apply(w, log_s, method, r_sign, rank, g_dist_active.load());
  return pt_result(out);
}

// ------------------------------------------------------------------------------------------------ weight plan / groups
// The model-wide weight forward and the grouped backward of mhaq_amd/multi.py (MultiTensorWeightQuant with
// joint_backward=False, _WeightGroup, _TablePool), host side in C++.
struct TablePool {
  // Device descriptor tables for launches whose pointers (the dL/dWq tensors autograd hands over) are only known at
  // backward time.  Device tables and pinned staging buffers are allocated up front: inside a hipGraph capture
  // nothing may be allocated, and a captured upload re-reads its staging buffer at every replay -- so an entry
  // filled during a capture is never reused (until release_captured()).
  std::vector<Tensor> dev, host;
  std::vector<std::vector<int64_t>> keys;
  std::vector<char> used, held;
  std::vector<hipEvent_t> events;
  std::vector<uint64_t> stamp;
  uint64_t clock = 0;

  TablePool(size_t nbytes, const Tensor& like, int size = 8) {
    for (int i = 0; i < size; ++i) {
      dev.push_back(at::empty({(int64_t)nbytes}, like.options().dtype(at::kByte)));
      host.push_back(at::empty({(int64_t)nbytes}, at::TensorOptions().dtype(at::kByte).pinned_memory(true)));
    }
    keys.resize(size);
    used.assign(size, 0);
    held.assign(size, 0);
    events.assign(size, nullptr);
    stamp.assign(size, 0);
  }
  ~TablePool() {
    for (auto e : events)
      if (e) (void)hipEventDestroy(e);
  }

  template <class Fill>
  const Tensor& get(const std::vector<int64_t>& key, Fill fill, void* stream) {
    ++clock;
    const bool cap = capturing();
    const int n = (int)keys.size();
    for (int i = 0; i < n; ++i)
      if (used[i] && keys[i] == key && (held[i] || !cap)) { stamp[i] = clock; return dev[i]; }
    int pick = -1;
    for (int i = 0; i < n && pick < 0; ++i)
      if (!used[i]) pick = i;
    if (pick < 0) {
      // (waiting on an eager upload's event is not a capturable call: a capture only takes unused entries)
      if (cap) throw MhaqError("weight-group descriptor tables: no unused entry left for a captured launch");
      for (int i = 0; i < n; ++i)
        if (!held[i] && (pick < 0 || stamp[i] < stamp[pick])) pick = i;
      if (pick < 0) throw MhaqError("weight-group descriptor tables exhausted by captured graphs");
      if (events[pick]) C10_HIP_CHECK(hipEventSynchronize(events[pick]));   // the staging buffer's previous upload must have run
    }
    fill(host[pick].mutable_data_ptr());
    C10_HIP_CHECK(hipMemcpyAsync(dev[pick].mutable_data_ptr(), host[pick].const_data_ptr(), (size_t)dev[pick].numel(),
                                 hipMemcpyHostToDevice, (hipStream_t)stream));
    keys[pick] = key;
    used[pick] = 1;
    held[pick] = cap;
    stamp[pick] = clock;
    if (!cap) {
      if (!events[pick]) C10_HIP_CHECK(hipEventCreateWithFlags(&events[pick], hipEventDisableTiming));
      C10_HIP_CHECK(hipEventRecord(events[pick], (hipStream_t)stream));
    }
    return dev[pick];
  }

  void release_captured() {
    for (size_t i = 0; i < keys.size(); ++i)
      if (held[i]) { held[i] = 0; used[i] = 0; keys[i].clear(); }
  }
};

struct Plan;
struct Group {
  Plan* plan = nullptr;
  int64_t first = 0, n = 0, chan0 = 0, elem0 = 0, co = 0, elems = 0, max_row = 0, method = 0;
  std::unique_ptr<TablePool> pool;
};

struct Plan {
  std::mutex mu;
  int64_t nlayers = 0, total_elems = 0, total_co = 0, max_row = 0;
  std::vector<int64_t> co, row, elem_off, chan_off, methods, group_of;
  std::vector<Group> groups;
  TableCache fwd_tables;    // pointers of (weights, log scales) -> device table
  Tensor cur_wq, cur_aux;   // this step's model-wide forward
  static constexpr size_t kEagerTables = 2;
};

Registry<Plan>& g_plans = *new Registry<Plan>("weight plan");

int64_t plan_create(std::vector<int64_t> co, std::vector<int64_t> row, std::vector<int64_t> methods,
                    std::vector<std::pair<int64_t, int64_t>> groups) {
  auto p = std::make_shared<Plan>();
  p->nlayers = (int64_t)co.size();
  TORCH_CHECK(row.size() == co.size() && methods.size() == co.size(), "plan_create: co / row / methods disagree");
  p->co = co; p->row = row; p->methods = methods;
  int64_t e = 0, c = 0;
  for (size_t i = 0; i < co.size(); ++i) {
    p->elem_off.push_back(e);
    p->chan_off.push_back(c);
    e += co[i] * row[i];
    c += co[i];
    p->max_row = std::max(p->max_row, row[i]);
  }
  p->total_elems = e;
  p->total_co = c;
  p->group_of.assign(co.size(), -1);
  for (auto& fl : groups) {
    TORCH_CHECK(0 <= fl.first && fl.first < fl.second && fl.second <= p->nlayers, "plan_create: bad group range");
    Group g;
    g.plan = p.get();
    g.first = fl.first;
    g.n = fl.second - fl.first;
    g.chan0 = p->chan_off[fl.first];
    g.elem0 = p->elem_off[fl.first];
    g.method = methods[fl.first];
    for (int64_t j = fl.first; j < fl.second; ++j) {
      g.co += co[j];
      g.elems += co[j] * row[j];
      g.max_row = std::max(g.max_row, row[j]);
      p->group_of[j] = (int64_t)p->groups.size();
    }
    p->groups.push_back(std::move(g));
  }
  return g_plans.add(std::move(p));
}

// One launch quantizes every layer of the plan; returns (wq_all, aux_all, per layer: wq view with the weight's own
// strides, s, zp, mx, lwq slices of aux_all).
std::tuple<Tensor, Tensor, std::vector<std::vector<Tensor>>> plan_forward(int64_t plan_id, const std::vector<Tensor>& ws,
                                                                           const std::vector<Tensor>& lss) {
  need_lib();
  auto p = g_plans.get(plan_id);
  std::lock_guard<std::mutex> g(p->mu);
  const int64_t n = p->nlayers;
  TORCH_CHECK((int64_t)ws.size() == n && (int64_t)lss.size() == n, "plan_forward: expected ", n, " weights and log scales");
  c10::OptionalDeviceGuard device_guard;
  if (n > 0) device_guard.reset_device(ws[0].device());      // see MHAQ_ON_DEVICE_OF
  std::vector<int64_t> key;
  key.reserve(2 * n);
  for (int64_t i = 0; i < n; ++i) {
    const Tensor& w = ws[i];
    TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kFloat && w.is_non_overlapping_and_dense() &&
                    w.numel() == p->co[i] * p->row[i],
                "plan_forward: weight ", i, " must be a dense float32 device tensor of the planned size");
    TORCH_CHECK(lss[i].is_cuda() && lss[i].scalar_type() == at::kFloat && lss[i].is_contiguous() &&
                    lss[i].numel() == p->co[i],
                "plan_forward: log scale ", i, " must be a contiguous float32 device tensor of the planned size");
    key.push_back((int64_t)(uintptr_t)w.const_data_ptr());
  }
  for (int64_t i = 0; i < n; ++i) key.push_back((int64_t)(uintptr_t)lss[i].const_data_ptr());
  const Tensor& like = ws[0];
  const Tensor table = p->fwd_tables.get(key, Plan::kEagerTables, like, [&] {
    std::vector<mhaq_wlayer_desc> descs(n);
    for (int64_t i = 0; i < n; ++i)
      descs[i] = mhaq_wlayer_desc{fptr(ws[i]), fptr(lss[i]), nullptr, nullptr, p->co[i], p->row[i], p->elem_off[i],
                                  p->chan_off[i]};
    return descs;
  });
  Tensor wq_all = at::empty({p->total_elems}, like.options());
  Tensor aux_all = at::empty({4, p->total_co}, like.options());
  check(A.mhaq_fq_wlayer_fwd_multi(static_cast<const mhaq_wlayer_desc*>(table.const_data_ptr()), (int)n,
                                   p->total_co, p->max_row, fptr_mut(wq_all), fptr_mut(aux_all), cur_stream(like)),
        "mhaq_fq_wlayer_fwd_multi");
  p->cur_wq = wq_all;
  p->cur_aux = aux_all;
  std::vector<std::vector<Tensor>> per(n);
  for (int64_t i = 0; i < n; ++i) {
    // the slab holds each layer in the physical order of its weight (a channels_last weight is [Co][kh][kw][Ci] in
    // memory): give the slice the weight's own strides
    Tensor wq = at::as_strided(wq_all, ws[i].sizes(), ws[i].strides(), p->elem_off[i]);
    Tensor s_i = aux_all.select(0, 0).narrow(0, p->chan_off[i], p->co[i]);
    Tensor zp_i = aux_all.select(0, 1).narrow(0, p->chan_off[i], p->co[i]);
    std::vector<int64_t> shp(ws[i].dim(), 1);
    shp[0] = p->co[i];
    // ... and s / zp once more in the [co, 1, ..] shape the layer publishes on its Quantizer (saves two Python view calls)
    per[i] = {wq, s_i, zp_i, aux_all.select(0, 2).narrow(0, p->chan_off[i], p->co[i]),
              aux_all.select(0, 3).narrow(0, p->chan_off[i], p->co[i]), s_i.view(shp), zp_i.view(shp)};
  }
  return {wq_all, aux_all, per};
}

// The autograd node of one backward group: outputs are the group's slices of this step's model-wide forward (no launch
// here); its backward is ONE launch (plus, for AEWGS under data parallelism, one statistics launch and ONE packed
// all-reduce).
class WeightGroupFn : public torch::autograd::Function<WeightGroupFn> {
 public:
  static variable_list forward(AutogradContext* ctx, int64_t plan_id, int64_t gi, at::TensorList tensors, int64_t rank,
                               bool distributed) {
    auto p = g_plans.get(plan_id);
    std::lock_guard<std::mutex> lk(p->mu);
    const Group& grp = p->groups.at(gi);
    const int64_t n = grp.n;
    TORCH_CHECK((int64_t)tensors.size() == 2 * n, "weight group: expected ", 2 * n, " tensors");
    TORCH_CHECK(p->cur_wq.defined(), "weight group: the model-wide forward of this step has not run");
    ctx->saved_data["plan"] = plan_id;
    ctx->saved_data["group"] = gi;
    ctx->saved_data["rank"] = rank;
    ctx->saved_data["dist"] = distributed;
    ctx->saved_data["aux"] = p->cur_aux;
    std::vector<std::vector<int64_t>> ls_shapes;
    variable_list ws(tensors.begin(), tensors.begin() + n);
    for (int64_t k = 0; k < n; ++k) ls_shapes.push_back(tensors[n + k].sizes().vec());
    ctx->saved_data["ls_shapes"] = ls_shapes;
    ctx->save_for_backward(ws);
    ctx->set_materialize_grads(false);
    variable_list outs;
    outs.reserve(2 * n);
    for (int64_t k = 0; k < n; ++k) {
      const int64_t i = grp.first + k;
      outs.push_back(at::as_strided(p->cur_wq, ws[k].sizes(), ws[k].strides(), p->elem_off[i]));
    }
    for (int64_t k = 0; k < n; ++k) {
      const int64_t i = grp.first + k;
      outs.push_back(p->cur_aux.select(0, 3).narrow(0, p->chan_off[i], p->co[i]));
    }
    return outs;
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    auto p = g_plans.get(ctx->saved_data["plan"].toInt());
    std::unique_lock<std::mutex> lk(p->mu);
    Group& grp = p->groups.at(ctx->saved_data["group"].toInt());
    const int64_t n = grp.n;
    auto ws = ctx->get_saved_variables();
    const Tensor aux_all = ctx->saved_data["aux"].toTensor();
    const Tensor& like = aux_all;
    void* stream = cur_stream(like);
    std::vector<Tensor> Gs(n), gl(n);
    for (int64_t k = 0; k < n; ++k) {
      Gs[k] = grads[k].defined() ? like_layout(grads[k], ws[k]) : at::zeros_like(ws[k]);
      if (grads[n + k].defined()) gl[k] = grads[n + k].contiguous();
    }
    if (!grp.pool) grp.pool = std::make_unique<TablePool>(sizeof(mhaq_wlayer_desc) * n, like);
    std::vector<int64_t> key;
    key.reserve(3 * n);
    for (int64_t k = 0; k < n; ++k) key.push_back((int64_t)(uintptr_t)ws[k].const_data_ptr());
    for (int64_t k = 0; k < n; ++k) key.push_back((int64_t)(uintptr_t)Gs[k].const_data_ptr());
    for (int64_t k = 0; k < n; ++k) key.push_back(gl[k].defined() ? (int64_t)(uintptr_t)gl[k].const_data_ptr() : 0);
    // held by value: the plan's lock is dropped around the statistics exchange below, and the pool may move on meanwhile
    const Tensor table = grp.pool->get(key, [&](void* dst) {
      auto* d = static_cast<mhaq_wlayer_desc*>(dst);
      for (int64_t k = 0; k < n; ++k) {
        const int64_t i = grp.first + k;
        d[k] = mhaq_wlayer_desc{fptr(ws[k]), nullptr, fptr(Gs[k]), fptr_or_null(gl[k]), p->co[i], p->row[i],
                                p->elem_off[i] - grp.elem0, p->chan_off[i] - grp.chan0};
      }
    }, stream);
    const auto* descs = static_cast<const mhaq_wlayer_desc*>(table.const_data_ptr());
    const float* aux = fptr(aux_all) + grp.chan0;       // the group's first channel in row 0 of [4][total_co]
    Tensor stats;
    if (grp.method == MHAQ_FQ_AEWGS && ctx->saved_data["dist"].toBool()) {
      stats = at::empty({3, grp.co}, like.options());
      check(A.mhaq_fq_wlayer_aewgs_stats_group(descs, (int)n, grp.co, aux, p->total_co, fptr_mut(stats), stream),
            "mhaq_fq_wlayer_aewgs_stats_group");
      // The exchange calls into Python (it takes the GIL on this autograd thread).  The plan_* entry points take this
      // plan's mutex WITH the GIL held: holding the mutex across the callback would invert that order and deadlock
      // against a Python thread that reads the plan's state during a distributed AEWGS backward.
      lk.unlock();
      allreduce_avg(stats);          // gdnsq.py:126-129, one message for the whole group
      lk.lock();
    }
    Tensor gw = at::empty({grp.elems}, like.options());
    Tensor gls = at::empty({grp.co}, like.options());
    const Draw d = draw_signs(false, grp.method, ctx->saved_data["rank"].toInt(), like);
    check(A.mhaq_fq_wlayer_bwd_group(descs, (int)n, grp.co, grp.max_row, aux, p->total_co, fptr_mut(gw), fptr_mut(gls),
                                     (int)grp.method, fptr_or_null(stats), d.seed, d.offset, d.offset_dev, stream),
          "mhaq_fq_wlayer_bwd_group");
    const auto ls_shapes = ctx->saved_data["ls_shapes"].to<std::vector<std::vector<int64_t>>>();
    variable_list out(2 + 2 * n + 2);
    for (int64_t k = 0; k < n; ++k) {
      const int64_t i = grp.first + k;
      out[2 + k] = at::as_strided(gw, ws[k].sizes(), ws[k].strides(), p->elem_off[i] - grp.elem0);
      out[2 + n + k] = gls.narrow(0, p->chan_off[i] - grp.chan0, p->co[i]).view(ls_shapes[k]);
    }
    return out;
  }
};

// (wq_k, lwq_k) for every layer k of group `gi`, as outputs of the group's autograd node
variable_list plan_group_apply(int64_t plan_id, int64_t gi, variable_list ws, variable_list lss, int64_t rank) {
  need_lib();
  c10::OptionalDeviceGuard device_guard;
  if (!ws.empty()) device_guard.reset_device(ws[0].device());      // see MHAQ_ON_DEVICE_OF
  variable_list all;
  all.reserve(ws.size() + lss.size());
  for (auto& t : ws) all.push_back(t);
  for (auto& t : lss) all.push_back(t);
  return WeightGroupFn::apply(plan_id, gi, at::TensorList(all), rank, g_dist_active.load());
}

// ------------------------------------------------------------------------------------------------ PotentialLoss
// gdnsq_loss.py:47-71 / 129-153 in one launch per direction.  Returns (ploss, stats[12]).
class PotentialLossFn : public torch::autograd::Function<PotentialLossFn> {
 public:
  static variable_list forward(AutogradContext* ctx, const Tensor& base_in, const Tensor& las_in, const Tensor& laq_in,
                               const Tensor& lws_in, const Tensor& lwq_in, const Tensor& state, double a_bits,
                               double w_bits, double p, bool lossless, bool update_state) {
    ctx->saved_data["shapes"] = std::vector<std::vector<int64_t>>{base_in.sizes().vec(), las_in.sizes().vec(),
                                                                  laq_in.sizes().vec(), lws_in.sizes().vec(),
                                                                  lwq_in.sizes().vec()};
    Tensor base = base_in.reshape({1}).contiguous();
    Tensor las = las_in.reshape({-1}).contiguous(), laq = laq_in.reshape({-1}).contiguous();
    Tensor lws = lws_in.reshape({-1}).contiguous(), lwq = lwq_in.reshape({-1}).contiguous();
    TORCH_CHECK(las.numel() == laq.numel() && lws.numel() == lwq.numel(),
                "potential_loss: scale and range vectors must pair up");
    Tensor out = at::empty({12}, base.options());
    check(A.mhaq_fq_potential_loss_fwd(fptr(base), fptr(las), fptr(laq), las.numel(), fptr(lws), fptr(lwq), lws.numel(),
                                       (float)a_bits, (float)w_bits, (float)p, lossless ? 1 : 0, fptr_mut(state),
                                       update_state ? 1 : 0, fptr_mut(out), cur_stream(base)),
          "mhaq_fq_potential_loss_fwd");
    ctx->save_for_backward({out, las, laq, lws, lwq});
    ctx->saved_data["a"] = a_bits;
    ctx->saved_data["w"] = w_bits;
    ctx->saved_data["p"] = p;
    ctx->mark_non_differentiable({out});
    return {out.select(0, 0).clone(), out};
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    auto saved = ctx->get_saved_variables();
    const Tensor &out = saved[0], &las = saved[1], &laq = saved[2], &lws = saved[3], &lwq = saved[4];
    Tensor g = grads[0].reshape({1}).contiguous();
    const int64_t na = las.numel(), nw = lws.numel();
    Tensor slab = at::empty({1 + 2 * na + 2 * nw}, out.options());
    Tensor g_base = slab.narrow(0, 0, 1), g_las = slab.narrow(0, 1, na), g_laq = slab.narrow(0, 1 + na, na),
           g_lws = slab.narrow(0, 1 + 2 * na, nw), g_lwq = slab.narrow(0, 1 + 2 * na + nw, nw);
    check(A.mhaq_fq_potential_loss_bwd(fptr(g), fptr(out), fptr(las), fptr(laq), na, fptr(lws), fptr(lwq), nw,
                                       (float)ctx->saved_data["a"].toDouble(), (float)ctx->saved_data["w"].toDouble(),
                                       (float)ctx->saved_data["p"].toDouble(), fptr_mut(g_base), fptr_mut(g_las),
                                       fptr_mut(g_laq), fptr_mut(g_lws), fptr_mut(g_lwq), cur_stream(out)),
          "mhaq_fq_potential_loss_bwd");
    const auto shapes = ctx->saved_data["shapes"].to<std::vector<std::vector<int64_t>>>();
    variable_list res(11);
    res[0] = g_base.reshape(shapes[0]);
    res[1] = g_las.reshape(shapes[1]);
    res[2] = g_laq.reshape(shapes[2]);
    res[3] = g_lws.reshape(shapes[3]);
    res[4] = g_lwq.reshape(shapes[4]);
    return res;
  }
};

std::pair<Tensor, Tensor> potential_loss(const Tensor& base, const Tensor& las, const Tensor& laq, const Tensor& lws,
                                         const Tensor& lwq, const Tensor& state, double a_bits, double w_bits, double p,
                                         bool lossless, bool update_state) {
  need_lib();
  MHAQ_ON_DEVICE_OF(base);
  for (const Tensor* t : {&base, &las, &laq, &lws, &lwq})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat, "potential_loss: inputs must be float32 device tensors");
  TORCH_CHECK(state.is_cuda() && state.scalar_type() == at::kFloat && state.numel() == 3 && state.is_contiguous(),
              "potential_loss: state must be a contiguous float32 device tensor {loss_sum, cnt, t}");
  auto out = PotentialLossFn::apply(base, las, laq, lws, lwq, state, a_bits, w_bits, p, lossless, update_state);
  return {out[0], out[1]};
}

// ------------------------------------------------------------------------------------------------ one-pass RAdam
// The optimizer step of mhaq_amd/optim.py (FusedRAdam) as ONE launch of mhaq_fq_radam_step.  The descriptor table changes
// every step -- c1 / c2 follow the step count, and the gradients are new tensors after zero_grad(set_to_none=True) --, so it
// comes from a TablePool: pinned staging, hipMemcpyAsync on the current stream, a ring of entries behind events.  The work
// list depends on the tensors' sizes alone: a TableCache uploads it once.  No host synchronisation (an entry of the ring is
// waited for only when the stream is 8 steps behind the host).
struct RadamTables {
  std::mutex mu;
  std::map<std::pair<int, int64_t>, std::unique_ptr<TablePool>> descs;   // (device, capacity in descriptors)
  std::map<int, TableCache> work;                                        // per device
  static constexpr size_t kWorkLists = 4;
  static constexpr int64_t kDescGrain = 64;
};
RadamTables& g_radam = *new RadamTables();     // never destroyed: it holds device tensors and HIP events
std::atomic<int64_t> g_fused_radam_steps{0};   // launches of mhaq_fq_radam_step so far

// equal strides once the dimensions of size 1 are dropped: the same element order in memory
bool same_memory_order(const Tensor& a, const Tensor& b) {
  if (a.sizes() != b.sizes()) return false;
  for (int64_t d = 0; d < a.dim(); ++d)
    if (a.size(d) != 1 && a.stride(d) != b.stride(d)) return false;
  return true;
}

void radam_step(const std::vector<Tensor>& params, const std::vector<Tensor>& grads, const std::vector<Tensor>& exp_avgs,
                const std::vector<Tensor>& exp_avg_sqs, const std::vector<double>& c1s, const std::vector<double>& c2s,
                double beta1, double beta2, double eps) {
  need_lib();
  const size_t n = params.size();
  TORCH_CHECK(grads.size() == n && exp_avgs.size() == n && exp_avg_sqs.size() == n && c1s.size() == n && c2s.size() == n,
              "radam_step: the six lists must have one length");
  if (n == 0) return;
  TORCH_CHECK(!capturing(), "radam_step: a captured launch would freeze the step-dependent scalars; step eagerly");
  const Tensor& like = params[0];
  TORCH_CHECK(like.is_cuda(), "radam_step: device tensors are required (there is no CPU path)");
  for (size_t i = 0; i < n; ++i) {
    const Tensor& p = params[i];
    for (const Tensor* t : {&p, &grads[i], &exp_avgs[i], &exp_avg_sqs[i]})
      TORCH_CHECK(t->defined() && t->device() == like.device() && t->scalar_type() == at::kFloat &&
                      t->is_non_overlapping_and_dense() && same_memory_order(*t, p),
                  "radam_step: tensor ", i, ": p, grad, exp_avg and exp_avg_sq must be dense float32 tensors on one device "
                  "in the same memory order");
  }
  MHAQ_ON_DEVICE_OF(like);
  void* st = cur_stream(like);
  const int dev = (int)like.device().index();
  const int64_t chunk = A.mhaq_fq_radam_chunk_elements();
  std::vector<mhaq_radam_desc> descs(n);
  std::vector<int64_t> key, sizes;
  key.reserve(6 * n);
  sizes.reserve(n);
  int64_t nwork = 0;
  for (size_t i = 0; i < n; ++i) {
    mhaq_radam_desc& d = descs[i];
    d.p = fptr_mut(params[i]);
    d.g = fptr(grads[i]);
    d.m = fptr_mut(exp_avgs[i]);
    d.v = fptr_mut(exp_avg_sqs[i]);
    d.n = params[i].numel();
    d.c1 = (float)c1s[i];
    d.c2 = (float)c2s[i];
    int64_t scalars;
    static_assert(sizeof(scalars) == 2 * sizeof(float), "two floats per key word");
    std::memcpy(&scalars, &d.c1, sizeof(scalars));
    for (int64_t w : {(int64_t)(uintptr_t)d.p, (int64_t)(uintptr_t)d.g, (int64_t)(uintptr_t)d.m, (int64_t)(uintptr_t)d.v,
                      d.n, scalars})
      key.push_back(w);
    sizes.push_back(d.n);
    nwork += (d.n + chunk - 1) / chunk;
  }
  if (nwork == 0) return;
  std::lock_guard<std::mutex> guard(g_radam.mu);
  const int64_t cap = ((int64_t)n + RadamTables::kDescGrain - 1) / RadamTables::kDescGrain * RadamTables::kDescGrain;
  auto& pool = g_radam.descs[{dev, cap}];
  if (!pool) pool = std::make_unique<TablePool>(sizeof(mhaq_radam_desc) * (size_t)cap, like);
  const Tensor& dtab = pool->get(key, [&](void* host) {
    std::memset(host, 0, sizeof(mhaq_radam_desc) * (size_t)cap);
    std::memcpy(host, descs.data(), sizeof(mhaq_radam_desc) * n);
  }, st);
  const Tensor wtab = g_radam.work[dev].get(sizes, RadamTables::kWorkLists, like, [&]() {
    std::vector<mhaq_radam_work> w;
    w.reserve((size_t)nwork);
    for (size_t i = 0; i < n; ++i)
      for (int64_t c = 0; c * chunk < sizes[i]; ++c) w.push_back({(int32_t)i, (int32_t)c});
    return w;
  });
  check(A.mhaq_fq_radam_step(static_cast<const mhaq_radam_desc*>(dtab.const_data_ptr()), (int)n,
                             static_cast<const mhaq_radam_work*>(wtab.const_data_ptr()), nwork, (float)(1.0 - beta1),
                             (float)beta2, (float)(1.0 - beta2), (float)eps, st),
        "mhaq_fq_radam_step");
  g_fused_radam_steps.fetch_add(1, std::memory_order_relaxed);
}

// ------------------------------------------------------------------------------------------------ distillation loss
// One of the six softmax-family distillation losses (mhaq_amd/loss.py: FusedDistillLoss) over the student's and the teacher's
// logits: mhaq_fq_distill_loss_fwd -- two launches -- forward, mhaq_fq_distill_loss_bwd -- one -- backward.  The workspace and
// gunit (d loss / d x for an upstream gradient of 1) come from the caching allocator; gunit only where x takes a gradient.
std::atomic<int64_t> g_distill_fused_launches{0};   // kernel launches of the two entry points so far: 2 forward, 1 backward

inline int distill_dtype(const Tensor& x) { return x.scalar_type() == at::kFloat ? MHAQ_FQ_DT_F32 : act_dtype(x); }

class DistillLossFn : public torch::autograd::Function<DistillLossFn> {
 public:
  static Tensor forward(AutogradContext* ctx, const Tensor& x, const Tensor& t, int64_t kind, bool need_grad) {
    const int64_t rows = x.size(0), cols = x.size(1);
    Tensor loss = at::empty({}, x.options().dtype(at::kFloat));
    Tensor ws = at::empty({(int64_t)A.mhaq_fq_distill_loss_workspace_bytes(rows)}, x.options().dtype(at::kByte));
    Tensor gunit;
    if (need_grad) gunit = at::empty({rows, cols}, x.options().dtype(at::kFloat));
    check(A.mhaq_fq_distill_loss_fwd(x.const_data_ptr(), distill_dtype(x), t.const_data_ptr(), distill_dtype(t), rows, cols,
                                     (int)kind, fptr_mut(loss), need_grad ? fptr_mut(gunit) : nullptr, ws.mutable_data_ptr(),
                                     (size_t)ws.numel(), cur_stream(x)),
          "mhaq_fq_distill_loss_fwd");
    g_distill_fused_launches.fetch_add(2, std::memory_order_relaxed);
    if (need_grad) ctx->save_for_backward({gunit});
    ctx->saved_data["dtype"] = (int64_t)distill_dtype(x);
    return loss;
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    auto saved = ctx->get_saved_variables();
    TORCH_CHECK(!saved.empty(), "distill_loss: the forward ran without a gradient to keep");
    const Tensor& gunit = saved[0];
    Tensor g = grads[0].reshape({1}).to(at::kFloat).contiguous();
    const int dt = (int)ctx->saved_data["dtype"].toInt();
    Tensor gx = at::empty(gunit.sizes(), gunit.options().dtype(dt == MHAQ_FQ_DT_F32    ? at::kFloat
                                                               : dt == MHAQ_FQ_DT_BF16 ? at::kBFloat16
                                                                                       : at::kHalf));
    check(A.mhaq_fq_distill_loss_bwd(fptr(gunit), fptr(g), gx.mutable_data_ptr(), dt, gunit.numel(), cur_stream(gunit)),
          "mhaq_fq_distill_loss_bwd");
    g_distill_fused_launches.fetch_add(1, std::memory_order_relaxed);
    return {gx, Tensor(), Tensor(), Tensor()};
  }
};

Tensor distill_loss(const Tensor& x, const Tensor& t, int64_t kind) {
  need_lib();
  if (!x.is_cuda() || !t.is_cuda()) throw MhaqError("distill_loss: device tensors are required (there is no CPU path)");
  MHAQ_ON_DEVICE_OF(x);
  for (const Tensor* p : {&x, &t})
    TORCH_CHECK(p->dim() == 2 && p->is_contiguous() && p->device() == x.device() &&
                    (p->scalar_type() == at::kFloat || act_dtype(*p) != 0),
                "distill_loss: input and target must be contiguous [rows, cols] float32, bfloat16 or float16 tensors on one device");
  TORCH_CHECK(x.sizes() == t.sizes() && x.numel() > 0, "distill_loss: input and target must have one non-empty shape");
  TORCH_CHECK(!(t.requires_grad() && at::GradMode::is_enabled()),
              "distill_loss: the target (the teacher's logits) takes no gradient; detach it");
  return DistillLossFn::apply(x, t, kind, x.requires_grad() && at::GradMode::is_enabled());
}

// ------------------------------------------------------------------------------------------------ classification head
// The hard-label cross-entropy of a training step (mhaq_amd/loss.py: FusedCrossEntropy): mhaq_fq_cls_head_fwd -- two launches
// -- forward, mhaq_fq_distill_loss_bwd -- one -- backward.  Returns {loss, flags}: the flag word (bit 2 = a label out of
// range) stays on the device for whoever wants to read it; gunit is allocated only where x takes a gradient.
std::atomic<int64_t> g_cls_head_launches{0};   // kernel launches of this node so far: 2 forward, 1 backward

class ClsHeadFn : public torch::autograd::Function<ClsHeadFn> {
 public:
  static variable_list forward(AutogradContext* ctx, const Tensor& x, const Tensor& target, int64_t ignore_index,
                               bool need_grad) {
    const int64_t rows = x.size(0), cols = x.size(1);
    Tensor loss = at::empty({}, x.options().dtype(at::kFloat));
    Tensor flags = at::empty({1}, x.options().dtype(at::kInt));
    Tensor aux = at::empty({4}, x.options().dtype(at::kLong));        // counts [3], then acc [2] in the fourth word
    Tensor ws = at::empty({(int64_t)A.mhaq_fq_cls_head_workspace_bytes(rows)}, x.options().dtype(at::kByte));
    Tensor gunit;
    if (need_grad) gunit = at::empty({rows, cols}, x.options().dtype(at::kFloat));
    int64_t* counts = static_cast<int64_t*>(aux.mutable_data_ptr());
    check(A.mhaq_fq_cls_head_fwd(x.const_data_ptr(), distill_dtype(x), static_cast<const int64_t*>(target.const_data_ptr()),
                                 rows, cols, ignore_index, 1, fptr_mut(loss), reinterpret_cast<float*>(counts + 3), counts,
                                 nullptr, nullptr, need_grad ? fptr_mut(gunit) : nullptr,
                                 static_cast<uint32_t*>(flags.mutable_data_ptr()), ws.mutable_data_ptr(), (size_t)ws.numel(),
                                 cur_stream(x)),
          "mhaq_fq_cls_head_fwd");
    g_cls_head_launches.fetch_add(2, std::memory_order_relaxed);
    if (need_grad) ctx->save_for_backward({gunit});
    ctx->saved_data["dtype"] = (int64_t)distill_dtype(x);
    ctx->mark_non_differentiable({flags});
    return {loss, flags};
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    auto saved = ctx->get_saved_variables();
    TORCH_CHECK(!saved.empty(), "cls_head_loss: the forward ran without a gradient to keep");
    const Tensor& gunit = saved[0];
    Tensor g = grads[0].reshape({1}).to(at::kFloat).contiguous();
    const int dt = (int)ctx->saved_data["dtype"].toInt();
    Tensor gx = at::empty(gunit.sizes(), gunit.options().dtype(dt == MHAQ_FQ_DT_F32    ? at::kFloat
                                                               : dt == MHAQ_FQ_DT_BF16 ? at::kBFloat16
                                                                                       : at::kHalf));
    check(A.mhaq_fq_distill_loss_bwd(fptr(gunit), fptr(g), gx.mutable_data_ptr(), dt, gunit.numel(), cur_stream(gunit)),
          "mhaq_fq_distill_loss_bwd");
    g_cls_head_launches.fetch_add(1, std::memory_order_relaxed);
    return {gx, Tensor(), Tensor(), Tensor()};
  }
};

std::vector<Tensor> cls_head_loss(const Tensor& x, const Tensor& target, int64_t ignore_index) {
  need_lib();
  if (!x.is_cuda() || !target.is_cuda()) throw MhaqError("cls_head_loss: device tensors are required (there is no CPU path)");
  MHAQ_ON_DEVICE_OF(x);
  TORCH_CHECK(x.dim() == 2 && x.is_contiguous() && x.numel() > 0 && (x.scalar_type() == at::kFloat || act_dtype(x) != 0),
              "cls_head_loss: the logits must be a non-empty contiguous [rows, cols] float32, bfloat16 or float16 tensor");
  TORCH_CHECK(target.dim() == 1 && target.is_contiguous() && target.scalar_type() == at::kLong &&
                  target.size(0) == x.size(0) && target.device() == x.device(),
              "cls_head_loss: the target must be a contiguous int64 [rows] tensor on the logits' device");
  return ClsHeadFn::apply(x, target, ignore_index, x.requires_grad() && at::GradMode::is_enabled());
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "compiled autograd binding of the mhaq_amd fused layer ops over the C ABI of include/mhaq_fq.h";
  // the torch this extension was COMPILED against (torch/version.h): mhaq_amd/_ext.py compares it with the running torch
  // before anything is bound -- the only check a stampless prebuilt extension can still be given
  m.attr("TORCH_VERSION") = TORCH_VERSION;
  static PyObject* err_class = nullptr;   // mhaq_amd._lib.MhaqFqError, installed by bind(); never released (see above)
  py::register_exception_translator([](std::exception_ptr p) {
    try {
      if (p) std::rethrow_exception(p);
    } catch (const MhaqError& e) {
      PyErr_SetString(err_class ? err_class : PyExc_RuntimeError, e.what());
    }
  });
  m.def("bind", [](const std::string& path, py::object error_class) {
    if (!err_class) err_class = error_class.inc_ref().ptr();
    bind_library(path);
  }, "dlopen the C-ABI library and resolve the entry points the nodes call");
  m.def("host_timers", [](bool reset) {
    py::dict d;
    for (int i = 0; i < T_N; ++i) {
      const int64_t n = g_tcnt[i].load(), ns = g_tns[i].load();
      d[kTimerNames[i]] = py::make_tuple(n, n ? (double)ns / (double)n * 1e-3 : 0.0);     // (calls, mean us)
      if (reset) { g_tcnt[i].store(0); g_tns[i].store(0); }
    }
    return d;
  }, py::arg("reset") = true);
  m.def("bound_library", []() { return A.path; });

  // sign streams
  m.def("rng_manual_seed", [](uint64_t seed) { std::lock_guard<std::mutex> g(R.mu); R.seed = seed; R.seeded = true; R.count = 0; });
  m.def("rng_seed", []() -> py::object { std::lock_guard<std::mutex> g(R.mu); return R.seeded ? py::object(py::int_(R.seed)) : py::none(); });
  m.def("rng_next", [](int64_t rank) {
    std::lock_guard<std::mutex> g(R.mu);
    if (!R.seeded) throw MhaqError("sign stream used before it was seeded");
    return std::make_pair(R.seed ^ ((uint64_t)rank * kGolden), ++R.count);
  });
  m.def("rng_drawn", []() { std::lock_guard<std::mutex> g(R.mu); return R.count; });
  m.def("rng_set_drawn", [](uint64_t n) { std::lock_guard<std::mutex> g(R.mu); R.count = n; });
  m.def("rng_set_base", [](const std::optional<Tensor>& base) {
    std::lock_guard<std::mutex> g(R.mu);
    R.base = (base.has_value() && base->defined()) ? *base : Tensor();
  });
  m.def("rng_base", []() -> std::optional<Tensor> {
    std::lock_guard<std::mutex> g(R.mu);
    return R.base.defined() ? std::optional<Tensor>(R.base) : std::nullopt;
  });

  // data-parallel hooks
  m.def("set_allreduce_avg", [](py::object fn) {
    g_allreduce_avg = fn.is_none() ? nullptr : fn.inc_ref().ptr();
  });
  m.def("set_dist_active", [](bool v) { g_dist_active.store(v); });

  // activation hub and the activation nodes
  m.def("hub_create", &hub_create);
  m.def("hub_destroy", [](int64_t id) { g_hubs.erase(id); });
  m.def("hub_begin", &hub_begin);
  m.def("hub_clear_pending", [](int64_t id) { auto h = g_hubs.get(id); std::lock_guard<std::mutex> g(h->mu); h->pending.clear(); });
  m.def("hub_release_captured", [](int64_t id) { g_hubs.get(id)->release_captured(); });
  m.def("hub_state", [](int64_t id) {
    auto h = g_hubs.get(id);
    std::lock_guard<std::mutex> g(h->mu);
    py::dict d;
    d["tables"] = h->tables.entries.size();
    d["captured_tables"] = h->tables.captured();
    d["retired"] = h->retired.size();
    d["pending"] = h->pending.size();
    d["has_table"] = h->last_table.defined();
    int64_t bytes = 0;
    for (auto& w : h->ws) if (w.defined()) bytes += w.numel();
    for (auto& w : h->retired) bytes += w.numel();
    d["workspace_bytes"] = bytes;
    return d;
  });
  m.def("act_layer", &act_layer, py::arg("x"), py::arg("log_act_s"), py::arg("log_act_q"), py::arg("act_b"),
        py::arg("method"), py::arg("r_sign") = py::none(), py::arg("hub") = 0, py::arg("slot") = 0, py::arg("rank") = 0);
  m.def("act_relu_layer", &act_relu_layer, py::arg("z"), py::arg("addend"), py::arg("log_act_s"), py::arg("log_act_q"),
        py::arg("act_b"), py::arg("method"), py::arg("want_act"), py::arg("hub") = 0, py::arg("slot") = 0,
        py::arg("rank") = 0);

  // training BatchNorm: the framework's forward (mhaq_fq_bn_fwd with hip_forward, where eligible), the HIP backward
  m.def("bn_train", &bn_train, py::arg("x"), py::arg("weight"), py::arg("bias"), py::arg("running_mean"),
        py::arg("running_var"), py::arg("momentum"), py::arg("eps"), py::arg("cudnn_enabled") = true,
        py::arg("x16") = false, py::arg("hip_forward") = false, py::arg("hip_forward_x16") = false);
  m.def("bn_hip_forwards", []() { return g_bn_hip_forwards.load(); },
        "number of BatchNorm forwards so far (bn_train and bn_pool_train) that ran mhaq_fq_bn_fwd instead of the framework's");
  m.def("bn_hip_forwards_x16", []() { return g_bn_hip_forwards_x16.load(); },
        "number of BatchNorm forwards so far (bn_train) that ran the 16-bit HIP kernels (mhaq_fq_bn_fwd_x16)");

  m.def("bn_hip_backwards", []() { return g_bn_hip_backwards.load(); },
        "number of BatchNorm backwards so far that ran the fp32 HIP kernels instead of the framework's backward");
  m.def("bn_hip_backwards_x16", []() { return g_bn_hip_backwards_x16.load(); },
        "number of BatchNorm backwards so far that ran the 16-bit HIP kernels (mhaq_fq_bn_bwd_x16)");
  // ... with the stem's 3x3 / stride 2 max pool in the same node
  m.def("bn_pool_train", &bn_pool_train, py::arg("x"), py::arg("weight"), py::arg("bias"), py::arg("running_mean"),
        py::arg("running_var"), py::arg("momentum"), py::arg("eps"), py::arg("cudnn_enabled") = true,
        py::arg("hip_forward") = false, py::arg("x16") = false, py::arg("pool_x16") = false,
        py::arg("hip_forward_x16") = false);
  m.def("bn_pool_hip_backwards", []() { return g_bn_pool_hip_backwards.load(); },
        "number of BatchNorm + pool backwards so far that ran mhaq_fq_bn_pool_bwd (the fallback is the two separate nodes)");
  m.def("bn_pool_hip_forwards_x16", []() { return g_bn_pool_hip_forwards_x16.load(); },
        "number of 16-bit BatchNorm + pool forwards so far that ran mhaq_fq_bn_fwd_x16 (statistics) and mhaq_fq_bn_norm_pool3s2_fwd_x16");
  m.def("bn_pool_hip_backwards_x16", []() { return g_bn_pool_hip_backwards_x16.load(); },
        "number of 16-bit BatchNorm + pool backwards so far that ran mhaq_fq_bn_pool_bwd_x16");

  // the frozen teacher's eval-mode BatchNorm with its ReLU, residual add and stem pool (no autograd)
  m.def("bn_infer_consts", &bn_infer_consts, py::arg("running_mean"), py::arg("running_var"), py::arg("weight"),
        py::arg("bias"), py::arg("eps"), py::arg("consts"));
  m.def("bn_infer_act", &bn_infer_act, py::arg("x"), py::arg("consts"), py::arg("mode"), py::arg("x2") = py::none(),
        py::arg("consts2") = py::none(), py::arg("residual") = py::none(), py::arg("x16") = false);
  m.def("bn_relu_pool", &bn_relu_pool, py::arg("x"), py::arg("consts"), py::arg("x16") = false);
  m.def("teacher_fused_calls", []() { return g_teacher_fused_calls.load(); },
        "number of fused launches so far on a frozen network's elementwise chain (bn_infer_act and bn_relu_pool), 16-bit included");
  m.def("teacher_fused_x16_calls", []() { return g_teacher_fused_x16_calls.load(); },
        "number of those launches that took the 16-bit entry points (mhaq_fq_bn_infer_act_x16, mhaq_fq_bn_relu_pool3s2_x16)");

  // weight layers
  m.def("weight_layer", &weight_layer, py::arg("w"), py::arg("log_wght_s"), py::arg("method"),
        py::arg("r_sign") = py::none(), py::arg("zp_grad") = false, py::arg("pre") = py::none(), py::arg("rank") = 0);
  m.def("weight_layer_pt", &weight_layer_pt, py::arg("w"), py::arg("log_wght_s"), py::arg("method"),
        py::arg("r_sign") = py::none(), py::arg("rank") = 0);
  m.def("weight_layer_ptl", &weight_layer_ptl, py::arg("w"), py::arg("log_wght_s"), py::arg("method"),
        py::arg("r_sign") = py::none(), py::arg("rank") = 0);

  // weight plan / groups
  m.def("plan_create", &plan_create);
  m.def("plan_destroy", [](int64_t id) { g_plans.erase(id); });
  m.def("plan_forward", &plan_forward);
  m.def("plan_group_apply", &plan_group_apply);
  m.def("plan_release_captured", [](int64_t id) {
    auto p = g_plans.get(id);
    std::lock_guard<std::mutex> g(p->mu);
    for (auto& grp : p->groups) if (grp.pool) grp.pool->release_captured();
    p->fwd_tables.release_captured();
  });
  m.def("plan_state", [](int64_t id) {
    auto p = g_plans.get(id);
    std::lock_guard<std::mutex> g(p->mu);
    py::dict d;
    d["fwd_tables"] = p->fwd_tables.entries.size();
    py::list pools;
    for (auto& grp : p->groups) {
      py::dict e;
      size_t used = 0, held = 0, size = 0;
      if (grp.pool) {
        size = grp.pool->keys.size();
        for (size_t i = 0; i < size; ++i) { used += grp.pool->used[i]; held += grp.pool->held[i]; }
      }
      e["size"] = size; e["used"] = used; e["held"] = held;
      pools.append(e);
    }
    d["pools"] = pools;
    return d;
  });

  m.def("potential_loss", &potential_loss);
  m.def("radam_step", &radam_step, py::arg("params"), py::arg("grads"), py::arg("exp_avgs"), py::arg("exp_avg_sqs"),
        py::arg("c1s"), py::arg("c2s"), py::arg("beta1"), py::arg("beta2"), py::arg("eps"),
        "one launch of mhaq_fq_radam_step over the listed tensors (mhaq_amd/optim.py)");
  m.def("distill_loss", &distill_loss, py::arg("input"), py::arg("target"), py::arg("kind"));
  m.def("distill_fused_launches", []() { return g_distill_fused_launches.load(); },
        "kernel launches of mhaq_fq_distill_loss_fwd (2) / _bwd (1) so far in this process");
  m.def("cls_head_loss", &cls_head_loss, py::arg("input"), py::arg("target"), py::arg("ignore_index"));
  m.def("cls_head_launches", []() { return g_cls_head_launches.load(); },
        "kernel launches of the compiled classification-head node so far in this process: mhaq_fq_cls_head_fwd (2), backward (1)");
  m.def("fused_radam_steps",[]() { return g_fused_radam_steps.load(); },
        "launches of mhaq_fq_radam_step so far (tests: the optimizer step took the HIP kernel)");
}
