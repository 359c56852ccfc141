// Object-detection validation (mhaq_fq_od_keys / mhaq_fq_od_nms / mhaq_fq_od_match, include/mhaq_fq.h): the YOLO head's
// non-maximum suppression and COCO's greedy matching of its output against the ground truth, where the framework loops over
// the images on the host (boolean indexing, nonzero, argsort, an NMS call: several synchronisations per image).
//
//   keys   one thread per (image, class, anchor): the score row is read once, coalesced along the anchors, and every pair
//          leaves a 64-bit key whose VALUE carries the order (descending score, then anchor, then class); a pair that is no
//          candidate leaves INT64_MAX.  The caller sorts each image's row ascending.
//   nms    one workgroup of kOdChunk threads per image.  The number of candidates is the position of the first INT64_MAX
//          (binary search); candidates are consumed kOdChunk at a time, thread t gathering candidate s + t through its key.
//          A candidate is first tested against the boxes kept from earlier chunks (LDS, broadcast reads); the chunk is then
//          resolved greedily: the lowest candidate still alive is kept (it is appended to the list in LDS and writes its own
//          output row), every later one tests itself against it, and so on until none is alive.  A box is only ever
//          tested against KEPT boxes -- the work is (kept boxes) x (candidates walked), never candidates squared, and a
//          box that a suppressed box would have suppressed survives, as the serial definition demands.  The walk ends when
//          max_det boxes are kept: whether a candidate is kept depends on earlier candidates only, so the exit is exact.
//   match  one workgroup of ten wavefronts per image, wavefront k = IoU threshold T_k, lanes over the image's ground truth;
//          per detection one arg-max reduction over the lanes.
// No atomics: every word has one writer.  The same inputs give the same bits at every call.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/mhaq_fq.h"
#include "fq_common.hpp"
#include "fq_io16.hpp"

namespace mhaq {

constexpr int kOdChunk = kBlock;          // candidates per sweep of the NMS workgroup (mhaq_fq_od_nms_chunk)
constexpr int kOdMaxDet = 1024;           // kept boxes held in LDS: 20 KiB
constexpr int kOdThr = 10;                // COCO's IoU thresholds
constexpr int kOdMatchBlock = kOdThr * kWave;
constexpr int64_t kOdNoKey = 0x7fffffffffffffffLL;

template <int DT>
__device__ __forceinline__ float od_ld(const void* p, int64_t i) {
  if constexpr (DT == MHAQ_FQ_DT_F32) return ldg(static_cast<const float*>(p) + i);
  else return io16::up1<DT>(*gptr(static_cast<const uint16_t*>(p) + i));
}

// min / max of the contract: a comparison and a select, so that a NaN (which compares false) has one defined outcome.
// `a` is the kept box's (the detection's) value, `b` the candidate's (the ground truth's).
__device__ __forceinline__ float od_min(float a, float b) { return b < a ? b : a; }
__device__ __forceinline__ float od_max(float a, float b) { return a < b ? b : a; }

typedef float od_f4 __attribute__((ext_vector_type(4)));      // x1, y1, x2, y2

__device__ __forceinline__ float od_iou(od_f4 a, float area_a, od_f4 b, float area_b) {
  const float iw = od_max(0.f, od_min(a.z, b.z) - od_max(a.x, b.x));
  const float ih = od_max(0.f, od_min(a.w, b.w) - od_max(a.y, b.y));
  const float inter = iw * ih;
  return inter / ((area_a + area_b) - inter);                 // 0 / 0 = NaN: compares false everywhere
}
__host__ __device__ __forceinline__ bool od_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }      // false for a NaN

// ---------------------------------------------------------------- keys
template <int DT>
__global__ __launch_bounds__(kBlock) void od_keys_kernel(const void* __restrict__ pred, int A, int nc, float conf_thr,
                                                         int64_t* __restrict__ keys) {
  const int a = (int)(blockIdx.x * kBlock + threadIdx.x), c = (int)blockIdx.y;
  if (a >= A) return;
  const int64_t b = blockIdx.z;
  const float s = od_ld<DT>(pred, (b * (4 + nc) + 4 + c) * A + a);
  int64_t key = kOdNoKey;
  if (s > conf_thr)                                           // false for a NaN; conf_thr >= 0, so the bits are a positive int32
    key = (int64_t)(((uint64_t)(uint32_t)(0x7fffffff - (int32_t)__float_as_uint(s)) << 32) | (uint32_t)(a * nc + c));
  *gptr(keys + (b * nc + c) * A + a) = key;
}

// ---------------------------------------------------------------- NMS
struct OdCand {
  od_f4 box;       // un-offset x1, y1, x2, y2
  od_f4 obox;      // offset by class * max_wh, each coordinate rounded once
  float area;      // of the offset box
  float score, cls;
  bool valid;
};

template <int DT>
__device__ __forceinline__ OdCand od_gather(const void* __restrict__ img, const int64_t* __restrict__ krow, int64_t j,
                                            int64_t limit, int A, int nc, float max_wh) {
  OdCand k;
  k.valid = false;
  if (j >= limit) return k;
  const int64_t key = *gptr(krow + j);
  const uint32_t idx = (uint32_t)key;
  if (idx >= (uint32_t)A * (uint32_t)nc) return k;           // not a key of mhaq_fq_od_keys: skipped, no address is formed
  const int a = (int)(idx / (uint32_t)nc), c = (int)(idx - (uint32_t)a * (uint32_t)nc);
  const float cx = od_ld<DT>(img, a), cy = od_ld<DT>(img, (int64_t)A + a);
  const float w = od_ld<DT>(img, 2 * (int64_t)A + a), h = od_ld<DT>(img, 3 * (int64_t)A + a);
  const float hw = w / 2.f, hh = h / 2.f;
  k.box = od_f4{cx - hw, cy - hh, cx + hw, cy + hh};
  k.cls = (float)c;
  const float o = k.cls * max_wh;
  k.obox = od_f4{k.box.x + o, k.box.y + o, k.box.z + o, k.box.w + o};
  k.area = (k.obox.z - k.obox.x) * (k.obox.w - k.obox.y);
  k.score = __uint_as_float((uint32_t)(0x7fffffff - (int32_t)(key >> 32)));
  k.valid = true;
  return k;
}

template <int DT>
__global__ __launch_bounds__(kOdChunk) void od_nms_kernel(const void* __restrict__ pred, const int64_t* __restrict__ keys,
                                                          int A, int nc, float iou_thr, float max_wh, int max_nms,
                                                          int max_det, float* __restrict__ det, int32_t* __restrict__ count,
                                                          int32_t* __restrict__ n_cand, uint32_t* __restrict__ img_flags) {
  __shared__ od_f4 s_box[kOdMaxDet];
  __shared__ float s_area[kOdMaxDet];
  __shared__ uint64_t s_alive[kOdChunk / kWave];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x, N = (int64_t)A * nc;
  const int64_t* krow = keys + b * N;
  const void* img = static_cast<const char*>(pred) + b * (4 + nc) * (int64_t)A * (DT == MHAQ_FQ_DT_F32 ? 4 : 2);
  float* drow = det + b * max_det * 6;
  // candidates of the image = position of the first INT64_MAX of its sorted row (uniform: every thread walks the same path)
  int64_t lo = 0, hi = N;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (*gptr(krow + mid) == kOdNoKey) hi = mid; else lo = mid + 1;
  }
  const int64_t ncand = lo, limit = ncand < max_nms ? ncand : (int64_t)max_nms;
  int cnt = 0;
  bool nonfinite = false;
  OdCand nxt = od_gather<DT>(img, krow, tid, limit, A, nc, max_wh);
  for (int64_t s = 0; s < limit && cnt < max_det; s += kOdChunk) {
    const OdCand cur = nxt;
    nxt = od_gather<DT>(img, krow, s + kOdChunk + tid, limit, A, nc, max_wh);      // in flight during this chunk's sweep
    const bool bad = cur.valid && !(od_finite(cur.box.x) && od_finite(cur.box.y) && od_finite(cur.box.z) && od_finite(cur.box.w));
    bool alive = cur.valid;
    for (int i = 0; i < cnt; ++i) {                           // the boxes kept from earlier chunks
      if (__ballot(alive) == 0) break;
      if (alive && od_iou(s_box[i], s_area[i], cur.obox, cur.area) > iou_thr) alive = false;
    }
    __syncthreads();                                          // the previous chunk's last read of s_alive is behind us
    int last = kOdChunk;                                      // index in the chunk at which max_det was reached
    for (;;) {
      const uint64_t m = __ballot(alive);
      if (lane == 0) s_alive[wave] = m;
      __syncthreads();
      int first = -1;
#pragma unroll
      for (int w = kOdChunk / kWave - 1; w >= 0; --w) {
        const uint64_t v = s_alive[w];
        if (v) first = w * kWave + __builtin_ctzll(v);
      }
      if (first < 0) break;                                   // block-uniform
      if (tid == first) {                                     // kept: joins the list and writes its own output row
        s_box[cnt] = cur.obox;
        s_area[cnt] = cur.area;
        float* r = drow + (int64_t)cnt * 6;
        stg(r, cur.box.x); stg(r + 1, cur.box.y); stg(r + 2, cur.box.z); stg(r + 3, cur.box.w);
        stg(r + 4, cur.score); stg(r + 5, cur.cls);
        alive = false;
      }
      ++cnt;
      if (cnt == max_det) { last = first; break; }
      __syncthreads();                                        // the kept box is visible; s_alive may be rewritten
      if (alive && od_iou(s_box[cnt - 1], s_area[cnt - 1], cur.obox, cur.area) > iou_thr) alive = false;
    }
    nonfinite |= bad && tid <= last;                          // only what was walked: up to the box that filled the list
  }
  const int any = __syncthreads_or(nonfinite ? 1 : 0);
  for (int i = cnt * 6 + tid; i < max_det * 6; i += kOdChunk) stg(drow + i, 0.f);
  if (tid == 0) {
    *gptr(count + b) = cnt;
    *gptr(n_cand + b) = (int32_t)ncand;
    *gptr(img_flags + b) = (any ? 1u : 0u) | (ncand > max_nms ? 2u : 0u);
  }
}

__global__ __launch_bounds__(kBlock) void od_flags_kernel(const uint32_t* __restrict__ img_flags, int64_t B,
                                                          uint32_t* __restrict__ flags) {
  uint32_t f = 0;
  for (int64_t i = threadIdx.x; i < B; i += kBlock) f |= *gptr(img_flags + i);
  const int b0 = __syncthreads_or((int)(f & 1u)), b1 = __syncthreads_or((int)(f & 2u));
  if (threadIdx.x == 0) *gptr(flags) = (b0 ? 1u : 0u) | (b1 ? 2u : 0u);
}

// ---------------------------------------------------------------- COCO matching
struct OdThresholds { double t[kOdThr]; };

__global__ __launch_bounds__(kOdMatchBlock) void od_match_kernel(const float* __restrict__ det, const int32_t* __restrict__ count,
                                                                 const float* __restrict__ gt_box,
                                                                 const int64_t* __restrict__ gt_label,
                                                                 const int64_t* __restrict__ gt_off, int64_t G, int nc,
                                                                 int max_det, int32_t* __restrict__ tp,
                                                                 uint32_t* __restrict__ flags, uint8_t* __restrict__ taken,
                                                                 OdThresholds thr) {
  __shared__ uint8_t s_tp[kOdThr][kOdMaxDet];
  const int tid = (int)threadIdx.x, lane = tid & 63, k = tid >> 6;
  const int64_t b = blockIdx.x;
  int n = *gptr(count + b);
  n = n < 0 ? 0 : (n > max_det ? max_det : n);
  int64_t g0 = *gptr(gt_off + b), g1 = *gptr(gt_off + b + 1);
  g0 = g0 < 0 ? 0 : g0;
  g1 = g1 > G ? G : g1;
  const double T = thr.t[k];
  uint8_t* mine = taken + (int64_t)k * G;                     // this wavefront's marks; ground truth g belongs to one lane
  for (int64_t g = g0 + lane; g < g1; g += kWave) *gptr(mine + g) = 0;
  const float* drow = det + b * max_det * 6;
  for (int d = 0; d < n; ++d) {
    const float* r = drow + (int64_t)d * 6;
    const od_f4 db = od_f4{ldg(r), ldg(r + 1), ldg(r + 2), ldg(r + 3)};
    const float darea = (db.z - db.x) * (db.w - db.y);
    const int64_t c = (int64_t)ldg(r + 5);
    float best = 0.f;
    int64_t best_g = -1;
    for (int64_t g = g0 + lane; g < g1; g += kWave) {
      if (*gptr(gt_label + g) != c || *gptr(mine + g)) continue;
      const float* q = gt_box + g * 4;
      const od_f4 gb = od_f4{ldg(q), ldg(q + 1), ldg(q + 2), ldg(q + 3)};
      const float iou = od_iou(db, darea, gb, (gb.z - gb.x) * (gb.w - gb.y));
      if (!((double)iou >= T)) continue;                      // a NaN never matches
      if (best_g < 0 || iou >= best) { best = iou; best_g = g; }      // g ascends: a tie goes to the higher index
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float oi = __shfl_xor(best, o, 64);
      const int64_t og = __shfl_xor(best_g, o, 64);
      if (og >= 0 && (best_g < 0 || oi > best || (oi == best && og > best_g))) { best = oi; best_g = og; }
    }
    if (best_g >= 0 && ((best_g - g0) & 63) == lane) *gptr(mine + best_g) = 1;
    if (lane == 0) s_tp[k][d] = best_g >= 0 ? 1 : 0;
  }
  __syncthreads();
  for (int d = tid; d < max_det; d += kOdMatchBlock) {
    int32_t w = 0;
    if (d < n) {
#pragma unroll
      for (int j = 0; j < kOdThr; ++j) w |= (int32_t)s_tp[j][d] << j;
    }
    *gptr(tp + b * max_det + d) = w;
  }
  if (b == 0) {                                               // the one writer of the flag word: every label of the batch
    int badl = 0;
    for (int64_t g = tid; g < G; g += kOdMatchBlock) {
      const int64_t l = *gptr(gt_label + g);
      badl |= (l < 0 || l >= nc) ? 1 : 0;
    }
    if (__syncthreads_or(badl) && tid == 0) *gptr(flags) = *gptr(flags) | 4u;
  }
}

template <class F>
void od_with_dtype(int dtype, F f) {
  if (dtype == MHAQ_FQ_DT_F32) f(std::integral_constant<int, MHAQ_FQ_DT_F32>{});
  else if (dtype == MHAQ_FQ_DT_BF16) f(std::integral_constant<int, MHAQ_FQ_DT_BF16>{});
  else f(std::integral_constant<int, MHAQ_FQ_DT_F16>{});
}
inline bool od_dtype_known(int dt) { return dt == MHAQ_FQ_DT_F32 || dt == MHAQ_FQ_DT_BF16 || dt == MHAQ_FQ_DT_F16; }
inline bool od_shape_supported(int64_t B, int64_t nc, int64_t A) {
  return B <= 65535 && nc <= 65535 && A <= 0x7fffffff && A * nc <= 0x7fffffff;
}

}  // namespace mhaq

using namespace mhaq;

extern "C" {

int mhaq_fq_od_nms_chunk(void) { return kOdChunk; }

int mhaq_fq_od_keys(const void* pred, int pred_dtype, int64_t B, int64_t nc, int64_t A, float conf_thr, int64_t* keys,
                    void* stream) {
  if (!pred || !keys || !od_dtype_known(pred_dtype) || B < 1 || nc < 1 || A < 1) return MHAQ_FQ_EINVAL;
  if (!(conf_thr >= 0.f) || !od_finite(conf_thr)) return MHAQ_FQ_EINVAL;
  if (((uintptr_t)pred & (pred_dtype == MHAQ_FQ_DT_F32 ? 3 : 1)) || ((uintptr_t)keys & 7)) return MHAQ_FQ_EALIGN;
  if (!od_shape_supported(B, nc, A)) return MHAQ_FQ_EUNSUPPORTED;
  const dim3 grid((unsigned)((A + kBlock - 1) / kBlock), (unsigned)nc, (unsigned)B);
  od_with_dtype(pred_dtype, [&](auto dt) {
    MHAQ_LAUNCH(od_keys_kernel<decltype(dt)::value>, grid, dim3(kBlock), 0, (hipStream_t)stream, pred, (int)A, (int)nc,
                conf_thr, keys);
  });
  return launch_status();
}

size_t mhaq_fq_od_nms_workspace_bytes(int64_t B) { return B > 0 ? (((size_t)B * 4 + 7) & ~(size_t)7) : 0; }

int mhaq_fq_od_nms(const void* pred, int pred_dtype, const int64_t* keys, int64_t B, int64_t nc, int64_t A, float iou_thr,
                   float max_wh, int max_nms, int max_det, float* det, int32_t* count, int32_t* n_cand, uint32_t* flags,
                   void* workspace, size_t workspace_bytes, void* stream) {
  if (!pred || !keys || !det || !count || !n_cand || !flags || !workspace || !od_dtype_known(pred_dtype) || B < 1 ||
      nc < 1 || A < 1 || max_nms < 1 || max_det < 1)
    return MHAQ_FQ_EINVAL;
  if (iou_thr != iou_thr || !od_finite(max_wh)) return MHAQ_FQ_EINVAL;
  if (workspace_bytes < mhaq_fq_od_nms_workspace_bytes(B)) return MHAQ_FQ_EWORKSPACE;
  if (((uintptr_t)pred & (pred_dtype == MHAQ_FQ_DT_F32 ? 3 : 1)) || ((uintptr_t)keys & 7) || ((uintptr_t)det & 3) ||
      ((uintptr_t)count & 3) || ((uintptr_t)n_cand & 3) || ((uintptr_t)flags & 3) || ((uintptr_t)workspace & 3))
    return MHAQ_FQ_EALIGN;
  if (!od_shape_supported(B, nc, A) || max_det > kOdMaxDet) return MHAQ_FQ_EUNSUPPORTED;
  uint32_t* img_flags = static_cast<uint32_t*>(workspace);
  const hipStream_t st = (hipStream_t)stream;
  od_with_dtype(pred_dtype, [&](auto dt) {
    MHAQ_LAUNCH(od_nms_kernel<decltype(dt)::value>, dim3((unsigned)B), dim3(kOdChunk), 0, st, pred, keys, (int)A, (int)nc,
                iou_thr, max_wh, max_nms, max_det, det, count, n_cand, img_flags);
  });
  if (launch_status() != 0) return launch_status();
  MHAQ_LAUNCH(od_flags_kernel, dim3(1), dim3(kBlock), 0, st, (const uint32_t*)img_flags, B, flags);
  return launch_status();
}

size_t mhaq_fq_od_match_workspace_bytes(int64_t G) { return G > 0 ? (((size_t)G * kOdThr + 7) & ~(size_t)7) : 0; }

int mhaq_fq_od_match(const float* det, const int32_t* count, int64_t B, int max_det, int64_t nc, const float* gt_box,
                     const int64_t* gt_label, const int64_t* gt_off, int64_t G, int32_t* tp, uint32_t* flags,
                     void* workspace, size_t workspace_bytes, void* stream) {
  if (!det || !count || !gt_off || !tp || !flags || B < 1 || max_det < 1 || nc < 1 || G < 0) return MHAQ_FQ_EINVAL;
  if (G > 0 && (!gt_box || !gt_label || !workspace)) return MHAQ_FQ_EINVAL;
  if (workspace_bytes < mhaq_fq_od_match_workspace_bytes(G)) return MHAQ_FQ_EWORKSPACE;
  if (((uintptr_t)det & 3) || ((uintptr_t)count & 3) || ((uintptr_t)gt_box & 3) || ((uintptr_t)gt_label & 7) ||
      ((uintptr_t)gt_off & 7) || ((uintptr_t)tp & 3) || ((uintptr_t)flags & 3))
    return MHAQ_FQ_EALIGN;
  if (B > 0x7fffffff || nc > 0x7fffffff || max_det > kOdMaxDet) return MHAQ_FQ_EUNSUPPORTED;
  // the fp64 values of numpy.linspace(0.5, 0.95, 10): k * ((0.95 - 0.5) / 9) + 0.5, the last one set to 0.95
  const OdThresholds thr = {{0x1.0000000000000p-1, 0x1.199999999999ap-1, 0x1.3333333333333p-1, 0x1.4cccccccccccdp-1,
                             0x1.6666666666666p-1, 0x1.8000000000000p-1, 0x1.999999999999ap-1, 0x1.b333333333333p-1,
                             0x1.cccccccccccccp-1, 0x1.e666666666666p-1}};
  MHAQ_LAUNCH(od_match_kernel, dim3((unsigned)B), dim3(kOdMatchBlock), 0, (hipStream_t)stream, det, count, gt_box, gt_label,
              gt_off, G, (int)nc, max_det, tp, flags, static_cast<uint8_t*>(workspace), thr);
  return launch_status();
}

}  // extern "C"
