// Object-detection training (mhaq_fq_od_assign, include/mhaq_fq.h): the YOLO task-aligned target assignment, where the
// framework runs about sixty eager launches over ten [B, G, A] tensors with two host synchronisations.  Here no [B, G, A]
// array reaches global memory: the workspace is O(B * G * k + B * A).
//
//   topk     one workgroup of kBlock threads per (image, ground truth).  The box and the label sit in scalars; the anchors are
//            walked coalesced, thread t owning anchors t, t + kBlock, ...; CIoU and the score gather run only for anchors
//            inside the box.  The metric of every anchor stays in LDS (4 * A bytes).  Each anchor has the 64-bit key
//            metric bits << 32 | ~anchor (the metric is >= 0, so its bits order as an unsigned integer, and the lower anchor
//            wins a tie); a thread carries the largest key of its own anchors.  k rounds: a DPP maximum within the
//            wavefront, LDS across the four of them (double-buffered: one barrier per round), then the winner's owner marks
//            it taken and rescans its own column of the LDS array.  A radix select would read the metrics a fixed four times
//            whatever k is; with k <= 32 and 4 * A bytes of LDS the rounds are shorter and need no histogram.
//   resolve  one workgroup of kOdResolveBlock threads per image.  The image's top-k rows are scattered into one LDS word per
//            anchor: count << 20 | sum of the ground-truth indices -- integer adds, so the order of the LDS atomics cannot
//            show, and with count == 1 the sum IS the index.  An anchor with count > 1 walks the ground truth (LDS, broadcast
//            reads) for the arg-max of the overlap.  Each positive then recomputes its metric and overlap with the function
//            the topk kernel called, raises its ground truth's maxima in LDS (an unsigned maximum of the bits of non-negative
//            floats) and, after a barrier, writes its compact row.
//   expand   elementwise: the dense target_scores rows and target_bboxes from the compact rows, every element written once;
//            workgroup 0 adds the images' partial sums in index order and ORs their flag words.
// No global atomics, no workgroup waits for another, every global word has one writer: the same bits at every call.
#include "od_common.hpp"

namespace mhaq {

constexpr int kOdAssignMaxA = 24576;      // anchors: 96 KiB of metrics in LDS
constexpr int kOdAssignMaxG = 1024;       // ground truth per image: count (11 bits) and index sum (20 bits) share a word
constexpr int kOdAssignMaxK = 32;
constexpr int kOdResolveBlock = 1024;
constexpr int kOdExpandRows = 64;         // anchors per workgroup of the expand kernel
constexpr uint32_t kOdTaken = 0xffffffffu;        // in place of a metric's bits (a NaN pattern no metric has)

// how the two exponents are taken: n >= 1 by multiplications (1 = identity), kOdExpSqrt by sqrtf, kOdExpPow by powf
constexpr int kOdExpPow = -1, kOdExpSqrt = -2;
struct OdAssignExp { float alpha, beta; int alpha_mode, beta_mode; };

__device__ __forceinline__ float od_assign_pow(float x, float e, int mode) {
  if (mode == kOdExpSqrt) return sqrtf(x);
  if (mode == kOdExpPow) return powf(x, e);
  float r = 1.f, b = x;
  for (int n = mode; n; n >>= 1) {
    if (n & 1) r = r * b;
    b = b * b;
  }
  return r;
}

// valid(g): the mask is set and the label lies in [0, nc); a NaN label is invalid
__device__ __forceinline__ bool od_assign_label_ok(float lab, int nc) { return lab >= 0.f && lab < (float)nc; }

// in(g, a): min(ax - x1, ay - y1, x2 - ax, y2 - ay) > eps, false when a difference is a NaN (as amin(...).gt_(eps) is)
__device__ __forceinline__ bool od_assign_in(od_f4 g, float ax, float ay, float eps) {
  return ax - g.x > eps && ay - g.y > eps && g.z - ax > eps && g.w - ay > eps;
}

template <int DT>
__device__ __forceinline__ od_f4 od_assign_box(const void* __restrict__ p, int64_t row) {
  return od_f4{iox::ld1<DT>(p, row * 4), iox::ld1<DT>(p, row * 4 + 1), iox::ld1<DT>(p, row * 4 + 2),
               iox::ld1<DT>(p, row * 4 + 3)};
}

struct OdPair { float ov, m; int bad; };

// The overlap and the metric of one (ground truth, anchor) pair that is in-box and valid: the reference's compute_iou with
// box1 = ground truth, box2 = prediction (od_ciou, od_common.hpp).  Both kernels call this one function.
__device__ __forceinline__ OdPair od_assign_pair(od_f4 g, od_f4 p, float sc, OdAssignExp e) {
  OdPair r = {0.f, 0.f, 0};
  if (!(od_finite(g.x) && od_finite(g.y) && od_finite(g.z) && od_finite(g.w) && od_finite(p.x) && od_finite(p.y) &&
        od_finite(p.z) && od_finite(p.w) && od_finite(sc))) {
    r.bad = 1;
    return r;
  }
  const float ciou = od_ciou(g, p).ciou;
  r.ov = ciou > 0.f ? ciou : 0.f;                             // clamp_(0); a NaN (an overflow on the way) counts as 0
  const float m = od_assign_pow(sc, e.alpha, e.alpha_mode) * od_assign_pow(r.ov, e.beta, e.beta_mode);
  r.m = m > 0.f ? m : 0.f;                                    // the key needs a non-negative metric: -0 and NaN count as 0
  return r;
}

// ---------------------------------------------------------------- top-k
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint64_t od_dpp_u64(uint64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, ROW_MASK, 0xF, true);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, ROW_MASK, 0xF, true);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t od_max_u64(uint64_t a, uint64_t b) { return a < b ? b : a; }

// wave64 maximum on the DPP network (the steps of wave_sum_dpp; a lane that receives nothing sees 0): wave-uniform result
__device__ inline uint64_t od_wave_max_u64(uint64_t v) {
  v = od_max_u64(v, od_dpp_u64<0xB1, 0xF>(v));    // quad_perm [1,0,3,2]
  v = od_max_u64(v, od_dpp_u64<0x4E, 0xF>(v));    // quad_perm [2,3,0,1]
  v = od_max_u64(v, od_dpp_u64<0x141, 0xF>(v));   // row_half_mirror
  v = od_max_u64(v, od_dpp_u64<0x140, 0xF>(v));   // row_mirror
  v = od_max_u64(v, od_dpp_u64<0x142, 0xA>(v));   // row_bcast:15 into rows 1 and 3
  v = od_max_u64(v, od_dpp_u64<0x143, 0xC>(v));   // row_bcast:31 into rows 2 and 3 -> lane 63 holds the maximum
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63);
  return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t od_assign_key(uint32_t mbits, int a) { return ((uint64_t)mbits << 32) | (uint32_t)~a; }

template <int DT>
__global__ __launch_bounds__(kBlock) void od_assign_topk_kernel(
    const void* __restrict__ pd_scores, const void* __restrict__ pd_bboxes, const float* __restrict__ anc,
    const float* __restrict__ gt_labels, const float* __restrict__ gt_bboxes, const float* __restrict__ mask_gt, int A, int nc,
    int G, int k, float eps, OdAssignExp e, int32_t* __restrict__ topk_idx, uint32_t* __restrict__ gt_flags) {
  extern __shared__ uint32_t s_m[];                           // [A] metric bits, kOdTaken once chosen; a column per thread
  __shared__ uint64_t s_w[2][kBlock / kWave];
  __shared__ int32_t s_out[kOdAssignMaxK];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.y, bg = b * G + blockIdx.x;
  int32_t* out = topk_idx + bg * k;
  const float labf = ldg(gt_labels + bg);
  if (!(ldg(mask_gt + bg) != 0.f && od_assign_label_ok(labf, nc))) {   // uniform: an empty row
    if (tid < k) *gptr(out + tid) = -1;
    if (tid == 0) *gptr(gt_flags + bg) = 0u;
    return;
  }
  const int label = (int)labf;
  const od_f4 gb = od_f4{ldg(gt_bboxes + bg * 4), ldg(gt_bboxes + bg * 4 + 1), ldg(gt_bboxes + bg * 4 + 2),
                         ldg(gt_bboxes + bg * 4 + 3)};
  uint64_t best = 0;                                          // 0 = no anchor left (an anchor's key has a low word >= 2^31)
  int bad = 0;
  for (int a = tid; a < A; a += kBlock) {
    uint32_t mb = 0;
    if (od_assign_in(gb, ldg(anc + 2 * (int64_t)a), ldg(anc + 2 * (int64_t)a + 1), eps)) {
      const int64_t row = b * A + a;
      const OdPair r = od_assign_pair(gb, od_assign_box<DT>(pd_bboxes, row), iox::ld1<DT>(pd_scores, row * nc + label), e);
      bad |= r.bad;
      mb = __float_as_uint(r.m);
    }
    s_m[a] = mb;
    best = od_max_u64(best, od_assign_key(mb, a));
  }
  for (int r = 0; r < k; ++r) {
    uint64_t w = od_wave_max_u64(best);
    if (lane == 0) s_w[r & 1][wave] = w;
    __syncthreads();
    w = od_max_u64(od_max_u64(s_w[r & 1][0], s_w[r & 1][1]), od_max_u64(s_w[r & 1][2], s_w[r & 1][3]));
    const int win = (int)~(uint32_t)w;
    if (tid == 0) s_out[r] = w ? win : -1;
    if (w && (win & (kBlock - 1)) == tid) {                   // the owner takes it out and looks its column through again
      s_m[win] = kOdTaken;
      best = 0;
      for (int a = tid; a < A; a += kBlock) {
        const uint32_t mb = s_m[a];
        if (mb != kOdTaken) best = od_max_u64(best, od_assign_key(mb, a));
      }
    }
  }
  __syncthreads();
  if (tid < k) {
    const int a = s_out[tid];
    const bool in = a >= 0 && a < A && od_assign_in(gb, ldg(anc + 2 * (int64_t)a), ldg(anc + 2 * (int64_t)a + 1), eps);
    *gptr(out + tid) = in ? a : -1;
  }
  bad = __syncthreads_or(bad);
  if (tid == 0) *gptr(gt_flags + bg) = bad ? 1u : 0u;
}

// ---------------------------------------------------------------- resolve
template <int DT>
__global__ __launch_bounds__(kOdResolveBlock) void od_assign_resolve_kernel(
    const void* __restrict__ pd_scores, const void* __restrict__ pd_bboxes, const float* __restrict__ anc,
    const float* __restrict__ gt_labels, const float* __restrict__ gt_bboxes, const float* __restrict__ mask_gt, int A, int nc,
    int G, int k, float eps, OdAssignExp e, const int32_t* __restrict__ topk_idx, const uint32_t* __restrict__ gt_flags,
    uint8_t* __restrict__ fg_mask, int32_t* __restrict__ gt_idx, int32_t* __restrict__ label_out, float* __restrict__ norm_out,
    double* __restrict__ partial, uint32_t* __restrict__ img_flags) {
  extern __shared__ uint32_t s_dyn[];
  uint32_t* s_acc = s_dyn;                                    // [A] count << 20 | index sum; later the metric's bits
  float* s_box = reinterpret_cast<float*>(s_acc + A);         // [G][4]
  int32_t* s_lab = reinterpret_cast<int32_t*>(s_box + 4 * (int64_t)G);      // [G] the label, -1 for an invalid ground truth
  uint32_t* s_pam = reinterpret_cast<uint32_t*>(s_lab + G);   // [G] bits of max m over the positives
  uint32_t* s_pov = s_pam + G;                                // [G] bits of max ov over the positives
  __shared__ double s_red[kOdResolveBlock / kWave];
  const int tid = (int)threadIdx.x;
  const int64_t b = blockIdx.x;
  uint32_t f = 0;
  for (int g = tid; g < G; g += kOdResolveBlock) {
    const int64_t bg = b * G + g;
    const float labf = ldg(gt_labels + bg);
    const bool masked = ldg(mask_gt + bg) != 0.f, ok = od_assign_label_ok(labf, nc);
    f |= (masked && !ok) ? 4u : 0u;
    f |= *gptr(gt_flags + bg);
    s_lab[g] = (masked && ok) ? (int)labf : -1;
#pragma unroll
    for (int j = 0; j < 4; ++j) s_box[4 * g + j] = ldg(gt_bboxes + bg * 4 + j);
    s_pam[g] = 0u;
    s_pov[g] = 0u;
  }
  for (int a = tid; a < A; a += kOdResolveBlock) s_acc[a] = 0u;
  __syncthreads();
  const int32_t* rows = topk_idx + b * G * k;
  for (int i = tid; i < G * k; i += kOdResolveBlock) {
    const int a = *gptr(rows + i);
    if ((uint32_t)a < (uint32_t)A) atomicAdd(&s_acc[a], (1u << 20) + (uint32_t)(i / k));
  }
  __syncthreads();
  for (int a = tid; a < A; a += kOdResolveBlock) {
    const uint32_t w = s_acc[a], cnt = w >> 20;
    const int64_t row = b * A + a;
    int gi = 0;
    uint32_t mb = 0;
    if (cnt) {
      const float ax = ldg(anc + 2 * (int64_t)a), ay = ldg(anc + 2 * (int64_t)a + 1);
      const od_f4 p = od_assign_box<DT>(pd_bboxes, row);
      if (cnt == 1) {
        gi = (int)(w & 0xfffffu);
      } else {                                                // arg-max of ov over ALL ground truth, the lowest on a tie
        float bo = -1.f;
        for (int g = 0; g < G; ++g) {
          const int lab = s_lab[g];
          const od_f4 gb = od_f4{s_box[4 * g], s_box[4 * g + 1], s_box[4 * g + 2], s_box[4 * g + 3]};
          float ov = 0.f;
          if (lab >= 0 && od_assign_in(gb, ax, ay, eps)) ov = od_assign_pair(gb, p, iox::ld1<DT>(pd_scores, row * nc + lab), e).ov;
          if (ov > bo) { bo = ov; gi = g; }
        }
      }
      const int lab = s_lab[gi];
      const od_f4 gb = od_f4{s_box[4 * gi], s_box[4 * gi + 1], s_box[4 * gi + 2], s_box[4 * gi + 3]};
      if (lab >= 0 && od_assign_in(gb, ax, ay, eps)) {        // the winner of an arg-max over zeros need not hold the anchor
        const OdPair r = od_assign_pair(gb, p, iox::ld1<DT>(pd_scores, row * nc + lab), e);
        mb = __float_as_uint(r.m);
        atomicMax(&s_pam[gi], mb);
        atomicMax(&s_pov[gi], __float_as_uint(r.ov));
      }
    }
    s_acc[a] = mb;                                            // anchor a is this thread's alone from here on
    *gptr(gt_idx + row) = gi;
    *gptr(fg_mask + row) = cnt ? 1 : 0;
  }
  __syncthreads();
  double acc = 0.0;
  for (int a = tid; a < A; a += kOdResolveBlock) {
    const int64_t row = b * A + a;
    const int gi = *gptr(gt_idx + row);                       // this thread's own stores
    float norm = 0.f, labf = 0.f;
    const float m = __uint_as_float(s_acc[a]);
    if (m > 0.f)                                              // a zero metric is a zero norm, also where pam + eps is 0
      norm = (m * __uint_as_float(s_pov[gi])) / (__uint_as_float(s_pam[gi]) + eps);
    if (G > 0) labf = ldg(gt_labels + b * G + gi);
    *gptr(label_out + row) = labf > 0.f ? (labf < 2147483520.f ? (int)labf : 0x7fffffff) : 0;   // clamp_(0); a NaN is 0
    *gptr(norm_out + row) = norm;
    acc += (double)norm;
  }
  acc = wave_sum(acc);                                        // a fixed tree: lanes, then the wavefronts in order
  if ((tid & 63) == 0) s_red[tid >> 6] = acc;
  const int f0 = __syncthreads_or((int)(f & 1u)), f2 = __syncthreads_or((int)(f & 4u));
  if (tid == 0) {
    double s = 0.0;
    for (int i = 0; i < kOdResolveBlock / kWave; ++i) s += s_red[i];
    *gptr(partial + b) = s;
    *gptr(img_flags + b) = (f0 ? 1u : 0u) | (f2 ? 4u : 0u);
  }
}

// ---------------------------------------------------------------- expand
// VEC: nc % 4 == 0 and both outputs 16-byte aligned -- a tile of kOdExpandRows rows then starts on a 16-byte boundary
template <bool VEC>
__global__ __launch_bounds__(kBlock) void od_assign_expand_kernel(
    const uint8_t* __restrict__ fg_mask, const int32_t* __restrict__ gt_idx, const int32_t* __restrict__ label,
    const float* __restrict__ norm, const float* __restrict__ gt_bboxes, int64_t rows, int A, int nc, int G, int n_partial,
    const double* __restrict__ partial, const uint32_t* __restrict__ img_flags, float* __restrict__ target_bboxes,
    float* __restrict__ target_scores, float* __restrict__ scores_sum, uint32_t* __restrict__ flags) {
  __shared__ int32_t s_label[kOdExpandRows];                  // -1 for a background row
  __shared__ float s_norm[kOdExpandRows];
  const int tid = (int)threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kOdExpandRows;
  const int nrows = (int)(rows - row0 < kOdExpandRows ? (rows - row0 < 0 ? 0 : rows - row0) : kOdExpandRows);
  if (tid < nrows) {
    const int64_t r = row0 + tid;
    s_label[tid] = *gptr(fg_mask + r) ? *gptr(label + r) : -1;
    s_norm[tid] = ldg(norm + r);
    float bx[4] = {0.f, 0.f, 0.f, 0.f};
    if (G > 0) {                                              // a background anchor carries ground truth 0's box
      const float* src = gt_bboxes + ((r / A) * G + *gptr(gt_idx + r)) * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) bx[j] = ldg(src + j);
    }
    if constexpr (VEC) stvg<4>(target_bboxes + r * 4, bx);
    else {
#pragma unroll
      for (int j = 0; j < 4; ++j) stg(target_bboxes + r * 4 + j, bx[j]);
    }
  }
  __syncthreads();
  float* dst = target_scores + row0 * nc;
  const int total = nrows * nc;
  if constexpr (VEC) {
    for (int e = tid * 4; e < total; e += kBlock * 4) {
      const int r = e / nc, c = e - r * nc, lab = s_label[r];
      const float n = s_norm[r];
      const float v[4] = {lab == c ? n : 0.f, lab == c + 1 ? n : 0.f, lab == c + 2 ? n : 0.f, lab == c + 3 ? n : 0.f};
      stvg<4>(dst + e, v);
    }
  } else {
    for (int e = tid; e < total; e += kBlock) {
      const int r = e / nc, c = e - r * nc;
      stg(dst + e, s_label[r] == c ? s_norm[r] : 0.f);
    }
  }
  if (blockIdx.x == 0 && tid == 0) {                          // the one writer of the sum and of the flag word
    double s = 0.0;
    uint32_t f = 0;
    for (int i = 0; i < n_partial; ++i) {
      s += *gptr(partial + i);
      f |= *gptr(img_flags + i);
    }
    stg(scores_sum, (float)s);
    *gptr(flags) = f;
  }
}

static int od_exp_mode(float e) {
  if (e == 0.5f) return kOdExpSqrt;
  if (e >= 1.f && e <= 64.f && e == (float)(int)e) return (int)e;
  return kOdExpPow;
}

}  // namespace mhaq

using namespace mhaq;

extern "C" {

size_t mhaq_fq_od_assign_workspace_bytes(int64_t b, int64_t g, int64_t a, int top_k) {
  if (b < 1 || a < 1 || g < 0 || top_k < 1 || b > 65535 || a > kOdAssignMaxA || g > kOdAssignMaxG || top_k > kOdAssignMaxK)
    return 0;
  const size_t B = (size_t)b, G = (size_t)g, A = (size_t)a;
  return od_r8(B * 8) + od_r8(B * G * (size_t)top_k * 4) + 2 * od_r8(B * A * 4) + od_r8(B * G * 4) + od_r8(B * 4);
}

int mhaq_fq_od_assign(const void* pd_scores, const void* pd_bboxes, int pd_dtype, const float* anc_points,
                      const float* gt_labels, const float* gt_bboxes, const float* mask_gt, int64_t b, int64_t a, int64_t nc,
                      int64_t g, int top_k, float alpha, float beta, float eps, float* target_bboxes, float* target_scores,
                      uint8_t* fg_mask, int32_t* target_gt_idx, float* scores_sum, uint32_t* flags, void* workspace,
                      size_t workspace_bytes, void* stream) {
  if (!scores_sum || !flags || b < 0 || a < 0 || g < 0 || nc < 1 || top_k < 1 || !iox::known_dtype(pd_dtype))
    return MHAQ_FQ_EINVAL;
  if (!(alpha >= 0.f) || !(beta >= 0.f) || !od_finite(alpha) || !od_finite(beta) || !(eps >= 0.f) || !od_finite(eps))
    return MHAQ_FQ_EINVAL;
  const bool empty = b == 0 || a == 0;
  if (!empty) {
    if (!pd_scores || !pd_bboxes || !anc_points || !target_bboxes || !target_scores || !fg_mask || !target_gt_idx ||
        !workspace || (g > 0 && (!gt_labels || !gt_bboxes || !mask_gt)) || a < top_k)
      return MHAQ_FQ_EINVAL;
    if (b > 65535 || a > kOdAssignMaxA || g > kOdAssignMaxG || top_k > kOdAssignMaxK || nc > 65535)
      return MHAQ_FQ_EUNSUPPORTED;
    if (workspace_bytes < mhaq_fq_od_assign_workspace_bytes(b, g, a, top_k)) return MHAQ_FQ_EWORKSPACE;
  }
  const uintptr_t pm = pd_dtype == MHAQ_FQ_DT_F32 ? 3 : 1;
  if (((uintptr_t)pd_scores & pm) || ((uintptr_t)pd_bboxes & pm) || ((uintptr_t)anc_points & 3) || ((uintptr_t)gt_labels & 3) ||
      ((uintptr_t)gt_bboxes & 3) || ((uintptr_t)mask_gt & 3) || ((uintptr_t)target_bboxes & 3) ||
      ((uintptr_t)target_scores & 3) || ((uintptr_t)target_gt_idx & 3) || ((uintptr_t)scores_sum & 3) ||
      ((uintptr_t)flags & 3) || ((uintptr_t)workspace & 7))
    return MHAQ_FQ_EALIGN;
  const hipStream_t st = (hipStream_t)stream;
  const int B = (int)b, A = (int)a, G = (int)g, NC = (int)nc, K = top_k;
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  double* partial = nullptr;
  int32_t *topk_idx = nullptr, *label = nullptr;
  float* norm = nullptr;
  uint32_t *gt_flags = nullptr, *img_flags = nullptr;
  if (!empty) {
    const size_t sB = (size_t)B, sG = (size_t)G, sA = (size_t)A;
    partial = reinterpret_cast<double*>(ws);                 ws += od_r8(sB * 8);
    topk_idx = reinterpret_cast<int32_t*>(ws);               ws += od_r8(sB * sG * (size_t)K * 4);
    label = reinterpret_cast<int32_t*>(ws);                  ws += od_r8(sB * sA * 4);
    norm = reinterpret_cast<float*>(ws);                     ws += od_r8(sB * sA * 4);
    gt_flags = reinterpret_cast<uint32_t*>(ws);              ws += od_r8(sB * sG * 4);
    img_flags = reinterpret_cast<uint32_t*>(ws);
    const OdAssignExp e = {alpha, beta, od_exp_mode(alpha), od_exp_mode(beta)};
    const size_t lds_topk = sA * 4, lds_resolve = sA * 4 + sG * 28;
    int rc = 0;
    iox::with_dtype(pd_dtype, [&](auto dt) {
      constexpr int DT = decltype(dt)::value;
      if (G > 0) {
        MHAQ_LAUNCH(od_assign_topk_kernel<DT>, dim3((unsigned)G, (unsigned)B), dim3(kBlock), lds_topk, st, pd_scores,
                    pd_bboxes, anc_points, gt_labels, gt_bboxes, mask_gt, A, NC, G, K, eps, e, topk_idx, gt_flags);
        if ((rc = launch_status()) != 0) return;
      }
      MHAQ_LAUNCH(od_assign_resolve_kernel<DT>, dim3((unsigned)B), dim3(kOdResolveBlock), lds_resolve, st, pd_scores,
                  pd_bboxes, anc_points, gt_labels, gt_bboxes, mask_gt, A, NC, G, K, eps, e, (const int32_t*)topk_idx,
                  (const uint32_t*)gt_flags, fg_mask, target_gt_idx, label, norm, partial, img_flags);
      rc = launch_status();
    });
    if (rc != 0) return rc;
  }
  const int64_t rows = empty ? 0 : b * a;
  const unsigned grid = rows ? (unsigned)((rows + kOdExpandRows - 1) / kOdExpandRows) : 1u;
  const bool vec = NC % 4 == 0 && !((uintptr_t)target_scores & 15) && !((uintptr_t)target_bboxes & 15);
  if (vec)
    MHAQ_LAUNCH(od_assign_expand_kernel<true>, dim3(grid), dim3(kBlock), 0, st, (const uint8_t*)fg_mask,
                (const int32_t*)target_gt_idx, (const int32_t*)label, (const float*)norm, gt_bboxes, rows, A, NC, G,
                empty ? 0 : B, (const double*)partial, (const uint32_t*)img_flags, target_bboxes, target_scores, scores_sum,
                flags);
  else
    MHAQ_LAUNCH(od_assign_expand_kernel<false>, dim3(grid), dim3(kBlock), 0, st, (const uint8_t*)fg_mask,
                (const int32_t*)target_gt_idx, (const int32_t*)label, (const float*)norm, gt_bboxes, rows, A, NC, G,
                empty ? 0 : B, (const double*)partial, (const uint32_t*)img_flags, target_bboxes, target_scores, scores_sum,
                flags);
  return launch_status();
}

}  // extern "C"
