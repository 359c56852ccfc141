// Classification head over one logit tensor and int64 labels (mhaq_fq_cls_head_fwd, include/mhaq_fq.h): the mean
// cross-entropy, the per-row nll, the rank of the label's logit -- and from it top-1 / top-k correctness as exact integer
// counts -- and optionally the gradient, from ONE read of the logits, in two launches, where the framework runs
// log_softmax / nll_loss, argmax / eq / mean and topk / eq / any / mean.  The backward is mhaq_fq_distill_loss_bwd (distill.hip).
//
// Geometry (distill.hip's): one workgroup of kBlock threads per row.
//   * the label y of the row is one wave-uniform load; a row whose label is ignore_index or out of range leaves before it
//     forms any address from y (zeros into its gunit row, rank = cols).  A valid row fetches x_y with one broadcast load, so
//     that the maximum, the two rank tallies and -- behind the same barrier -- the count V of valid rows (needed by gunit only)
//     come out of the single pass over the row.
//   * cols <= kClsRegCols: every thread holds its (up to 16) elements in registers, all loads issued before the first wait;
//     groups of 4 consecutive elements where cols % 4 == 0 and the bases allow it, lane-strided elements otherwise.
//   * longer rows are walked again out of L2 (maximum and tallies, exponent sum, gunit).
//   Two block reductions per row: {max, tallies, V} and the exponent sum (fp64).  A row leaves its nll as an fp64 partial, its
//   rank and a status word; a one-workgroup finalize adds them up in a fixed order, divides and rounds once.
// No atomics, no NaN screening: a NaN or infinite logit turns its own row's nll to NaN (or inf) by plain IEEE arithmetic.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/mhaq_fq.h"
#include "fq_common.hpp"
#include "fq_io16.hpp"

namespace mhaq {

constexpr int kClsPer = 16;                        // elements of a row per lane, register path
constexpr int kClsRegCols = kBlock * kClsPer;      // 4096

// status word of a row (workspace): what the finalize counts
enum { kClsValid = 1, kClsNonFinite = 2, kClsBadTarget = 4 };

template <int DT>
__device__ __forceinline__ float cls_ld1(const void* row, int64_t i) {
  if constexpr (DT == MHAQ_FQ_DT_F32) return ldg(static_cast<const float*>(row) + i);
  else return io16::up1<DT>(*gptr(static_cast<const uint16_t*>(row) + i));
}
// elements 4 * g .. 4 * g + 3 of a row whose base is aligned to 4 elements
template <int DT>
__device__ __forceinline__ void cls_ld4(const void* row, int g, float (&v)[4]) {
  if constexpr (DT == MHAQ_FQ_DT_F32) {
    ldvg<4>(static_cast<const float*>(row) + 4 * g, v);
  } else {
    typedef uint32_t vu2 __attribute__((ext_vector_type(2)));
    const vu2 w = *gptr(reinterpret_cast<const vu2*>(static_cast<const uint16_t*>(row) + 4 * g));
    io16::up2<DT>(w.x, v[0], v[1]);
    io16::up2<DT>(w.y, v[2], v[3]);
  }
}
template <int DT>
__host__ __device__ constexpr int cls_esize() { return DT == MHAQ_FQ_DT_F32 ? 4 : 2; }

__device__ __forceinline__ bool cls_target_valid(int64_t y, int64_t cols, int64_t ignore_index) {
  return y != ignore_index && y >= 0 && y < cols;
}

// The label's place in the order of a stable descending sort: `above` = v sorts strictly before x_y (NaN above +inf),
// `same` = v ties with x_y (NaN ties with NaN, +0 with -0) -- it counts only at a column left of the label.
struct ClsOrder {
  float xy;
  bool ny;
  __device__ __forceinline__ explicit ClsOrder(float xy_) : xy(xy_), ny(xy_ != xy_) {}
  __device__ __forceinline__ bool above(float v) const { return !ny && (v != v || v > xy); }
  __device__ __forceinline__ bool same(float v) const { return ny ? v != v : v == xy; }
};

// the row maximum and three integer tallies of a block, in every thread after one barrier
__device__ inline void block_max_tally3_all(float& m, int& c0, int& c1, int& c2, float* smf, int* smi) {
  m = wave_max(m);
  c0 = wave_sum_dpp_i32(c0);
  c1 = wave_sum_dpp_i32(c1);
  c2 = wave_sum_dpp_i32(c2);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  if (lane == 0) {
    smf[wave] = m;
    smi[3 * wave] = c0; smi[3 * wave + 1] = c1; smi[3 * wave + 2] = c2;
  }
  __syncthreads();
  m = smf[0]; c0 = smi[0]; c1 = smi[1]; c2 = smi[2];
  for (int w = 1; w < nw; ++w) {
    m = fmaxf(m, smf[w]);
    c0 += smi[3 * w]; c1 += smi[3 * w + 1]; c2 += smi[3 * w + 2];
  }
}

// this thread's share of V = number of valid rows of the batch (only a row that writes a gradient needs it)
__device__ __forceinline__ int cls_count_valid(const int64_t* __restrict__ target, int64_t rows, int64_t cols,
                                               int64_t ignore_index) {
  int v = 0;
  for (int64_t r = threadIdx.x; r < rows; r += kBlock) v += cls_target_valid(*gptr(target + r), cols, ignore_index) ? 1 : 0;
  return v;
}

// nll of the row from its shifted label logit and its exponent sum: log S - (x_y - m), the framework's order of operations
__device__ __forceinline__ float cls_nll(float xy, float m, float S) { return logf(S) - (xy - m); }
__device__ __forceinline__ float cls_g(float e, float S, bool is_label, double inv_v) {
  const float p = e / S;
  return (float)((double)(is_label ? p - 1.0f : p) * inv_v);
}

struct ClsRowOut { float nll; int rank; };

// ---- register path.  VEC: lane owns the groups g = tid + u * kBlock of 4 consecutive elements; else elements tid + k * kBlock
template <int DT, bool VEC>
__device__ __forceinline__ ClsRowOut cls_row_regs(const void* __restrict__ xr, int cols, int y, float xy, int vshare,
                                                  float* __restrict__ gr, float* smf, int* smi, double* smd) {
  const int tid = (int)threadIdx.x;
  float a[kClsPer];
  auto index = [&](int k) { return VEC ? 4 * (tid + (k >> 2) * kBlock) + (k & 3) : tid + k * kBlock; };
  if constexpr (VEC) {
#pragma unroll
    for (int u = 0; u < kClsPer / 4; ++u) {
      const int g = tid + u * kBlock;
      if (4 * g < cols) {
        float v[4];
        cls_ld4<DT>(xr, g, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) a[4 * u + j] = v[j];
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < kClsPer; ++k) {
      const int i = tid + k * kBlock;
      if (i < cols) a[k] = cls_ld1<DT>(xr, i);
    }
  }
  const ClsOrder ord(xy);
  float m = -INFINITY;
  int above = 0, same = 0;
#pragma unroll
  for (int k = 0; k < kClsPer; ++k)
    if (index(k) < cols) {
      m = fmaxf(m, a[k]);
      above += ord.above(a[k]) ? 1 : 0;
      same += (index(k) < y && ord.same(a[k])) ? 1 : 0;
    }
  block_max_tally3_all(m, above, same, vshare, smf, smi);
  double s[1] = {0.0};
#pragma unroll
  for (int k = 0; k < kClsPer; ++k)
    if (index(k) < cols) {
      a[k] = expf(a[k] - m);
      s[0] += (double)a[k];
    }
  block_sum_all<1>(s, smd);
  const float S = (float)s[0];
  if (gr) {
    const double inv_v = 1.0 / (double)vshare;
    if constexpr (VEC) {
#pragma unroll
      for (int u = 0; u < kClsPer / 4; ++u) {
        const int g = tid + u * kBlock;
        if (4 * g < cols) {
          float o[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = cls_g(a[4 * u + j], S, 4 * g + j == y, inv_v);
          stvg<4>(gr + 4 * g, o);
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < kClsPer; ++k) {
        const int i = tid + k * kBlock;
        if (i < cols) stg(gr + i, cls_g(a[k], S, i == y, inv_v));
      }
    }
  }
  return ClsRowOut{cls_nll(xy, m, S), above + same};
}

// ---- long rows: the second and third pass come out of L2
template <int DT>
__device__ __forceinline__ ClsRowOut cls_row_walk(const void* __restrict__ xr, int64_t cols, int64_t y, float xy, int vshare,
                                                  float* __restrict__ gr, float* smf, int* smi, double* smd) {
  const int tid = (int)threadIdx.x;
  const ClsOrder ord(xy);
  float m = -INFINITY;
  int above = 0, same = 0;
  for (int64_t i = tid; i < cols; i += kBlock) {
    const float v = cls_ld1<DT>(xr, i);
    m = fmaxf(m, v);
    above += ord.above(v) ? 1 : 0;
    same += (i < y && ord.same(v)) ? 1 : 0;
  }
  block_max_tally3_all(m, above, same, vshare, smf, smi);
  double s[1] = {0.0};
  for (int64_t i = tid; i < cols; i += kBlock) s[0] += (double)expf(cls_ld1<DT>(xr, i) - m);
  block_sum_all<1>(s, smd);
  const float S = (float)s[0];
  if (gr) {
    const double inv_v = 1.0 / (double)vshare;
    for (int64_t i = tid; i < cols; i += kBlock) stg(gr + i, cls_g(expf(cls_ld1<DT>(xr, i) - m), S, i == y, inv_v));
  }
  return ClsRowOut{cls_nll(xy, m, S), above + same};
}

template <int DT>
__global__ __launch_bounds__(kBlock) void cls_head_row_kernel(const void* __restrict__ x, const int64_t* __restrict__ target,
                                                              int64_t rows, int64_t cols, int64_t ignore_index,
                                                              double* __restrict__ partials, int32_t* __restrict__ ws_rank,
                                                              int32_t* __restrict__ ws_status, float* __restrict__ nll,
                                                              int32_t* __restrict__ rank, float* __restrict__ gunit) {
  __shared__ float smf[kBlock / kWave];
  __shared__ int smi[3 * (kBlock / kWave)];
  __shared__ double smd[kBlock / kWave];
  const int tid = (int)threadIdx.x;
  const int64_t row = blockIdx.x, e0 = row * cols;
  const void* xr = static_cast<const char*>(x) + e0 * cls_esize<DT>();
  float* gr = gunit ? gunit + e0 : nullptr;
  const int64_t y = *gptr(target + row);
  if (!cls_target_valid(y, cols, ignore_index)) {          // block-uniform: no address is ever formed from this y
    if (gr)
      for (int64_t i = tid; i < cols; i += kBlock) stg(gr + i, 0.f);
    if (tid == 0) {
      *gptr(partials + row) = 0.0;
      *gptr(ws_rank + row) = (int32_t)cols;
      *gptr(ws_status + row) = y == ignore_index ? 0 : kClsBadTarget;
      if (nll) stg(nll + row, 0.f);
      if (rank) *gptr(rank + row) = (int32_t)cols;
    }
    return;
  }
  const float xy = cls_ld1<DT>(xr, y);
  const int vshare = gr ? cls_count_valid(target, rows, cols, ignore_index) : 0;
  ClsRowOut o;
  if (cols > kClsRegCols) {
    o = cls_row_walk<DT>(xr, cols, y, xy, vshare, gr, smf, smi, smd);
  } else {
    const bool vec = (cols & 3) == 0 && ((uintptr_t)xr & (4 * cls_esize<DT>() - 1)) == 0 && ((uintptr_t)gr & 15) == 0;
    if (vec) o = cls_row_regs<DT, true>(xr, (int)cols, (int)y, xy, vshare, gr, smf, smi, smd);
    else o = cls_row_regs<DT, false>(xr, (int)cols, (int)y, xy, vshare, gr, smf, smi, smd);
  }
  if (tid == 0) {
    const bool finite = fabsf(o.nll) <= 3.4028234663852886e38f;      // false for NaN and the infinities
    *gptr(partials + row) = (double)o.nll;
    *gptr(ws_rank + row) = o.rank;
    *gptr(ws_status + row) = kClsValid | (finite ? 0 : kClsNonFinite);
    if (nll) stg(nll + row, o.nll);
    if (rank) *gptr(rank + row) = o.rank;
  }
}

// the rows in a fixed order: thread i takes rows i, i + kBlock, ..., then the block sum (the tallies as fp64: exact integers)
__global__ __launch_bounds__(kBlock) void cls_head_finalize_kernel(const double* __restrict__ partials,
                                                                   const int32_t* __restrict__ ws_rank,
                                                                   const int32_t* __restrict__ ws_status, int64_t rows, int topk,
                                                                   float* __restrict__ loss, float* __restrict__ acc,
                                                                   int64_t* __restrict__ counts, uint32_t* __restrict__ flags) {
  __shared__ double sm[6 * (kBlock / kWave)];
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // sum nll, V, rank == 0, rank < topk, non-finite rows, bad targets
  for (int64_t i = threadIdx.x; i < rows; i += kBlock) {
    const int st = *gptr(ws_status + i);
    if (st & kClsValid) {
      const int r = *gptr(ws_rank + i);
      v[0] += *gptr(partials + i);
      v[1] += 1.0;
      v[2] += r == 0 ? 1.0 : 0.0;
      v[3] += r < topk ? 1.0 : 0.0;
      v[4] += (st & kClsNonFinite) ? 1.0 : 0.0;
    }
    v[5] += (st & kClsBadTarget) ? 1.0 : 0.0;
  }
  block_sum<6>(v, sm);
  if (threadIdx.x == 0) {
    const float V = (float)v[1];
    stg(loss, (float)(v[0] / v[1]));                  // V == 0: 0 / 0 = NaN, as the framework's mean over no rows
    stg(acc, v[1] > 0.0 ? (float)v[2] / V : 0.f);
    stg(acc + 1, v[1] > 0.0 ? (float)v[3] / V : 0.f);
    *gptr(counts) = (int64_t)v[1];
    *gptr(counts + 1) = (int64_t)v[2];
    *gptr(counts + 2) = (int64_t)v[3];
    *gptr(flags) = (v[4] > 0.0 ? 2u : 0u) | (v[5] > 0.0 ? 4u : 0u);
  }
}

}  // namespace mhaq

using namespace mhaq;

extern "C" {

// per row: the fp64 nll partial, the rank and the status word
size_t mhaq_fq_cls_head_workspace_bytes(int64_t rows) { return rows > 0 ? (size_t)rows * 16 : 0; }

int mhaq_fq_cls_head_fwd(const void* x, int x_dtype, const int64_t* target, int64_t rows, int64_t cols, int64_t ignore_index,
                         int topk, float* loss, float* acc, int64_t* counts, float* nll, int32_t* rank, float* gunit,
                         uint32_t* flags, void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !target || !loss || !acc || !counts || !flags || !workspace || rows < 1 || cols < 1 || topk < 1)
    return MHAQ_FQ_EINVAL;
  if (x_dtype != MHAQ_FQ_DT_F32 && x_dtype != MHAQ_FQ_DT_BF16 && x_dtype != MHAQ_FQ_DT_F16) return MHAQ_FQ_EINVAL;
  if (workspace_bytes < mhaq_fq_cls_head_workspace_bytes(rows)) return MHAQ_FQ_EWORKSPACE;
  const int esize = x_dtype == MHAQ_FQ_DT_F32 ? 4 : 2;
  if (((uintptr_t)x & (esize - 1)) || ((uintptr_t)target & 7) || ((uintptr_t)loss & 3) || ((uintptr_t)acc & 3) ||
      ((uintptr_t)counts & 7) || ((uintptr_t)nll & 3) || ((uintptr_t)rank & 3) || ((uintptr_t)gunit & 3) ||
      ((uintptr_t)flags & 3) || ((uintptr_t)workspace & 7))
    return MHAQ_FQ_EALIGN;
  if (rows > 0x7fffffff || cols > 0x7fffffff) return MHAQ_FQ_EUNSUPPORTED;
  double* partials = static_cast<double*>(workspace);
  int32_t* ws_rank = reinterpret_cast<int32_t*>(partials + rows);
  int32_t* ws_status = ws_rank + rows;
  const hipStream_t st = (hipStream_t)stream;
  auto row_launch = [&](auto dt) {
    MHAQ_LAUNCH(cls_head_row_kernel<decltype(dt)::value>, dim3((unsigned)rows), dim3(kBlock), 0, st, x, target, rows, cols,
                ignore_index, partials, ws_rank, ws_status, nll, rank, gunit);
  };
  if (x_dtype == MHAQ_FQ_DT_F32) row_launch(std::integral_constant<int, MHAQ_FQ_DT_F32>{});
  else if (x_dtype == MHAQ_FQ_DT_BF16) row_launch(std::integral_constant<int, MHAQ_FQ_DT_BF16>{});
  else row_launch(std::integral_constant<int, MHAQ_FQ_DT_F16>{});
  if (launch_status() != 0) return launch_status();
  MHAQ_LAUNCH(cls_head_finalize_kernel, dim3(1), dim3(kBlock), 0, st, (const double*)partials, (const int32_t*)ws_rank,
              (const int32_t*)ws_status, rows, topk, loss, acc, counts, flags);
  return launch_status();
}

}  // extern "C"
