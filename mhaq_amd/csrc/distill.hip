// Distillation losses over two logit tensors (mhaq_fq_distill_loss_fwd / _bwd, include/mhaq_fq.h): the six softmax-family
// losses a config can name -- Cross-Entropy, Symmetrical Cross-Entropy, KL, Symmetrical KL, JSD, Hellinger -- in two launches
// forward and one backward, where the framework runs a chain of log_softmax / kl_div / sum / mean ops and its autograd mirror.
//
// Per row of logits all six are the same computation: two softmaxes, one row scalar and an elementwise term, and the gradient
// with respect to the student's logits has a closed form in exactly those quantities (the table in the header).
//
// Geometry.  The work is latency-bound ([250, 1000] logits are 1 MB per tensor): one workgroup of kBlock threads per row.
//   * cols <= kDistillRegCols: every thread holds its (up to 16) elements of x and of t in registers -- one read of each
//     input, all loads issued before the first wait.  Where cols % 4 == 0 and the row's bases allow it a lane owns groups of
//     4 consecutive elements (a 16-byte load of fp32, an 8-byte load of 16-bit elements, 16-byte stores of gunit), so that
//     x and t share one layout whatever their types; any other row (odd cols puts every second row at an unaligned base)
//     takes the element layout, lane-strided.
//   * longer rows are walked again out of L2 for each of the four passes, element by element.
//   Three block reductions per row: the two maxima, the two exponent sums (fp64), the row scalar with the term sum (fp64).
//   The row leaves ONE fp64 partial; a one-workgroup finalize sums the partials in a fixed order, divides and rounds once.
// No atomics, no NaN screening: a NaN or infinite logit turns its own row to NaN by plain IEEE arithmetic.
#include <hip/hip_runtime.h>

#include "../../include/mhaq_fq.h"
#include "fq_common.hpp"
#include "fq_io16.hpp"

namespace mhaq {

constexpr int kDistillPer = 16;                          // elements of a row per lane and tensor, register path
constexpr int kDistillRegCols = kBlock * kDistillPer;    // 4096

// ---- element access: DT = MHAQ_FQ_DT_F32 / _BF16 / _F16, converted up exactly
template <int DT>
__device__ __forceinline__ float distill_ld1(const void* row, int64_t i) {
  if constexpr (DT == MHAQ_FQ_DT_F32) return ldg(static_cast<const float*>(row) + i);
  else return io16::up1<DT>(*gptr(static_cast<const uint16_t*>(row) + i));
}
// elements 4 * g .. 4 * g + 3 of a row whose base is aligned to 4 elements
template <int DT>
__device__ __forceinline__ void distill_ld4(const void* row, int g, float (&v)[4]) {
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
__host__ __device__ constexpr int distill_esize() { return DT == MHAQ_FQ_DT_F32 ? 4 : 2; }

// ---- the two maxima / K fp64 sums of a block, in every thread after one barrier (own LDS buffer per call site)
__device__ inline void block_max2_all(float& a, float& b, float* sm) {
  a = wave_max(a);
  b = wave_max(b);
  const int nw = (blockDim.x + 63) >> 6;
  if ((threadIdx.x & 63) == 0) { sm[2 * (threadIdx.x >> 6)] = a; sm[2 * (threadIdx.x >> 6) + 1] = b; }
  __syncthreads();
  a = sm[0]; b = sm[1];
  for (int w = 1; w < nw; ++w) { a = fmaxf(a, sm[2 * w]); b = fmaxf(b, sm[2 * w + 1]); }
}

// ---- per element: probabilities and log-probabilities from the shifted logit a = x - max, e = exp(a), S = sum e, lS = log S
struct DistillP { float ps, pt, ls, lt; };
__device__ __forceinline__ DistillP distill_probs(float ax, float ex, float at, float et, float Sx, float St, float lSx,
                                                  float lSt) {
  DistillP p;
  p.ps = ex / Sx;
  p.pt = et / St;
  p.ls = ax - lSx;
  p.lt = at - lSt;
  return p;
}
// the element's term of the loss and its share of the row scalar (M, K or H of the table; 0 where the kind has none)
__device__ __forceinline__ void distill_term(int kind, const DistillP& p, float& term, float& sc) {
  switch (kind) {
    case MHAQ_FQ_DISTILL_CE:
      term = -(p.pt * p.ls); sc = 0.f; break;
    case MHAQ_FQ_DISTILL_SCE:
      sc = p.ps * p.lt; term = -(p.pt * p.ls) - sc; break;
    case MHAQ_FQ_DISTILL_KL:
      term = p.pt * (p.lt - p.ls); sc = 0.f; break;
    case MHAQ_FQ_DISTILL_HELLINGER: {
      const float a = sqrtf(p.ps), df = a - sqrtf(p.pt);
      term = df * df; sc = a * df; break;
    }
    default: {                       // SKL, JSD
      const float d = p.ls - p.lt;
      term = (p.ps - p.pt) * d; sc = p.ps * d; break;
    }
  }
}
// r_j = denom * gunit_j
__device__ __forceinline__ float distill_r(int kind, const DistillP& p, float sc) {
  switch (kind) {
    case MHAQ_FQ_DISTILL_CE:
    case MHAQ_FQ_DISTILL_KL:
      return p.ps - p.pt;
    case MHAQ_FQ_DISTILL_SCE:
      return p.ps - p.pt - p.ps * (p.lt - sc);
    case MHAQ_FQ_DISTILL_HELLINGER: {
      const float a = sqrtf(p.ps);
      return a * (a - sqrtf(p.pt)) - p.ps * sc;
    }
    default:
      return p.ps - p.pt + p.ps * ((p.ls - p.lt) - sc);
  }
}
__device__ __forceinline__ float distill_scale(float r, double inv_denom) { return (float)((double)r * inv_denom); }

// ---- register path.  VEC: lane owns the groups g = tid + u * kBlock of 4 consecutive elements; else elements tid + k * kBlock
template <int XDT, int TDT, bool VEC>
__device__ __forceinline__ void distill_row_regs(const void* __restrict__ xr, const void* __restrict__ tr, int cols,
                                                 int kind, double inv_denom, double* __restrict__ partial,
                                                 float* __restrict__ gr, float* smf, double* smd1, double* smd2) {
  const int tid = (int)threadIdx.x;
  float ax[kDistillPer], at[kDistillPer], ex[kDistillPer], et[kDistillPer];
  auto index = [&](int k) { return VEC ? 4 * (tid + (k >> 2) * kBlock) + (k & 3) : tid + k * kBlock; };
  if constexpr (VEC) {
#pragma unroll
    for (int u = 0; u < kDistillPer / 4; ++u) {
      const int g = tid + u * kBlock;
      if (4 * g < cols) {
        float v[4], w[4];
        distill_ld4<XDT>(xr, g, v);
        distill_ld4<TDT>(tr, g, w);
#pragma unroll
        for (int j = 0; j < 4; ++j) { ax[4 * u + j] = v[j]; at[4 * u + j] = w[j]; }
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < kDistillPer; ++k) {
      const int i = tid + k * kBlock;
      if (i < cols) { ax[k] = distill_ld1<XDT>(xr, i); at[k] = distill_ld1<TDT>(tr, i); }
    }
  }
  float mx = -INFINITY, mt = -INFINITY;
#pragma unroll
  for (int k = 0; k < kDistillPer; ++k)
    if (index(k) < cols) { mx = fmaxf(mx, ax[k]); mt = fmaxf(mt, at[k]); }
  block_max2_all(mx, mt, smf);
  double s[2] = {0.0, 0.0};
#pragma unroll
  for (int k = 0; k < kDistillPer; ++k)
    if (index(k) < cols) {
      ax[k] = ax[k] - mx; at[k] = at[k] - mt;
      ex[k] = expf(ax[k]); et[k] = expf(at[k]);
      s[0] += (double)ex[k]; s[1] += (double)et[k];
    }
  block_sum_all<2>(s, smd1);
  const float Sx = (float)s[0], St = (float)s[1];
  const float lSx = logf(Sx), lSt = logf(St);
  double a[2] = {0.0, 0.0};                      // term sum, row scalar
#pragma unroll
  for (int k = 0; k < kDistillPer; ++k)
    if (index(k) < cols) {
      const DistillP p = distill_probs(ax[k], ex[k], at[k], et[k], Sx, St, lSx, lSt);
      ex[k] = p.ps; et[k] = p.pt; ax[k] = p.ls; at[k] = p.lt;
      float term, sc;
      distill_term(kind, p, term, sc);
      a[0] += (double)term; a[1] += (double)sc;
    }
  block_sum_all<2>(a, smd2);
  if (tid == 0) *partial = a[0];
  if (!gr) return;
  const float sc = (float)a[1];
  if constexpr (VEC) {
#pragma unroll
    for (int u = 0; u < kDistillPer / 4; ++u) {
      const int g = tid + u * kBlock;
      if (4 * g < cols) {
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = 4 * u + j;
          o[j] = distill_scale(distill_r(kind, DistillP{ex[k], et[k], ax[k], at[k]}, sc), inv_denom);
        }
        stvg<4>(gr + 4 * g, o);
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < kDistillPer; ++k) {
      const int i = tid + k * kBlock;
      if (i < cols) stg(gr + i, distill_scale(distill_r(kind, DistillP{ex[k], et[k], ax[k], at[k]}, sc), inv_denom));
    }
  }
}

// ---- long rows: four passes over the row, the second to fourth out of L2
template <int XDT, int TDT>
__device__ __forceinline__ void distill_row_walk(const void* __restrict__ xr, const void* __restrict__ tr, int64_t cols,
                                                 int kind, double inv_denom, double* __restrict__ partial,
                                                 float* __restrict__ gr, float* smf, double* smd1, double* smd2) {
  const int tid = (int)threadIdx.x;
  float mx = -INFINITY, mt = -INFINITY;
  for (int64_t i = tid; i < cols; i += kBlock) {
    mx = fmaxf(mx, distill_ld1<XDT>(xr, i));
    mt = fmaxf(mt, distill_ld1<TDT>(tr, i));
  }
  block_max2_all(mx, mt, smf);
  double s[2] = {0.0, 0.0};
  for (int64_t i = tid; i < cols; i += kBlock) {
    s[0] += (double)expf(distill_ld1<XDT>(xr, i) - mx);
    s[1] += (double)expf(distill_ld1<TDT>(tr, i) - mt);
  }
  block_sum_all<2>(s, smd1);
  const float Sx = (float)s[0], St = (float)s[1];
  const float lSx = logf(Sx), lSt = logf(St);
  auto probs = [&](int64_t i) {
    const float bx = distill_ld1<XDT>(xr, i) - mx, bt = distill_ld1<TDT>(tr, i) - mt;
    return distill_probs(bx, expf(bx), bt, expf(bt), Sx, St, lSx, lSt);
  };
  double a[2] = {0.0, 0.0};
  for (int64_t i = tid; i < cols; i += kBlock) {
    float term, sc;
    distill_term(kind, probs(i), term, sc);
    a[0] += (double)term; a[1] += (double)sc;
  }
  block_sum_all<2>(a, smd2);
  if (tid == 0) *partial = a[0];
  if (!gr) return;
  const float sc = (float)a[1];
  for (int64_t i = tid; i < cols; i += kBlock) stg(gr + i, distill_scale(distill_r(kind, probs(i), sc), inv_denom));
}

template <int XDT, int TDT>
__global__ __launch_bounds__(kBlock) void distill_row_kernel(const void* __restrict__ x, const void* __restrict__ t,
                                                             int64_t cols, int kind, double inv_denom,
                                                             double* __restrict__ partials, float* __restrict__ gunit) {
  __shared__ float smf[2 * (kBlock / kWave)];
  __shared__ double smd1[2 * (kBlock / kWave)], smd2[2 * (kBlock / kWave)];
  const int64_t row = blockIdx.x, e0 = row * cols;
  const void* xr = static_cast<const char*>(x) + e0 * distill_esize<XDT>();
  const void* tr = static_cast<const char*>(t) + e0 * distill_esize<TDT>();
  float* gr = gunit ? gunit + e0 : nullptr;
  double* partial = partials + row;
  if (cols > kDistillRegCols) {
    distill_row_walk<XDT, TDT>(xr, tr, cols, kind, inv_denom, partial, gr, smf, smd1, smd2);
    return;
  }
  const bool vec = (cols & 3) == 0 && ((uintptr_t)xr & (4 * distill_esize<XDT>() - 1)) == 0 &&
                   ((uintptr_t)tr & (4 * distill_esize<TDT>() - 1)) == 0 && ((uintptr_t)gr & 15) == 0;
  if (vec) distill_row_regs<XDT, TDT, true>(xr, tr, (int)cols, kind, inv_denom, partial, gr, smf, smd1, smd2);
  else distill_row_regs<XDT, TDT, false>(xr, tr, (int)cols, kind, inv_denom, partial, gr, smf, smd1, smd2);
}

// the row partials in a fixed order: thread i takes rows i, i + kBlock, ..., then the block sum; one division, one rounding
__global__ __launch_bounds__(kBlock) void distill_finalize_kernel(const double* __restrict__ partials, int64_t rows,
                                                                  double denom, float* __restrict__ loss) {
  __shared__ double sm[kBlock / kWave];
  double v[1] = {0.0};
  for (int64_t i = threadIdx.x; i < rows; i += kBlock) v[0] += partials[i];
  block_sum<1>(v, sm);
  if (threadIdx.x == 0) *gptr(loss) = (float)(v[0] / denom);
}

// ---- backward: gx = gunit * g[0], rounded once
template <int DT>
__device__ __forceinline__ void distill_st1(void* gx, int64_t i, float v) {
  if constexpr (DT == MHAQ_FQ_DT_F32) stg(static_cast<float*>(gx) + i, v);
  else *gptr(static_cast<uint16_t*>(gx) + i) = io16::down1<DT>(v);
}
template <int DT>
__global__ __launch_bounds__(kBlock) void distill_bwd_kernel(const float* __restrict__ gunit, const float* __restrict__ g,
                                                             void* __restrict__ gx, int64_t n, int vec) {
  const float gv = *g;
  const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x, nth = (int64_t)gridDim.x * kBlock;
  if (vec) {
    const int64_t nv = n >> 2;
    for (int64_t v = tid; v < nv; v += nth) {
      float u[4];
      ldvg<4>(gunit + 4 * v, u);
#pragma unroll
      for (int j = 0; j < 4; ++j) u[j] = u[j] * gv;
      if constexpr (DT == MHAQ_FQ_DT_F32) {
        stvg<4>(static_cast<float*>(gx) + 4 * v, u);
      } else {
        typedef uint32_t vu2 __attribute__((ext_vector_type(2)));
        const vu2 w = {io16::down2<DT>(u[0], u[1]), io16::down2<DT>(u[2], u[3])};
        *gptr(reinterpret_cast<vu2*>(static_cast<uint16_t*>(gx) + 4 * v)) = w;
      }
    }
    const int64_t i = (nv << 2) + tid;             // the n % 4 tail
    if (i < n) distill_st1<DT>(gx, i, ldg(gunit + i) * gv);
  } else {
    for (int64_t i = tid; i < n; i += nth) distill_st1<DT>(gx, i, ldg(gunit + i) * gv);
  }
}

inline bool distill_dtype_ok(int dt) { return dt == MHAQ_FQ_DT_F32 || dt == MHAQ_FQ_DT_BF16 || dt == MHAQ_FQ_DT_F16; }
inline int distill_esize_of(int dt) { return dt == MHAQ_FQ_DT_F32 ? 4 : 2; }
// f receives the dtype as a std::integral_constant (the entry points have checked it)
template <class F>
auto distill_with_dtype(int dt, F f) {
  if (dt == MHAQ_FQ_DT_F32) return f(std::integral_constant<int, MHAQ_FQ_DT_F32>{});
  if (dt == MHAQ_FQ_DT_BF16) return f(std::integral_constant<int, MHAQ_FQ_DT_BF16>{});
  return f(std::integral_constant<int, MHAQ_FQ_DT_F16>{});
}

}  // namespace mhaq

using namespace mhaq;

extern "C" {

size_t mhaq_fq_distill_loss_workspace_bytes(int64_t rows) { return rows > 0 ? (size_t)rows * sizeof(double) : 0; }

int mhaq_fq_distill_loss_fwd(const void* x, int x_dtype, const void* t, int t_dtype, int64_t rows, int64_t cols, int kind,
                             float* loss, float* gunit, void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !t || !loss || !workspace || rows <= 0 || cols <= 0) return MHAQ_FQ_EINVAL;
  if (kind < MHAQ_FQ_DISTILL_CE || kind > MHAQ_FQ_DISTILL_HELLINGER) return MHAQ_FQ_EINVAL;
  if (!distill_dtype_ok(x_dtype) || !distill_dtype_ok(t_dtype)) return MHAQ_FQ_EINVAL;
  if (workspace_bytes < mhaq_fq_distill_loss_workspace_bytes(rows)) return MHAQ_FQ_EWORKSPACE;
  if (((uintptr_t)x & (distill_esize_of(x_dtype) - 1)) || ((uintptr_t)t & (distill_esize_of(t_dtype) - 1)) ||
      ((uintptr_t)loss & 3) || ((uintptr_t)gunit & 3) || ((uintptr_t)workspace & 7))
    return MHAQ_FQ_EALIGN;
  if (rows > 0x7fffffff) return MHAQ_FQ_EUNSUPPORTED;
  const double n = (double)rows * (double)cols;
  const double denom = (kind == MHAQ_FQ_DISTILL_KL || kind == MHAQ_FQ_DISTILL_HELLINGER) ? n
                       : kind == MHAQ_FQ_DISTILL_JSD                                     ? 2.0 * n
                                                                                         : (double)rows;
  double* partials = static_cast<double*>(workspace);
  const hipStream_t st = (hipStream_t)stream;
  distill_with_dtype(x_dtype, [&](auto xdt) {
    distill_with_dtype(t_dtype, [&](auto tdt) {
      MHAQ_LAUNCH((distill_row_kernel<decltype(xdt)::value, decltype(tdt)::value>), dim3((unsigned)rows), dim3(kBlock), 0,
                  st, x, t, cols, kind, 1.0 / denom, partials, gunit);
      return 0;
    });
    return 0;
  });
  if (launch_status() != 0) return launch_status();
  MHAQ_LAUNCH(distill_finalize_kernel, dim3(1), dim3(kBlock), 0, st, partials, rows, denom, loss);
  return launch_status();
}

int mhaq_fq_distill_loss_bwd(const float* gunit, const float* g, void* gx, int gx_dtype, int64_t n, void* stream) {
  if (!gunit || !g || !gx || n <= 0 || !distill_dtype_ok(gx_dtype)) return MHAQ_FQ_EINVAL;
  if (((uintptr_t)gunit & 3) || ((uintptr_t)g & 3) || ((uintptr_t)gx & (distill_esize_of(gx_dtype) - 1))) return MHAQ_FQ_EALIGN;
  const int vec = ((uintptr_t)gunit & 15) == 0 && ((uintptr_t)gx & (4 * distill_esize_of(gx_dtype) - 1)) == 0;
  const int64_t per = (int64_t)kBlock * 4;
  int64_t blocks = (n + per - 1) / per;
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  distill_with_dtype(gx_dtype, [&](auto dt) {
    MHAQ_LAUNCH(distill_bwd_kernel<decltype(dt)::value>, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, gunit,
                g, gx, n, vec);
    return 0;
  });
  return launch_status();
}

}  // extern "C"
