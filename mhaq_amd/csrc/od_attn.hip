// YOLOv11 PSA attention (mhaq_fq_od_attn_fwd, mhaq_fq_od_attn_bwd; include/mhaq_fq.h): the three statements of the reference's
// Attention.forward -- softmax(q^T k * scale) applied to v, plus the positional branch -- on the qkv convolution's output WHERE
// IT IS: [B][nh][32 q | 32 k | 64 v][N], every row N contiguous elements.  No [N][N] array exists anywhere; the library's first
// matrix instructions.
//
// One MMA step for the three dtypes (mma16): acc[16x16] += A[16x16] * B[16x16] per wavefront, lane l = 16 * g + c holding
// a[t] = A[c][4g + t], b[t] = B[4g + t][c] and acc[r] = C[4g + r][c].  bf16 / fp16: one v_mfma_f32_16x16x16; fp32: four chained
// v_mfma_f32_16x16x4_f32, one per t (the sum over k has no order in the contract).  An accumulator IS a B operand after a dtype
// conversion, so every product below is (an operand tile read from LDS) x (registers), and a score tile never passes LDS.
//
// One kernel body, three modes.  Grid (tiles of 64 "outer" positions, nh, B), 256 threads; wavefront w owns 16 outer positions
// (lane column c) and keeps their operand fragments in registers.  The workgroup walks the "inner" positions in blocks of 64: two
// row groups X1 [32][64] and X2 [64][64] are staged per block in LDS -- loads coalesced along N, one element per lane, columns
// beyond N zero-filled, double-buffered with one barrier per block -- and all four wavefronts read their A fragments from there
// in two patterns: by column (a[t] = X[4g + t + 16 s][col], a transposed tile) and by row (a[t] = X[row][col + 4g + t], one
// 8- or 16-byte read).  The ragged tail lives in the staging and in one mask on the score tile; tail outer positions are not
// stored.  The row misalignment of N % 4 != 0 never matters: no global access is wider than an element.
//   forward   outer = queries (Q in registers), inner = keys (X1 = K, X2 = V).  T = S^T[j][i] = X1^T Q; online softmax down the
//             columns (over r in registers and lanes l, l ^ 16, l ^ 32); O^T[e][i] += X2 (by row) * P^T.
//   bwd, dQ   outer = queries (Q, dO in registers), inner = keys, walked twice: sweep 0 D_i = sum_j P dP with P = exp(s - lse),
//             dP^T = X2^T dO; sweep 1 dS^T = P (dP - D), dQ += X1 (by row) * dS^T.  Writes D for the second launch.
//   bwd, dKV  outer = keys (K, V in registers), inner = queries (X1 = Q, X2 = dO, and their lse and D staged beside them):
//             T = S[i][j], dP = X2^T V, dV += X2 (by row) * P, dK += X1 (by row) * dS.
// No atomics, every global word has one writer, fixed summation order: the same bits at every call.
#include "od_common.hpp"

namespace mhaq {

constexpr int kAtDk = 32, kAtDh = 64;               // the only compiled head sizes (every YOLOv11 width has them)
constexpr int kAtRows = 2 * kAtDk + kAtDh;          // qkv rows per head
constexpr int kAtTile = 64;                         // outer positions per workgroup = inner positions per staged block
constexpr int kAtStage = kAtDk + kAtDh;             // staged rows per block: X1 then X2
constexpr int kAtMaxN = 16384;
enum { kAtFwd = 0, kAtBwdQ = 1, kAtBwdKV = 2 };

// element, fragment and padded LDS row of a dtype.  rs * sizeof(elem) is a multiple of the by-row read (16 / 8 bytes); fp32:
// 4 * rs = 16 mod 32 banks, so the four lane groups of a by-column read fall on two disjoint bank halves
template <int DT> struct AtT { typedef uint16_t elem; typedef io16::vu2 frag; static constexpr int rs = 72; };
template <> struct AtT<MHAQ_FQ_DT_F32> { typedef float elem; typedef vf4 frag; static constexpr int rs = 68; };

template <int DT>
__device__ __forceinline__ typename AtT<DT>::frag at_pack(typename AtT<DT>::elem e0, typename AtT<DT>::elem e1,
                                                          typename AtT<DT>::elem e2, typename AtT<DT>::elem e3) {
  if constexpr (DT == MHAQ_FQ_DT_F32) return vf4{e0, e1, e2, e3};
  else return io16::vu2{(uint32_t)e0 | ((uint32_t)e1 << 16), (uint32_t)e2 | ((uint32_t)e3 << 16)};
}
// an accumulator tile as the B operand of the next product: fp32 as it is, 16-bit rounded once to nearest-even
template <int DT>
__device__ __forceinline__ typename AtT<DT>::frag at_operand(vf4 p) {
  if constexpr (DT == MHAQ_FQ_DT_F32) return p;
  else return io16::vu2{io16::down2<DT>(p.x, p.y), io16::down2<DT>(p.z, p.w)};
}
template <int DT>
__device__ __forceinline__ vf4 mma16(vf4 acc, typename AtT<DT>::frag a, typename AtT<DT>::frag b) {
  if constexpr (DT == MHAQ_FQ_DT_F32) {
#pragma unroll
    for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], b[t], acc, 0, 0, 0);
    return acc;
  } else if constexpr (DT == MHAQ_FQ_DT_BF16) {
    typedef short s4 __attribute__((ext_vector_type(4)));
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s4, a), __builtin_bit_cast(s4, b), acc, 0, 0, 0);
  } else {
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    return __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(h4, a), __builtin_bit_cast(h4, b), acc, 0, 0, 0);
  }
}

template <int DT>
__device__ __forceinline__ typename AtT<DT>::elem at_ld(const void* p, int64_t i, bool valid) {
  typedef typename AtT<DT>::elem E;
  return valid ? *gptr(static_cast<const E*>(p) + i) : (E)0;
}
// the B fragment of slice s of a [16 s' rows][N] operand for outer column o: b[t] = Y[16 s + 4g + t][o]
template <int DT>
__device__ __forceinline__ typename AtT<DT>::frag at_outer_frag(const void* y, int64_t n, int s, int g, int o, bool valid) {
  const int64_t base = (int64_t)(16 * s + 4 * g) * n + o;
  return at_pack<DT>(at_ld<DT>(y, base, valid), at_ld<DT>(y, base + n, valid), at_ld<DT>(y, base + 2 * n, valid),
                     at_ld<DT>(y, base + 3 * n, valid));
}
// A fragments from a staged row group x ([rows][rs]): by column and by row (col + 4g a multiple of 4: aligned)
template <int DT>
__device__ __forceinline__ typename AtT<DT>::frag at_frag_col(const typename AtT<DT>::elem* x, int s, int g, int col) {
  constexpr int rs = AtT<DT>::rs;
  const typename AtT<DT>::elem* p = x + (16 * s + 4 * g) * rs + col;
  return at_pack<DT>(p[0], p[rs], p[2 * rs], p[3 * rs]);
}
template <int DT>
__device__ __forceinline__ typename AtT<DT>::frag at_frag_row(const typename AtT<DT>::elem* x, int row, int col) {
  return *reinterpret_cast<const typename AtT<DT>::frag*>(x + row * AtT<DT>::rs + col);
}

__device__ __forceinline__ float at_col_max(float v) {      // over the four lanes of a column: l, l ^ 16, l ^ 32
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float at_col_sum(float v) {      // commutative at both steps: the same bits in all four lanes
  v = v + __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// rows [row0 + 16 t + 4g + r][o] of a [.][n] tensor from T accumulator tiles, times mul (+ addend): 16 lanes along N per store
template <int DT, int T>
__device__ __forceinline__ void at_store(void* dst, const void* addend, int64_t n, int row0, int g, int o, bool valid,
                                         const vf4 (&acc)[T], float mul) {
  if (!valid) return;
#pragma unroll
  for (int t = 0; t < T; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t i = (int64_t)(row0 + 16 * t + 4 * g + r) * n + o;
      float v = acc[t][r] * mul;
      if (addend) v = v + iox::ld1<DT>(addend, i);
      iox::st1<DT>(dst, i, v);
    }
  }
}

// qkv [B][nh][128][n]; go (backward) and addend (forward, nullable) [B][nh][64][n]; dst = out [B][nh][64][n] (forward) or
// d qkv [B][nh][128][n] (backward); lse, dvec [B][nh][n] fp32
template <int DT, int MODE>
__global__ __launch_bounds__(kBlock) void od_attn_kernel(const void* __restrict__ qkv, const void* __restrict__ go,
                                                         const void* __restrict__ addend, void* __restrict__ dst,
                                                         float* __restrict__ lse, float* __restrict__ dvec, int n, int nh,
                                                         float scale) {
  typedef typename AtT<DT>::elem E;
  typedef typename AtT<DT>::frag F;
  constexpr int rs = AtT<DT>::rs;
  constexpr bool kBwd = MODE != kAtFwd, kKV = MODE == kAtBwdKV;
  __shared__ __attribute__((aligned(16))) E sx[2][kAtStage][rs];
  __shared__ float ss[2][2][kAtTile];                         // dKV: lse and D of the staged queries
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
  const int64_t bh = (int64_t)blockIdx.z * nh + blockIdx.y, nn = n;
  const E* q_p = static_cast<const E*>(qkv) + bh * kAtRows * nn;
  const E* k_p = q_p + kAtDk * nn;
  const E* v_p = k_p + kAtDk * nn;
  const E* g_p = kBwd ? static_cast<const E*>(go) + bh * kAtDh * nn : nullptr;
  const E* x1_p = kKV ? q_p : k_p;                            // staged, 32 rows
  const E* x2_p = kKV ? g_p : v_p;                            // staged, 64 rows
  const int o = (int)blockIdx.x * kAtTile + wave * 16 + c;    // this lane's outer position
  const bool ov = o < n;

  F b1[2], b2[4];                                             // the outer operands: Q | K, and dO | V (backward)
#pragma unroll
  for (int s = 0; s < 2; ++s) b1[s] = at_outer_frag<DT>(kKV ? k_p : q_p, nn, s, g, o, ov);
  if constexpr (kBwd) {
#pragma unroll
    for (int s = 0; s < 4; ++s) b2[s] = at_outer_frag<DT>(kKV ? v_p : g_p, nn, s, g, o, ov);
  }

  // staging: lane = column of the block, wavefront w takes rows w, w + 4, ... of both groups
  E pre[kAtStage / 4];
  float pre_s = 0.f;
  auto fetch = [&](int blk) {
    const int col = blk * kAtTile + lane;
    const bool v = col < n;
#pragma unroll
    for (int k = 0; k < kAtDk / 4; ++k) pre[k] = at_ld<DT>(x1_p, (int64_t)(wave + 4 * k) * nn + col, v);
#pragma unroll
    for (int k = 0; k < kAtDh / 4; ++k) pre[kAtDk / 4 + k] = at_ld<DT>(x2_p, (int64_t)(wave + 4 * k) * nn + col, v);
    if constexpr (kKV) {                                      // a tail query: lse = +inf makes its P zero
      if (wave == 0) pre_s = v ? ldg(lse + bh * nn + col) : INFINITY;
      if (wave == 1) pre_s = v ? ldg(dvec + bh * nn + col) : 0.f;
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int k = 0; k < kAtStage / 4; ++k) sx[buf][wave + 4 * k][lane] = pre[k];
    if constexpr (kKV) {
      if (wave < 2) ss[buf][wave][lane] = pre_s;
    }
  };

  const vf4 zero4 = {0.f, 0.f, 0.f, 0.f};
  vf4 acc1[2] = {zero4, zero4};                               // dQ | dK
  vf4 acc2[4] = {zero4, zero4, zero4, zero4};                 // O^T | dV
  float m_run = -INFINITY, l_run = 0.f;                       // forward: running maximum, this lane's share of the sum
  float d_run = 0.f;                                          // dQ: this lane's share of D, then D
  const float lse_o = (MODE == kAtBwdQ && ov) ? ldg(lse + bh * nn + o) : 0.f;

  const int nblk = (n + kAtTile - 1) / kAtTile, iters = MODE == kAtBwdQ ? 2 * nblk : nblk;
  fetch(0);
  stash(0);
  __syncthreads();
  for (int it = 0; it < iters; ++it) {
    const int cur = it & 1, blk = it >= nblk ? it - nblk : it;
    const bool more = it + 1 < iters;
    if (more) fetch(it + 1 >= nblk ? it + 1 - nblk : it + 1);
    const E* x1 = &sx[cur][0][0];
    const E* x2 = &sx[cur][kAtDk][0];
    if (MODE == kAtBwdQ && it == nblk) d_run = at_col_sum(d_run);

    if constexpr (MODE == kAtFwd) {
      vf4 s[4];
      float mx = -INFINITY;
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        vf4 t = zero4;
#pragma unroll
        for (int dd = 0; dd < 2; ++dd) t = mma16<DT>(t, at_frag_col<DT>(x1, dd, g, jt * 16 + c), b1[dd]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          s[jt][r] = blk * kAtTile + jt * 16 + 4 * g + r < n ? t[r] * scale : -INFINITY;
          mx = fmaxf(mx, s[jt][r]);
        }
      }
      const float m_new = fmaxf(m_run, at_col_max(mx));       // finite: every block has a valid key
      const float alpha = expf(m_run - m_new);
      m_run = m_new;
      l_run = l_run * alpha;
#pragma unroll
      for (int et = 0; et < 4; ++et) acc2[et] = acc2[et] * alpha;
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        vf4 p;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          p[r] = expf(s[jt][r] - m_new);
          l_run = l_run + p[r];
        }
        const F pf = at_operand<DT>(p);
#pragma unroll
        for (int et = 0; et < 4; ++et) acc2[et] = mma16<DT>(acc2[et], at_frag_row<DT>(x2, et * 16 + c, jt * 16 + 4 * g), pf);
      }
    } else {
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        vf4 t = zero4, dp = zero4, p, ds;
#pragma unroll
        for (int dd = 0; dd < 2; ++dd) t = mma16<DT>(t, at_frag_col<DT>(x1, dd, g, jt * 16 + c), b1[dd]);
#pragma unroll
        for (int ee = 0; ee < 4; ++ee) dp = mma16<DT>(dp, at_frag_col<DT>(x2, ee, g, jt * 16 + c), b2[ee]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int li = jt * 16 + 4 * g + r;                 // the inner position of accumulator row r
          if constexpr (kKV) {
            p[r] = expf(t[r] * scale - ss[cur][0][li]);
            ds[r] = p[r] * (dp[r] - ss[cur][1][li]);
          } else {
            p[r] = blk * kAtTile + li < n ? expf(t[r] * scale - lse_o) : 0.f;
            ds[r] = p[r] * (dp[r] - d_run);                   // read in sweep 1 only, where d_run is D
            if (it < nblk) d_run = d_run + p[r] * dp[r];
          }
        }
        if (kKV || it >= nblk) {
          const F dsf = at_operand<DT>(ds);
#pragma unroll
          for (int dt = 0; dt < 2; ++dt) acc1[dt] = mma16<DT>(acc1[dt], at_frag_row<DT>(x1, dt * 16 + c, jt * 16 + 4 * g), dsf);
        }
        if constexpr (kKV) {
          const F pf = at_operand<DT>(p);
#pragma unroll
          for (int et = 0; et < 4; ++et) acc2[et] = mma16<DT>(acc2[et], at_frag_row<DT>(x2, et * 16 + c, jt * 16 + 4 * g), pf);
        }
      }
    }
    if (more) stash(cur ^ 1);
    __syncthreads();
  }

  if constexpr (MODE == kAtFwd) {
    const float l = at_col_sum(l_run);
#pragma unroll
    for (int et = 0; et < 4; ++et) acc2[et] = acc2[et] / l;
    at_store<DT, 4>(static_cast<E*>(dst) + bh * kAtDh * nn, addend ? static_cast<const E*>(addend) + bh * kAtDh * nn : nullptr,
                    nn, 0, g, o, ov, acc2, 1.f);
    if (lse && ov && g == 0) stg(lse + bh * nn + o, m_run + logf(l));
  } else if constexpr (MODE == kAtBwdQ) {
    at_store<DT, 2>(static_cast<E*>(dst) + bh * kAtRows * nn, nullptr, nn, 0, g, o, ov, acc1, scale);
    if (ov && g == 0) stg(dvec + bh * nn + o, d_run);
  } else {
    at_store<DT, 2>(static_cast<E*>(dst) + bh * kAtRows * nn, nullptr, nn, kAtDk, g, o, ov, acc1, scale);
    at_store<DT, 4>(static_cast<E*>(dst) + bh * kAtRows * nn, nullptr, nn, 2 * kAtDk, g, o, ov, acc2, 1.f);
  }
}

// ---------------------------------------------------------------- host
// the shape of a call, checked -> 0 or an error code; *empty when nothing is to be launched
static int at_shape_check(int dtype, int64_t b, int64_t nh, int64_t n, int dk, int dh, bool* empty) {
  if (!iox::known_dtype(dtype) || b < 0 || nh < 1 || n < 0 || dk < 1 || dh < 1) return MHAQ_FQ_EINVAL;
  if (dk != kAtDk || dh != kAtDh || n > kAtMaxN || nh > 65535 || b > 65535) return MHAQ_FQ_EUNSUPPORTED;
  *empty = b * n == 0;
  return 0;
}
static bool at_misaligned(const void* p, int dtype) { return ((uintptr_t)p & (uintptr_t)(iox::esize(dtype) - 1)) != 0; }
static float at_scale(int dk) { return (float)(1.0 / sqrt((double)dk)); }      // dim_key ** -0.5, rounded once as aten does

template <int MODE>
static int at_launch(int dtype, int64_t b, int64_t nh, int64_t n, int dk, const void* qkv, const void* go, const void* addend,
                     void* dst, float* lse, float* dvec, hipStream_t st) {
  const dim3 grid((unsigned)((n + kAtTile - 1) / kAtTile), (unsigned)nh, (unsigned)b);
  iox::with_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    MHAQ_LAUNCH((od_attn_kernel<DT, MODE>), grid, dim3(kBlock), 0, st, qkv, go, addend, dst, lse, dvec, (int)n, (int)nh,
                at_scale(dk));
  });
  return launch_status();
}

}  // namespace mhaq

using namespace mhaq;

extern "C" {

int mhaq_fq_od_attn_fwd(const void* qkv, const void* addend, int dtype, int64_t b, int64_t nh, int64_t n, int dk, int dh,
                        void* out, float* lse, void* stream) {
  bool empty = false;
  const int rc = at_shape_check(dtype, b, nh, n, dk, dh, &empty);
  if (rc != 0) return rc;
  if (empty) return 0;
  if (!qkv || !out) return MHAQ_FQ_EINVAL;
  if (at_misaligned(qkv, dtype) || at_misaligned(addend, dtype) || at_misaligned(out, dtype) || ((uintptr_t)lse & 3))
    return MHAQ_FQ_EALIGN;
  return at_launch<kAtFwd>(dtype, b, nh, n, dk, qkv, nullptr, addend, out, lse, nullptr, (hipStream_t)stream);
}

size_t mhaq_fq_od_attn_bwd_workspace_bytes(int64_t b, int64_t nh, int64_t n) {
  if (b < 1 || nh < 1 || n < 1 || b > 65535 || nh > 65535 || n > kAtMaxN) return 0;
  return (size_t)b * (size_t)nh * (size_t)n * sizeof(float);
}

int mhaq_fq_od_attn_bwd(const void* qkv, const void* grad_out, const float* lse, int dtype, int64_t b, int64_t nh, int64_t n,
                        int dk, int dh, void* grad_qkv, void* workspace, size_t workspace_bytes, void* stream) {
  bool empty = false;
  int rc = at_shape_check(dtype, b, nh, n, dk, dh, &empty);
  if (rc != 0) return rc;
  if (empty) return 0;
  if (!qkv || !grad_out || !lse || !grad_qkv || !workspace) return MHAQ_FQ_EINVAL;
  if (at_misaligned(qkv, dtype) || at_misaligned(grad_out, dtype) || at_misaligned(grad_qkv, dtype) || ((uintptr_t)lse & 3) ||
      ((uintptr_t)workspace & 3))
    return MHAQ_FQ_EALIGN;
  if (workspace_bytes < mhaq_fq_od_attn_bwd_workspace_bytes(b, nh, n)) return MHAQ_FQ_EWORKSPACE;
  const hipStream_t st = (hipStream_t)stream;
  float* dvec = static_cast<float*>(workspace);
  float* lse_rw = const_cast<float*>(lse);                    // the kernels only read it
  if ((rc = at_launch<kAtBwdQ>(dtype, b, nh, n, dk, qkv, grad_out, nullptr, grad_qkv, lse_rw, dvec, st)) != 0) return rc;
  return at_launch<kAtBwdKV>(dtype, b, nh, n, dk, qkv, grad_out, nullptr, grad_qkv, lse_rw, dvec, st);
}

}  // extern "C"
