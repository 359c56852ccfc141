// Backward of training-mode BatchNorm for gfx950, dense fp32 NHWC seen as [M = N*H*W][C], C % 4 == 0.
//
// The forward stays with the framework (it saves the batch mean and invstd); this file replaces the three launches of
// its backward with three bandwidth-bound ones:
//   bn_bwd_reduce_kernel     one read of x and dy   -> per-block fp64 partial rows of  sum dy  and  sum dy * (x - mean)
//   bn_bwd_finalize_kernel   fixed-order fp64 sum of the partial rows -> dbias, dweight, per-channel constants
//   bn_bwd_dx_kernel         a 2R1W stream in the shape of pt_bwd_kernel (fq_pt.hip):
//                            dx = (gamma * invstd) * ((dy - dbias / M) - ((x - mean) * invstd) * (dweight / M))
// The mean is NOT folded into an additive constant (B * x + D cancels when |mean| >> sigma): every term above is the
// closed form's own, so the error of dx is bounded on |dy| + |dbias| / M + |xhat| * |dweight| / M.
// Deterministic: fixed partition, fixed-order sums, no float atomics, no last-block ticket.
#include "fq_common.hpp"

namespace mhaq {

// 16 B / lane accesses with the cache policy as a template argument (as ld4 / st4 of fq_pt.hip)
template <bool NT>
__device__ __forceinline__ vf4 bn_ld4(const float* p, int64_t vidx) {
  const vf4* q = reinterpret_cast<const vf4*>(p) + vidx;
  return NT ? __builtin_nontemporal_load(q) : *q;
}
__device__ __forceinline__ void bn_st4(float* p, int64_t vidx, vf4 v) {
  __builtin_nontemporal_store(v, reinterpret_cast<vf4*>(p) + vidx);
}

// ---------------------------------------------------------------- geometry of the reduction
// A block of the reduction owns `rows` consecutive rows of up to kBnCols float4 columns (64 channels: 256 contiguous
// bytes of a row, two whole cache lines; narrower tensors are read as one contiguous range).  Its 256 threads form
// 256 / cols rows of lanes; a lane keeps its 4 channels and walks down the rows, kBnRedU rows in flight per stream.
//   rows >= kBnMinRows: the partial rows ([2][C] doubles per row chunk) stay below 4 / 448 = 0.9 % of the tensor's bytes
//   row chunks <= kBnMaxChunks: a few rows per thread for the finalize
// The column split buys blocks where the 1 % rule leaves few row chunks: [12250][512] is 28 row chunks x 8 column chunks.
constexpr int kBnCols = 16;
constexpr int kBnRedU = 4;
constexpr int kBnMinRows = 448;
constexpr int kBnMaxChunks = 2048;
constexpr int kBnDxU = 2;             // float4 per lane and stream in the dx kernel (kBwdU of fq_pt.hip)
constexpr int64_t kBnMaxChannels = 1ll << 22;
constexpr int kBnNConst = 5;          // per-channel constants of the dx kernel: mean, invstd, gamma * invstd, dbias / M, dweight / M

struct BnGeom {
  int64_t rows;      // rows per block
  int64_t nchunks;   // grid.x
  int ncol;          // grid.y
};
static inline BnGeom bn_geom(int64_t m, int64_t c) {
  const int64_t cv = c >> 2;
  const int64_t cols = cv < kBnCols ? cv : kBnCols;
  const int64_t rpp = kBlock / cols;                       // rows per pass of a block
  const int64_t unit = rpp * kBnRedU;
  int64_t rows = (m + kBnMaxChunks - 1) / kBnMaxChunks;
  if (rows < kBnMinRows) rows = kBnMinRows;
  rows = (rows + unit - 1) / unit * unit;
  BnGeom g;
  g.rows = rows;
  g.nchunks = (m + rows - 1) / rows;
  g.ncol = (int)((cv + kBnCols - 1) / kBnCols);
  return g;
}

// Cache policy of the loads, by tensor size and pass (measured per size, docs/NOTEBOOK.md section 6 "BatchNorm backward").
// x and dy are read twice within three launches.  Below kBnReduceNtElems the first read loads with the default policy
// (the lines stay in the 256 MiB Infinity Cache for the second read), from there up it streams through non-temporally;
// the second read is non-temporal from kBnDxNtElems up.  Stores of dx are non-temporal at every size.
constexpr int64_t kBnReduceNtElems = 28ll << 20;
constexpr int64_t kBnDxNtElems = 28ll << 20;
// occupancy of the dx kernel by size: the rule of pt_bwd_kernel (fq_pt.hip)
constexpr int64_t kBnBigElems = 20ll << 20;
constexpr int kBnMinWaves = 8, kBnBigMaxWaves = 6;

// ---------------------------------------------------------------- 1. partial sums
// partials[chunk][2][C] (fp64): row 0 = sum dy, row 1 = sum dy * (x - mean) over the chunk's rows.
// Every sum is fp64 from the product on -- x - mean and dy * (x - mean) are exact in fp64 --, per lane, across the block
// and in the partial rows.  The reason is dx, not dweight / dbias themselves: dx subtracts dbias / M and xhat * dweight / M
// from dy, and its bound is stated on |dbias| and |dweight| AFTER the cancellation in their sums.  In a channel whose sum
// nearly cancels (some always do among 64-512 channels: |sum| ~ M^1/2 |term| or less) an fp32 rounding anywhere on the way
// -- 6e-8 of a product, of a lane's or a block's subtotal -- is an error of 6e-8 M^1/2 |term|, several 1e-6 of that |sum|;
// the framework's fp32 sums measure 3e-6 to 6e-6 of the bound's term sum at M = 245 ... 25 088 for that reason.  fp64 adds
// run at the fp32 rate on this chip and the kernel stays memory-bound (20 VALU operations per 32 loaded bytes).
template <bool NT>
__global__ __launch_bounds__(kBlock) void bn_bwd_reduce_kernel(
    const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ mean,
    double* __restrict__ partials, int64_t m, int cv, int64_t rows) {
  const int c0 = (int)blockIdx.y * kBnCols;
  const int cols = (cv - c0) < kBnCols ? (cv - c0) : kBnCols;
  const int rpp = kBlock / cols;
  const int ty = (int)(threadIdx.x / (uint32_t)cols), tx = (int)threadIdx.x - ty * cols;
  const bool live = ty < rpp;                                  // 256 % cols lanes idle (C = 20: one)
  const int64_t row0 = (int64_t)blockIdx.x * rows;
  const int64_t rend = (row0 + rows < m) ? row0 + rows : m;    // > row0: the grid has ceil(m / rows) chunks
  const int64_t colv = c0 + tx;
  float mu[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) mu[j] = mean[colv * 4 + j];
  double s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
  for (int64_t rb = row0 + ty; rb - ty < rend; rb += (int64_t)rpp * kBnRedU) {
    // unconditional, clamped loads: all 2 * U in flight before anything waits; lanes past the chunk's end re-read its
    // last row and drop it
    vf4 a[kBnRedU], b[kBnRedU];
    bool ok[kBnRedU];
#pragma unroll
    for (int u = 0; u < kBnRedU; ++u) {
      const int64_t r = rb + (int64_t)u * rpp;
      ok[u] = live && r < rend;
      const int64_t vidx = (ok[u] ? r : rend - 1) * cv + colv;
      a[u] = bn_ld4<NT>(x, vidx);
      b[u] = bn_ld4<NT>(dy, vidx);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < kBnRedU; ++u) {
      const float av[4] = {a[u].x, a[u].y, a[u].z, a[u].w}, bv[4] = {b[u].x, b[u].y, b[u].z, b[u].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double g = ok[u] ? (double)bv[j] : 0.0;          // a select, not a product: a dropped NaN stays dropped
        const double d = ok[u] ? (double)av[j] - (double)mu[j] : 0.0;
        s1[j] += g;
        s2[j] = fma(g, d, s2[j]);
      }
    }
  }
  // across the block's rows of lanes: LDS [ty][2][4 * cols], then thread (k, c) adds its column in row order
  __shared__ __align__(16) double sm[kBlock * 8];
  const int w = 4 * cols;
  if (live) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sm[(ty * 2 + 0) * w + tx * 4 + j] = s1[j];
      sm[(ty * 2 + 1) * w + tx * 4 + j] = s2[j];
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < 2 * w) {
    const int k = (int)threadIdx.x >= w ? 1 : 0, c = (int)threadIdx.x - k * w;
    double tot = 0.0;
    for (int r = 0; r < rpp; ++r) tot += sm[(r * 2 + k) * w + c];
    partials[((int64_t)blockIdx.x * 2 + k) * ((int64_t)cv * 4) + (int64_t)c0 * 4 + c] = tot;
  }
}

// ---------------------------------------------------------------- 2. fixed-order final sums and the constants of dx
// One block per group of 4 channels: thread t adds the partial rows t, t + 256, ... , block_sum adds the threads in wave
// and lane order.  consts[5][C] = {mean, invstd, gamma * invstd, dbias / M, dweight / M}: each rounded to fp32 ONCE from
// the fp64 sum.
__global__ __launch_bounds__(kBlock) void bn_bwd_finalize_kernel(
    const double* __restrict__ partials, int nchunks, int c, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ weight, double inv_m, float* __restrict__ consts,
    float* __restrict__ dweight, float* __restrict__ dbias) {
  const int ch = (int)blockIdx.x * 4;
  double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < nchunks; i += kBlock) {
    const double* p0 = partials + ((int64_t)i * 2 + 0) * c + ch;
    const double* p1 = partials + ((int64_t)i * 2 + 1) * c + ch;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] += p0[j];
      v[4 + j] += p1[j];
    }
  }
  __shared__ double sm[8 * (kBlock / 64)];
  block_sum<8>(v, sm);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float is = invstd[ch + j], g = weight ? weight[ch + j] : 1.0f;
      const double db = v[j], dw = (double)is * v[4 + j];
      consts[0 * c + ch + j] = mean[ch + j];
      consts[1 * c + ch + j] = is;
      consts[2 * c + ch + j] = g * is;
      consts[3 * c + ch + j] = (float)(db * inv_m);
      consts[4 * c + ch + j] = (float)(dw * inv_m);
      if (dweight) dweight[ch + j] = (float)dw;
      if (dbias) dbias[ch + j] = (float)db;
    }
  }
}

// ---------------------------------------------------------------- 3. dx
// Block b owns the 256 * U consecutive float4 at b * 256 * U, one pass; data loads first and unconditional (ragged lanes
// clamp their index), the per-channel constants arrive under them.  The column of a float4 is its index modulo C / 4:
// two wave-uniform 32-bit modulos per block, one per lane, a conditional subtract per further float4 -- and no
// second fetch of the constants when 256 % (C / 4) == 0 (every power-of-two width up to 1024 channels).
template <bool NT, bool BIG>
__global__ __attribute__((amdgpu_waves_per_eu((BIG ? 1 : kBnMinWaves), (BIG ? kBnBigMaxWaves : kBnMinWaves))))
__launch_bounds__(kBlock) void bn_bwd_dx_kernel(
    const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx, int64_t nvec, int cv,
    const float* __restrict__ consts) {
  const int64_t blk0 = (int64_t)blockIdx.x * (kBlock * kBnDxU);
  const int64_t base = blk0 + threadIdx.x;
  const bool full = blk0 + kBlock * kBnDxU <= nvec;
  vf4 a[kBnDxU], b[kBnDxU];
#pragma unroll
  for (int u = 0; u < kBnDxU; ++u) {
    const int64_t idx = base + u * kBlock;
    const int64_t idc = (full || idx < nvec) ? idx : nvec - 1;
    a[u] = bn_ld4<NT>(x, idc);
    b[u] = bn_ld4<NT>(dy, idc);
  }
  __builtin_amdgcn_sched_barrier(0);
  // column of the block's first float4: (b * 512) mod cv from two 32-bit modulos (cv <= 2^20: the product fits)
  const uint32_t ucv = (uint32_t)cv;
  const uint32_t cb = ((blockIdx.x % ucv) * ((uint32_t)(kBlock * kBnDxU) % ucv)) % ucv;      // wave-uniform
  const uint32_t step = (uint32_t)kBlock % ucv;                                               // wave-uniform
  uint32_t col = (cb + threadIdx.x) % ucv;
  const int64_t c = (int64_t)cv * 4;
  float k[kBnNConst][4];
#pragma unroll
  for (int u = 0; u < kBnDxU; ++u) {
    const int64_t idx = base + u * kBlock;
    if (u > 0) {
      col += step;
      if (col >= ucv) col -= ucv;
    }
    if (u == 0 || step != 0) {
#pragma unroll
      for (int q = 0; q < kBnNConst; ++q) ldv<4>(consts + q * c + (int64_t)col * 4, k[q]);
    }
    if (full || idx < nvec) {
      const float xv[4] = {a[u].x, a[u].y, a[u].z, a[u].w}, gv[4] = {b[u].x, b[u].y, b[u].z, b[u].w};
      float o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float xh = (xv[j] - k[0][j]) * k[1][j];
        o[j] = k[2][j] * ((gv[j] - k[3][j]) - xh * k[4][j]);
      }
      bn_st4(dx, idx, vf4{o[0], o[1], o[2], o[3]});
    }
  }
}

static inline bool bn_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace mhaq

using namespace mhaq;

extern "C" {

size_t mhaq_fq_bn_bwd_workspace_bytes(int64_t m, int64_t c) {
  if (m <= 0 || c <= 0 || (c & 3) || c > kBnMaxChannels) return 0;
  return ((size_t)kBnNConst * sizeof(float) + 2 * (size_t)bn_geom(m, c).nchunks * sizeof(double)) * (size_t)c;
}

int mhaq_fq_bn_bwd(const float* x, const float* dy, const float* mean, const float* invstd, const float* weight,
                   float* dx, float* dweight, float* dbias, int64_t m, int64_t c, void* workspace,
                   size_t workspace_bytes, void* stream) {
  if (m <= 0 || c <= 0 || !x || !dy || !mean || !invstd || !workspace) return MHAQ_FQ_EINVAL;
  // C % 4: a lane owns 4 channels; the width bound keeps the column arithmetic of the dx kernel in 32 bits
  if ((c & 3) || c > kBnMaxChannels || m > (INT64_MAX >> 3) / c) return MHAQ_FQ_EUNSUPPORTED;
  if (workspace_bytes < mhaq_fq_bn_bwd_workspace_bytes(m, c)) return MHAQ_FQ_EWORKSPACE;
  if (!bn_aligned(x, 16) || !bn_aligned(dy, 16) || !bn_aligned(dx, 16) || !bn_aligned(workspace, 16) ||
      !bn_aligned(mean, 4) || !bn_aligned(invstd, 4) || !bn_aligned(weight, 4) || !bn_aligned(dweight, 4) ||
      !bn_aligned(dbias, 4))
    return MHAQ_FQ_EALIGN;
  const BnGeom g = bn_geom(m, c);
  const int64_t nvec = m * (c >> 2);
  const int64_t dx_grid = (nvec + kBlock * kBnDxU - 1) / (kBlock * kBnDxU);
  if (g.nchunks > 0x7fffffff || dx_grid > 0x7fffffff) return MHAQ_FQ_EUNSUPPORTED;
  if (!dx && !dweight && !dbias) return 0;
  hipStream_t st = (hipStream_t)stream;
  float* consts = (float*)workspace;
  double* parts = (double*)(consts + kBnNConst * c);      // 20 * c bytes in: 16-byte aligned (c % 4 == 0)
  const int cv = (int)(c >> 2);
  const bool nt_r = m * c >= kBnReduceNtElems, nt_d = m * c >= kBnDxNtElems, big = m * c >= kBnBigElems;
  const dim3 rgrid((unsigned)g.nchunks, (unsigned)g.ncol);
  if (nt_r) MHAQ_LAUNCH(bn_bwd_reduce_kernel<true>, rgrid, dim3(kBlock), 0, st, x, dy, mean, parts, m, cv, g.rows);
  else MHAQ_LAUNCH(bn_bwd_reduce_kernel<false>, rgrid, dim3(kBlock), 0, st, x, dy, mean, parts, m, cv, g.rows);
  int rc = launch_status();
  if (rc) return rc;
  MHAQ_LAUNCH(bn_bwd_finalize_kernel, dim3((unsigned)cv), dim3(kBlock), 0, st, (const double*)parts, (int)g.nchunks,
              (int)c, mean, invstd, weight, 1.0 / (double)m, consts, dweight, dbias);
  rc = launch_status();
  if (rc || !dx) return rc;
  const dim3 dgrid((unsigned)dx_grid);
#define MHAQ_LAUNCH_BN_DX(NT, BG) \
  MHAQ_LAUNCH((bn_bwd_dx_kernel<NT, BG>), dgrid, dim3(kBlock), 0, st, x, dy, dx, nvec, cv, (const float*)consts)
  if (big) { if (nt_d) MHAQ_LAUNCH_BN_DX(true, true); else MHAQ_LAUNCH_BN_DX(false, true); }
  else { if (nt_d) MHAQ_LAUNCH_BN_DX(true, false); else MHAQ_LAUNCH_BN_DX(false, false); }
#undef MHAQ_LAUNCH_BN_DX
  return launch_status();
}

}  // extern "C"
