// Super-resolution validation metrics (mhaq_fq_sr_metrics, include/mhaq_fq.h): per-image PSNR and SSIM of the clamped
// prediction against the target, and the L1 criterion on the unclamped one, in three launches -- where the framework runs
// div, clamp, two luminance mul/sum pairs, sub, square, mean, two average pools, five depthwise 11x11 convolutions and some
// fifteen elementwise maps (about forty launches, a dozen passes over full-resolution images).
//
//   1. prepare  reads s and h ONCE: s' = s / sr_div, |s' - h| and (x - y)^2 partials (fp64), NaN-keeping clamp, the planes
//               (luminance or the channels), the flag bits, and the f x f average-pooled planes xp, yp into the workspace.
//               A workgroup owns a band of G row groups (f rows each) x one column chunk; a lane owns 8 consecutive pixels
//               of every channel (16-byte loads where all row bases of the item allow it, element loads elsewhere).  For
//               f > 1 the f rows of plane values are staged in LDS and pooled from there; f == 1 stores them directly.
//   2. ssim     a workgroup owns a 32 x 32 tile of valid window positions of one plane of one image: the 42 x 42 inputs in
//               LDS, the separable 11-tap Gaussian over x, y, x^2, y^2, x*y horizontally into LDS, then vertically per
//               position, ss in fp32, ONE fp64 partial per workgroup.
//   3. finalize one workgroup: a wave per image sums its partials in a fixed order in fp64, then the block the batch; one
//               rounding per output.
// No atomics, no host synchronisation; the same inputs give the same bits at every call.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/mhaq_fq.h"
#include "fq_common.hpp"
#include "fq_io16.hpp"

namespace mhaq {

constexpr int kSrPx = 8;                          // consecutive pixels of a row per lane
constexpr int kSrMaxChunk = kBlock * kSrPx;       // 2048 pixels: one item per lane
constexpr int kSrLdsFloats = 12288;               // 48 KB of staged plane rows (prepare, f > 1)
constexpr int kSrBandPixels = 2048;               // a workgroup's band holds at least this many pixels when it can

constexpr int kSrTile = 32;                       // valid window positions per tile side
constexpr int kSrWin = 11;
constexpr int kSrIn = kSrTile + kSrWin - 1;       // 42 inputs per tile side

// the luminance weights of the reference: fp32([65.738, 129.057, 25.064]) / 256 (a power of two: exact)
#define MHAQ_SR_K0 (65.738f / 256.0f)
#define MHAQ_SR_K1 (129.057f / 256.0f)
#define MHAQ_SR_K2 (25.064f / 256.0f)

// 11-tap Gaussian, sigma 1.5, normalised to sum 1: computed in fp64, rounded to fp32 once; tap k and tap 10 - k share w[k]
struct SrTaps { float w[6]; };

__host__ __device__ constexpr int sr_esize(int dt) { return dt == MHAQ_FQ_DT_F32 ? 4 : 2; }

struct SrGeom {
  int64_t n, c, h, w;
  int p, f;                 // planes per image, pool factor
  int64_t hp, wp;           // pooled plane
  int chunk, nchunk;        // prepare: pixels per column chunk (a multiple of 8 and of f), chunks per row
  int64_t groups;           // row groups of f rows (the last may be short: the rows the pool drops)
  int band;                 // row groups per workgroup
  int64_t nband;
  int64_t tx, ty;           // ssim tiles per plane
  // workspace layout, bytes
  size_t off_yp, off_part1, off_part2, off_img, off_flags, total;
  int64_t nblk1, nblk2;     // per image
};

inline int64_t sr_gcd(int64_t a, int64_t b) { while (b) { const int64_t t = a % b; a = b; b = t; } return a; }

// 0, or the error the geometry meets (argument checks that need no pointer)
inline int sr_geometry(int64_t n, int64_t c, int64_t h, int64_t w, int to_luminance, int pool, SrGeom& g) {
  if (n <= 0 || c <= 0 || h <= 0 || w <= 0 || pool < 1) return MHAQ_FQ_EINVAL;
  if (to_luminance && c != 3) return MHAQ_FQ_EINVAL;
  if (c != 1 && c != 3) return MHAQ_FQ_EUNSUPPORTED;
  g.n = n; g.c = c; g.h = h; g.w = w;
  g.p = to_luminance ? 1 : (int)c;
  g.f = pool;
  g.hp = h / pool; g.wp = w / pool;
  if (g.hp < kSrWin || g.wp < kSrWin) return MHAQ_FQ_EUNSUPPORTED;
  if (n > 65535 || h > 0x7fffffff || w > 0x7fffffff) return MHAQ_FQ_EUNSUPPORTED;
  // prepare: the chunk is a multiple of lcm(8, f) so that no lane's 8 pixels and no pool window straddles two chunks
  const int64_t unit = (int64_t)kSrPx * pool / sr_gcd(kSrPx, pool);
  int64_t cap = kSrMaxChunk;
  if (pool > 1) cap = std::min<int64_t>(cap, kSrLdsFloats / (2 * (int64_t)g.p * pool));
  const int64_t m = cap / unit;
  if (m < 1) return MHAQ_FQ_EUNSUPPORTED;
  const int64_t need = (w + unit - 1) / unit;                 // units that cover a row
  g.chunk = (int)(std::min(m, need) * unit);
  const int64_t nchunk = (w + g.chunk - 1) / g.chunk;
  g.groups = (h + pool - 1) / pool;
  const int64_t per_group = (int64_t)pool * std::min<int64_t>(g.chunk, w);
  g.band = (int)std::max<int64_t>(1, std::min<int64_t>(g.groups, (kSrBandPixels + per_group - 1) / per_group));
  g.nband = (g.groups + g.band - 1) / g.band;
  if (nchunk > 0x7fffffff || g.nband > 65535) return MHAQ_FQ_EUNSUPPORTED;
  g.nchunk = (int)nchunk;
  g.tx = (g.wp - (kSrWin - 1) + kSrTile - 1) / kSrTile;
  g.ty = (g.hp - (kSrWin - 1) + kSrTile - 1) / kSrTile;
  if (g.tx * g.ty > 0x7fffffff || n * g.p > 65535) return MHAQ_FQ_EUNSUPPORTED;
  g.nblk1 = g.nband * g.nchunk;
  g.nblk2 = (int64_t)g.p * g.tx * g.ty;
  const size_t plane = (((size_t)n * g.p * g.hp * g.wp * sizeof(float)) + 15) & ~(size_t)15;
  g.off_yp = plane;
  g.off_part1 = 2 * plane;
  g.off_part2 = g.off_part1 + (size_t)n * g.nblk1 * 2 * sizeof(double);
  g.off_img = g.off_part2 + (size_t)n * g.nblk2 * sizeof(double);
  g.off_flags = g.off_img + (size_t)n * 3 * sizeof(double);
  g.total = g.off_flags + (((size_t)n * g.nblk1 * sizeof(uint32_t) + 7) & ~(size_t)7);
  return 0;
}

// ---------------------------------------------------------------- launch 1: prepare
template <int DT>
__device__ __forceinline__ float sr_ld1(const void* row, int64_t i) {
  if constexpr (DT == MHAQ_FQ_DT_F32) return ldg(static_cast<const float*>(row) + i);
  else return io16::up1<DT>(*gptr(static_cast<const uint16_t*>(row) + i));
}
// pixels i .. i + 7 of a row whose address at i is 16-byte aligned
template <int DT>
__device__ __forceinline__ void sr_ld8(const void* row, int64_t i, float (&v)[kSrPx]) {
  if constexpr (DT == MHAQ_FQ_DT_F32) {
    float a[4], b[4];
    ldvg<4>(static_cast<const float*>(row) + i, a);
    ldvg<4>(static_cast<const float*>(row) + i + 4, b);
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = a[j]; v[4 + j] = b[j]; }
  } else {
    const io16::vu4 q = *gptr(reinterpret_cast<const io16::vu4*>(static_cast<const uint16_t*>(row) + i));
    io16::up2<DT>(q.x, v[0], v[1]);
    io16::up2<DT>(q.y, v[2], v[3]);
    io16::up2<DT>(q.z, v[4], v[5]);
    io16::up2<DT>(q.w, v[6], v[7]);
  }
}
__device__ __forceinline__ bool sr_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }
// torch.clamp(v, 0, 1): a NaN stays
__device__ __forceinline__ float sr_clamp01(float v) {
  const float t = fminf(fmaxf(v, 0.f), 1.f);
  return (v != v) ? v : t;
}

struct SrPrepArgs {
  const void* s;
  const void* h;
  float* xp;
  float* yp;
  double* part;        // [n][nblk1][2]: sum |s' - h|, sum (x - y)^2
  uint32_t* flags;     // [n][nblk1]
  int64_t H, W, Hp, Wp;
  float div;
  int C, P, f, chunk, band;
};

template <int SDT, int HDT, int C>
__global__ __launch_bounds__(kBlock) void sr_prepare_kernel(const SrPrepArgs a) {
  extern __shared__ __align__(16) float sr_lds[];          // f > 1: [2][P][f][chunk]
  __shared__ double smd[2 * (kBlock / kWave)];
  const int tid = (int)threadIdx.x;
  const int64_t img = blockIdx.z;
  const int64_t c0 = (int64_t)blockIdx.x * a.chunk;        // first pixel column of the chunk
  const int cw = (int)min((int64_t)a.chunk, a.W - c0);     // its width
  const int P = a.P, f = a.f;
  const bool lum = (C == 3 && P == 1);
  const int items = (cw + kSrPx - 1) / kSrPx;              // 8-pixel items per row of the chunk
  const int64_t plane_in = a.H * a.W;
  const char* sb = static_cast<const char*>(a.s) + img * C * plane_in * sr_esize(SDT);
  const char* hb = static_cast<const char*>(a.h) + img * C * plane_in * sr_esize(HDT);
  double acc[2] = {0.0, 0.0};
  uint32_t fl = 0;
  const float k0 = MHAQ_SR_K0, k1 = MHAQ_SR_K1, k2 = MHAQ_SR_K2;

  // f > 1: one pass per row group (its f rows meet in LDS); f == 1: nothing to pool, the band's rows are ONE pass, so that
  // a narrow image still gives every lane an item
  const int grows = (f == 1) ? a.band : f, npass = (f == 1) ? 1 : a.band;
  for (int gi = 0; gi < npass; ++gi) {
    const int64_t g = (int64_t)blockIdx.y * npass + gi;    // f > 1: the row group, rows g * f .. g * f + f - 1
    const int64_t r0 = g * grows;
    if (r0 >= a.H) break;                                  // uniform over the workgroup
    const int rows = (int)min((int64_t)grows, a.H - r0);
    const bool pooled = (f > 1 && g < a.Hp);               // a full group: it has a pooled row
    for (int it = tid; it < rows * items; it += kBlock) {
      const int rl = it / items, ig = it - rl * items;
      const int64_t row = r0 + rl;
      const int64_t px = c0 + (int64_t)ig * kSrPx;         // first pixel of the item
      const int npx = min(kSrPx, (int)(c0 + cw - px));
      float sv[C][kSrPx], hv[C][kSrPx];
      // 16-byte loads where every row base of the item allows it
      bool vec = (npx == kSrPx);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int64_t e = (c * a.H + row) * a.W + px;
        vec = vec && (((uintptr_t)(sb + e * sr_esize(SDT)) & 15) == 0) && (((uintptr_t)(hb + e * sr_esize(HDT)) & 15) == 0);
      }
      if (vec) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const int64_t e = (c * a.H + row) * a.W + px;
          sr_ld8<SDT>(sb, e, sv[c]);
          sr_ld8<HDT>(hb, e, hv[c]);
        }
      } else {
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const int64_t e = (c * a.H + row) * a.W + px;
#pragma unroll
          for (int j = 0; j < kSrPx; ++j) {
            sv[c][j] = (j < npx) ? sr_ld1<SDT>(sb, e + j) : 0.f;
            hv[c][j] = (j < npx) ? sr_ld1<HDT>(hb, e + j) : 0.f;
          }
        }
      }
      float xv[C][kSrPx], yv[C][kSrPx];                    // plane values; [0] alone with luminance
#pragma unroll
      for (int j = 0; j < kSrPx; ++j) {
        if (j < npx) {
          float cl[C];
#pragma unroll
          for (int c = 0; c < C; ++c) {
            const float sp = sv[c][j] / a.div;             // IEEE division
            const float hh = hv[c][j];
            if (sr_nonfinite(sp) || sr_nonfinite(hh)) fl |= 1u;
            acc[0] += (double)fabsf(sp - hh);
            cl[c] = sr_clamp01(sp);
          }
          if (lum) {
            xv[0][j] = (cl[0] * k0 + cl[C > 1 ? 1 : 0] * k1) + cl[C > 2 ? 2 : 0] * k2;
            yv[0][j] = (hv[0][j] * k0 + hv[C > 1 ? 1 : 0][j] * k1) + hv[C > 2 ? 2 : 0][j] * k2;
          } else {
#pragma unroll
            for (int c = 0; c < C; ++c) { xv[c][j] = cl[c]; yv[c][j] = hv[c][j]; }
          }
#pragma unroll
          for (int p = 0; p < C; ++p) {
            if (p < P) {
              const float d = xv[p][j] - yv[p][j];
              acc[1] += (double)(d * d);
              if (yv[p][j] < 0.f || yv[p][j] > 1.f) fl |= 2u;
            }
          }
        } else {
#pragma unroll
          for (int p = 0; p < C; ++p) { xv[p][j] = 0.f; yv[p][j] = 0.f; }
        }
      }
      if (f == 1) {
        // the planes themselves: Hp == H, Wp == W
#pragma unroll
        for (int p = 0; p < C; ++p) {
          if (p < P) {
            const int64_t o = ((img * P + p) * a.Hp + row) * a.Wp + px;
            if (npx == kSrPx && (((uintptr_t)(a.xp + o) & 15) == 0)) {   // yp - xp is a multiple of 16 bytes
              stvg<4>(a.xp + o, reinterpret_cast<const float(&)[4]>(xv[p][0]));
              stvg<4>(a.xp + o + 4, reinterpret_cast<const float(&)[4]>(xv[p][4]));
              stvg<4>(a.yp + o, reinterpret_cast<const float(&)[4]>(yv[p][0]));
              stvg<4>(a.yp + o + 4, reinterpret_cast<const float(&)[4]>(yv[p][4]));
            } else {
#pragma unroll
              for (int j = 0; j < kSrPx; ++j)
                if (j < npx) { stg(a.xp + o + j, xv[p][j]); stg(a.yp + o + j, yv[p][j]); }
            }
          }
        }
      } else if (pooled) {
        // stage: chunk is a multiple of 8, so a lane's 8 floats are 32-byte aligned in LDS
#pragma unroll
        for (int p = 0; p < C; ++p) {
          if (p < P) {
            float* lx = sr_lds + ((0 * P + p) * f + rl) * a.chunk + ig * kSrPx;
            float* ly = sr_lds + ((1 * P + p) * f + rl) * a.chunk + ig * kSrPx;
            stv<4>(lx, reinterpret_cast<const float(&)[4]>(xv[p][0]));
            stv<4>(lx + 4, reinterpret_cast<const float(&)[4]>(xv[p][4]));
            stv<4>(ly, reinterpret_cast<const float(&)[4]>(yv[p][0]));
            stv<4>(ly + 4, reinterpret_cast<const float(&)[4]>(yv[p][4]));
          }
        }
      }
    }
    if (f > 1) {
      __syncthreads();
      if (pooled) {
        // pooled columns of this chunk: windows in row-major order, one division
        const int64_t pc0 = c0 / f;
        const int npc = (int)min((int64_t)(a.chunk / f), a.Wp - pc0);
        const float area = (float)(f * f);
        for (int q = tid; q < npc * 2 * P; q += kBlock) {
          const int which = q / npc, j = q - which * npc;  // which = side * P + plane
          const float* src = sr_lds + (which * f) * a.chunk + j * f;
          float sum = 0.f;
          for (int rr = 0; rr < f; ++rr)
            for (int cc = 0; cc < f; ++cc) sum += src[rr * a.chunk + cc];
          const int side = which / P, p = which - side * P;
          float* dst = side ? a.yp : a.xp;
          stg(dst + ((img * P + p) * a.Hp + g) * a.Wp + pc0 + j, sum / area);
        }
      }
      __syncthreads();
    }
  }
  const int any0 = __syncthreads_or((int)(fl & 1u));
  const int any1 = __syncthreads_or((int)(fl & 2u));
  block_sum<2>(acc, smd);
  if (tid == 0) {
    const int64_t b = (img * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    a.part[2 * b] = acc[0];
    a.part[2 * b + 1] = acc[1];
    *gptr(a.flags + b) = (any0 ? 1u : 0u) | (any1 ? 2u : 0u);
  }
}

// ---------------------------------------------------------------- launch 2: SSIM tiles
// w[0] * (q0 + q10), then the pairs inwards and the centre tap, each one fused multiply-add: the SAME operations in the same
// order for every quantity, so equal inputs give equal bits
__device__ __forceinline__ float sr_taps11(const float (&q)[kSrWin], const SrTaps& t) {
  float acc = t.w[0] * (q[0] + q[10]);
  acc = __fmaf_rn(t.w[1], q[1] + q[9], acc);
  acc = __fmaf_rn(t.w[2], q[2] + q[8], acc);
  acc = __fmaf_rn(t.w[3], q[3] + q[7], acc);
  acc = __fmaf_rn(t.w[4], q[4] + q[6], acc);
  acc = __fmaf_rn(t.w[5], q[5], acc);
  return acc;
}

// LDS pitches.  Every access of both passes is one dword per lane in which the 32 lanes of a half-wave (the unit in which
// ds_read_b32 / ds_write_b32 meet bank conflicts, bank = dword address mod 32) address 32 CONSECUTIVE dwords of ONE row:
// horizontal pass lanes = 32 output columns of one input row, vertical pass lanes = the 32 columns of one output row, tap k
// moves the whole half-wave by k dwords (horizontal) or k rows (vertical).  32 consecutive dwords are 32 different banks
// whatever the row's base, so no pitch can produce a conflict and none is padded: the input rows keep their 42 dwords, the
// filtered rows their 32.
constexpr int kSrInPitch = kSrIn;        // 42
constexpr int kSrHPitch = kSrTile;       // 32

__global__ __launch_bounds__(kBlock) void sr_ssim_kernel(const float* __restrict__ xp, const float* __restrict__ yp,
                                                         int64_t Hp, int64_t Wp, int64_t tiles_x, const SrTaps taps,
                                                         double* __restrict__ part) {
  __shared__ float sx[kSrIn * kSrInPitch], sy[kSrIn * kSrInPitch];       // 2 x 7056 B
  __shared__ float hb[5][kSrIn * kSrHPitch];                             // 26880 B
  __shared__ double smd[kBlock / kWave];
  const int tid = (int)threadIdx.x;
  const int64_t plane = blockIdx.y;                        // img * P + p
  const int64_t tyi = blockIdx.x / tiles_x, txi = blockIdx.x - tyi * tiles_x;
  const int64_t oy0 = tyi * kSrTile, ox0 = txi * kSrTile;  // first valid position of the tile = first input of its halo
  const int64_t Ho = Hp - (kSrWin - 1), Wo = Wp - (kSrWin - 1);
  const int nh = (int)min((int64_t)kSrTile, Ho - oy0), nw = (int)min((int64_t)kSrTile, Wo - ox0);
  const float* xb = xp + plane * Hp * Wp;
  const float* yb = yp + plane * Hp * Wp;
  // The variances are differences of nearly equal numbers (G * x^2 - mx^2 against c2 = 9e-4), and they do not change when a
  // constant is taken off the plane: the tile works on x - px and y - py, px / py = the plane's value in the middle of the
  // tile's inputs, which makes the products -- and with them their rounding errors -- as small as the tile's contrast.  The
  // means get their pivot back.  Equal x and y have equal pivots, so the exactness at equal bits is kept.
  const int64_t pr = oy0 + (nh + kSrWin - 1) / 2, pc = ox0 + (nw + kSrWin - 1) / 2;      // inside the plane
  const float px = ldg(xb + pr * Wp + pc), py = ldg(yb + pr * Wp + pc);
  // stage: inputs outside the plane (a short tile) are zeros and feed only positions that are not counted
  for (int i = tid; i < kSrIn * kSrIn; i += kBlock) {
    const int r = i / kSrIn, c = i - r * kSrIn;
    const int64_t gy = oy0 + r, gx = ox0 + c;
    const bool in = gy < Hp && gx < Wp;
    sx[r * kSrInPitch + c] = in ? ldg(xb + gy * Wp + gx) - px : 0.f;
    sy[r * kSrInPitch + c] = in ? ldg(yb + gy * Wp + gx) - py : 0.f;
  }
  __syncthreads();
  // horizontal: 42 rows x 32 columns
  for (int i = tid; i < kSrIn * kSrTile; i += kBlock) {
    const int r = i >> 5, c = i & 31;
    float x[kSrWin], y[kSrWin], q[kSrWin];
#pragma unroll
    for (int k = 0; k < kSrWin; ++k) { x[k] = sx[r * kSrInPitch + c + k]; y[k] = sy[r * kSrInPitch + c + k]; }
    hb[0][r * kSrHPitch + c] = sr_taps11(x, taps);
    hb[1][r * kSrHPitch + c] = sr_taps11(y, taps);
#pragma unroll
    for (int k = 0; k < kSrWin; ++k) q[k] = x[k] * x[k];
    hb[2][r * kSrHPitch + c] = sr_taps11(q, taps);
#pragma unroll
    for (int k = 0; k < kSrWin; ++k) q[k] = y[k] * y[k];
    hb[3][r * kSrHPitch + c] = sr_taps11(q, taps);
#pragma unroll
    for (int k = 0; k < kSrWin; ++k) q[k] = x[k] * y[k];
    hb[4][r * kSrHPitch + c] = sr_taps11(q, taps);
  }
  __syncthreads();
  // vertical + ss: 32 x 32 positions, 4 per thread
  const float c1 = 1e-4f, c2 = 9e-4f;
  double acc[1] = {0.0};
  for (int i = tid; i < kSrTile * kSrTile; i += kBlock) {
    const int r = i >> 5, c = i & 31;
    if (r < nh && c < nw) {
      float v[5];
#pragma unroll
      for (int m = 0; m < 5; ++m) {
        float q[kSrWin];
#pragma unroll
        for (int k = 0; k < kSrWin; ++k) q[k] = hb[m][(r + k) * kSrHPitch + c];
        v[m] = sr_taps11(q, taps);
      }
      const float sxx = v[2] - v[0] * v[0], syy = v[3] - v[1] * v[1], sxy = v[4] - v[0] * v[1];
      const float mx = v[0] + px, my = v[1] + py;
      const float mxx = mx * mx, myy = my * my, mxy = mx * my;
      const float cs = (2.f * sxy + c2) / (sxx + syy + c2);
      const float ss = (2.f * mxy + c1) / (mxx + myy + c1) * cs;
      acc[0] += (double)ss;
    }
  }
  block_sum<1>(acc, smd);
  if (tid == 0) part[plane * gridDim.x + blockIdx.x] = acc[0];
}

// ---------------------------------------------------------------- launch 3: finalize
struct SrFinArgs {
  const double* part1;      // [n][nblk1][2]
  const double* part2;      // [n][nblk2]
  const uint32_t* bflags;   // [n][nblk1]
  double* per_image;        // [n][3]: sum |s' - h|, PSNR, SSIM in fp64, between the two phases of the launch
  int64_t n, nblk1, nblk2;
  double inv_l1, inv_mse, inv_ssim;     // 1 / element counts
  float* psnr;
  float* ssim;
  float* l1;
  float* mean;
  uint32_t* flags;
};

__global__ __launch_bounds__(kBlock) void sr_finalize_kernel(const SrFinArgs a) {
  __shared__ double smd[3 * (kBlock / kWave)];
  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  uint32_t fl = 0;
  // one wave per image: lane i takes partials i, i + 64, ..., then the wave sum
  for (int64_t img = wave; img < a.n; img += kBlock / kWave) {
    double v[3] = {0.0, 0.0, 0.0};
    for (int64_t i = lane; i < a.nblk1; i += kWave) {
      const int64_t b = img * a.nblk1 + i;
      v[0] += a.part1[2 * b];
      v[1] += a.part1[2 * b + 1];
      fl |= a.bflags[b];
    }
    for (int64_t i = lane; i < a.nblk2; i += kWave) v[2] += a.part2[img * a.nblk2 + i];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = wave_sum(v[k]);
    if (lane == 0) {
      const double p = -10.0 * log10(v[1] * a.inv_mse + 1e-8);
      const double s = v[2] * a.inv_ssim;
      *gptr(a.psnr + img) = (float)p;
      *gptr(a.ssim + img) = (float)s;
      a.per_image[3 * img] = v[0];
      a.per_image[3 * img + 1] = p;
      a.per_image[3 * img + 2] = s;
    }
  }
  __threadfence_block();
  __syncthreads();                                         // the per-image values of this workgroup's own waves
  // the batch: thread i takes images i, i + 256, ..., then the block sum
  double t[3] = {0.0, 0.0, 0.0};
  for (int64_t img = tid; img < a.n; img += kBlock) {
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] += a.per_image[3 * img + k];
  }
  block_sum<3>(t, smd);
  const double l1 = t[0], mp = t[1], ms = t[2];
  const int any0 = __syncthreads_or((int)(fl & 1u));
  const int any1 = __syncthreads_or((int)(fl & 2u));
  if (tid == 0) {
    *gptr(a.l1) = (float)(l1 * a.inv_l1);
    *gptr(a.mean) = (float)(mp / (double)a.n);
    *gptr(a.mean + 1) = (float)(ms / (double)a.n);
    const uint32_t bits = (any0 ? 1u : 0u) | (any1 ? 2u : 0u);
    if (bits) *gptr(a.flags) = *gptr(a.flags) | bits;
  }
}

inline bool sr_dtype_ok(int dt) { return dt == MHAQ_FQ_DT_F32 || dt == MHAQ_FQ_DT_BF16 || dt == MHAQ_FQ_DT_F16; }
template <class F>
auto sr_with_dtype(int dt, F f) {
  if (dt == MHAQ_FQ_DT_F32) return f(std::integral_constant<int, MHAQ_FQ_DT_F32>{});
  if (dt == MHAQ_FQ_DT_BF16) return f(std::integral_constant<int, MHAQ_FQ_DT_BF16>{});
  return f(std::integral_constant<int, MHAQ_FQ_DT_F16>{});
}

inline SrTaps sr_make_taps() {
  double g[kSrWin], sum = 0.0;
  for (int k = 0; k < kSrWin; ++k) { const double d = k - 5; g[k] = std::exp(-(d * d) / (2.0 * 1.5 * 1.5)); sum += g[k]; }
  SrTaps t;
  for (int k = 0; k < 6; ++k) t.w[k] = (float)(g[k] / sum);
  return t;
}

}  // namespace mhaq

using namespace mhaq;

extern "C" {

size_t mhaq_fq_sr_metrics_workspace_bytes(int64_t n, int64_t c, int64_t h, int64_t w, int to_luminance, int pool) {
  SrGeom g;
  return sr_geometry(n, c, h, w, to_luminance, pool, g) == 0 ? g.total : 0;
}

int mhaq_fq_sr_metrics(const void* sr, int sr_dtype, const void* hr, int hr_dtype, int64_t n, int64_t c, int64_t h,
                       int64_t w, float sr_div, int to_luminance, int pool, float* psnr, float* ssim, float* l1,
                       float* mean, uint32_t* flags, void* workspace, size_t workspace_bytes, void* stream) {
  if (!sr || !hr || !psnr || !ssim || !l1 || !mean || !flags || !workspace) return MHAQ_FQ_EINVAL;
  if (!sr_dtype_ok(sr_dtype) || !sr_dtype_ok(hr_dtype)) return MHAQ_FQ_EINVAL;
  if (n <= 0 || c <= 0 || h <= 0 || w <= 0 || pool < 1 || !std::isfinite(sr_div) || sr_div == 0.f) return MHAQ_FQ_EINVAL;
  if (to_luminance && c != 3) return MHAQ_FQ_EINVAL;
  SrGeom g;
  const int grc = sr_geometry(n, c, h, w, to_luminance, pool, g);
  if (grc == MHAQ_FQ_EINVAL) return grc;
  if (grc == 0 && workspace_bytes < g.total) return MHAQ_FQ_EWORKSPACE;
  if (((uintptr_t)sr & (sr_esize(sr_dtype) - 1)) || ((uintptr_t)hr & (sr_esize(hr_dtype) - 1)) || ((uintptr_t)psnr & 7) ||
      ((uintptr_t)ssim & 7) || ((uintptr_t)l1 & 7) || ((uintptr_t)mean & 7) || ((uintptr_t)flags & 7) ||
      ((uintptr_t)workspace & 7))
    return MHAQ_FQ_EALIGN;
  if (grc != 0) return grc;                                // MHAQ_FQ_EUNSUPPORTED

  char* ws = static_cast<char*>(workspace);
  const hipStream_t st = (hipStream_t)stream;
  SrPrepArgs pa;
  pa.s = sr; pa.h = hr;
  pa.xp = reinterpret_cast<float*>(ws);
  pa.yp = reinterpret_cast<float*>(ws + g.off_yp);
  pa.part = reinterpret_cast<double*>(ws + g.off_part1);
  pa.flags = reinterpret_cast<uint32_t*>(ws + g.off_flags);
  pa.H = h; pa.W = w; pa.Hp = g.hp; pa.Wp = g.wp;
  pa.div = sr_div;
  pa.C = (int)c; pa.P = g.p; pa.f = pool; pa.chunk = g.chunk; pa.band = g.band;
  const size_t lds = pool > 1 ? (size_t)2 * g.p * pool * g.chunk * sizeof(float) : 0;
  const dim3 grid1((unsigned)g.nchunk, (unsigned)g.nband, (unsigned)n);
  sr_with_dtype(sr_dtype, [&](auto sdt) {
    sr_with_dtype(hr_dtype, [&](auto hdt) {
      if (c == 3)
        MHAQ_LAUNCH((sr_prepare_kernel<decltype(sdt)::value, decltype(hdt)::value, 3>), grid1, dim3(kBlock), lds, st, pa);
      else
        MHAQ_LAUNCH((sr_prepare_kernel<decltype(sdt)::value, decltype(hdt)::value, 1>), grid1, dim3(kBlock), lds, st, pa);
      return 0;
    });
    return 0;
  });
  if (launch_status() != 0) return launch_status();

  double* part2 = reinterpret_cast<double*>(ws + g.off_part2);
  MHAQ_LAUNCH(sr_ssim_kernel, dim3((unsigned)(g.tx * g.ty), (unsigned)(n * g.p)), dim3(kBlock), 0, st,
              (const float*)pa.xp, (const float*)pa.yp, g.hp, g.wp, g.tx, sr_make_taps(), part2);
  if (launch_status() != 0) return launch_status();

  SrFinArgs fa;
  fa.part1 = pa.part; fa.part2 = part2; fa.bflags = pa.flags;
  fa.per_image = reinterpret_cast<double*>(ws + g.off_img);
  fa.n = n; fa.nblk1 = g.nblk1; fa.nblk2 = g.nblk2;
  fa.inv_l1 = 1.0 / ((double)n * (double)c * (double)h * (double)w);
  fa.inv_mse = 1.0 / ((double)g.p * (double)h * (double)w);
  fa.inv_ssim = 1.0 / ((double)g.p * (double)(g.hp - (kSrWin - 1)) * (double)(g.wp - (kSrWin - 1)));
  fa.psnr = psnr; fa.ssim = ssim; fa.l1 = l1; fa.mean = mean; fa.flags = flags;
  MHAQ_LAUNCH(sr_finalize_kernel, dim3(1), dim3(kBlock), 0, st, fa);
  return launch_status();
}

}  // extern "C"
