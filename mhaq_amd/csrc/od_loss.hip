// Object-detection training (mhaq_fq_od_decode, mhaq_fq_od_loss_fwd, mhaq_fq_od_loss_bwd; include/mhaq_fq.h): what the
// reference's ComputeYoloLoss.__call__ does around its assigner -- box decode, CIoU, DFL and BCE with their backward -- on the
// head's outputs WHERE THEY ARE: up to four levels [B][no][H][W], no = 4 * 16 + nc.  No cat / permute copy of the logits, no
// dense BCE target, no boolean-mask gather, no host read.
//
// The three big kernels share one split.  Grid (anchor tiles, B), kBlock threads, a tile = 64 consecutive anchors of ONE level
// (a level's last tile is ragged; a tile never straddles a level).  In the [channel][anchor] layout the 64 lanes of a wavefront
// are 64 consecutive anchors of one channel row: every global access is coalesced along anchors.
//   box part    wavefront w is side w of (l, t, r, b): a lane holds its side's 16 logits in registers and does the softmax /
//               log-softmax there; the four sides of an anchor meet through LDS ([64][4] floats).  The per-anchor record (fg,
//               label, weight, target box) is read by each wavefront for its own lanes: a few coalesced loads, no barrier.
//   class part  wavefront w walks class rows w, w + 4, ...; the BCE target is t = weight at (anchor, label), else 0.
//   decode      transposes the sigmoided scores [nc][64] -> [64][nc] through a padded LDS tile in class chunks of 64.
// A tile without a foreground anchor (the common case) skips its 64 distribution rows by a wavefront-uniform vote.
// Sums: fp32 elements, fp64 accumulation in a fixed order (thread, wavefront shuffle, the four wavefronts in order; then the
// one-workgroup finalize: thread t adds tiles t, t + 256, ... in index order, and the same tree).  No global atomics, every
// global word has one writer: the same bits at every call.
#include "od_common.hpp"

namespace mhaq {

constexpr int kOdLossR = 16;              // bins per side, the only compiled count
constexpr int kOdLossTile = 64;           // anchors per workgroup
constexpr int kOdLossMaxLevels = 4;
constexpr int kOdLossMaxA = 24576;        // od_assign's range
constexpr int kOdLossDist = 4 * kOdLossR; // distribution channels, in front of the class channels

struct OdLevel {
  const void* p;          // [B][no][H * W]
  void* g;                // the gradient in the same layout (backward only)
  int hw, w, a0, tile0;   // anchors, row length, first anchor index, first tile index
  float stride;
};
struct OdLevels { OdLevel l[kOdLossMaxLevels]; int n; };

// the level of a tile: a select chain over the table in the kernel arguments (a runtime index would put it in scratch)
__device__ __forceinline__ OdLevel od_level_of(const OdLevels& lv, int tile) {
  OdLevel L = lv.l[0];
#pragma unroll
  for (int i = 1; i < kOdLossMaxLevels; ++i)
    if (i < lv.n && tile >= lv.l[i].tile0) L = lv.l[i];
  return L;
}

__device__ __forceinline__ float od_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// One side's 16 logits of one anchor (element base + j * hw): softmax p[], its expectation sum p_j * j (returned) and, if LOGP,
// the log-softmax lp[].  Every index is a compile-time constant after unrolling: the arrays are registers.
template <int DT, bool LOGP>
__device__ __forceinline__ float od_side_softmax(const void* __restrict__ src, int64_t base, int64_t hw, bool valid,
                                                 float (&p)[kOdLossR], float (&lp)[kOdLossR]) {
  float x[kOdLossR];
#pragma unroll
  for (int j = 0; j < kOdLossR; ++j) x[j] = valid ? iox::ld1<DT>(src, base + j * hw) : 0.f;
  float m = x[0];
#pragma unroll
  for (int j = 1; j < kOdLossR; ++j) m = fmaxf(m, x[j]);
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < kOdLossR; ++j) {
    x[j] = x[j] - m;
    p[j] = expf(x[j]);
    s = s + p[j];
  }
  const float ls = LOGP ? logf(s) : 0.f;
  float e = 0.f;
#pragma unroll
  for (int j = 0; j < kOdLossR; ++j) {
    p[j] = p[j] / s;
    lp[j] = LOGP ? x[j] - ls : 0.f;
    e = e + p[j] * (float)j;
  }
  return e;
}

// The per-anchor record of the loss kernels, as every wavefront reads it for its own lane's anchor.  fg: a foreground anchor
// with a ground-truth index inside [0, G).  label: -1 unless it lies in [0, nc) -- no address is formed from an unchecked one.
// w: target_scores[b][a][label], the row's one non-zero (0 without a label).  tb: gt_bboxes[gt_idx] / stride.
struct OdTarget { bool fg; int label; float w; od_f4 tb; };

__device__ __forceinline__ OdTarget od_target(const uint8_t* __restrict__ fg_mask, const int32_t* __restrict__ gt_idx,
                                              const float* __restrict__ ts, const float* __restrict__ gt_labels,
                                              const float* __restrict__ gt_bboxes, int64_t row, int64_t b, int nc, int G,
                                              float stride, bool valid) {
  OdTarget t = {false, -1, 0.f, od_f4{0.f, 0.f, 0.f, 0.f}};
  if (!valid || G <= 0 || !*gptr(fg_mask + row)) return t;
  const int gi = *gptr(gt_idx + row);
  if ((uint32_t)gi >= (uint32_t)G) return t;
  t.fg = true;
  const int64_t bg = b * G + gi;
  const float labf = ldg(gt_labels + bg);
  if (labf >= 0.f && labf < (float)nc) {
    t.label = (int)labf;
    t.w = ldg(ts + row * nc + t.label);
  }
  t.tb = od_f4{ldg(gt_bboxes + bg * 4) / stride, ldg(gt_bboxes + bg * 4 + 1) / stride, ldg(gt_bboxes + bg * 4 + 2) / stride,
               ldg(gt_bboxes + bg * 4 + 3) / stride};
  return t;
}

// The DFL target of side `side` (0..3 = l, t, r, b) of an anchor at (ax, ay): clamp(distance, 0, R - 1 - 0.01) by fmaxf / fminf,
// so a NaN becomes 0 and never an index.  -> tl in [0, R - 2], wl = tl + 1 - target, wr = 1 - wl.
struct OdDfl { int tl; float wl, wr; };
__device__ __forceinline__ OdDfl od_dfl_target(int side, float ax, float ay, od_f4 tb) {
  const float d = side == 0 ? ax - tb.x : (side == 1 ? ay - tb.y : (side == 2 ? tb.z - ax : tb.w - ay));
  const float tg = fminf(fmaxf(d, 0.f), (float)(kOdLossR - 1) - 0.01f);
  OdDfl r;
  r.tl = (int)tg;
  r.wl = (float)(r.tl + 1) - tg;
  r.wr = 1.f - r.wl;
  return r;
}

// torch's gradient share of one operand of minimum / maximum: all of it where it wins, half where the two are equal
__device__ __forceinline__ float od_share(bool wins, bool equal) { return wins ? 1.f : (equal ? 0.5f : 0.f); }

// d ciou / d p[coord] of c = od_ciou(p, g) (od_common.hpp; box1 = the prediction p, box2 = the target g), coord = 0..3 =
// x1, y1, x2, y2 (wave-uniform in the caller); alpha is a constant, clamp(0) passes the gradient at the bound.
__device__ __forceinline__ float od_ciou_grad(const OdCiou& c, od_f4 p, od_f4 g, int coord) {
  const bool isx = (coord & 1) == 0, lo = coord < 2;
  const float pl = isx ? p.x : p.y, ph = isx ? p.z : p.w, gl = isx ? g.x : g.y, gh = isx ? g.z : g.w;
  const float pass = (isx ? c.ix : c.iy) >= 0.f ? 1.f : 0.f;
  // along this coordinate's axis: the intersection and the enclosing extent
  const float di = lo ? -pass * od_share(pl > gl, pl == gl) : pass * od_share(ph < gh, ph == gh);
  const float de = lo ? -od_share(pl < gl, pl == gl) : od_share(ph > gh, ph == gh);
  const float dinter = (isx ? c.ih : c.iw) * di;
  const float dwh = (isx ? c.h1 : c.w1) * (lo ? -1.f : 1.f);
  const float diou = (dinter - c.iou * (dwh - dinter)) / c.uni;
  const float dc2 = 2.f * (isx ? c.cw : c.ch) * de;
  const float drho2 = -(isx ? c.dx : c.dy) / 2.f;
  const float dpen = (drho2 - (c.rho2 / c.c2) * dc2) / c.c2;
  const float r = c.w1 / c.h1, dat = 1.f / (1.f + r * r);
  const float dda = (isx ? dat / c.h1 : -(dat * r) / c.h1) * (lo ? 1.f : -1.f);
  const float dv = (2.f * 0.40528473456935109f) * c.da * dda;
  return (diou - dpen) - c.al * dv;
}

struct OdTileCtx { OdLevel L; int i, lane, wave; bool valid; int64_t b, hw, row; float ax, ay; };
__device__ __forceinline__ OdTileCtx od_tile_ctx(const OdLevels& lv, int A) {
  OdTileCtx c;
  const int tid = (int)threadIdx.x, tile = (int)blockIdx.x;
  c.lane = tid & 63;
  c.wave = tid >> 6;
  c.L = od_level_of(lv, tile);
  c.i = (tile - c.L.tile0) * kOdLossTile + c.lane;
  c.valid = c.i < c.L.hw;
  c.b = blockIdx.y;
  c.hw = c.L.hw;
  c.row = c.b * A + c.L.a0 + c.i;
  c.ax = (float)(c.i % c.L.w) + 0.5f;
  c.ay = (float)(c.i / c.L.w) + 0.5f;
  return c;
}

// ---------------------------------------------------------------- decode
template <int DT>
__global__ __launch_bounds__(kBlock) void od_decode_kernel(OdLevels lv, int no, int nc, int A, float* __restrict__ pd_bboxes,
                                                           float* __restrict__ pd_scores, float* __restrict__ anc) {
  __shared__ float s_side[kOdLossTile][4];
  __shared__ float s_t[kOdLossTile][kOdLossTile + 1];         // [class][anchor], padded: both walks are conflict-free
  const OdTileCtx c = od_tile_ctx(lv, A);
  const int i0 = c.i - c.lane, nvalid = c.L.hw - i0 < kOdLossTile ? c.L.hw - i0 : kOdLossTile;
  float p[kOdLossR], lp[kOdLossR];
  s_side[c.lane][c.wave] = od_side_softmax<DT, false>(c.L.p, (c.b * no + c.wave * kOdLossR) * c.hw + c.i, c.hw, c.valid, p, lp);
  __syncthreads();
  if (c.wave == 0 && c.valid) {
    const float s = c.L.stride;
    const float v[4] = {(c.ax - s_side[c.lane][0]) * s, (c.ay - s_side[c.lane][1]) * s, (c.ax + s_side[c.lane][2]) * s,
                        (c.ay + s_side[c.lane][3]) * s};
    stvg<4>(pd_bboxes + c.row * 4, v);
    if (c.b == 0) {
      stg(anc + 2 * (int64_t)(c.L.a0 + c.i), c.ax * s);
      stg(anc + 2 * (int64_t)(c.L.a0 + c.i) + 1, c.ay * s);
    }
  }
  const int64_t cbase = (c.b * no + kOdLossDist) * c.hw + c.i;
  float* dst = pd_scores + (c.b * A + c.L.a0 + i0) * nc;
  for (int c0 = 0; c0 < nc; c0 += kOdLossTile) {
    const int ncl = nc - c0 < kOdLossTile ? nc - c0 : kOdLossTile;
    if (c.valid)
      for (int cl = c.wave; cl < ncl; cl += kBlock / kWave) s_t[cl][c.lane] = od_sigmoid(iox::ld1<DT>(c.L.p, cbase + (c0 + cl) * c.hw));
    __syncthreads();
    if (c.lane < ncl)
      for (int al = c.wave; al < nvalid; al += kBlock / kWave) stg(dst + (int64_t)al * nc + c0 + c.lane, s_t[c.lane][al]);
    __syncthreads();
  }
}

// ---------------------------------------------------------------- loss forward
template <int DT>
__global__ __launch_bounds__(kBlock) void od_loss_fwd_kernel(
    OdLevels lv, int no, int nc, int A, int G, const uint8_t* __restrict__ fg_mask, const int32_t* __restrict__ gt_idx,
    const float* __restrict__ ts, const float* __restrict__ gt_labels, const float* __restrict__ gt_bboxes,
    double* __restrict__ partial) {
  __shared__ float s_side[kOdLossTile][4];
  __shared__ float s_dfl[kOdLossTile][4];
  __shared__ double s_red[3 * kBlock / kWave];
  const OdTileCtx c = od_tile_ctx(lv, A);
  const OdTarget t = od_target(fg_mask, gt_idx, ts, gt_labels, gt_bboxes, c.row, c.b, nc, G, c.L.stride, c.valid);
  double acc[3] = {0.0, 0.0, 0.0};                            // box, cls, dfl
  if (c.valid) {
    const int64_t cbase = (c.b * no + kOdLossDist) * c.hw + c.i;
    for (int k = c.wave; k < nc; k += kBlock / kWave) {
      const float x = iox::ld1<DT>(c.L.p, cbase + k * c.hw);
      const float tt = k == t.label ? t.w : 0.f;
      acc[1] += (double)((fmaxf(x, 0.f) - x * tt) + log1pf(expf(-fabsf(x))));
    }
  }
  if (__ballot(t.fg) != 0) {                                  // the same vote in all four wavefronts: the barrier is uniform
    float p[kOdLossR], lp[kOdLossR];
    s_side[c.lane][c.wave] = od_side_softmax<DT, true>(c.L.p, (c.b * no + c.wave * kOdLossR) * c.hw + c.i, c.hw, c.valid, p, lp);
    const OdDfl d = od_dfl_target(c.wave, c.ax, c.ay, t.tb);
    float ll = 0.f, lr = 0.f;
#pragma unroll
    for (int j = 0; j < kOdLossR; ++j) {
      ll = j == d.tl ? lp[j] : ll;
      lr = j == d.tl + 1 ? lp[j] : lr;
    }
    s_dfl[c.lane][c.wave] = (-ll) * d.wl + (-lr) * d.wr;
    __syncthreads();
    if (c.wave == 0 && t.fg) {
      const od_f4 pb = od_f4{c.ax - s_side[c.lane][0], c.ay - s_side[c.lane][1], c.ax + s_side[c.lane][2],
                             c.ay + s_side[c.lane][3]};
      acc[0] = (double)((1.f - od_ciou(pb, t.tb).ciou) * t.w);
      const float dfl = (((s_dfl[c.lane][0] + s_dfl[c.lane][1]) + s_dfl[c.lane][2]) + s_dfl[c.lane][3]) / 4.f;
      acc[2] = (double)(dfl * t.w);
    }
  }
  block_sum<3>(acc, s_red);
  if (threadIdx.x == 0) {
    double* dst = partial + (c.b * gridDim.x + blockIdx.x) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) *gptr(dst + k) = acc[k];
  }
}

// one workgroup: loss[k] = sum_k / max(scores_sum, 1) * gain_k, rounded once; the denominator goes to the backward
__global__ __launch_bounds__(kBlock) void od_loss_finalize_kernel(const double* __restrict__ partial, int64_t n,
                                                                  const float* __restrict__ scores_sum, float gain_box,
                                                                  float gain_cls, float gain_dfl, float* __restrict__ loss,
                                                                  float* __restrict__ denom) {
  __shared__ double s_red[3 * kBlock / kWave];
  double acc[3] = {0.0, 0.0, 0.0};
  for (int64_t t = threadIdx.x; t < n; t += kBlock) {
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[k] += *gptr(partial + 3 * t + k);
  }
  block_sum<3>(acc, s_red);
  if (threadIdx.x == 0) {
    const float s = ldg(scores_sum), den = s < 1.f ? 1.f : s; // max(sum, 1); a NaN stays
    stg(loss, (float)((acc[0] / (double)den) * (double)gain_box));
    stg(loss + 1, (float)((acc[1] / (double)den) * (double)gain_cls));
    stg(loss + 2, (float)((acc[2] / (double)den) * (double)gain_dfl));
    stg(denom, den);
  }
}

// ---------------------------------------------------------------- loss backward
// Recomputes its tile; writes every element of the gradient once, in the head's layout and dtype.
template <int DT>
__global__ __launch_bounds__(kBlock) void od_loss_bwd_kernel(
    OdLevels lv, int no, int nc, int A, int G, const uint8_t* __restrict__ fg_mask, const int32_t* __restrict__ gt_idx,
    const float* __restrict__ ts, const float* __restrict__ gt_labels, const float* __restrict__ gt_bboxes,
    const float* __restrict__ grad_out, const float* __restrict__ denom, float gain_box, float gain_cls, float gain_dfl) {
  __shared__ float s_side[kOdLossTile][4];
  const OdTileCtx c = od_tile_ctx(lv, A);
  const OdTarget t = od_target(fg_mask, gt_idx, ts, gt_labels, gt_bboxes, c.row, c.b, nc, G, c.L.stride, c.valid);
  const float den = ldg(denom);
  const float g_box = (ldg(grad_out) * gain_box) / den, g_cls = (ldg(grad_out + 1) * gain_cls) / den,
              g_dfl = (ldg(grad_out + 2) * gain_dfl) / den;
  if (c.valid) {
    const int64_t cbase = (c.b * no + kOdLossDist) * c.hw + c.i;
    for (int k = c.wave; k < nc; k += kBlock / kWave) {
      const float x = iox::ld1<DT>(c.L.p, cbase + k * c.hw);
      iox::st1<DT>(c.L.g, cbase + k * c.hw, g_cls * (od_sigmoid(x) - (k == t.label ? t.w : 0.f)));
    }
  }
  const int64_t dbase = (c.b * no + c.wave * kOdLossR) * c.hw + c.i;
  float gj[kOdLossR];
#pragma unroll
  for (int j = 0; j < kOdLossR; ++j) gj[j] = 0.f;
  if (__ballot(t.fg) != 0) {
    float p[kOdLossR], lp[kOdLossR];
    const float e = od_side_softmax<DT, false>(c.L.p, dbase, c.hw, c.valid, p, lp);
    s_side[c.lane][c.wave] = e;
    __syncthreads();
    if (t.fg) {
      const od_f4 pb = od_f4{c.ax - s_side[c.lane][0], c.ay - s_side[c.lane][1], c.ax + s_side[c.lane][2],
                             c.ay + s_side[c.lane][3]};
      const float dc = od_ciou_grad(od_ciou(pb, t.tb), pb, t.tb, c.wave);
      // box term (1 - ciou) * w;  x1 = ax - l, y1 = ay - t, x2 = ax + r, y2 = ay + b
      const float gs = g_box * (c.wave < 2 ? t.w * dc : -(t.w * dc));
      const float gd = g_dfl * (t.w / 4.f);
      const OdDfl d = od_dfl_target(c.wave, c.ax, c.ay, t.tb);
#pragma unroll
      for (int j = 0; j < kOdLossR; ++j) {
        const float hit = (j == d.tl ? d.wl : 0.f) + (j == d.tl + 1 ? d.wr : 0.f);
        gj[j] = gs * (p[j] * ((float)j - e)) + gd * (p[j] - hit);
      }
    }
  }
  if (c.valid) {
#pragma unroll
    for (int j = 0; j < kOdLossR; ++j) iox::st1<DT>(c.L.g, dbase + j * c.hw, gj[j]);
  }
}

// ---------------------------------------------------------------- host
// The level table from the caller's host arrays, checked.  -> 0 or an error code; *A anchors, *tiles anchor tiles.
static int od_levels_build(const void* const* ptr, void* const* grad, bool want_grad, const int32_t* h, const int32_t* w,
                           const float* stride, int levels, int dtype, int64_t b, int64_t nc, int reg_max, OdLevels* out,
                           int64_t* A, int* tiles) {
  if (!ptr || !h || !w || !stride || (want_grad && !grad) || levels < 1 || !iox::known_dtype(dtype) || b < 0 || nc < 1 ||
      reg_max < 1)
    return MHAQ_FQ_EINVAL;
  if (levels > kOdLossMaxLevels || reg_max != kOdLossR || b > 65535 || nc > 65535) return MHAQ_FQ_EUNSUPPORTED;
  int64_t a = 0;
  int nt = 0;
  const uintptr_t mask = dtype == MHAQ_FQ_DT_F32 ? 3 : 1;
  out->n = levels;
  for (int i = 0; i < kOdLossMaxLevels; ++i) out->l[i] = OdLevel{nullptr, nullptr, 0, 1, 0, 0, 1.f};
  for (int i = 0; i < levels; ++i) {
    if (h[i] < 0 || w[i] < 0 || !(stride[i] > 0.f) || !od_finite(stride[i])) return MHAQ_FQ_EINVAL;
    const int64_t hw = (int64_t)h[i] * w[i];
    if (a + hw > kOdLossMaxA) return MHAQ_FQ_EUNSUPPORTED;
    if (b > 0 && hw > 0 && (!ptr[i] || (want_grad && !grad[i]))) return MHAQ_FQ_EINVAL;
    if (((uintptr_t)ptr[i] & mask) || (want_grad && ((uintptr_t)grad[i] & mask))) return MHAQ_FQ_EALIGN;
    out->l[i] = OdLevel{ptr[i], want_grad ? grad[i] : nullptr, (int)hw, w[i] > 0 ? w[i] : 1, (int)a, nt, stride[i]};
    a += hw;
    nt += (int)((hw + kOdLossTile - 1) / kOdLossTile);
  }
  *A = a;
  *tiles = nt;
  return 0;
}

// the assigner's record and the ground truth, as the loss calls take them
static int od_record_check(int64_t rows, int64_t g, const uint8_t* fg_mask, const int32_t* gt_idx, const float* ts,
                           const float* gt_labels, const float* gt_bboxes) {
  if (g < 0) return MHAQ_FQ_EINVAL;
  if (rows > 0 && (!fg_mask || !gt_idx || !ts || (g > 0 && (!gt_labels || !gt_bboxes)))) return MHAQ_FQ_EINVAL;
  if (g > 0x7fffffff) return MHAQ_FQ_EUNSUPPORTED;
  if (((uintptr_t)gt_idx & 3) || ((uintptr_t)ts & 3) || ((uintptr_t)gt_labels & 3) || ((uintptr_t)gt_bboxes & 3))
    return MHAQ_FQ_EALIGN;
  return 0;
}

}  // namespace mhaq

using namespace mhaq;

extern "C" {

int mhaq_fq_od_decode(const void* const* level_ptr, const int32_t* level_h, const int32_t* level_w, const float* level_stride,
                      int levels, int dtype, int64_t b, int64_t nc, int reg_max, float* pd_bboxes, float* pd_scores,
                      float* anc_points, void* stream) {
  OdLevels lv;
  int64_t A = 0;
  int tiles = 0;
  const int rc = od_levels_build(level_ptr, nullptr, false, level_h, level_w, level_stride, levels, dtype, b, nc, reg_max, &lv,
                                 &A, &tiles);
  if (rc != 0) return rc;
  if (b == 0 || A == 0) return 0;
  if (!pd_bboxes || !pd_scores || !anc_points) return MHAQ_FQ_EINVAL;
  if (((uintptr_t)pd_bboxes & 15) || ((uintptr_t)pd_scores & 3) || ((uintptr_t)anc_points & 3)) return MHAQ_FQ_EALIGN;
  const int NO = kOdLossDist + (int)nc;
  iox::with_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    MHAQ_LAUNCH(od_decode_kernel<DT>, dim3((unsigned)tiles, (unsigned)b), dim3(kBlock), 0, (hipStream_t)stream, lv, NO, (int)nc,
                (int)A, pd_bboxes, pd_scores, anc_points);
  });
  return launch_status();
}

size_t mhaq_fq_od_loss_workspace_bytes(int64_t b, int64_t a, int levels) {
  if (b < 1 || a < 1 || levels < 1 || b > 65535 || a > kOdLossMaxA || levels > kOdLossMaxLevels) return 0;
  return (size_t)b * (size_t)(a / kOdLossTile + levels) * 3 * sizeof(double);
}

int mhaq_fq_od_loss_fwd(const void* const* level_ptr, const int32_t* level_h, const int32_t* level_w, const float* level_stride,
                        int levels, int dtype, int64_t b, int64_t nc, int reg_max, const uint8_t* fg_mask,
                        const int32_t* target_gt_idx, const float* target_scores, const float* scores_sum,
                        const float* gt_labels, const float* gt_bboxes, int64_t g, float gain_box, float gain_cls,
                        float gain_dfl, float* loss, float* denom, void* workspace, size_t workspace_bytes, void* stream) {
  OdLevels lv;
  int64_t A = 0;
  int tiles = 0;
  int rc = od_levels_build(level_ptr, nullptr, false, level_h, level_w, level_stride, levels, dtype, b, nc, reg_max, &lv, &A,
                           &tiles);
  if (rc != 0) return rc;
  if (!scores_sum || !loss || !denom) return MHAQ_FQ_EINVAL;
  const bool empty = b == 0 || A == 0;
  if ((rc = od_record_check(empty ? 0 : b * A, g, fg_mask, target_gt_idx, target_scores, gt_labels, gt_bboxes)) != 0) return rc;
  if (!empty && !workspace) return MHAQ_FQ_EINVAL;
  if (((uintptr_t)scores_sum & 3) || ((uintptr_t)loss & 3) || ((uintptr_t)denom & 3) || ((uintptr_t)workspace & 7))
    return MHAQ_FQ_EALIGN;
  if (!empty && workspace_bytes < mhaq_fq_od_loss_workspace_bytes(b, A, levels)) return MHAQ_FQ_EWORKSPACE;
  const hipStream_t st = (hipStream_t)stream;
  double* partial = static_cast<double*>(workspace);
  if (!empty) {
    const int NO = kOdLossDist + (int)nc;
    iox::with_dtype(dtype, [&](auto dt) {
      constexpr int DT = decltype(dt)::value;
      MHAQ_LAUNCH(od_loss_fwd_kernel<DT>, dim3((unsigned)tiles, (unsigned)b), dim3(kBlock), 0, st, lv, NO, (int)nc, (int)A,
                  (int)g, fg_mask, target_gt_idx, target_scores, gt_labels, gt_bboxes, partial);
    });
    if ((rc = launch_status()) != 0) return rc;
  }
  MHAQ_LAUNCH(od_loss_finalize_kernel, dim3(1), dim3(kBlock), 0, st, (const double*)partial, empty ? (int64_t)0 : b * tiles,
              scores_sum, gain_box, gain_cls, gain_dfl, loss, denom);
  return launch_status();
}

int mhaq_fq_od_loss_bwd(const void* const* level_ptr, const int32_t* level_h, const int32_t* level_w, const float* level_stride,
                        int levels, int dtype, int64_t b, int64_t nc, int reg_max, const uint8_t* fg_mask,
                        const int32_t* target_gt_idx, const float* target_scores, const float* gt_labels, const float* gt_bboxes,
                        int64_t g, const float* grad_out, const float* denom, float gain_box, float gain_cls, float gain_dfl,
                        void* const* grad_level_ptr, void* stream) {
  OdLevels lv;
  int64_t A = 0;
  int tiles = 0;
  int rc = od_levels_build(level_ptr, grad_level_ptr, true, level_h, level_w, level_stride, levels, dtype, b, nc, reg_max, &lv,
                           &A, &tiles);
  if (rc != 0) return rc;
  if (!grad_out || !denom) return MHAQ_FQ_EINVAL;
  const bool empty = b == 0 || A == 0;
  if ((rc = od_record_check(empty ? 0 : b * A, g, fg_mask, target_gt_idx, target_scores, gt_labels, gt_bboxes)) != 0) return rc;
  if (((uintptr_t)grad_out & 3) || ((uintptr_t)denom & 3)) return MHAQ_FQ_EALIGN;
  if (empty) return 0;
  const int NO = kOdLossDist + (int)nc;
  iox::with_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    MHAQ_LAUNCH(od_loss_bwd_kernel<DT>, dim3((unsigned)tiles, (unsigned)b), dim3(kBlock), 0, (hipStream_t)stream, lv, NO,
                (int)nc, (int)A, (int)g, fg_mask, target_gt_idx, target_scores, gt_labels, gt_bboxes, grad_out, denom, gain_box,
                gain_cls, gain_dfl);
  });
  return launch_status();
}

}  // extern "C"
