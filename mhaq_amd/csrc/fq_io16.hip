// Per-tensor activation fake-quant with 16-bit I/O (bf16 / fp16) for gfx950: the NoisyAct forward and backward of a
// model trained under torch.autocast, whose convolutions hand every activation quantizer a 16-bit tensor.
//
// Contract (include/mhaq_fq.h, "16-bit activations"): every element is converted UP exactly and runs the fp32 arithmetic
// of fq_pt.hip unchanged (quant_core / quant_core_bwd / make_bwd_ctx / dequant / noise_grad_v / sign_tile_fill of
// fq_common.hpp); y and gx are rounded to nearest-even ONCE on the way out.  So y == RNE(y_fp32(x.float())) and
// gx == RNE(gx_fp32(x.float(), g.float())) bit for bit, and the reduced parameter gradients are the fp32 ones.
//
// Layout: as the fp32 streaming kernels (fq_pt.hip) with 16 B per lane = 8 elements per access.  The backward block
// covers 8 * 256 * U consecutive elements -- 16 * U Philox calls of the v3 sign stream, each lane taking one BYTE of
// the tile where the fp32 kernel takes a nibble -- so element i draws exactly the sign the fp32 kernel draws for it.
// Partial rows use the ACT column layout of fq_pt.hip's write_partials<ACT> + publish_act_scales, and never more rows
// than the fp32 launch over the same n: mhaq_fq_act_bwd_workspace_bytes(n) sizes both, and
// mhaq_fq_act_bwd_finalize_multi serves 16-bit and fp32 quantizers in the same pass.
//
// The element bodies below are COPIES of fq_pt.hip's fwd_elem (WRITE_Q = false) and bwd_elem / bwd_elem_fast
// (COUNT = false), verbatim in arithmetic: fq_pt.hip stays untouched because the committed traffic profile
// (profiles/r06_traffic.json) is tied to its hash.  tests/test_gpu_act16.py holds the copies to the fp32 kernels bit
// for bit; folding both into a shared header belongs to the next change that re-measures traffic anyway.  Inside this
// file nothing is kept twice: the plain and the ReLU backward kernel are one body (x16_bwd_body), and their entry
// points share one validation / geometry / launch path (bwd_partials).
//
// ReLU (+ residual add) forms (mhaq_fq_act_relu_*_x16, further down): the NoisyAct behind a ReLU as ONE launch per direction,
// as fq_pt.hip's pt_fwd_relu_kernel / pt_bwd_relu_kernel.  Their contract is NOT "the fp32 result rounded once" but the bits of
// the separate 16-bit launches they replace (torch's 16-bit add / relu / threshold_backward / gradient accumulation around the
// kernels above): z + addend is rounded to 16 bits before the ReLU, and the gradient gq is rounded to 16 bits BEFORE g_a is
// added and the sum is rounded again -- two roundings, as the quantizer's 16-bit gx and autograd's 16-bit add give them.
// Partial rows, geometry, sign tile and workspace rule are those of x16_act_bwd_kernel on (relu(z), g_y).

#include "fq_io16.hpp"   // up2 / down2 / ld8 / st8, known_dtype / with_dtype: shared with bn_bwd.hip

namespace mhaq {
namespace io16 {

constexpr int kFwdU = 1;             // training forward: 2048 elements per block
constexpr int kFwdStatsU = 2;        // eval forward: 4096 elements per block (fq_pt.hip's kFwdStatsU = 4 on float4)
// big tensors: 2 x 16 B per lane per stream, the bytes in flight per lane of the fp32 kernel; the small-tensor form
// takes 1: at the 8-wave bound (64 VGPRs) 2 spilled
constexpr int kBwdU = 2;
constexpr int bwd_u(bool big) { return big ? kBwdU : 1; }
constexpr int64_t kFwdPlainLoadElems = 16ll << 20;     // as fq_pt.hip: non-temporal loads above this size
constexpr int64_t kBwdBigElems = 20ll << 20;           // as fq_pt.hip (a lower threshold would never give more rows)
constexpr int kFinalThreads = 1024;

// =============================================================== forward
struct FwdStats { float qmin, qmax; bool bad; };

// fq_pt.hip fwd_elem<WRITE_Q = false, STATS>, verbatim in arithmetic
template <bool STATS>
__device__ inline float fwd_elem(float x, float s, float zp, float lo, float hi, FwdStats& st) {
  QCore c = quant_core(x, s, zp, lo, hi);
  if (STATS) {
    st.qmin = fminf(st.qmin, c.q);
    st.qmax = fmaxf(st.qmax, c.q);
    st.bad |= (c.q != c.q);          // q is not an integer <=> q is NaN (see fq_pt.hip fwd_elem)
  }
  return dequant(c.q, s, zp);
}

// NoisyAct.forward from its learnable parameters (fq_pt.hip pt_fwd_kernel<LOGP = true>): block 0 publishes
// params_out[5] = {s, zp, lo, hi, qr}; STATS (eval) leaves {min q, max q, flag word} columns [3][grid] in `partials`.
template <int DT, bool STATS, bool ALIGNED, bool NTLD, int FU>
__global__ __launch_bounds__(kBlock) void x16_act_fwd_kernel(
    const uint16_t* __restrict__ x, uint16_t* __restrict__ y, int64_t n, const float* __restrict__ ps,
    const float* __restrict__ pq, const float* __restrict__ pb, float* __restrict__ partials,
    float* __restrict__ params_out) {
  const int64_t nvec = n >> 3;
  const int64_t base = (int64_t)blockIdx.x * (kBlock * FU) + threadIdx.x;
  const bool full = ((int64_t)blockIdx.x + 1) * (kBlock * FU) <= nvec;
  vu4 a[FU];
  if (ALIGNED) {
#pragma unroll
    for (int u = 0; u < FU; ++u) {
      const int64_t idx = base + u * kBlock;
      if (full || idx < nvec) a[u] = ld8<NTLD>(x, idx);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  const float s = exp2f(*ps);
  const float qr = exp2f(*pq);
  const float zp = *pb, lo = zp;
  const float hi = (zp + qr) - s;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    params_out[0] = s; params_out[1] = zp; params_out[2] = lo; params_out[3] = hi; params_out[4] = qr;
  }
  float qlo = 0.f, qhi = 0.f;
  if (STATS) {
    qlo = floorf((lo - zp) / s);
    qhi = ceilf((hi - zp) / s);
  }
  FwdStats st{INFINITY, -INFINITY, false};

  if (ALIGNED) {
#pragma unroll
    for (int u = 0; u < FU; ++u) {
      const int64_t idx = base + u * kBlock;
      if (full || idx < nvec) {
        vu4 o;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          float e0, e1;
          up2<DT>(a[u][w], e0, e1);
          const float r0 = fwd_elem<STATS>(e0, s, zp, lo, hi, st);
          const float r1 = fwd_elem<STATS>(e1, s, zp, lo, hi, st);
          o[w] = down2<DT>(r0, r1);
        }
        st8<true>(y, idx, o);
      }
    }
    const int64_t t = (nvec << 3) + threadIdx.x;       // n % 8 tail elements
    if (blockIdx.x == 0 && t < n) y[t] = down1<DT>(fwd_elem<STATS>(up1<DT>(x[t]), s, zp, lo, hi, st));
  } else {
    // pointers not 16-byte aligned (tensor views): element accesses, grid-stride
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
      y[i] = down1<DT>(fwd_elem<STATS>(up1<DT>(x[i]), s, zp, lo, hi, st));
  }

  if (STATS) {
    const int lane = threadIdx.x & 63;
    __shared__ float smn[kBlock / 64], smx[kBlock / 64];
    __shared__ int sfl[kBlock / 64];
    float mn = wave_min(st.qmin), mx = wave_max(st.qmax);
    int fl = st.bad ? MHAQ_FQ_FLAG_NOT_INTEGER : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) fl |= __shfl_down(fl, o, 64);
    if (lane == 0) { smn[threadIdx.x >> 6] = mn; smx[threadIdx.x >> 6] = mx; sfl[threadIdx.x >> 6] = fl; }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < kBlock / 64; ++w) { mn = fminf(mn, smn[w]); mx = fmaxf(mx, smx[w]); fl |= sfl[w]; }
      if (mn < qlo) fl |= MHAQ_FQ_FLAG_BELOW_MIN;
      if (mx > qhi) fl |= MHAQ_FQ_FLAG_ABOVE_MAX;
      const int64_t nb = gridDim.x;
      partials[blockIdx.x] = mn;
      partials[nb + blockIdx.x] = mx;
      partials[2 * nb + blockIdx.x] = __int_as_float(fl);
    }
  }
}

// fq_pt.hip pt_fwd_finalize_kernel (a device symbol of another translation unit is out of reach without -fgpu-rdc):
// one workgroup per column of the [3][nparts] partials
__global__ __launch_bounds__(kFinalThreads) void x16_fwd_finalize_kernel(const float* __restrict__ partials, int nparts,
                                                                          float* __restrict__ qstats,
                                                                          int32_t* __restrict__ flags) {
  const int col = blockIdx.x;
  const float* p = partials + (int64_t)col * nparts;
  float v = (col == 0) ? INFINITY : -INFINITY;
  int fl = 0;
  constexpr int kUnroll = 8;
  for (int i0 = threadIdx.x; i0 < nparts; i0 += kUnroll * kFinalThreads) {
    float t[kUnroll];
#pragma unroll
    for (int k = 0; k < kUnroll; ++k) {
      const int i = i0 + k * kFinalThreads;
      t[k] = p[i < nparts ? i : i0];
    }
#pragma unroll
    for (int k = 0; k < kUnroll; ++k) {
      if (col == 0) v = fminf(v, t[k]);
      else if (col == 1) v = fmaxf(v, t[k]);
      else fl |= __float_as_int(t[k]);
    }
  }
  __shared__ float sv[kFinalThreads / 64];
  __shared__ int sf[kFinalThreads / 64];
  v = (col == 0) ? wave_min(v) : wave_max(v);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) fl |= __shfl_down(fl, o, 64);
  if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = v; sf[threadIdx.x >> 6] = fl; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kFinalThreads / 64; ++w) {
      v = (col == 0) ? fminf(v, sv[w]) : fmaxf(v, sv[w]);
      fl |= sf[w];
    }
    if (col == 0) { if (qstats) qstats[0] = v; }
    else if (col == 1) { if (qstats) qstats[1] = v; }
    else if (flags) *flags = fl;
  }
}

// =============================================================== backward
constexpr int kAcc = 4;   // d/ds, d/dzp, d/dlo, d/dhi (no tie counter: activations only)

// fq_pt.hip bwd_elem<METHOD, COUNT = false>, verbatim in arithmetic (METHOD: STE, LSQ or EWGS; delta is AEWGS-only)
template <int METHOD>
__device__ inline float bwd_elem(float x, float g, float r, float delta, const BwdCtx& k, float (&acc)[kAcc]) {
  QCore c = quant_core_bwd(x, k);
  const float gq = g * k.s;
  const float gv = gq + noise_grad_v<METHOD>(gq, c.n, delta);
  float g1;
  if ((METHOD == MHAQ_FQ_STE || METHOD == MHAQ_FQ_LSQ) && k.fast_div)
    g1 = __fmaf_rn(__fmaf_rn(-k.s, g, gv), k.rs, g);
  else
    g1 = gv / k.s;
  const float noise_s = (METHOD == MHAQ_FQ_LSQ) ? gq * c.n : (MHAQ_INV_SQRT3 * gq) * r;
  if (METHOD == MHAQ_FQ_STE || METHOD == MHAQ_FQ_LSQ)
    acc[0] += g * c.n + noise_s;
  else
    acc[0] += (g * c.q + (-gv) * (c.v / k.s)) + noise_s;
  acc[1] += g - g1;
  const bool lt = x < k.lo, gt = x > k.hi;
  acc[2] += (lt && k.lo_lt_hi) ? g1 : 0.f;
  acc[3] += (gt || k.hi_lt_lo) ? g1 : 0.f;
  return ((x >= k.lo) && (x <= k.hi)) ? g1 : 0.f;
}

// fq_pt.hip bwd_elem_fast<METHOD, COUNT = false>, verbatim in arithmetic (STE / LSQ on a well-formed quantizer)
template <int METHOD>
__device__ __forceinline__ float bwd_elem_fast(float x, float g, float rsc, const BwdCtx& k, float (&acc)[kAcc]) {
  const bool lt = x < k.lo, gt = x > k.hi, ord = (x == x);
  const float v0 = gt ? k.hi : (lt ? k.lo : x);
  const float v1 = v0 - k.zp;
  const float q0 = v1 * k.rs;
  const float q1 = __fmaf_rn(__fmaf_rn(-k.s, q0, v1), k.rs, q0);
  const float v = __fmaf_rn(__fmaf_rn(-k.s, q1, v1), k.rs, q1);
  const float n = rintf(v) - v;
  const float gq = g * k.s;
  const float gv = __fmaf_rn(gq, 0.f, gq);
  const float g1 = __fmaf_rn(__fmaf_rn(-k.s, g, gv), k.rs, g);
  if (METHOD == MHAQ_FQ_LSQ) acc[0] = __fmaf_rn(g + gq, n, acc[0]);
  else acc[0] = __fmaf_rn(g, n + rsc, acc[0]);
  acc[1] += g - g1;
  acc[2] += lt ? g1 : 0.f;
  acc[3] += gt ? g1 : 0.f;
  return (ord && !lt && !gt) ? g1 : 0.f;
}

// fq_pt.hip signed_half_scale: +-h with the sign of stream bit `bit` of `nb` INVERTED (nb = ~sign bits)
__device__ __forceinline__ float signed_half_scale(uint32_t nb, int bit, float h) {
  const uint32_t sgn = nb << (31 - bit);
  return __uint_as_float((sgn & 0x80000000u) | (__float_as_uint(h) & 0x7fffffffu));
}

// fq_pt.hip write_partials<ACT = true> + publish_act_scales: columns {d/ds - d/dhi, d/dhi, d/dzp + d/dlo + d/dhi}
// and {s, qr} behind them, the layout mhaq_fq_act_bwd_finalize_multi reads
template <class T>
__device__ inline void write_act_partials(float* __restrict__ partials, const T (&t)[kAcc], int64_t nb, int64_t b) {
  partials[0 * nb + b] = (float)(t[0] - t[3]);
  partials[1 * nb + b] = (float)t[3];
  partials[2 * nb + b] = (float)((t[1] + t[2]) + t[3]);
}
__device__ inline void publish_act_scales(float* __restrict__ partials, const float* __restrict__ params, int64_t nb) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    partials[3 * nb] = params[0];
    partials[3 * nb + 1] = params[4];
  }
}

// =============================================================== ReLU (+ residual add) fused in, 16-bit
// fq_pt.hip's pt_fwd_relu_kernel / pt_bwd_relu_kernel on 16-bit tensors (mhaq_fq_act_relu_*_x16): the NoisyAct behind a
// ReLU under torch.autocast.  The target is the BITS of the separate 16-bit launches -- torch's add, relu,
// threshold_backward and autograd's accumulation around the kernels above -- so every 16-bit tensor those launches would
// have written is rounded here where they round it, in registers:
//   forward    t = addend ? R(up(z) + up(addend)) : z        (torch's 16-bit add: one fp32 sum, rounded once)
//              a = relu(t)   (exact; NaN passes)             y = R(fwd_elem(up(a)))
//   backward   a = relu(up(z))                               gq = R(bwd_elem(a, up(g_y)))
//              gs = g_a ? R(up(gq) + up(g_a)) : gq           gx = (up(z) <= 0) ? +0 : gs
// gs is rounded TWICE on purpose: unfused, the quantizer writes a 16-bit gq and autograd adds the other consumer's 16-bit
// gradient to it with a 16-bit add.  R(fp32 gq + g_a) would be closer to the exact sum and a different training run.
// The parameter sums take the fp32 (a, up(g_y)) of every element, masked or not: geometry, sign tile and partial rows are
// the plain backward's on (a, g_y), byte for byte -- both kernels are x16_bwd_body below.
__device__ __forceinline__ float relu_elem(float x) { return (x <= 0.f) ? 0.f : x; }

// keep-masks of a packed pair: threshold_backward / relu zero the halves whose value is <= 0 (a NaN keeps its half)
__device__ __forceinline__ uint32_t keep2(float v0, float v1) {
  return ((v0 <= 0.f) ? 0u : 0x0000ffffu) | ((v1 <= 0.f) ? 0u : 0xffff0000u);
}

// a = relu(z [+ addend]) of a packed pair: values a0, a1 and the bits of a (a is a 16-bit value or +0: no rounding)
template <int DT, bool HAS_ADD>
__device__ __forceinline__ uint32_t relu_in2(uint32_t zw, uint32_t dw, float& a0, float& a1) {
  uint32_t tw = zw;
  if (HAS_ADD) {
    float z0, z1, d0, d1;
    up2<DT>(zw, z0, z1);
    up2<DT>(dw, d0, d1);
    tw = down2<DT>(z0 + d0, z1 + d1);
  }
  float t0, t1;
  up2<DT>(tw, t0, t1);
  a0 = relu_elem(t0);
  a1 = relu_elem(t1);
  return tw & keep2(t0, t1);
}
template <int DT, bool HAS_ADD>
__device__ __forceinline__ uint16_t relu_in1(uint16_t z, uint16_t d, float& a) {
  uint16_t tb = z;
  if (HAS_ADD) tb = down1<DT>(up1<DT>(z) + up1<DT>(d));
  const float t = up1<DT>(tb);
  a = relu_elem(t);
  return (t <= 0.f) ? (uint16_t)0 : tb;
}

// gx of a packed pair from the fp32 results q0, q1 of the element body, the other consumers' gradient cw and z
template <int DT, bool HAS_GA>
__device__ __forceinline__ uint32_t relu_out2(float q0, float q1, uint32_t cw, float z0, float z1) {
  uint32_t w = down2<DT>(q0, q1);
  if (HAS_GA) {
    float r0, r1, c0, c1;
    up2<DT>(w, r0, r1);
    up2<DT>(cw, c0, c1);
    w = down2<DT>(r0 + c0, r1 + c1);
  }
  return w & keep2(z0, z1);
}
template <int DT, bool HAS_GA>
__device__ __forceinline__ uint16_t relu_out1(float q, uint16_t c, float z) {
  uint16_t w = down1<DT>(q);
  if (HAS_GA) w = down1<DT>(up1<DT>(w) + up1<DT>(c));
  return (z <= 0.f) ? (uint16_t)0 : w;
}

template <int DT, bool HAS_ADD, bool WRITE_A, bool ALIGNED, bool NTLD>
__global__ __launch_bounds__(kBlock) void x16_act_relu_fwd_kernel(
    const uint16_t* __restrict__ z, const uint16_t* __restrict__ addend, uint16_t* __restrict__ y,
    uint16_t* __restrict__ a_out, int64_t n, const float* __restrict__ ps, const float* __restrict__ pq,
    const float* __restrict__ pb, float* __restrict__ params_out) {
  const int64_t nvec = n >> 3;
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  vu4 a = {0u, 0u, 0u, 0u}, b = {0u, 0u, 0u, 0u};
  if (ALIGNED) {
    // unconditional loads, lanes past the end re-read the last vector (the launcher sends n < 8 to the element kernel)
    const int64_t idc = (idx < nvec) ? idx : nvec - 1;
    a = ld8<NTLD>(z, idc);
    if (HAS_ADD) b = ld8<NTLD>(addend, idc);
    __builtin_amdgcn_sched_barrier(0);
  }
  const float s = exp2f(*ps);
  const float qr = exp2f(*pq);
  const float zp = *pb, lo = zp;
  const float hi = (zp + qr) - s;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    params_out[0] = s; params_out[1] = zp; params_out[2] = lo; params_out[3] = hi; params_out[4] = qr;
  }
  FwdStats st{INFINITY, -INFINITY, false};
  if (ALIGNED) {
    if (idx < nvec) {
      vu4 o, av;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        float a0, a1;
        av[w] = relu_in2<DT, HAS_ADD>(a[w], b[w], a0, a1);
        const float r0 = fwd_elem<false>(a0, s, zp, lo, hi, st);
        const float r1 = fwd_elem<false>(a1, s, zp, lo, hi, st);
        o[w] = down2<DT>(r0, r1);
      }
      st8<true>(y, idx, o);
      if (WRITE_A) st8<true>(a_out, idx, av);
    }
    const int64_t t = (nvec << 3) + threadIdx.x;       // n % 8 tail elements
    if (blockIdx.x == 0 && t < n) {
      float av;
      const uint16_t ab = relu_in1<DT, HAS_ADD>(z[t], HAS_ADD ? addend[t] : (uint16_t)0, av);
      y[t] = down1<DT>(fwd_elem<false>(av, s, zp, lo, hi, st));
      if (WRITE_A) a_out[t] = ab;
    }
  } else {
    // pointers not 16-byte aligned (tensor views) / n < 8: element accesses, grid-stride
    for (int64_t i = idx; i < n; i += (int64_t)gridDim.x * kBlock) {
      float av;
      const uint16_t ab = relu_in1<DT, HAS_ADD>(z[i], HAS_ADD ? addend[i] : (uint16_t)0, av);
      y[i] = down1<DT>(fwd_elem<false>(av, s, zp, lo, hi, st));
      if (WRITE_A) a_out[i] = ab;
    }
  }
}

// =============================================================== backward, plain and ReLU forms
// what the two forms feed the element bodies and store: x or relu(z); the rounded result, or that with g_a and the mask
template <bool RELU>
__device__ __forceinline__ float act_in(float x) { return RELU ? relu_elem(x) : x; }
template <int DT, bool RELU, bool HAS_GA>
__device__ __forceinline__ uint32_t bwd_out2(float q0, float q1, uint32_t cw, float x0, float x1) {
  return RELU ? relu_out2<DT, HAS_GA>(q0, q1, cw, x0, x1) : down2<DT>(q0, q1);
}
template <int DT, bool RELU, bool HAS_GA>
__device__ __forceinline__ uint16_t bwd_out1(float q, uint16_t c, float x) {
  return RELU ? relu_out1<DT, HAS_GA>(q, c, x) : down1<DT>(q);
}

// The backward of both forms.  RELU: x is the ReLU's input z, the element bodies see relu(z) and the store adds g_a
// (HAS_GA) and masks; everything that reaches the partial rows is the same code either way.  RSIGN: the caller's signs
// (r_sign, one int8 per element) instead of the in-kernel stream.  Instantiated for the plain kernel with
// <RELU = false, HAS_GA = false> and for the ReLU kernel with <RSIGN = false>; BIG only with ALIGNED.
// nblk is gridDim.x, read by the kernel: read in here, the compiler no longer reduces the launch-geometry queries of
// the epilogues (this one and block_sum_f32's blockDim.x) to one scalar load each, and every wave of the BIG form then
// waits on a dependent global load, and with it on its own stores, before the block sum (1-3 % of the launch).
template <int DT, int METHOD, bool RELU, bool RSIGN, bool ALIGNED, bool HAS_GA, bool BIG>
__device__ __forceinline__ void x16_bwd_body(
    const uint16_t* __restrict__ x, const uint16_t* __restrict__ g, const uint16_t* __restrict__ ga,
    uint16_t* __restrict__ gx, int64_t n, const float* __restrict__ params, const int8_t* __restrict__ r_sign,
    uint64_t seed, uint64_t offset, const uint64_t* __restrict__ offset_dev, float* __restrict__ partials,
    const int64_t nblk) {
  constexpr bool NEED_R = (METHOD != MHAQ_FQ_LSQ);
  constexpr bool FAST_METHOD = (METHOD == MHAQ_FQ_STE || METHOD == MHAQ_FQ_LSQ);
  constexpr int U = bwd_u(BIG);
  constexpr int kTileCalls = 16 * U;              // 2048 * U elements per block / 128 per call
  float acc[kAcc] = {0.f, 0.f, 0.f, 0.f};
  const int64_t nvec = n >> 3;
  const int64_t base = (int64_t)blockIdx.x * (kBlock * U) + threadIdx.x;
  const bool full = ((int64_t)blockIdx.x + 1) * (kBlock * U) <= nvec;
  vu4 a[U], b[U], c[U];
  uint64_t rs[U];
  if (ALIGNED) {
    // unconditional loads, all in flight before anything waits; lanes past the end re-read the last vector (fq_pt.hip);
    // the launcher sends n < 8 to the element kernel, so nvec >= 1 here
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t idx = base + u * kBlock;
      const int64_t idc = (full || idx < nvec) ? idx : nvec - 1;
      a[u] = ld8<true>(x, idc);
      b[u] = ld8<true>(g, idc);
      if (HAS_GA) c[u] = ld8<true>(ga, idc);
      else c[u] = vu4{0u, 0u, 0u, 0u};
      if (NEED_R && RSIGN) rs[u] = reinterpret_cast<const uint64_t*>(r_sign)[idc];
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  offset = stream_offset(offset, offset_dev);
  const float p_s = params[0], p_zp = params[1], p_lo = params[2], p_hi = params[3];
  __shared__ __align__(16) uint32_t stile[4 * kTileCalls];
  if (ALIGNED && NEED_R && !RSIGN) {
    sign_tile_fill(stile, (int64_t)blockIdx.x * kTileCalls, kTileCalls, seed, offset);
    __syncthreads();
  }
  const BwdCtx k = make_bwd_ctx(p_s, p_zp, p_lo, p_hi);

  if (ALIGNED) {
    // this lane's sign byte: vector u*256 + t of the block = bits [8*(u*256 + t), +8) of the tile, inverted once
    uint32_t nb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      nb[u] = 0;
      if (NEED_R && !RSIGN) nb[u] = ~(stile[(u * kBlock + (int)threadIdx.x) >> 2] >> (((int)threadIdx.x & 3) * 8));
    }
    const bool fast = FAST_METHOD && k.fast_div && (k.lo < k.hi) && (k.s > 0.f);      // wave-uniform
    if (FAST_METHOD && fast) {
      const float hcs = (MHAQ_INV_SQRT3 * k.s) * 0.5f;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t idx = base + u * kBlock;
        if (full || idx < nvec) {
          vu4 o;
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            float x0, x1, g0, g1;
            up2<DT>(a[u][w], x0, x1);
            up2<DT>(b[u][w], g0, g1);
            float rc0 = 0.f, rc1 = 0.f;
            if (NEED_R) {
              if (RSIGN) {
                rc0 = ((int8_t)((rs[u] >> (16 * w)) & 0xff) > 0) ? hcs : -hcs;
                rc1 = ((int8_t)((rs[u] >> (16 * w + 8)) & 0xff) > 0) ? hcs : -hcs;
              } else {
                rc0 = signed_half_scale(nb[u], 2 * w, hcs);
                rc1 = signed_half_scale(nb[u], 2 * w + 1, hcs);
              }
            }
            const float y0 = bwd_elem_fast<METHOD>(act_in<RELU>(x0), g0, rc0, k, acc);
            const float y1 = bwd_elem_fast<METHOD>(act_in<RELU>(x1), g1, rc1, k, acc);
            o[w] = bwd_out2<DT, RELU, HAS_GA>(y0, y1, c[u][w], x0, x1);
          }
          st8<true>(gx, idx, o);
        }
      }
    } else {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t idx = base + u * kBlock;
        if (full || idx < nvec) {
          vu4 o;
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            float x0, x1, g0, g1;
            up2<DT>(a[u][w], x0, x1);
            up2<DT>(b[u][w], g0, g1);
            float r0 = 0.f, r1 = 0.f;
            if (NEED_R) {
              if (RSIGN) {
                r0 = sign_half((int8_t)((rs[u] >> (16 * w)) & 0xff));
                r1 = sign_half((int8_t)((rs[u] >> (16 * w + 8)) & 0xff));
              } else {
                const uint32_t bits = ~nb[u];
                r0 = ((bits >> (2 * w)) & 1u) ? 0.5f : -0.5f;
                r1 = ((bits >> (2 * w + 1)) & 1u) ? 0.5f : -0.5f;
              }
            }
            const float y0 = bwd_elem<METHOD>(act_in<RELU>(x0), g0, r0, 0.f, k, acc);
            const float y1 = bwd_elem<METHOD>(act_in<RELU>(x1), g1, r1, 0.f, k, acc);
            o[w] = bwd_out2<DT, RELU, HAS_GA>(y0, y1, c[u][w], x0, x1);
          }
          st8<true>(gx, idx, o);
        }
      }
    }
    const int64_t t = (nvec << 3) + threadIdx.x;
    if (blockIdx.x == 0 && t < n) {   // n % 8 tail elements
      float r = 0.f;
      if (NEED_R) r = RSIGN ? sign_half(r_sign[t]) : philox_r(t, seed, offset);
      const float xx = up1<DT>(x[t]);
      const float v = bwd_elem<METHOD>(act_in<RELU>(xx), up1<DT>(g[t]), r, 0.f, k, acc);
      gx[t] = bwd_out1<DT, RELU, HAS_GA>(v, HAS_GA ? ga[t] : (uint16_t)0, xx);
    }
    // partial rows in the ACT layout: one per block (fp64 totals) in the BIG form, one per wave below it
    if (BIG) {
      __shared__ float smf[kAcc * (kBlock / 64)];
      double tot[kAcc];
      block_sum_f32<kAcc>(acc, tot, smf);
      if (threadIdx.x == 0) write_act_partials(partials, tot, nblk, (int64_t)blockIdx.x);
      publish_act_scales(partials, params, nblk);
    } else {
      float wsum[kAcc];
#pragma unroll
      for (int q = 0; q < kAcc; ++q) wsum[q] = wave_sum_dpp(acc[q]);
      const int64_t nrows = nblk * (kBlock / 64);
      if ((threadIdx.x & 63) == 0)
        write_act_partials(partials, wsum, nrows, (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6));
      publish_act_scales(partials, params, nrows);
    }
  } else {
    // unaligned tensor views / n < 8: element accesses, grid-stride, fp64 per-thread accumulators, one row per block
    double dacc[kAcc] = {0, 0, 0, 0};
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += nblk * kBlock) {
      float r = 0.f;
      if (NEED_R) r = RSIGN ? sign_half(r_sign[i]) : philox_r(i, seed, offset);
      const float xx = up1<DT>(x[i]);
      float a1[kAcc] = {0.f, 0.f, 0.f, 0.f};
      const float v = bwd_elem<METHOD>(act_in<RELU>(xx), up1<DT>(g[i]), r, 0.f, k, a1);
      gx[i] = bwd_out1<DT, RELU, HAS_GA>(v, HAS_GA ? ga[i] : (uint16_t)0, xx);
#pragma unroll
      for (int q = 0; q < kAcc; ++q) dacc[q] += (double)a1[q];
    }
    __shared__ double sm[kAcc * (kBlock / 64)];
    block_sum<kAcc>(dacc, sm);
    if (threadIdx.x == 0) write_act_partials(partials, dacc, nblk, (int64_t)blockIdx.x);
    publish_act_scales(partials, params, nblk);
  }
}

// The two kernels are that body behind their own names and argument lists (profiles name them; with kernarg preload the
// argument layout is part of the code).  Occupancy by size as fq_pt.hip pt_bwd_kernel: at least 8 waves per SIMD on the
// latency-limited small tensors, at most 6 on the bandwidth-limited big ones (the element kernel of unaligned views
// carries no lower bound).
#define MHAQ_X16_BWD_OCC \
  __attribute__((amdgpu_waves_per_eu(((BIG || !ALIGNED) ? 1 : 8), (BIG ? 6 : 8)))) __launch_bounds__(kBlock)

template <int DT, int METHOD, bool RSIGN, bool ALIGNED, bool BIG>
__global__ MHAQ_X16_BWD_OCC void x16_act_bwd_kernel(
    const uint16_t* __restrict__ x, const uint16_t* __restrict__ g, uint16_t* __restrict__ gx, int64_t n,
    const float* __restrict__ params, const int8_t* __restrict__ r_sign, uint64_t seed, uint64_t offset,
    const uint64_t* __restrict__ offset_dev, float* __restrict__ partials) {
  x16_bwd_body<DT, METHOD, false, RSIGN, ALIGNED, false, BIG>(x, g, nullptr, gx, n, params, r_sign, seed, offset,
                                                              offset_dev, partials, (int64_t)gridDim.x);
}

template <int DT, int METHOD, bool ALIGNED, bool HAS_GA, bool BIG>
__global__ MHAQ_X16_BWD_OCC void x16_act_relu_bwd_kernel(
    const uint16_t* __restrict__ z, const uint16_t* __restrict__ g, const uint16_t* __restrict__ ga,
    uint16_t* __restrict__ gx, int64_t n, const float* __restrict__ params, uint64_t seed, uint64_t offset,
    const uint64_t* __restrict__ offset_dev, float* __restrict__ partials) {
  x16_bwd_body<DT, METHOD, true, false, ALIGNED, HAS_GA, BIG>(z, g, ga, gx, n, params, nullptr, seed, offset,
                                                              offset_dev, partials, (int64_t)gridDim.x);
}

// fq_pt.hip act_finalize_kernel: column sums -> {dL/dlog_act_s, dL/dlog_act_q, dL/dact_b}, same partition and order
__global__ __launch_bounds__(kFinalThreads) void x16_act_finalize_kernel(const float* __restrict__ partials, int nparts,
                                                                          const float* __restrict__ params,
                                                                          float* __restrict__ out) {
  const float* col = partials + (int64_t)blockIdx.x * nparts;
  double v[1] = {0.0};
  int i = threadIdx.x;
  for (; i + 7 * kFinalThreads < nparts; i += 8 * kFinalThreads) {
    float t[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = col[i + j * kFinalThreads];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[0] += (double)t[j];
  }
  for (; i < nparts; i += kFinalThreads) v[0] += (double)col[i];
  __shared__ double sm[kFinalThreads / 64];
  block_sum<1>(v, sm);
  if (threadIdx.x == 0) {
    const float gs = (float)v[0];
    if (blockIdx.x == 0) out[0] = (gs * params[0]) * 0.69314718055994531f;
    else if (blockIdx.x == 1) out[1] = (gs * params[4]) * 0.69314718055994531f;
    else out[2] = gs;
  }
}

// ---------------------------------------------------------------- host side
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }
inline bool aligned2(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 1u) == 0; }
inline int64_t blocks8(int64_t n, int u) {          // blocks of 256 * u lanes x 8 elements
  const int64_t per = (int64_t)kBlock * u;
  const int64_t b = ((n >> 3) + per - 1) / per;
  return b < 1 ? 1 : b;
}
inline int64_t simple_grid(int64_t n) {            // fq_pt.hip simple_grid
  int64_t b = (n + kBlock - 1) / kBlock;
  if (b < 1) b = 1;
  if (b > kMaxBlocks) b = kMaxBlocks;
  return b;
}

// A runtime value as a template argument, as with_dtype (fq_io16.hpp): the entry points have checked the method before
// they get here.
template <class F>
void with_method(int method, F f) {
  switch (method) {
    case MHAQ_FQ_STE: f(std::integral_constant<int, MHAQ_FQ_STE>{}); break;
    case MHAQ_FQ_EWGS: f(std::integral_constant<int, MHAQ_FQ_EWGS>{}); break;
    default: f(std::integral_constant<int, MHAQ_FQ_LSQ>{}); break;
  }
}
// f(ALIGNED, SECOND): the element kernel has one form, the aligned kernel two by size (NTLD forward, BIG backward)
template <class F>
void with_form(bool aligned, bool second, F f) {
  if (!aligned) f(std::false_type{}, std::false_type{});
  else if (second) f(std::true_type{}, std::true_type{});
  else f(std::true_type{}, std::false_type{});
}

// One backward call of either form: the plain one has no g_a, the ReLU one no caller-supplied signs.
struct BwdCall {
  const void *x, *g, *ga;
  void* gx;
  int64_t n;
  int dtype;
  const float* params;
  int method;
  bool relu;
  const int8_t* r_sign;
  uint64_t seed, offset;
  const uint64_t* offset_dev;
  void* workspace;
  size_t workspace_bytes;
  void* stream;
};

// (dtype, method, relu, r_sign, g_a, aligned, big) -> the instantiation.  Nothing else instantiates a backward kernel,
// so there is no <RELU, RSIGN = true> and no <ALIGNED = false, BIG = true> in the library.
inline void launch_bwd(const BwdCall& c, int grid, bool al, bool big) {
  const uint16_t *x = (const uint16_t*)c.x, *g = (const uint16_t*)c.g, *ga = (const uint16_t*)c.ga;
  uint16_t* gx = (uint16_t*)c.gx;
  float* parts = (float*)c.workspace;
  hipStream_t st = (hipStream_t)c.stream;
  with_dtype(c.dtype, [&](auto dt) {
    with_method(c.method, [&](auto m) {
      with_form(al, big, [&](auto a, auto bg) {
        constexpr int DT = decltype(dt)::value, M = decltype(m)::value;
        constexpr bool AL = decltype(a)::value, BG = decltype(bg)::value;
        if (c.relu)
          MHAQ_LAUNCH((ga ? x16_act_relu_bwd_kernel<DT, M, AL, true, BG>
                          : x16_act_relu_bwd_kernel<DT, M, AL, false, BG>),
                      dim3(grid), dim3(kBlock), 0, st, x, g, ga, gx, c.n, c.params, c.seed, c.offset, c.offset_dev,
                      parts);
        else
          MHAQ_LAUNCH((c.r_sign ? x16_act_bwd_kernel<DT, M, true, AL, BG>
                                : x16_act_bwd_kernel<DT, M, false, AL, BG>),
                      dim3(grid), dim3(kBlock), 0, st, x, g, gx, c.n, c.params, c.r_sign, c.seed, c.offset,
                      c.offset_dev, parts);
      });
    });
  });
}

// mhaq_fq_act_bwd_partials_x16 / mhaq_fq_act_relu_bwd_partials_x16: checks (in the order include/mhaq_fq.h gives their
// codes), geometry, launch.
inline int bwd_partials(const BwdCall& c, int32_t* nparts_out) {
  const int64_t n = c.n;
  if (n < 0 || !c.params || (n > 0 && (!c.x || !c.g || !c.gx))) return MHAQ_FQ_EINVAL;
  if (!known_dtype(c.dtype)) return MHAQ_FQ_EINVAL;
  if (c.method != MHAQ_FQ_STE && c.method != MHAQ_FQ_LSQ && c.method != MHAQ_FQ_EWGS)
    return (c.method == MHAQ_FQ_AEWGS) ? MHAQ_FQ_EUNSUPPORTED : MHAQ_FQ_EINVAL;
  if (!aligned2(c.x) || !aligned2(c.g) || !aligned2(c.ga) || !aligned2(c.gx)) return MHAQ_FQ_EALIGN;
  if (!c.workspace || c.workspace_bytes < mhaq_fq_act_bwd_workspace_bytes(n)) return MHAQ_FQ_EWORKSPACE;
  const bool al = n >= 8 && aligned16(c.x) && aligned16(c.g) && aligned16(c.gx) && (!c.ga || aligned16(c.ga)) &&
                  (!c.r_sign || aligned8(c.r_sign));
  const bool big = al && n >= kBwdBigElems;
  const int64_t grid64 = al ? blocks8(n, bwd_u(big)) : simple_grid(n);
  if (grid64 > 0x7fffffff) return MHAQ_FQ_EUNSUPPORTED;
  // partial rows: one per wave of the aligned kernel below kBwdBigElems, one per block from there up and in the element
  // kernel -- at most the fp32 launch's count, so the fp32 workspace query serves (checked, not assumed)
  const int64_t rows64 = (al && !big) ? grid64 * (kBlock / 64) : grid64;
  if (rows64 > 0x7fffffff) return MHAQ_FQ_EUNSUPPORTED;
  if ((size_t)(3 * rows64 + 2) * sizeof(float) > c.workspace_bytes) return MHAQ_FQ_EWORKSPACE;
  if (nparts_out) *nparts_out = (int32_t)rows64;
  launch_bwd(c, (int)grid64, al, big);
  return launch_status();
}

// mhaq_fq_act_bwd_x16 / mhaq_fq_act_relu_bwd_x16: the partial rows, then their column sums
inline int bwd_with_finalize(const BwdCall& c, float* grads) {
  if (!grads) return MHAQ_FQ_EINVAL;
  int32_t nparts = 0;
  const int rc = bwd_partials(c, &nparts);
  if (rc) return rc;
  MHAQ_LAUNCH(x16_act_finalize_kernel, dim3(3), dim3(kFinalThreads), 0, (hipStream_t)c.stream,
              (const float*)c.workspace, (int)nparts, c.params, grads);
  return launch_status();
}

}  // namespace io16
}  // namespace mhaq

using namespace mhaq;

extern "C" {

int mhaq_fq_act_fwd_x16(const void* x, void* y, int64_t n, int dtype, const float* log_s, const float* log_q,
                        const float* b, float* params_out, float* qstats, int32_t* flags, void* workspace,
                        size_t workspace_bytes, void* stream) {
  if (n < 0 || !log_s || !log_q || !b || !params_out || (n > 0 && (!x || !y))) return MHAQ_FQ_EINVAL;
  if (!io16::known_dtype(dtype)) return MHAQ_FQ_EINVAL;
  if (!io16::aligned2(x) || !io16::aligned2(y)) return MHAQ_FQ_EALIGN;
  const bool stats = qstats || flags;
  if (stats && (!workspace || workspace_bytes < mhaq_fq_pt_fwd_workspace_bytes(n))) return MHAQ_FQ_EWORKSPACE;
  const bool al = io16::aligned16(x) && io16::aligned16(y);
  const int64_t grid64 = al ? io16::blocks8(n, stats ? io16::kFwdStatsU : io16::kFwdU) : io16::simple_grid(n);
  if (grid64 > 0x7fffffff) return MHAQ_FQ_EUNSUPPORTED;
  // the workspace rule (include/mhaq_fq.h): never more partial rows than the fp32 launch over the same n
  if (stats && (size_t)grid64 * 3 * sizeof(float) > workspace_bytes) return MHAQ_FQ_EWORKSPACE;
  const int grid = (int)grid64;
  hipStream_t st = (hipStream_t)stream;
  float* parts = (float*)workspace;
  const uint16_t* xs = (const uint16_t*)x;
  uint16_t* ys = (uint16_t*)y;
  io16::with_dtype(dtype, [&](auto dt) {
    io16::with_form(al, n > io16::kFwdPlainLoadElems, [&](auto a, auto nt) {
      constexpr int DT = decltype(dt)::value;
      constexpr bool AL = decltype(a)::value, NT = decltype(nt)::value;
      MHAQ_LAUNCH((stats ? io16::x16_act_fwd_kernel<DT, true, AL, NT, io16::kFwdStatsU>
                         : io16::x16_act_fwd_kernel<DT, false, AL, NT, io16::kFwdU>),
                  dim3(grid), dim3(kBlock), 0, st, xs, ys, n, log_s, log_q, b, parts, params_out);
    });
  });
  int rc = launch_status();
  if (rc) return rc;
  if (stats) {
    MHAQ_LAUNCH(io16::x16_fwd_finalize_kernel, dim3(3), dim3(io16::kFinalThreads), 0, st, parts, grid, qstats, flags);
    rc = launch_status();
  }
  return rc;
}

int mhaq_fq_act_bwd_partials_x16(const void* x, const void* g, void* gx, int64_t n, int dtype, const float* params,
                                 int method, const int8_t* r_sign, uint64_t seed, uint64_t offset,
                                 const uint64_t* offset_dev, void* workspace, size_t workspace_bytes,
                                 int32_t* nparts_out, void* stream) {
  return io16::bwd_partials({x, g, nullptr, gx, n, dtype, params, method, false, r_sign, seed, offset, offset_dev,
                             workspace, workspace_bytes, stream}, nparts_out);
}

int mhaq_fq_act_bwd_x16(const void* x, const void* g, void* gx, int64_t n, int dtype, const float* params, int method,
                        const int8_t* r_sign, uint64_t seed, uint64_t offset, const uint64_t* offset_dev, float* grads,
                        void* workspace, size_t workspace_bytes, void* stream) {
  return io16::bwd_with_finalize({x, g, nullptr, gx, n, dtype, params, method, false, r_sign, seed, offset, offset_dev,
                                  workspace, workspace_bytes, stream}, grads);
}

// ---- ReLU (+ residual add) fused into the 16-bit NoisyAct launches (x16_act_relu_fwd_kernel / x16_act_relu_bwd_kernel)
int mhaq_fq_act_relu_fwd_x16(const void* z, const void* addend, void* y, void* a_out, int64_t n, int dtype,
                             const float* log_s, const float* log_q, const float* b, float* params_out, void* stream) {
  if (n < 0 || !log_s || !log_q || !b || !params_out || (n > 0 && (!z || !y))) return MHAQ_FQ_EINVAL;
  if (!io16::known_dtype(dtype)) return MHAQ_FQ_EINVAL;
  if (!io16::aligned2(z) || !io16::aligned2(addend) || !io16::aligned2(y) || !io16::aligned2(a_out))
    return MHAQ_FQ_EALIGN;
  const bool al = n >= 8 && io16::aligned16(z) && io16::aligned16(y) && (!addend || io16::aligned16(addend)) &&
                  (!a_out || io16::aligned16(a_out));
  const int64_t grid64 = al ? io16::blocks8(n, io16::kFwdU) : io16::simple_grid(n);
  if (grid64 > 0x7fffffff) return MHAQ_FQ_EUNSUPPORTED;
  const int grid = (int)grid64;
  hipStream_t st = (hipStream_t)stream;
  const uint16_t *zs = (const uint16_t*)z, *ds = (const uint16_t*)addend;
  uint16_t *ys = (uint16_t*)y, *as = (uint16_t*)a_out;
  io16::with_dtype(dtype, [&](auto dt) {
    io16::with_form(al, n > io16::kFwdPlainLoadElems, [&](auto a, auto nt) {
      constexpr int DT = decltype(dt)::value;
      constexpr bool AL = decltype(a)::value, NT = decltype(nt)::value;
      MHAQ_LAUNCH((ds ? (as ? io16::x16_act_relu_fwd_kernel<DT, true, true, AL, NT>
                            : io16::x16_act_relu_fwd_kernel<DT, true, false, AL, NT>)
                      : (as ? io16::x16_act_relu_fwd_kernel<DT, false, true, AL, NT>
                            : io16::x16_act_relu_fwd_kernel<DT, false, false, AL, NT>)),
                  dim3(grid), dim3(kBlock), 0, st, zs, ds, ys, as, n, log_s, log_q, b, params_out);
    });
  });
  return launch_status();
}

int mhaq_fq_act_relu_bwd_partials_x16(const void* z, const void* g_y, const void* g_a, void* gx, int64_t n, int dtype,
                                      const float* params, int method, uint64_t seed, uint64_t offset,
                                      const uint64_t* offset_dev, void* workspace, size_t workspace_bytes,
                                      int32_t* nparts_out, void* stream) {
  return io16::bwd_partials({z, g_y, g_a, gx, n, dtype, params, method, true, nullptr, seed, offset, offset_dev,
                             workspace, workspace_bytes, stream}, nparts_out);
}

int mhaq_fq_act_relu_bwd_x16(const void* z, const void* g_y, const void* g_a, void* gx, int64_t n, int dtype,
                             const float* params, int method, uint64_t seed, uint64_t offset,
                             const uint64_t* offset_dev, float* grads, void* workspace, size_t workspace_bytes,
                             void* stream) {
  return io16::bwd_with_finalize({z, g_y, g_a, gx, n, dtype, params, method, true, nullptr, seed, offset, offset_dev,
                                  workspace, workspace_bytes, stream}, grads);
}

}  // extern "C"

