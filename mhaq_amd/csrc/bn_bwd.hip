// The BatchNorm kernels for gfx950, and the stem's max pool that some of them absorb.  Every tensor is dense NHWC seen as
// [M = N*H*W][C]: fp32 with C % 4 == 0, or bf16 / fp16 with C % 8 == 0 -- a lane owns 16 bytes of a row either way, and every
// streaming kernel is written ONCE over that element type (IoF32 / Io16<dtype>, "the element type" below).  A 16-bit element
// is converted UP exactly and takes the fp32 arithmetic unchanged; a result is rounded to nearest-even ONCE on the way out
// (IO::pack: a plain cast, NaN stays NaN, fp16 overflow gives +-inf).  Statistics, weight, bias, their gradients, the constant
// rows and the workspaces stay fp32 / fp64.  In the order of the file:
//
// The backward of training-mode BatchNorm (mhaq_fq_bn_bwd*), three bandwidth-bound launches in place of the framework's:
//   bn_bwd_reduce_kernel     one read of x and dy   -> per-block fp64 partial rows of  sum dy  and  sum dy * (x - mean)
//   bn_bwd_finalize_kernel   fixed-order fp64 sum of the partial rows -> dbias, dweight, per-channel constants
//   bn_bwd_dx_kernel         a 2R1W stream in the shape of pt_bwd_kernel (fq_pt.hip):
//                            dx = (gamma * invstd) * ((dy - dbias / M) - ((x - mean) * invstd) * (dweight / M))
// The mean is NOT folded into an additive constant (B * x + D cancels when |mean| >> sigma): every term above is the
// closed form's own, so the error of dx is bounded on |dy| + |dbias| / M + |xhat| * |dweight| / M.
// Deterministic: fixed partition, fixed-order sums, no float atomics, no last-block ticket.
// Where dy comes from is a template argument of the two streaming kernels: a tensor in memory (DyMem / DyMem16) or the
// gradient of a 3x3 / stride 2 / padding 1 max pool behind the BatchNorm, gathered on the fly from the pooled gradient and a
// 1-byte argmax code per output (DyPool, mhaq_fq_bn_pool_bwd; the codes are written by maxpool3s2_fwd_kernel).  The element
// type comes with the source (Dy::IO); partition, sums, finalize and the dx expression are one code for all of them.  The
// pool's gather on 16-bit tensors (DyPool16, mhaq_fq_bn_pool_bwd_x16) rounds its dy to 16 bits in registers where the
// framework's pool backward rounds the tensor it would have written.
//
// The training forward (opt-in: mhaq_fq_bn_fwd*; by default it stays with the framework, which saves the batch mean and
// invstd): bn_fwd_reduce_kernel, bn_fwd_finalize_kernel, bn_fwd_norm_kernel over the backward's partition.
//
// The frozen forward (mhaq_fq_bn_infer_*: the teacher): eval-mode BatchNorm from the running statistics with the ReLU and
// the residual add behind it in one launch, bn_infer_act_kernel, and with the stem's pool, bn_relu_pool3s2_kernel.
//
// The pool's forward (mhaq_fq_maxpool3s2_fwd*): values and argmax codes, maxpool3s2_fwd_kernel; taken of the training
// forward's output without storing it, the pooled stem forward (PoolOfNorm, mhaq_fq_bn_norm_pool3s2_fwd_x16).
//
// The host side is written once per family ("the host path of the entry points" at the end): a status function holds the
// argument checks of the fp32 and the *_x16 entry point in the order include/mhaq_fq.h promises -- bn_bwd_status of all four
// backward forms, pool_fwd_status of the pool forwards (the pooled stem forward included), bn_relu_pool_status of the frozen
// stem --, bn_workspace_bytes stands behind the four backward workspace queries, and io16::with_dtype (fq_io16.hpp) turns the
// dtype of an *_x16 call into the template argument, so that every launch is named in one place.
#include "fq_io16.hpp"

// The two tunables of the 16-bit pool gather (DyPool16), overridable at build time: tools/stem_pool_bench.py --dtype bf16 times
// builds with other values next to the product's.  Rows in flight in the reduction (2: 163 VGPRs, 3 waves / SIMD; 4: 229 VGPRs,
// 2 waves; neither spills) and the cache policy of the loads of g and the codes (default: their 2.25-fold re-read has to hit
// cache).
#ifndef MHAQ_BN_POOL16_RED_U
#define MHAQ_BN_POOL16_RED_U 2
#endif
#ifndef MHAQ_BN_POOL16_G_NT
#define MHAQ_BN_POOL16_G_NT 0
#endif

namespace mhaq {

// 16 B / lane accesses with the cache policy as a template argument (as ld4 / st4 of fq_pt.hip)
template <bool NT>
__device__ __forceinline__ vf4 bn_ld4(const float* p, int64_t vidx) {
  const vf4* q = reinterpret_cast<const vf4*>(p) + vidx;
  return NT ? __builtin_nontemporal_load(q) : *q;
}
template <bool NT>
__device__ __forceinline__ void bn_st4(float* p, int64_t vidx, vf4 v) {
  vf4* q = reinterpret_cast<vf4*>(p) + vidx;
  if (NT) __builtin_nontemporal_store(v, q); else *q = v;
}

// ---------------------------------------------------------------- the element type of the streamed tensors
// One 16-byte access of a lane: kW elements, unpacked to / packed from fp32 (16-bit elements: converted up exactly, rounded
// to nearest-even once by pack).  `st` is the non-temporal store of the training kernels, whose output nothing reads soon;
// `stv<NT>` stores a packed vector with the policy the caller names.
// For the pool forward: `Code` is one argmax byte per element of the lane; a 16-bit type also hands out the ORIGINAL 16 bits
// of element j of a vector (`bits`; an fp32 element is its own bits), packs eight of them again and names -inf in that form.
struct IoF32 {
  using T = float;
  using Vec = vf4;
  using Code = uint32_t;
  static constexpr int kW = 4;
  template <bool NT>
  static __device__ __forceinline__ Vec ld(const T* p, int64_t vidx) { return bn_ld4<NT>(p, vidx); }
  static __device__ __forceinline__ void unpack(const Vec& v, float (&o)[4]) {
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  }
  static __device__ __forceinline__ Vec pack(const float (&o)[4]) { return vf4{o[0], o[1], o[2], o[3]}; }
  template <bool NT>
  static __device__ __forceinline__ void stv(T* p, int64_t vidx, Vec v) { bn_st4<NT>(p, vidx, v); }
  static __device__ __forceinline__ void st(T* p, int64_t vidx, const float (&o)[4]) { stv<true>(p, vidx, pack(o)); }
  static __device__ __forceinline__ Code pack_codes(const uint32_t (&cd)[4]) {
    return cd[0] | (cd[1] << 8) | (cd[2] << 16) | (cd[3] << 24);
  }
};
template <int DT>
struct Io16 {
  typedef uint32_t vu2 __attribute__((ext_vector_type(2)));
  using T = uint16_t;
  using Vec = io16::vu4;
  using Code = vu2;
  static constexpr int kW = 8;
  static constexpr uint32_t kNegInfBits = DT == MHAQ_FQ_DT_BF16 ? 0xFF80u : 0xFC00u;
  template <bool NT>
  static __device__ __forceinline__ Vec ld(const T* p, int64_t vidx) { return io16::ld8<NT>(p, vidx); }
  static __device__ __forceinline__ void unpack(const Vec& v, float (&o)[8]) {
#pragma unroll
    for (int w = 0; w < 4; ++w) io16::up2<DT>(v[w], o[2 * w], o[2 * w + 1]);
  }
  static __device__ __forceinline__ Vec pack(const float (&o)[8]) {
    Vec v;
#pragma unroll
    for (int w = 0; w < 4; ++w) v[w] = io16::down2<DT>(o[2 * w], o[2 * w + 1]);
    return v;
  }
  template <bool NT>
  static __device__ __forceinline__ void stv(T* p, int64_t vidx, Vec v) { io16::st8<NT>(p, vidx, v); }
  static __device__ __forceinline__ void st(T* p, int64_t vidx, const float (&o)[8]) { stv<true>(p, vidx, pack(o)); }
  static __device__ __forceinline__ uint32_t bits(const Vec& v, int j) { return (v[j >> 1] >> (16 * (j & 1))) & 0xFFFFu; }
  static __device__ __forceinline__ Vec from_bits(const uint32_t (&b)[8]) {
    Vec v;
#pragma unroll
    for (int w = 0; w < 4; ++w) v[w] = b[2 * w] | (b[2 * w + 1] << 16);
    return v;
  }
  static __device__ __forceinline__ Code pack_codes(const uint32_t (&cd)[8]) {
    return Code{cd[0] | (cd[1] << 8) | (cd[2] << 16) | (cd[3] << 24), cd[4] | (cd[5] << 8) | (cd[6] << 16) | (cd[7] << 24)};
  }
};

// ---------------------------------------------------------------- where dy comes from
// A source hands out, per 16-byte vector of x, a bundle of loads (issued with x's, before anything waits) and later the IO::kW dy
// values out of it.  `Walk` follows a lane's rows through the reduction: (n, ih, iw) of a row, advanced by a fixed row
// step without a division.
// dy as a tensor in memory, of the element type IOT
template <class IOT>
struct DyMemT {
  using IO = IOT;
  const typename IO::T* __restrict__ dy;
  // fp32: the occupancy the dx kernel is held to below kBnBigElems
  // 16-bit: 70 VGPRs (40 of them the constants of 8 channels): 8 waves would spill
  static constexpr int kDxWaves = IO::kW == 8 ? 6 : 8;
  static constexpr bool kGather = false;           // (the dx kernel hands a gathering source the pixel of each vector)
  struct Walk {
    __device__ __forceinline__ Walk(const DyMemT&, uint32_t, uint32_t) {}
    __device__ __forceinline__ void next() {}
  };
  struct Loads { typename IO::Vec v; };
  template <bool NT>
  __device__ __forceinline__ Loads load(int64_t vidx, const Walk&, bool, uint32_t, uint32_t) const {
    return Loads{IO::template ld<NT>(dy, vidx)};
  }
  template <bool NT>
  __device__ __forceinline__ Loads load_at_pixel(int64_t vidx, uint32_t, bool, uint32_t, uint32_t) const {
    return Loads{IO::template ld<NT>(dy, vidx)};
  }
  __device__ __forceinline__ void value(const Loads& l, float (&o)[IO::kW]) const { IO::unpack(l.v, o); }
};
using DyMem = DyMemT<IoF32>;                        // dy as an fp32 tensor in memory
template <int DT>
using DyMem16 = DyMemT<Io16<DT>>;                   // ... as a 16-bit one

// dy[n, ih, iw, .] of max_pool2d(kernel 3, stride 2, padding 1) from the pooled gradient g[n, oh, ow, .] and the argmax
// code (kh * 3 + kw of the chosen element, one byte per output element).  The windows that cover row ih are
//   oh = ih / 2          with kh = 1 + ih % 2, always there, and
//   oh = ih / 2 + 1      with kh = 0, for an odd ih when that row of windows exists,
// likewise along iw: 1, 2 or 4 candidates.  The value is that of the framework's channels_last backward, bit for bit: with ONE
// candidate window dy is its g where its code names (ih, iw) and 0.0f where not (no add: a -0.0f arrives as -0.0f); with
// more, dy = 0.0f and g of every candidate whose code names (ih, iw) is added in ascending oh, then ascending ow, in fp32.
// All four (g, code) pairs are loaded whatever the parity: a candidate that does not exist re-reads its neighbour's address
// and can match no code.
constexpr uint32_t kPoolNoCode = 0xFFu;           // codes are 0 .. 8, and kPoolNoneChosen:
constexpr uint32_t kPoolNoneChosen = 9u;          // a window that chose no element (maxpool3s2_fwd_kernel)
struct DyPool {
  using IO = IoF32;
  const float* __restrict__ g;
  const uint8_t* __restrict__ code;
  uint32_t h, w, oh, ow;
  static constexpr int kDxWaves = 5;               // 84 VGPRs with the gather's loads in flight: 8 waves would spill
  static constexpr bool kGather = true;
  struct Walk {
    uint32_t n, ih, iw, dn, dh, dw, h, w;
    // row -> (n, ih, iw) once per lane; step = dn * h * w + dh * w + dw
    template <class Src>
    __device__ __forceinline__ Walk(const Src& s, uint32_t row, uint32_t step) : h(s.h), w(s.w) {
      const uint32_t q = row / w, sq = step / w;
      iw = row - q * w;
      n = q / h;
      ih = q - n * h;
      dw = step - sq * w;
      dn = sq / h;
      dh = sq - dn * h;
    }
    __device__ __forceinline__ void next() {
      iw += dw;
      const bool cw = iw >= w;
      iw -= cw ? w : 0u;
      ih += dh + (cw ? 1u : 0u);
      const bool ch = ih >= h;                      // ih < 2 h: dh <= h - 1
      ih -= ch ? h : 0u;
      n += dn + (ch ? 1u : 0u);
    }
  };
  struct Loads { vf4 g[4]; uint32_t c[4]; uint32_t want; };      // want: the four codes to match, one byte each
  // the four candidate windows of (n, ih, iw): their pixels in g / code, and the code of each that names (ih, iw)
  struct Cand { uint32_t px[4]; uint32_t want; };
  static __device__ __forceinline__ Cand candidates(uint32_t n, uint32_t ih, uint32_t iw, bool ok, uint32_t oh, uint32_t ow) {
    if (!ok) n = ih = iw = 0u;                      // (a dropped row: any valid address)
    const uint32_t oa = ih >> 1, pa = iw >> 1;
    const bool vh = (ih & 1u) && oa + 1u < oh, vw = (iw & 1u) && pa + 1u < ow;
    const uint32_t ob = vh ? oa + 1u : oa, pb = vw ? pa + 1u : pa;
    const uint32_t kh = 1u + (ih & 1u), kw = 1u + (iw & 1u);
    const uint32_t w00 = kh * 3u + kw, w01 = vw ? kh * 3u : kPoolNoCode, w10 = vh ? kw : kPoolNoCode,
                   w11 = (vh && vw) ? 0u : kPoolNoCode;
    const uint32_t ra = (n * oh + oa) * ow, rb = (n * oh + ob) * ow;      // < n * h * w < 2^31
    return Cand{{ra + pa, ra + pb, rb + pa, rb + pb}, w00 | (w01 << 8) | (w10 << 16) | (w11 << 24)};
  }
  // one candidate window: its g is passed on, not added to 0.0f
  static __device__ __forceinline__ bool single(uint32_t want) { return (want >> 8) == 0xFFFFFFu; }
  // byte j of the result == 0: candidate k is the argmax of channel j (c: four codes of candidate k)
  static __device__ __forceinline__ uint32_t miss(uint32_t c, uint32_t want, int k) {
    return c ^ (((want >> (8 * k)) & 0xFFu) * 0x01010101u);
  }
  // dy of one channel from g of its four candidates: hit bit k says that candidate k's code names the element
  static __device__ __forceinline__ float gather(const float (&gk)[4], const bool (&hit)[4], bool one) {
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float sum = (k == 0 && one) ? gk[k] : acc + gk[k];
      acc = hit[k] ? sum : acc;                    // a select: an unselected NaN stays out
    }
    return acc;
  }
  __device__ __forceinline__ Loads load_at(uint32_t n, uint32_t ih, uint32_t iw, bool ok, uint32_t col, uint32_t cv) const {
    const Cand cd = candidates(n, ih, iw, ok, oh, ow);
    Loads l;
    l.want = cd.want;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t vidx = (int64_t)cd.px[k] * cv + col;
      l.g[k] = bn_ld4<false>(g, vidx);
      l.c[k] = reinterpret_cast<const uint32_t*>(code)[vidx];
    }
    return l;
  }
  template <bool NT>
  __device__ __forceinline__ Loads load(int64_t, const Walk& k, bool ok, uint32_t col, uint32_t cv) const {
    return load_at(k.n, k.ih, k.iw, ok, col, cv);
  }
  template <bool NT>
  __device__ __forceinline__ Loads load_at_pixel(int64_t, uint32_t pixel, bool ok, uint32_t col, uint32_t cv) const {
    const uint32_t q = pixel / w, n = q / h;
    return load_at(n, q - n * h, pixel - q * w, ok, col, cv);
  }
  __device__ __forceinline__ void value(const Loads& l, float (&o)[4]) const {
    uint32_t d[4];                                  // byte j of d[k] == 0: candidate k is the argmax of channel j
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = miss(l.c[k], l.want, k);
    const float gk[4][4] = {{l.g[0].x, l.g[1].x, l.g[2].x, l.g[3].x}, {l.g[0].y, l.g[1].y, l.g[2].y, l.g[3].y},
                            {l.g[0].z, l.g[1].z, l.g[2].z, l.g[3].z}, {l.g[0].w, l.g[1].w, l.g[2].w, l.g[3].w}};
    const bool one = single(l.want);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bool hit[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) hit[k] = ((d[k] >> (8 * j)) & 0xFFu) == 0u;
      o[j] = gather(gk[j], hit, one);
    }
  }
};

// The same gather on 16-bit tensors: g and dy of the element type DT, a lane owns 8 channels (one 16-byte load of g and one
// 8-byte load of codes per candidate window).  The framework's pool backward writes a 16-bit dy, and this source hands out
// the bits of that tensor, upcast: where ONE window covers (ih, iw) its g passes through unchanged (or +0.0); where two or
// four do, the framework adds up(g) of the windows whose code names the element in an fp32 accumulator that starts at 0.0f,
// in ascending oh, then ascending ow, and rounds the sum to 16 bits ONCE -- with its own conversions: fp16 the hardware's
// (io16::down1), bf16 the framework's software rounding, which gives the one quiet NaN 0x7FC0 for every NaN.
// A 1 x 1 plane is the exception to the first rule (`summed`): NHWC and NCHW are the same memory there, the framework takes
// its contiguous kernel, and that one sums and rounds every element: dy = R16(0.0f + up(g)), a -0.0 arrives as +0.0.
template <int DT>
struct DyPool16 {
  using IO = Io16<DT>;
  using vu2 = typename IO::Code;
  const uint16_t* __restrict__ g;
  const uint8_t* __restrict__ code;
  uint32_t h, w, oh, ow;
  bool summed;                                     // h == w == 1
  static constexpr int kDxWaves = 3;               // 133 VGPRs with the gather's loads of two vectors in flight: 4 waves spill
  static constexpr bool kGather = true;
  static constexpr bool kGNt = MHAQ_BN_POOL16_G_NT != 0;
  using Walk = DyPool::Walk;
  struct Loads { io16::vu4 g[4]; vu2 c[4]; uint32_t want; };
  __device__ __forceinline__ Loads load_at(uint32_t n, uint32_t ih, uint32_t iw, bool ok, uint32_t col, uint32_t cv) const {
    const DyPool::Cand cd = DyPool::candidates(n, ih, iw, ok, oh, ow);
    Loads l;
    l.want = cd.want;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t vidx = (int64_t)cd.px[k] * cv + col;
      l.g[k] = io16::ld8<kGNt>(g, vidx);
      const vu2* cq = reinterpret_cast<const vu2*>(code) + vidx;
      l.c[k] = kGNt ? __builtin_nontemporal_load(cq) : *cq;
    }
    return l;
  }
  template <bool NT>
  __device__ __forceinline__ Loads load(int64_t, const Walk& k, bool ok, uint32_t col, uint32_t cv) const {
    return load_at(k.n, k.ih, k.iw, ok, col, cv);
  }
  template <bool NT>
  __device__ __forceinline__ Loads load_at_pixel(int64_t, uint32_t pixel, bool ok, uint32_t col, uint32_t cv) const {
    const uint32_t q = pixel / w, n = q / h;
    return load_at(n, q - n * h, pixel - q * w, ok, col, cv);
  }
  // the fp32 sum as the framework stores it in a 16-bit dy, upcast again
  static __device__ __forceinline__ float round16(float f) {
    if constexpr (DT == MHAQ_FQ_DT_BF16) return io16::up1<DT>(f != f ? (uint16_t)0x7FC0u : io16::down1<DT>(f));
    else return io16::up1<DT>(io16::down1<DT>(f));
  }
  __device__ __forceinline__ void value(const Loads& l, float (&o)[8]) const {
    uint32_t d[4][2];                               // byte j of d[k][j / 4]: DyPool::miss
    float gk[4][8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      d[k][0] = DyPool::miss(l.c[k].x, l.want, k);
      d[k][1] = DyPool::miss(l.c[k].y, l.want, k);
      IO::unpack(l.g[k], gk[k]);
    }
    const bool one = DyPool::single(l.want) && !summed;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float gj[4] = {gk[0][j], gk[1][j], gk[2][j], gk[3][j]};
      bool hit[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) hit[k] = ((d[k][j >> 2] >> (8 * (j & 3))) & 0xFFu) == 0u;
      const float acc = DyPool::gather(gj, hit, one);
      o[j] = one ? acc : round16(acc);             // (one window: g itself or +0.0, already a 16-bit value)
    }
  }
};

// ---------------------------------------------------------------- geometry of the reduction
// A block of the reduction owns `rows` consecutive rows of up to kBnCols float4 columns (64 channels: 256 contiguous
// bytes of a row, two whole cache lines; narrower tensors are read as one contiguous range).  Its 256 threads form
// 256 / cols rows of lanes; a lane keeps its 4 channels and walks down the rows, kBnRedU rows in flight per stream.
//   rows >= kBnMinRows: the partial rows ([2][C] doubles per row chunk) stay below 4 / 448 = 0.9 % of the tensor's bytes
//   row chunks <= kBnMaxChunks: a few rows per thread for the finalize
// The column split buys blocks where the 1 % rule leaves few row chunks: [12250][512] is 28 row chunks x 8 column chunks.
constexpr int kBnCols = 16;
constexpr int kBnRedU = 4;
constexpr int kBnPoolRedU = 4;        // rows in flight with the pool's gather (9 loads per row, 163 VGPRs, no scratch); 2 measured the same
constexpr int kBnPool16RedU = MHAQ_BN_POOL16_RED_U;      // ... and with the 16-bit gather (DyPool16)
constexpr int kBnMinRows = 448;
constexpr int kBnMaxChunks = 2048;
constexpr int kBnDxU = 2;             // 16-byte vectors per lane and stream in the dx kernel (kBwdU of fq_pt.hip)
constexpr int64_t kBnMaxChannels = 1ll << 22;
constexpr int kBnNConst = 5;          // per-channel constants of the dx kernel: mean, invstd, gamma * invstd, dbias / M, dweight / M

struct BnGeom {
  int64_t rows;      // rows per block
  int64_t nchunks;   // grid.x
  int ncol;          // grid.y
};
// cv = 16-byte vectors per row
static inline BnGeom bn_geom_of(int64_t m, int64_t cv, int64_t min_rows) {
  const int64_t cols = cv < kBnCols ? cv : kBnCols;
  const int64_t rpp = kBlock / cols;                       // rows per pass of a block
  const int64_t unit = rpp * kBnRedU;
  int64_t rows = (m + kBnMaxChunks - 1) / kBnMaxChunks;
  if (rows < min_rows) rows = min_rows;
  rows = (rows + unit - 1) / unit * unit;
  BnGeom g;
  g.rows = rows;
  g.nchunks = (m + rows - 1) / rows;
  g.ncol = (int)((cv + kBnCols - 1) / kBnCols);
  return g;
}
static inline BnGeom bn_geom(int64_t m, int64_t c) { return bn_geom_of(m, c >> 2, kBnMinRows); }
// 16-bit tensors: a lane owns 8 channels, so a block's 16 columns are 128 channels (the same 256 bytes of a row) and there
// are twice as many rows of lanes per column.  A row of the tensor is 2 C bytes against 16 C of a partial row: the 0.9 %
// rule asks for 2 * kBnMinRows rows, and a block never takes fewer rows than the fp32 geometry gives the same [m][c].
constexpr int kBn16MinRows = 2 * kBnMinRows;
static inline BnGeom bn_geom16(int64_t m, int64_t c) {
  const int64_t rows32 = bn_geom(m, c).rows;
  return bn_geom_of(m, c >> 3, rows32 > kBn16MinRows ? rows32 : kBn16MinRows);
}
template <class IO>
static inline BnGeom bn_geom_io(int64_t m, int64_t c) { return IO::kW == 8 ? bn_geom16(m, c) : bn_geom(m, c); }

// Cache policy of the loads, by tensor size and pass (measured per size, docs/NOTEBOOK.md section 6 "BatchNorm backward").
// x and dy are read twice within three launches.  Below kBnReduceNtElems the first read loads with the default policy
// (the lines stay in the 256 MiB Infinity Cache for the second read), from there up it streams through non-temporally;
// the second read is non-temporal from kBnDxNtElems up.  Stores of dx are non-temporal at every size.
constexpr int64_t kBnReduceNtElems = 28ll << 20;
constexpr int64_t kBnDxNtElems = 28ll << 20;
// occupancy of the dx kernel by size: the rule of pt_bwd_kernel (fq_pt.hip)
constexpr int64_t kBnBigElems = 20ll << 20;
constexpr int kBnBigMaxWaves = 6;     // (below kBnBigElems the kernel is held to Dy::kDxWaves: 8 with dy in memory)
// The same three for 16-bit elements (4 B of x + dy and 2 B of dx per element).  The cache policy goes by BYTES: x + dy fit
// the Infinity Cache up to twice the fp32 element count; the occupancy rule goes by elements, as in fq_io16.hip
// (docs/NOTEBOOK.md section 6, "BatchNorm backward, 16-bit").
// Each can be overridden at build time: tools/bn_bwd16_bench.py times builds with a forced policy next to the product's.
#ifndef MHAQ_BN16_REDUCE_NT_ELEMS
#define MHAQ_BN16_REDUCE_NT_ELEMS (56ll << 20)
#endif
#ifndef MHAQ_BN16_DX_NT_ELEMS
#define MHAQ_BN16_DX_NT_ELEMS (56ll << 20)
#endif
#ifndef MHAQ_BN16_BIG_ELEMS
#define MHAQ_BN16_BIG_ELEMS (20ll << 20)
#endif
constexpr int64_t kBn16ReduceNtElems = MHAQ_BN16_REDUCE_NT_ELEMS;
constexpr int64_t kBn16DxNtElems = MHAQ_BN16_DX_NT_ELEMS;
constexpr int64_t kBn16BigElems = MHAQ_BN16_BIG_ELEMS;

// ---------------------------------------------------------------- the two ends of a reduction's sums
// (shared by the backward and the training forward: bn_*_reduce_kernel leaves partials[chunk][2][C], bn_*_finalize_kernel adds them)
// The tail of a reduce kernel: the lanes' sums s1, s2 of K channels each across the block's rows of lanes -- LDS
// [ty][2][K * cols], then thread (k, c) adds its column in row order -- into the block's two partial rows.
template <int K>
__device__ __forceinline__ void bn_block_partials(const double (&s1)[K], const double (&s2)[K], bool live, int ty, int tx,
                                                  int cols, int rpp, int c0, int cv, double* __restrict__ partials) {
  __shared__ __align__(16) double sm[kBlock * 2 * K];
  const int w = K * cols;
  if (live) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      sm[(ty * 2 + 0) * w + tx * K + j] = s1[j];
      sm[(ty * 2 + 1) * w + tx * K + j] = s2[j];
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < 2 * w) {
    const int k = (int)threadIdx.x >= w ? 1 : 0, c = (int)threadIdx.x - k * w;
    double tot = 0.0;
    for (int r = 0; r < rpp; ++r) tot += sm[(r * 2 + k) * w + c];
    partials[((int64_t)blockIdx.x * 2 + k) * ((int64_t)cv * K) + (int64_t)c0 * K + c] = tot;
  }
}

// ---------------------------------------------------------------- 1. partial sums
// partials[chunk][2][C] (fp64): row 0 = sum dy, row 1 = sum dy * (x - mean) over the chunk's rows.
// Every sum is fp64 from the product on -- x - mean and dy * (x - mean) are exact in fp64 --, per lane, across the block
// and in the partial rows.  The reason is dx, not dweight / dbias themselves: dx subtracts dbias / M and xhat * dweight / M
// from dy, and its bound is stated on |dbias| and |dweight| AFTER the cancellation in their sums.  In a channel whose sum
// nearly cancels (some always do among 64-512 channels: |sum| ~ M^1/2 |term| or less) an fp32 rounding anywhere on the way
// -- 6e-8 of a product, of a lane's or a block's subtotal -- is an error of 6e-8 M^1/2 |term|, several 1e-6 of that |sum|;
// the framework's fp32 sums measure 3e-6 to 6e-6 of the bound's term sum at M = 245 ... 25 088 for that reason.  fp64 adds
// run at the fp32 rate on this chip and the kernel stays memory-bound (20 VALU operations per 32 loaded bytes).
template <bool NT, class Dy, int U>
__global__ __launch_bounds__(kBlock) void bn_bwd_reduce_kernel(
    const typename Dy::IO::T* __restrict__ x, const Dy dy, const float* __restrict__ mean,
    double* __restrict__ partials, int64_t m, int cv, int64_t rows) {
  using IO = typename Dy::IO;
  constexpr int K = IO::kW;                                    // channels of a lane
  const int c0 = (int)blockIdx.y * kBnCols;
  const int cols = (cv - c0) < kBnCols ? (cv - c0) : kBnCols;
  const int rpp = kBlock / cols;
  const int ty = (int)(threadIdx.x / (uint32_t)cols), tx = (int)threadIdx.x - ty * cols;
  const bool live = ty < rpp;                                  // 256 % cols lanes idle (C = 20: one)
  const int64_t row0 = (int64_t)blockIdx.x * rows;
  const int64_t rend = (row0 + rows < m) ? row0 + rows : m;    // > row0: the grid has ceil(m / rows) chunks
  const int64_t colv = c0 + tx;
  float mu[K];
#pragma unroll
  for (int j = 0; j < K; ++j) mu[j] = mean[colv * K + j];
  double s1[K] = {}, s2[K] = {};
  typename Dy::Walk walk(dy, (uint32_t)(row0 + ty), (uint32_t)rpp);       // (the pool's source: m < 2^31)
  for (int64_t rb = row0 + ty; rb - ty < rend; rb += (int64_t)rpp * U) {
    // unconditional, clamped loads: all of the U rows in flight before anything waits; lanes past the chunk's end
    // re-read its last row and drop it
    typename IO::Vec a[U];
    typename Dy::Loads b[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t r = rb + (int64_t)u * rpp;
      ok[u] = live && r < rend;
      const int64_t vidx = (ok[u] ? r : rend - 1) * cv + colv;
      a[u] = IO::template ld<NT>(x, vidx);
      b[u] = dy.template load<NT>(vidx, walk, ok[u], (uint32_t)colv, (uint32_t)cv);
      walk.next();
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float av[K], bv[K];
      IO::unpack(a[u], av);
      dy.value(b[u], bv);
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const double g = ok[u] ? (double)bv[j] : 0.0;          // a select, not a product: a dropped NaN stays dropped
        const double d = ok[u] ? (double)av[j] - (double)mu[j] : 0.0;
        s1[j] += g;
        s2[j] = fma(g, d, s2[j]);
      }
    }
  }
  bn_block_partials<K>(s1, s2, live, ty, tx, cols, rpp, c0, cv, partials);
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
// The column of a lane's 16-byte vectors in the streaming kernels (dx, norm, the frozen forward), whose block b owns the
// kBlock * kBnDxU consecutive vectors at b * kBlock * kBnDxU.  The column of a vector is its index modulo cv: (b * 512) mod cv
// for the block's first from two wave-uniform 32-bit modulos (cv <= 2^20: the product fits), one modulo per lane, a conditional
// subtract per further vector (next) -- and step == 0, no second fetch of the constants, when 256 % cv == 0 (every
// power-of-two width up to 1024 fp32 channels).  (cb is computed before step, as the kernels had it written out: the other
// order changes the instruction streams of the fp32 kernels.)
struct BnColWalk {
  uint32_t ucv, step, col;
  __device__ __forceinline__ explicit BnColWalk(int cv) : ucv((uint32_t)cv) {
    const uint32_t cb = ((blockIdx.x % ucv) * ((uint32_t)(kBlock * kBnDxU) % ucv)) % ucv;      // wave-uniform
    step = (uint32_t)kBlock % ucv;                                                              // wave-uniform
    col = (cb + threadIdx.x) % ucv;
  }
  __device__ __forceinline__ void next() {
    col += step;
    if (col >= ucv) col -= ucv;
  }
};

// Block b owns the 256 * U consecutive vectors at b * 256 * U, one pass; data loads first and unconditional (ragged lanes
// clamp their index), the per-channel constants arrive under them, by the column of each vector (BnColWalk).
// The pool's source needs the pixel of a float4 as well: pixel and column of the block's first float4 from 32-bit
// wave-uniform divisions (b = q * cv + r: b * 512 / cv = q * 512 + r * 512 / cv, r * 512 < 2^29), one 32-bit division by cv
// per lane and float4 on top, two more inside the source for (n, ih, iw).
template <bool NT, bool BIG, class Dy>
__global__ __attribute__((amdgpu_waves_per_eu(
    (BIG ? 1 : Dy::kDxWaves), (BIG && kBnBigMaxWaves < Dy::kDxWaves ? kBnBigMaxWaves : Dy::kDxWaves))))
__launch_bounds__(kBlock) void bn_bwd_dx_kernel(
    const typename Dy::IO::T* __restrict__ x, const Dy dy, typename Dy::IO::T* __restrict__ dx, int64_t nvec, int cv,
    const float* __restrict__ consts) {
  using IO = typename Dy::IO;
  constexpr int K = IO::kW;
  const int64_t blk0 = (int64_t)blockIdx.x * (kBlock * kBnDxU);
  const int64_t base = blk0 + threadIdx.x;
  const bool full = blk0 + kBlock * kBnDxU <= nvec;
  typename IO::Vec a[kBnDxU];
  typename Dy::Loads b[kBnDxU];
  uint32_t pix0 = 0, col0 = 0;
  if constexpr (Dy::kGather) {
    const uint32_t q = blockIdx.x / (uint32_t)cv, r = (blockIdx.x - q * (uint32_t)cv) * (uint32_t)(kBlock * kBnDxU);
    const uint32_t rq = r / (uint32_t)cv;
    pix0 = q * (uint32_t)(kBlock * kBnDxU) + rq;
    col0 = r - rq * (uint32_t)cv + threadIdx.x;
  }
#pragma unroll
  for (int u = 0; u < kBnDxU; ++u) {
    const int64_t idx = base + u * kBlock;
    const bool ok = full || idx < nvec;
    const int64_t idc = ok ? idx : nvec - 1;
    a[u] = IO::template ld<NT>(x, idc);
    const uint32_t t = col0 + (uint32_t)(u * kBlock), tq = t / (uint32_t)cv;
    b[u] = dy.template load_at_pixel<NT>(idc, pix0 + tq, ok, t - tq * (uint32_t)cv, (uint32_t)cv);
  }
  __builtin_amdgcn_sched_barrier(0);
  BnColWalk cw(cv);
  const int64_t c = (int64_t)cv * K;
  float k[kBnNConst][K / 4][4];
#pragma unroll
  for (int u = 0; u < kBnDxU; ++u) {
    const int64_t idx = base + u * kBlock;
    if (u > 0) cw.next();
    if (u == 0 || cw.step != 0) {
#pragma unroll
      for (int q = 0; q < kBnNConst; ++q)
#pragma unroll
        for (int h = 0; h < K / 4; ++h) ldv<4>(consts + q * c + (int64_t)cw.col * K + 4 * h, k[q][h]);
    }
    if (full || idx < nvec) {
      float xv[K], gv[K], o[K];
      IO::unpack(a[u], xv);
      dy.value(b[u], gv);
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const int h = j >> 2, i = j & 3;
        const float xh = (xv[j] - k[0][h][i]) * k[1][h][i];
        o[j] = k[2][h][i] * ((gv[j] - k[3][h][i]) - xh * k[4][h][i]);
      }
      IO::st(dx, idx, o);
    }
  }
}

static inline bool bn_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// What the four backward entry points have in common, with the element type of x, the gradient source and dx erased.
struct BnCall {
  const void *x, *src;                              // src: dy, or the pooled gradient g
  const float *mean, *invstd, *weight;
  void* dx;
  float *dweight, *dbias;
  void* workspace;
  size_t workspace_bytes;
  void* stream;
};

// The three launches behind every entry point (arguments checked by bn_bwd_status); RU = rows in flight in the reduction.
template <class Dy, int RU>
static int bn_bwd_launch(const BnCall& a, const Dy dy, int64_t m, int64_t c) {
  using IO = typename Dy::IO;
  constexpr bool x16 = IO::kW == 8;
  const typename IO::T* x = (const typename IO::T*)a.x;
  typename IO::T* dx = (typename IO::T*)a.dx;
  hipStream_t st = (hipStream_t)a.stream;
  const BnGeom g = bn_geom_io<IO>(m, c);
  const int64_t nvec = m * (c / IO::kW);
  const int64_t dx_grid = (nvec + kBlock * kBnDxU - 1) / (kBlock * kBnDxU);
  if (g.nchunks > 0x7fffffff || dx_grid > 0x7fffffff) return MHAQ_FQ_EUNSUPPORTED;
  if (!dx && !a.dweight && !a.dbias) return 0;
  float* consts = (float*)a.workspace;
  double* parts = (double*)(consts + kBnNConst * c);      // 20 * c bytes in: 16-byte aligned (c % 4 == 0)
  const int cv = (int)(c / IO::kW);
  const bool nt_r = m * c >= (x16 ? kBn16ReduceNtElems : kBnReduceNtElems);
  const bool nt_d = m * c >= (x16 ? kBn16DxNtElems : kBnDxNtElems), big = m * c >= (x16 ? kBn16BigElems : kBnBigElems);
  const dim3 rgrid((unsigned)g.nchunks, (unsigned)g.ncol);
  MHAQ_LAUNCH((nt_r ? bn_bwd_reduce_kernel<true, Dy, RU> : bn_bwd_reduce_kernel<false, Dy, RU>), rgrid, dim3(kBlock), 0, st, x,
              dy, a.mean, parts, m, cv, g.rows);
  int rc = launch_status();
  if (rc) return rc;
  MHAQ_LAUNCH(bn_bwd_finalize_kernel, dim3((unsigned)(c >> 2)), dim3(kBlock), 0, st, (const double*)parts, (int)g.nchunks,
              (int)c, a.mean, a.invstd, a.weight, 1.0 / (double)m, consts, a.dweight, a.dbias);
  rc = launch_status();
  if (rc || !dx) return rc;
  MHAQ_LAUNCH((big ? (nt_d ? bn_bwd_dx_kernel<true, true, Dy> : bn_bwd_dx_kernel<false, true, Dy>)
                   : (nt_d ? bn_bwd_dx_kernel<true, false, Dy> : bn_bwd_dx_kernel<false, false, Dy>)),
              dim3((unsigned)dx_grid), dim3(kBlock), 0, st, x, dy, dx, nvec, cv, (const float*)consts);
  return launch_status();
}

// ---------------------------------------------------------------- the training forward (mhaq_fq_bn_fwd, mhaq_fq_bn_fwd_x16)
// The sibling of the three launches above, over the same partition:
//   bn_fwd_reduce_kernel     one read of x -> per-block fp64 partial rows of  sum (x - k)  and  sum (x - k)^2
//   bn_fwd_finalize_kernel   fixed-order fp64 sum of the partial rows -> mean, invstd, the running statistics, the constants
//   bn_fwd_norm_kernel       a 1R1W stream in the shape of bn_bwd_dx_kernel:  y = (x - mean) * (gamma * invstd) + beta
// k is a per-channel shift, the same for every block: x[row 0][c].  x - k is exact in fp64, and with the shift the
// cancellation in E[(x - k)^2] - (E[x - k])^2 is bounded whatever the mean: k is one of the M samples, so
// (mean - k)^2 <= (M - 1) var.  (Unshifted, a channel at 1e4 +- 1 loses eight digits of its variance.)  A constant channel
// sums exact zeros: mean = k, var = 0, y = beta.  As in the backward the mean is not folded into an additive constant.
// Workspace: consts[3][C] = {mean, gamma * invstd, beta} and shift[C] (fp32), then partials[chunk][2][C] (fp64).
// The cache policy of the two reads of x, each overridable at build time (tools/bn_fwd_bench.py times builds with a forced
// policy next to the product's): the byte-equivalent of the backward's rule -- one fp32 stream instead of two fits the
// Infinity Cache up to twice the element count.
#ifndef MHAQ_BN_FWD_REDUCE_NT_ELEMS
#define MHAQ_BN_FWD_REDUCE_NT_ELEMS (56ll << 20)
#endif
#ifndef MHAQ_BN_FWD_NORM_NT_ELEMS
#define MHAQ_BN_FWD_NORM_NT_ELEMS (56ll << 20)
#endif
constexpr int64_t kBnFwdReduceNtElems = MHAQ_BN_FWD_REDUCE_NT_ELEMS;
constexpr int64_t kBnFwdNormNtElems = MHAQ_BN_FWD_NORM_NT_ELEMS;
// The same two for 16-bit elements (mhaq_fq_bn_fwd_x16), by BYTES: one 2-byte stream fits the cache up to four times the
// backward's fp32 element count.  tools/bn_fwd_bench.py --dtype times builds with a forced policy next to the product's.
#ifndef MHAQ_BN_FWD16_REDUCE_NT_ELEMS
#define MHAQ_BN_FWD16_REDUCE_NT_ELEMS (112ll << 20)
#endif
#ifndef MHAQ_BN_FWD16_NORM_NT_ELEMS
#define MHAQ_BN_FWD16_NORM_NT_ELEMS (112ll << 20)
#endif
constexpr int64_t kBnFwd16ReduceNtElems = MHAQ_BN_FWD16_REDUCE_NT_ELEMS;
constexpr int64_t kBnFwd16NormNtElems = MHAQ_BN_FWD16_NORM_NT_ELEMS;
constexpr int kBnFwdNConst = 3;       // per-channel constants of the norm kernel: mean, gamma * invstd, beta
constexpr int kBnFwdRows32 = kBnFwdNConst + 1;      // fp32 rows at the head of the workspace: the constants and the shift

// partials[chunk][2][C] (fp64): row 0 = sum (x - k), row 1 = sum (x - k)^2 over the chunk's rows; the blocks of the first
// row chunk leave k in shift[C].  Partition, clamped loads and the block sum are bn_bwd_reduce_kernel's.
template <bool NT, class IO, int U>
__global__ __launch_bounds__(kBlock) void bn_fwd_reduce_kernel(
    const typename IO::T* __restrict__ x, float* __restrict__ shift, double* __restrict__ partials, int64_t m, int cv,
    int64_t rows) {
  constexpr int K = IO::kW;
  const int c0 = (int)blockIdx.y * kBnCols;
  const int cols = (cv - c0) < kBnCols ? (cv - c0) : kBnCols;
  const int rpp = kBlock / cols;
  const int ty = (int)(threadIdx.x / (uint32_t)cols), tx = (int)threadIdx.x - ty * cols;
  const bool live = ty < rpp;
  const int64_t row0 = (int64_t)blockIdx.x * rows;
  const int64_t rend = (row0 + rows < m) ? row0 + rows : m;
  const int64_t colv = c0 + tx;
  float kf[K];
  IO::unpack(IO::template ld<false>(x, colv), kf);             // row 0 of the tensor: every block reads the same shift
  if (blockIdx.x == 0 && ty == 0) {
#pragma unroll
    for (int j = 0; j < K; ++j) shift[colv * K + j] = kf[j];
  }
  double s1[K] = {}, s2[K] = {};
  for (int64_t rb = row0 + ty; rb - ty < rend; rb += (int64_t)rpp * U) {
    typename IO::Vec a[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t r = rb + (int64_t)u * rpp;
      ok[u] = live && r < rend;
      a[u] = IO::template ld<NT>(x, (ok[u] ? r : rend - 1) * cv + colv);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float av[K];
      IO::unpack(a[u], av);
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const double d = ok[u] ? (double)av[j] - (double)kf[j] : 0.0;      // a select: a dropped NaN stays dropped
        s1[j] += d;
        s2[j] = fma(d, d, s2[j]);
      }
    }
  }
  bn_block_partials<K>(s1, s2, live, ty, tx, cols, rpp, c0, cv, partials);
}

// One block per group of 4 channels, the sums as in bn_bwd_finalize_kernel.  Everything is fp64 and every result is rounded
// to fp32 ONCE:  mean = k + S1 / M,  var = max(S2 / M - (S1 / M)^2, 0) (biased; a NaN stays a NaN),  invstd = (var + eps)^-1/2;
// running_mean = R32((1 - f) running_mean + f mean),  running_var = R32((1 - f) running_var + f var M / (M - 1)).
__global__ __launch_bounds__(kBlock) void bn_fwd_finalize_kernel(
    const double* __restrict__ partials, int nchunks, int c, const float* __restrict__ shift,
    const float* __restrict__ weight, const float* __restrict__ bias, double m, double factor, double eps,
    float* __restrict__ consts, float* __restrict__ save_mean, float* __restrict__ save_invstd,
    float* __restrict__ running_mean, float* __restrict__ running_var) {
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
      const double e1 = v[j] / m, e2 = v[4 + j] / m;
      const double d = e2 - e1 * e1;
      const double var = d < 0.0 ? 0.0 : d;                     // (not fmax: a NaN stays)
      const double mean = (double)shift[ch + j] + e1;
      const float mean32 = (float)mean, is32 = (float)(1.0 / sqrt(var + eps));
      save_mean[ch + j] = mean32;
      save_invstd[ch + j] = is32;
      consts[0 * c + ch + j] = mean32;
      consts[1 * c + ch + j] = (weight ? weight[ch + j] : 1.0f) * is32;
      consts[2 * c + ch + j] = bias ? bias[ch + j] : 0.0f;
      if (running_mean) {
        running_mean[ch + j] = (float)((1.0 - factor) * (double)running_mean[ch + j] + factor * mean);
        running_var[ch + j] = (float)((1.0 - factor) * (double)running_var[ch + j] + factor * (var * m / (m - 1.0)));
      }
    }
  }
}

// The element body of the training forward, y = (x - mean) * a + beta in fp32, in this order (the build contracts nothing):
// bn_fwd_norm_kernel's, and that of the pooled stem forward further down (PoolOfNorm in maxpool3s2_fwd_kernel).
__device__ __forceinline__ float bn_norm_elem(float x, float mean, float a, float beta) { return (x - mean) * a + beta; }

// y = bn_norm_elem(x, ..) per element.  Block, loads and the column arithmetic of
// the constants are bn_bwd_dx_kernel's; occupancy by size likewise.
template <class IO>
constexpr int kBnFwdWaves = IO::kW == 8 ? 6 : 8;
template <bool NT, bool BIG, class IO>
__global__ __attribute__((amdgpu_waves_per_eu(
    (BIG ? 1 : kBnFwdWaves<IO>), (BIG && kBnBigMaxWaves < kBnFwdWaves<IO> ? kBnBigMaxWaves : kBnFwdWaves<IO>))))
__launch_bounds__(kBlock) void bn_fwd_norm_kernel(
    const typename IO::T* __restrict__ x, typename IO::T* __restrict__ y, int64_t nvec, int cv,
    const float* __restrict__ consts) {
  constexpr int K = IO::kW;
  const int64_t blk0 = (int64_t)blockIdx.x * (kBlock * kBnDxU);
  const int64_t base = blk0 + threadIdx.x;
  const bool full = blk0 + kBlock * kBnDxU <= nvec;
  typename IO::Vec a[kBnDxU];
#pragma unroll
  for (int u = 0; u < kBnDxU; ++u) {
    const int64_t idx = base + u * kBlock;
    a[u] = IO::template ld<NT>(x, (full || idx < nvec) ? idx : nvec - 1);
  }
  __builtin_amdgcn_sched_barrier(0);
  BnColWalk cw(cv);
  const int64_t c = (int64_t)cv * K;
  float k[kBnFwdNConst][K / 4][4];
#pragma unroll
  for (int u = 0; u < kBnDxU; ++u) {
    const int64_t idx = base + u * kBlock;
    if (u > 0) cw.next();
    if (u == 0 || cw.step != 0) {
#pragma unroll
      for (int q = 0; q < kBnFwdNConst; ++q)
#pragma unroll
        for (int h = 0; h < K / 4; ++h) ldv<4>(consts + q * c + (int64_t)cw.col * K + 4 * h, k[q][h]);
    }
    if (full || idx < nvec) {
      float xv[K], o[K];
      IO::unpack(a[u], xv);
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const int h = j >> 2, i = j & 3;
        o[j] = bn_norm_elem(xv[j], k[0][h][i], k[1][h][i], k[2][h][i]);
      }
      IO::st(y, idx, o);
    }
  }
}

struct BnFwdCall {
  const void* x;
  const float *weight, *bias;
  void* y;
  float *save_mean, *save_invstd, *running_mean, *running_var;
  double factor, eps;
  void* workspace;
  size_t workspace_bytes;
  void* stream;
};

// workspace of a forward over [m][c]: 4 fp32 rows and 2 fp64 partial rows per row chunk; 0 for an unsupported shape
static size_t bn_fwd_workspace_bytes(int64_t m, int64_t c, int kw) {
  if (m < 2 || c <= 0 || (c & (kw - 1)) || c > kBnMaxChannels) return 0;
  const BnGeom g = kw == 8 ? bn_geom16(m, c) : bn_geom(m, c);
  return ((size_t)kBnFwdRows32 * sizeof(float) + 2 * (size_t)g.nchunks * sizeof(double)) * (size_t)c;
}

// Status of a forward call before anything is launched, in bn_bwd_status's order: required pointers and positive sizes, width
// and range (m == 1 has no unbiased variance), the workspace, the alignment.
static int bn_fwd_status(const BnFwdCall& a, int kw, int64_t m, int64_t c) {
  if (!a.x || !a.save_mean || !a.save_invstd || !a.workspace || m <= 0 || c <= 0 || !a.running_mean != !a.running_var)
    return MHAQ_FQ_EINVAL;
  if ((c & (kw - 1)) || c > kBnMaxChannels || m > (INT64_MAX >> 3) / c || m < 2) return MHAQ_FQ_EUNSUPPORTED;
  if (a.workspace_bytes < bn_fwd_workspace_bytes(m, c, kw)) return MHAQ_FQ_EWORKSPACE;
  if (!bn_aligned(a.x, 16) || !bn_aligned(a.y, 16) || !bn_aligned(a.workspace, 16) || !bn_aligned(a.weight, 4) ||
      !bn_aligned(a.bias, 4) || !bn_aligned(a.save_mean, 4) || !bn_aligned(a.save_invstd, 4) ||
      !bn_aligned(a.running_mean, 4) || !bn_aligned(a.running_var, 4))
    return MHAQ_FQ_EALIGN;
  return 0;
}

// The three launches (arguments checked by bn_fwd_status).
template <class IO>
static int bn_fwd_launch(const BnFwdCall& a, int64_t m, int64_t c) {
  const typename IO::T* x = (const typename IO::T*)a.x;
  typename IO::T* y = (typename IO::T*)a.y;
  hipStream_t st = (hipStream_t)a.stream;
  const BnGeom g = bn_geom_io<IO>(m, c);
  const int64_t nvec = m * (c / IO::kW);
  const int64_t grid = (nvec + kBlock * kBnDxU - 1) / (kBlock * kBnDxU);
  if (g.nchunks > 0x7fffffff || grid > 0x7fffffff) return MHAQ_FQ_EUNSUPPORTED;
  float* consts = (float*)a.workspace;
  float* shift = consts + kBnFwdNConst * c;
  double* parts = (double*)(consts + kBnFwdRows32 * c);     // 16 * c bytes in: 16-byte aligned
  const int cv = (int)(c / IO::kW);
  constexpr bool x16 = IO::kW == 8;
  const bool nt_r = m * c >= (x16 ? kBnFwd16ReduceNtElems : kBnFwdReduceNtElems);
  const bool nt_n = m * c >= (x16 ? kBnFwd16NormNtElems : kBnFwdNormNtElems), big = m * c >= kBnBigElems;
  const dim3 rgrid((unsigned)g.nchunks, (unsigned)g.ncol);
  MHAQ_LAUNCH((nt_r ? bn_fwd_reduce_kernel<true, IO, kBnRedU> : bn_fwd_reduce_kernel<false, IO, kBnRedU>), rgrid,
              dim3(kBlock), 0, st, x, shift, parts, m, cv, g.rows);
  int rc = launch_status();
  if (rc) return rc;
  MHAQ_LAUNCH(bn_fwd_finalize_kernel, dim3((unsigned)(c >> 2)), dim3(kBlock), 0, st, (const double*)parts, (int)g.nchunks,
              (int)c, (const float*)shift, a.weight, a.bias, (double)m, a.factor, a.eps, consts, a.save_mean, a.save_invstd,
              a.running_mean, a.running_var);
  rc = launch_status();
  if (rc || !y) return rc;
  MHAQ_LAUNCH((big ? (nt_n ? bn_fwd_norm_kernel<true, true, IO> : bn_fwd_norm_kernel<false, true, IO>)
                   : (nt_n ? bn_fwd_norm_kernel<true, false, IO> : bn_fwd_norm_kernel<false, false, IO>)),
              dim3((unsigned)grid), dim3(kBlock), 0, st, x, y, nvec, cv, (const float*)consts);
  return launch_status();
}

// ---------------------------------------------------------------- the frozen forward (mhaq_fq_bn_infer_*)
// Eval-mode BatchNorm from the running statistics with what follows it in a frozen ResNet block, one launch per place:
//   bn_infer_consts_kernel     consts[3][C] = {running_mean, gamma * (running_var + eps)^-1/2, beta}: the three rows of the
//                              training forward; the product in fp64, rounded to fp32 ONCE.  Launched when the parameters change.
//   bn_infer_act_kernel        bn_fwd_norm_kernel with the ReLU, and the residual add in front of it, in the same pass:
//                              BN_RELU        y = relu(t)                    1R1W
//                              BN_ADD_RELU    y = relu(t + r)                2R1W  (r: the block's input)
//                              BN2_ADD_RELU   y = relu(t + t2)               2R1W  (t2: the downsample branch, its own constants)
//   bn_relu_pool3s2_kernel     max_pool2d(relu(t), 3, 2, 1) without a stored t (behind the pool's forward, further down)
// t = (x - mean) * a + beta in fp32, in this order, uncontracted; the add and the ReLU round where torch's separate add and
// clamp_min round, so every output is the bits of those ops on the same constants.  relu keeps a NaN.
// The two streaming kernels are written over the element type IO: fp32 (mhaq_fq_bn_infer_act, mhaq_fq_bn_relu_pool3s2) or
// bf16 / fp16 (the *_x16 entry points: the teacher under autocast).  A 16-bit element is converted UP exactly and takes the
// expression above unchanged -- the sum is rounded to fp32 before the ReLU --; the result is rounded to nearest-even ONCE on
// the way out (IO::pack: a plain cast, a NaN stays a NaN, fp16 overflow gives +-inf).
// Cache policy: loads go by the byte rule of the training forward -- non-temporal once the INPUT streams together exceed
// 224 MiB (56 Mi fp32 elements, 112 Mi 16-bit ones) --; the output is read again by the next convolution, so stores take the
// default policy (IO::stv<false>, not the non-temporal IO::st).  Occupancy goes by elements: kBnBigElems, and as in
// fq_io16.hip for 16-bit tensors.  Each can be overridden at build time: tools/teacher_fwd_bench.py [--dtype bf16] times
// builds with forced policies next to the product's.
#ifndef MHAQ_BN_INFER_NT_ELEMS
#define MHAQ_BN_INFER_NT_ELEMS (56ll << 20)
#endif
#ifndef MHAQ_BN_INFER_ST_NT
#define MHAQ_BN_INFER_ST_NT 0
#endif
#ifndef MHAQ_BN_INFER16_NT_ELEMS
#define MHAQ_BN_INFER16_NT_ELEMS (112ll << 20)
#endif
#ifndef MHAQ_BN_INFER16_BIG_ELEMS
#define MHAQ_BN_INFER16_BIG_ELEMS (20ll << 20)
#endif
#ifndef MHAQ_BN_INFER16_ST_NT
#define MHAQ_BN_INFER16_ST_NT 0
#endif
constexpr int64_t kBnInferNtElems = MHAQ_BN_INFER_NT_ELEMS;
constexpr bool kBnInferStNt = MHAQ_BN_INFER_ST_NT != 0;
constexpr int64_t kBnInfer16NtElems = MHAQ_BN_INFER16_NT_ELEMS;
constexpr int64_t kBnInfer16BigElems = MHAQ_BN_INFER16_BIG_ELEMS;
constexpr bool kBnInfer16StNt = MHAQ_BN_INFER16_ST_NT != 0;

__device__ __forceinline__ float bn_relu(float v) { return v > 0.0f ? v : (v != v ? v : 0.0f); }

__global__ __launch_bounds__(kBlock) void bn_infer_consts_kernel(
    const float* __restrict__ mean, const float* __restrict__ var, const float* __restrict__ weight,
    const float* __restrict__ bias, double eps, int c, float* __restrict__ consts) {
  const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (i >= c) return;
  const double is = 1.0 / sqrt((double)var[i] + eps);
  consts[i] = mean[i];
  consts[c + i] = (float)((weight ? (double)weight[i] : 1.0) * is);
  consts[2 * c + i] = bias ? bias[i] : 0.0f;
}

// Block, loads, column arithmetic and occupancy are bn_fwd_norm_kernel's.  x2 is the residual (BN_ADD_RELU) or the second
// branch's input with its constants k2 (BN2_ADD_RELU).
template <bool NT, bool BIG, int MODE, class IO>
__global__ __attribute__((amdgpu_waves_per_eu(
    (BIG ? 1 : kBnFwdWaves<IO>), (BIG && kBnBigMaxWaves < kBnFwdWaves<IO> ? kBnBigMaxWaves : kBnFwdWaves<IO>))))
__launch_bounds__(kBlock) void bn_infer_act_kernel(
    const typename IO::T* __restrict__ x, const typename IO::T* __restrict__ x2, typename IO::T* __restrict__ y, int64_t nvec,
    int cv, const float* __restrict__ k1, const float* __restrict__ k2) {
  constexpr int K = IO::kW;
  constexpr bool kTwo = MODE != MHAQ_FQ_BN_RELU, kBn2 = MODE == MHAQ_FQ_BN2_ADD_RELU;
  constexpr bool kStNt = K == 8 ? kBnInfer16StNt : kBnInferStNt;
  const int64_t blk0 = (int64_t)blockIdx.x * (kBlock * kBnDxU);
  const int64_t base = blk0 + threadIdx.x;
  const bool full = blk0 + kBlock * kBnDxU <= nvec;
  typename IO::Vec a[kBnDxU], b[kBnDxU];
#pragma unroll
  for (int u = 0; u < kBnDxU; ++u) {
    const int64_t idx = base + u * kBlock;
    const int64_t idc = (full || idx < nvec) ? idx : nvec - 1;
    a[u] = IO::template ld<NT>(x, idc);
    if constexpr (kTwo) b[u] = IO::template ld<NT>(x2, idc);
  }
  __builtin_amdgcn_sched_barrier(0);
  BnColWalk cw(cv);
  const int64_t c = (int64_t)cv * K;
  float k[kBnFwdNConst][K / 4][4], kk[kBnFwdNConst][K / 4][4];
#pragma unroll
  for (int u = 0; u < kBnDxU; ++u) {
    const int64_t idx = base + u * kBlock;
    if (u > 0) cw.next();
    if (u == 0 || cw.step != 0) {
#pragma unroll
      for (int q = 0; q < kBnFwdNConst; ++q)
#pragma unroll
        for (int h = 0; h < K / 4; ++h) {
          ldv<4>(k1 + q * c + (int64_t)cw.col * K + 4 * h, k[q][h]);
          if constexpr (kBn2) ldv<4>(k2 + q * c + (int64_t)cw.col * K + 4 * h, kk[q][h]);
        }
    }
    if (full || idx < nvec) {
      float xv[K], bv[K], o[K];
      IO::unpack(a[u], xv);
      if constexpr (kTwo) IO::unpack(b[u], bv);
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const int h = j >> 2, i = j & 3;
        float t = (xv[j] - k[0][h][i]) * k[1][h][i] + k[2][h][i];
        if constexpr (kTwo) t = t + (kBn2 ? (bv[j] - kk[0][h][i]) * kk[1][h][i] + kk[2][h][i] : bv[j]);
        o[j] = bn_relu(t);
      }
      IO::template stv<kStNt>(y, idx, IO::pack(o));
    }
  }
}

// Status of the elementwise entry points before anything is launched, in bn_fwd_status's order: required pointers,
// positive sizes and a known mode; width and range; (no workspace;) the alignment -- the constant rows are read 16 bytes at a time.
static int bn_infer_consts_status(const float* mean, const float* var, const float* weight, const float* bias, int64_t c,
                                  const float* consts) {
  if (!mean || !var || !consts || c <= 0) return MHAQ_FQ_EINVAL;
  if ((c & 3) || c > kBnMaxChannels) return MHAQ_FQ_EUNSUPPORTED;
  if (!bn_aligned(mean, 4) || !bn_aligned(var, 4) || !bn_aligned(weight, 4) || !bn_aligned(bias, 4) ||
      !bn_aligned(consts, 16))
    return MHAQ_FQ_EALIGN;
  return 0;
}
// A mode's own operands are required and the other mode's refused: a residual with BN_ADD_RELU only, x2 and consts2 with
// BN2_ADD_RELU only.  kw: the channels of a lane's 16 bytes (4, or 8 with the dtype of a 16-bit call, checked behind the mode
// as in bn_bwd_status).
static int bn_infer_act_status(const void* x, const float* consts, const void* x2, const float* consts2,
                               const void* residual, const void* y, int64_t m, int64_t c, int mode, int kw, int dtype) {
  if (!x || !consts || !y || m <= 0 || c <= 0) return MHAQ_FQ_EINVAL;
  if (mode != MHAQ_FQ_BN_RELU && mode != MHAQ_FQ_BN_ADD_RELU && mode != MHAQ_FQ_BN2_ADD_RELU) return MHAQ_FQ_EINVAL;
  if (!residual != (mode != MHAQ_FQ_BN_ADD_RELU) || !x2 != (mode != MHAQ_FQ_BN2_ADD_RELU) || !x2 != !consts2)
    return MHAQ_FQ_EINVAL;
  if (kw == 8 && !io16::known_dtype(dtype)) return MHAQ_FQ_EINVAL;
  if ((c & (kw - 1)) || c > kBnMaxChannels || m > (INT64_MAX >> 3) / c ||
      (m * (c / kw) + kBlock * kBnDxU - 1) / (kBlock * kBnDxU) > 0x7fffffff)
    return MHAQ_FQ_EUNSUPPORTED;
  if (!bn_aligned(x, 16) || !bn_aligned(consts, 16) || !bn_aligned(x2, 16) || !bn_aligned(consts2, 16) ||
      !bn_aligned(residual, 16) || !bn_aligned(y, 16))
    return MHAQ_FQ_EALIGN;
  return 0;
}

// The one launch (arguments checked by bn_infer_act_status); x2: the mode's second stream.
template <int MODE, class IO>
static int bn_infer_act_launch(const void* x, const float* k1, const void* x2, const float* k2, void* y, int64_t m,
                               int64_t c, hipStream_t st) {
  using T = typename IO::T;
  constexpr bool x16 = IO::kW == 8;
  const int64_t nvec = m * (c / IO::kW);
  const int64_t grid = (nvec + kBlock * kBnDxU - 1) / (kBlock * kBnDxU);
  const bool nt = m * c * (MODE == MHAQ_FQ_BN_RELU ? 1 : 2) >= (x16 ? kBnInfer16NtElems : kBnInferNtElems);
  const bool big = m * c >= (x16 ? kBnInfer16BigElems : kBnBigElems);
  MHAQ_LAUNCH((big ? (nt ? bn_infer_act_kernel<true, true, MODE, IO> : bn_infer_act_kernel<false, true, MODE, IO>)
                   : (nt ? bn_infer_act_kernel<true, false, MODE, IO> : bn_infer_act_kernel<false, false, MODE, IO>)),
              dim3((unsigned)grid), dim3(kBlock), 0, st, (const T*)x, (const T*)x2, (T*)y, nvec, (int)(c / IO::kW), k1, k2);
  return launch_status();
}
// ... of the mode asked for, with that mode's operands
template <class IO>
static int bn_infer_act_mode(const void* x, const float* consts, const void* x2, const float* consts2, const void* residual,
                             void* y, int64_t m, int64_t c, int mode, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (mode == MHAQ_FQ_BN_RELU) return bn_infer_act_launch<MHAQ_FQ_BN_RELU, IO>(x, consts, nullptr, nullptr, y, m, c, st);
  if (mode == MHAQ_FQ_BN_ADD_RELU)
    return bn_infer_act_launch<MHAQ_FQ_BN_ADD_RELU, IO>(x, consts, residual, nullptr, y, m, c, st);
  return bn_infer_act_launch<MHAQ_FQ_BN2_ADD_RELU, IO>(x, consts, x2, consts2, y, m, c, st);
}

// ---------------------------------------------------------------- the pool's forward: values and argmax codes
// max_pool2d(kernel 3, stride 2, padding 1) of a dense NHWC tensor of the element type IO: one lane per 16 bytes of the output
// (4 fp32 or 8 16-bit channels), nine 16-byte loads, a 16-byte store of p and one byte of code per channel.  The selection
// is the framework's channels_last kernel's: the window's in-range positions in kh, then kw order, starting at -inf and
// replacing on  val > max || isnan(val)  (so the LAST NaN of a window wins).  code = kh * 3 + kw of the chosen position.  A
// window in which nothing replaces the start (all -inf) keeps the framework's initial index, 0 -- element (0, 0) of the plane,
// which only the window (0, 0) contains (there it is code 4); every other such window gets kPoolNoneChosen, which no input
// element matches: like the framework's backward, it sends its gradient nowhere.  16-bit values are compared exactly upcast
// (the framework's kernel compares in fp32 too); what is stored is the chosen element's ORIGINAL bits, so a NaN keeps its
// payload: the maximum itself in fp32, the 16 bits kept beside it (`raw`) for a 16-bit element.  The nine loads are unconditional on clamped coordinates and take the default cache policy like the
// stores: every element of t is wanted again by up to three neighbouring windows, p and code by the quantizer behind and by
// the backward (non-temporal loads of t measured 236 us against 212 us on fp32 [250,64,112,112]; docs/NOTEBOOK.md section 6,
// "Stem pool").
// `Pre` says what the pool is taken of: the loaded tensor itself (PoolOfTensor, mhaq_fq_maxpool3s2_fwd and its _x16 form: no
// further argument, and nothing is compiled in) or the training BatchNorm's output of it, which is never stored (PoolOfNorm,
// mhaq_fq_bn_norm_pool3s2_fwd_x16: the stem's forward, the BatchNorm's third launch and the pool in one).  A `Pre` is built
// from the kernel's trailing arguments, fetches what it needs for the lane's channels under the data loads and turns each
// loaded vector into the values the selection runs on.
struct PoolOfTensor {
  static constexpr bool kTransforms = false;
  struct K {};
};
// y = R16(bn_norm_elem(up(x), mean, a, beta)), the 16 bits bn_fwd_norm_kernel stores: a = weight * invstd is
// bn_fwd_finalize_kernel's fp32 product, the rounding Io16::pack's, as in Io16::st.  The selection then runs on THOSE values, not on
// x: two x that round to one y are a tie that the first in-range position wins, gamma < 0 reverses the order and gamma == 0
// ties every window, as in the pool of the stored y.  (All nine vectors are converted, the out-of-range ones too: 36 packed
// converts and no branch.)  The four rows are fp32 [C], 4-byte aligned: scalar indexing, as bn_bwd_reduce_kernel reads the mean.
struct PoolOfNorm {
  static constexpr bool kTransforms = true;
  const float* __restrict__ mean;
  const float* __restrict__ invstd;
  const float* __restrict__ weight;                // NULL: 1
  const float* __restrict__ bias;                  // NULL: 0
  struct K { float mu[8], a[8], beta[8]; };
  __device__ __forceinline__ K fetch(uint32_t col) const {
    K k;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t ch = col * 8u + (uint32_t)j;
      k.mu[j] = mean[ch];
      k.a[j] = (weight ? weight[ch] : 1.0f) * invstd[ch];
      k.beta[j] = bias ? bias[ch] : 0.0f;
      // Where two NaNs meet in one multiply or add, the operand ORDER of the instruction decides whose sign and payload survive,
      // and the compiler orders the operands of each kernel as it likes.  bn_fwd_norm_kernel has them in the order of the
      // source -- the NaN of x - mean survives a NaN a, the NaN of the product a NaN beta --, so the channels in which two can
      // meet (a NaN statistic: an x that holds a NaN) get constants that cannot be NaN where the result is decided anyway:
      // y = NaN(x - mean) * 1 + 0 under a NaN mean, y = NaN(.. * a) + 0 under a NaN a.  The same bits, in either operand order.
      if (k.mu[j] != k.mu[j]) k.a[j] = 1.0f;
      if (k.mu[j] != k.mu[j] || k.a[j] != k.a[j]) k.beta[j] = 0.0f;
    }
    return k;
  }
  template <class IO>
  static __device__ __forceinline__ void apply(const K& k, typename IO::Vec& v) {
    static_assert(IO::kW == 8, "the pooled stem forward exists for 16-bit tensors");
    float e[8];
    IO::unpack(v, e);
#pragma unroll
    for (int j = 0; j < 8; ++j) e[j] = bn_norm_elem(e[j], k.mu[j], k.a[j], k.beta[j]);
    v = IO::pack(e);
  }
};
template <class IO, class Pre = PoolOfTensor, class... PreArgs>
__global__ __launch_bounds__(kBlock) void maxpool3s2_fwd_kernel(
    const typename IO::T* __restrict__ t, typename IO::T* __restrict__ p, uint8_t* __restrict__ code, uint32_t h, uint32_t w,
    uint32_t oh, uint32_t ow, uint32_t cv, int64_t nvec, PreArgs... pre_args) {
  constexpr int K = IO::kW;
  // pixel and column of the block's first vector, as in bn_bwd_dx_kernel
  const uint32_t bq = blockIdx.x / cv, br = (blockIdx.x - bq * cv) * (uint32_t)kBlock, brq = br / cv;
  const uint32_t tt = br - brq * cv + threadIdx.x, tq = tt / cv;
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool ok = idx < nvec;
  const uint32_t pixel = ok ? bq * (uint32_t)kBlock + brq + tq : 0u, col = tt - tq * cv;
  const uint32_t q = pixel / ow, n = q / oh, po = q - n * oh, pw = pixel - q * ow;
  const int ih0 = (int)(po * 2u) - 1, iw0 = (int)(pw * 2u) - 1;
  typename IO::Vec v[9];
  bool in[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int ih = ih0 + k / 3, iw = iw0 + k % 3;
    in[k] = ih >= 0 && ih < (int)h && iw >= 0 && iw < (int)w;
    const uint32_t ihc = (uint32_t)(ih < 0 ? 0 : (ih < (int)h ? ih : (int)h - 1));
    const uint32_t iwc = (uint32_t)(iw < 0 ? 0 : (iw < (int)w ? iw : (int)w - 1));
    v[k] = IO::template ld<false>(t, (int64_t)((n * h + ihc) * w + iwc) * cv + col);
  }
  __builtin_amdgcn_sched_barrier(0);
  [[maybe_unused]] typename Pre::K pk;
  if constexpr (Pre::kTransforms) pk = Pre{pre_args...}.fetch(col);
  if (!ok) return;
  if constexpr (Pre::kTransforms) {
#pragma unroll
    for (int k = 0; k < 9; ++k) Pre::template apply<IO>(pk, v[k]);
  }
  const uint32_t start = (po == 0u && pw == 0u) ? 4u : kPoolNoneChosen;     // the framework's initial index 0
  float mx[K];
  [[maybe_unused]] uint32_t raw[K];               // K == 8: the chosen element's 16 bits (-inf until one is chosen)
  uint32_t cd[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    mx[j] = -INFINITY;
    if constexpr (K == 8) raw[j] = IO::kNegInfBits;
    cd[j] = start;
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    float e[K];
    IO::unpack(v[k], e);
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const bool take = in[k] && (e[j] > mx[j] || e[j] != e[j]);
      mx[j] = take ? e[j] : mx[j];
      if constexpr (K == 8) raw[j] = take ? IO::bits(v[k], j) : raw[j];
      cd[j] = take ? (uint32_t)k : cd[j];
    }
  }
  // (fp32: the maxima are the bits; the vector is written out because IO::pack(mx), an array handed on by reference, is
  // lowered otherwise and reorders the instruction stream)
  if constexpr (K == 8) IO::template stv<false>(p, idx, IO::from_bits(raw));
  else IO::template stv<false>(p, idx, vf4{mx[0], mx[1], mx[2], mx[3]});
  reinterpret_cast<typename IO::Code*>(code)[idx] = IO::pack_codes(cd);
}

// The frozen stem (mhaq_fq_bn_relu_pool3s2 and its _x16 form): p = max_pool2d(relu((x - mean) * a + beta), 3, 2, 1) of a dense
// NHWC x, the BatchNorm output never stored.  Geometry, the nine clamped loads, their cache policy and the selection are the
// kernel's above, without the codes (nothing is differentiated); the constants of the lane's channels arrive under the data
// loads, and each in-range value takes bn_infer_act_kernel's fp32 arithmetic before it is compared in fp32.  A 16-bit maximum
// is rounded ONCE at the end -- rounding is monotone, so this is the value of rounding all nine first, for 4 packed converts
// instead of 36.  A NaN that wins stays a NaN through the cast.
template <class IO>
__global__ __launch_bounds__(kBlock) void bn_relu_pool3s2_kernel(
    const typename IO::T* __restrict__ x, typename IO::T* __restrict__ p, uint32_t h, uint32_t w, uint32_t oh, uint32_t ow,
    uint32_t cv, int64_t nvec, const float* __restrict__ consts) {
  constexpr int K = IO::kW;
  const uint32_t bq = blockIdx.x / cv, br = (blockIdx.x - bq * cv) * (uint32_t)kBlock, brq = br / cv;
  const uint32_t tt = br - brq * cv + threadIdx.x, tq = tt / cv;
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool ok = idx < nvec;
  const uint32_t pixel = ok ? bq * (uint32_t)kBlock + brq + tq : 0u, col = tt - tq * cv;
  const uint32_t q = pixel / ow, n = q / oh, po = q - n * oh, pw = pixel - q * ow;
  const int ih0 = (int)(po * 2u) - 1, iw0 = (int)(pw * 2u) - 1;
  typename IO::Vec v[9];
  bool in[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int ih = ih0 + k / 3, iw = iw0 + k % 3;
    in[k] = ih >= 0 && ih < (int)h && iw >= 0 && iw < (int)w;
    const uint32_t ihc = (uint32_t)(ih < 0 ? 0 : (ih < (int)h ? ih : (int)h - 1));
    const uint32_t iwc = (uint32_t)(iw < 0 ? 0 : (iw < (int)w ? iw : (int)w - 1));
    v[k] = IO::template ld<false>(x, (int64_t)((n * h + ihc) * w + iwc) * cv + col);
  }
  __builtin_amdgcn_sched_barrier(0);
  float kc[kBnFwdNConst][K / 4][4];
#pragma unroll
  for (int r = 0; r < kBnFwdNConst; ++r)
#pragma unroll
    for (int hh = 0; hh < K / 4; ++hh) ldv<4>(consts + ((int64_t)r * cv + col) * K + 4 * hh, kc[r][hh]);
  if (!ok) return;
  float mx[K];
#pragma unroll
  for (int j = 0; j < K; ++j) mx[j] = -INFINITY;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    float e[K];
    IO::unpack(v[k], e);
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const int hh = j >> 2, i = j & 3;
      const float r = bn_relu((e[j] - kc[0][hh][i]) * kc[1][hh][i] + kc[2][hh][i]);
      const bool take = in[k] && (r > mx[j] || r != r);
      mx[j] = take ? r : mx[j];
    }
  }
  IO::template stv<false>(p, idx, IO::pack(mx));
}

// pooled extent of kernel 3, stride 2, padding 1, dilation 1, ceil_mode = false
static inline int64_t pool_out(int64_t in) { return (in - 1) / 2 + 1; }
// n, h, w, c of a pool entry point (kw channels per lane): 0, or the error code
static inline int pool_dims_status(int64_t n, int64_t h, int64_t w, int64_t c, int kw) {
  if (n <= 0 || h <= 0 || w <= 0 || c <= 0) return MHAQ_FQ_EINVAL;
  // the pixel arithmetic of the kernels is 32-bit: n * h * w < 2^31
  if ((c & (kw - 1)) || c > kBnMaxChannels || h >= (1ll << 31) || w >= (1ll << 31) || n >= (1ll << 31) ||
      n * h >= (1ll << 31) || n * h * w >= (1ll << 31))
    return MHAQ_FQ_EUNSUPPORTED;
  return 0;
}

// ---------------------------------------------------------------- the host path of the entry points
// Written once for fp32 and 16-bit elements, told apart by kw, the channels of a lane's 16 bytes (4 or 8): C % kw == 0, and the
// argmax codes, one byte per channel, are kw-byte aligned.
// workspace of a backward over [m][c]: 5 fp32 constant rows and 2 fp64 partial rows per row chunk; 0 for an unsupported shape
static size_t bn_workspace_bytes(int64_t m, int64_t c, int kw) {
  if (m <= 0 || c <= 0 || (c & (kw - 1)) || c > kBnMaxChannels) return 0;
  const BnGeom g = kw == 8 ? bn_geom16(m, c) : bn_geom(m, c);
  return ((size_t)kBnNConst * sizeof(float) + 2 * (size_t)g.nchunks * sizeof(double)) * (size_t)c;
}

// Status of a backward call before anything is launched, in the order include/mhaq_fq.h promises: required pointers and
// positive sizes, the dtype (kw == 8), width and range, the workspace, the alignment.  `code` and (h, w) belong to the pool
// forms (pool); the plain forms pass their m as n.
static int bn_bwd_status(const BnCall& a, int kw, int dtype, bool pool, const uint8_t* code, int64_t n, int64_t h, int64_t w,
                         int64_t c) {
  if (!a.x || !a.src || !a.mean || !a.invstd || !a.workspace || (pool ? !code : n <= 0 || c <= 0)) return MHAQ_FQ_EINVAL;
  if (kw == 8 && !io16::known_dtype(dtype)) return MHAQ_FQ_EINVAL;
  if (pool) {
    if (const int rc = pool_dims_status(n, h, w, c, kw)) return rc;
  } else if ((c & (kw - 1)) || c > kBnMaxChannels || n > (INT64_MAX >> 3) / c) {
    return MHAQ_FQ_EUNSUPPORTED;      // a lane owns kw channels; the width bound keeps the dx kernel's column arithmetic in 32 bits
  }
  if (a.workspace_bytes < bn_workspace_bytes(n * h * w, c, kw)) return MHAQ_FQ_EWORKSPACE;
  if (!bn_aligned(a.x, 16) || !bn_aligned(a.src, 16) || !bn_aligned(code, kw) || !bn_aligned(a.dx, 16) ||
      !bn_aligned(a.workspace, 16) || !bn_aligned(a.mean, 4) || !bn_aligned(a.invstd, 4) || !bn_aligned(a.weight, 4) ||
      !bn_aligned(a.dweight, 4) || !bn_aligned(a.dbias, 4))
    return MHAQ_FQ_EALIGN;
  return 0;
}

// A pool forward: its status in the same order, then its one launch (T: float or a 16-bit element, 16 / sizeof(T) per lane).
static int pool_fwd_status(const void* t, const void* p, const uint8_t* code, int kw, int dtype, int64_t n, int64_t h,
                           int64_t w, int64_t c) {
  if (!t || !p || !code) return MHAQ_FQ_EINVAL;
  if (kw == 8 && !io16::known_dtype(dtype)) return MHAQ_FQ_EINVAL;
  if (const int rc = pool_dims_status(n, h, w, c, kw)) return rc;
  if (!bn_aligned(t, 16) || !bn_aligned(p, 16) || !bn_aligned(code, kw)) return MHAQ_FQ_EALIGN;
  return 0;
}
// the one launch of a pool forward over [n][h][w][c]: one lane per kw output channels
struct PoolGrid {
  int64_t oh, ow, nvec, blocks;
};
static inline PoolGrid pool_grid(int64_t n, int64_t h, int64_t w, int64_t c, int64_t kw) {
  const int64_t oh = pool_out(h), ow = pool_out(w), nvec = n * oh * ow * (c / kw);
  return PoolGrid{oh, ow, nvec, (nvec + kBlock - 1) / kBlock};
}
// (More: what the kernel takes behind nvec -- the statistics and parameters of PoolOfNorm)
template <class T, class... More>
using PoolKernel = void (*)(const T*, T*, uint8_t*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, int64_t, More...);
template <class T, class... More>
static int pool_fwd_launch(PoolKernel<T, More...> kernel, const void* t, void* p, uint8_t* code, int64_t n, int64_t h,
                           int64_t w, int64_t c, void* stream, More... more) {
  constexpr int64_t kw = 16 / sizeof(T);
  const PoolGrid g = pool_grid(n, h, w, c, kw);
  if (g.blocks > 0x7fffffff) return MHAQ_FQ_EUNSUPPORTED;
  MHAQ_LAUNCH(kernel, dim3((unsigned)g.blocks), dim3(kBlock), 0, (hipStream_t)stream, (const T*)t, (T*)p, code, (uint32_t)h,
              (uint32_t)w, (uint32_t)g.oh, (uint32_t)g.ow, (uint32_t)(c / kw), g.nvec, more...);
  return launch_status();
}

// The frozen stem's pool (no codes): required pointers, the dtype (kw == 8), width and range with the size of the grid, the
// alignment -- the constant rows are read 16 bytes at a time --; then its one launch.
static int bn_relu_pool_status(const void* x, const float* consts, const void* p, int kw, int dtype, int64_t n, int64_t h,
                               int64_t w, int64_t c) {
  if (!x || !consts || !p) return MHAQ_FQ_EINVAL;
  if (kw == 8 && !io16::known_dtype(dtype)) return MHAQ_FQ_EINVAL;
  if (const int rc = pool_dims_status(n, h, w, c, kw)) return rc;
  if (pool_grid(n, h, w, c, kw).blocks > 0x7fffffff) return MHAQ_FQ_EUNSUPPORTED;
  if (!bn_aligned(x, 16) || !bn_aligned(consts, 16) || !bn_aligned(p, 16)) return MHAQ_FQ_EALIGN;
  return 0;
}
template <class IO>
static int bn_relu_pool_launch(const void* x, const float* consts, void* p, int64_t n, int64_t h, int64_t w, int64_t c,
                               void* stream) {
  using T = typename IO::T;
  const PoolGrid g = pool_grid(n, h, w, c, IO::kW);
  MHAQ_LAUNCH(bn_relu_pool3s2_kernel<IO>, dim3((unsigned)g.blocks), dim3(kBlock), 0, (hipStream_t)stream, (const T*)x, (T*)p,
              (uint32_t)h, (uint32_t)w, (uint32_t)g.oh, (uint32_t)g.ow, (uint32_t)(c / IO::kW), g.nvec, consts);
  return launch_status();
}

}  // namespace mhaq

using namespace mhaq;

extern "C" {

size_t mhaq_fq_bn_bwd_workspace_bytes(int64_t m, int64_t c) { return bn_workspace_bytes(m, c, 4); }
size_t mhaq_fq_bn_bwd_x16_workspace_bytes(int64_t m, int64_t c) { return bn_workspace_bytes(m, c, 8); }
size_t mhaq_fq_bn_pool_bwd_workspace_bytes(int64_t n, int64_t h, int64_t w, int64_t c) {
  return pool_dims_status(n, h, w, c, 4) ? 0 : bn_workspace_bytes(n * h * w, c, 4);
}
size_t mhaq_fq_bn_pool_bwd_x16_workspace_bytes(int64_t n, int64_t h, int64_t w, int64_t c) {
  return pool_dims_status(n, h, w, c, 8) ? 0 : bn_workspace_bytes(n * h * w, c, 8);
}

int mhaq_fq_bn_bwd(const float* x, const float* dy, const float* mean, const float* invstd, const float* weight,
                   float* dx, float* dweight, float* dbias, int64_t m, int64_t c, void* workspace,
                   size_t workspace_bytes, void* stream) {
  const BnCall a{x, dy, mean, invstd, weight, dx, dweight, dbias, workspace, workspace_bytes, stream};
  if (const int rc = bn_bwd_status(a, 4, 0, false, nullptr, m, 1, 1, c)) return rc;
  return bn_bwd_launch<DyMem, kBnRedU>(a, DyMem{dy}, m, c);
}

size_t mhaq_fq_bn_fwd_workspace_bytes(int64_t m, int64_t c) { return bn_fwd_workspace_bytes(m, c, 4); }

int mhaq_fq_bn_fwd(const float* x, const float* weight, const float* bias, float* y, float* save_mean, float* save_invstd,
                   float* running_mean, float* running_var, double factor, double eps, int64_t m, int64_t c,
                   void* workspace, size_t workspace_bytes, void* stream) {
  const BnFwdCall a{x, weight, bias, y, save_mean, save_invstd, running_mean, running_var, factor, eps, workspace,
                    workspace_bytes, stream};
  if (const int rc = bn_fwd_status(a, 4, m, c)) return rc;
  return bn_fwd_launch<IoF32>(a, m, c);
}

size_t mhaq_fq_bn_fwd_x16_workspace_bytes(int64_t m, int64_t c) { return bn_fwd_workspace_bytes(m, c, 8); }

int mhaq_fq_bn_fwd_x16(const void* x, const float* weight, const float* bias, void* y, float* save_mean, float* save_invstd,
                       float* running_mean, float* running_var, double factor, double eps, int64_t m, int64_t c, int dtype,
                       void* workspace, size_t workspace_bytes, void* stream) {
  const BnFwdCall a{x, weight, bias, y, save_mean, save_invstd, running_mean, running_var, factor, eps, workspace,
                    workspace_bytes, stream};
  const int rc = bn_fwd_status(a, 8, m, c);
  if (rc == MHAQ_FQ_EINVAL || !io16::known_dtype(dtype)) return MHAQ_FQ_EINVAL;      // the dtype: behind the NULL checks
  if (rc) return rc;
  return io16::with_dtype(dtype, [&](auto dt) { return bn_fwd_launch<Io16<decltype(dt)::value>>(a, m, c); });
}

int mhaq_fq_bn_infer_consts(const float* running_mean, const float* running_var, const float* weight, const float* bias,
                            double eps, int64_t c, float* consts, void* stream) {
  if (const int rc = bn_infer_consts_status(running_mean, running_var, weight, bias, c, consts)) return rc;
  MHAQ_LAUNCH(bn_infer_consts_kernel, dim3((unsigned)((c + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
              running_mean, running_var, weight, bias, eps, (int)c, consts);
  return launch_status();
}

int mhaq_fq_bn_infer_act(const float* x, const float* consts, const float* x2, const float* consts2, const float* residual,
                         float* y, int64_t m, int64_t c, int mode, void* stream) {
  if (const int rc = bn_infer_act_status(x, consts, x2, consts2, residual, y, m, c, mode, 4, 0)) return rc;
  return bn_infer_act_mode<IoF32>(x, consts, x2, consts2, residual, y, m, c, mode, stream);
}

int mhaq_fq_bn_infer_act_x16(const void* x, const float* consts, const void* x2, const float* consts2, const void* residual,
                             void* y, int64_t m, int64_t c, int mode, int dtype, void* stream) {
  if (const int rc = bn_infer_act_status(x, consts, x2, consts2, residual, y, m, c, mode, 8, dtype)) return rc;
  return io16::with_dtype(dtype, [&](auto dt) {
    return bn_infer_act_mode<Io16<decltype(dt)::value>>(x, consts, x2, consts2, residual, y, m, c, mode, stream);
  });
}

int mhaq_fq_bn_relu_pool3s2_x16(const void* x, const float* consts, void* p, int64_t n, int64_t h, int64_t w, int64_t c,
                                int dtype, void* stream) {
  if (const int rc = bn_relu_pool_status(x, consts, p, 8, dtype, n, h, w, c)) return rc;
  return io16::with_dtype(dtype, [&](auto dt) {
    return bn_relu_pool_launch<Io16<decltype(dt)::value>>(x, consts, p, n, h, w, c, stream);
  });
}

int mhaq_fq_bn_relu_pool3s2(const float* x, const float* consts, float* p, int64_t n, int64_t h, int64_t w, int64_t c,
                            void* stream) {
  if (const int rc = bn_relu_pool_status(x, consts, p, 4, 0, n, h, w, c)) return rc;
  return bn_relu_pool_launch<IoF32>(x, consts, p, n, h, w, c, stream);
}

int mhaq_fq_bn_bwd_x16(const void* x, const void* dy, const float* mean, const float* invstd, const float* weight, void* dx,
                       float* dweight, float* dbias, int64_t m, int64_t c, int dtype, void* workspace,
                       size_t workspace_bytes, void* stream) {
  const BnCall a{x, dy, mean, invstd, weight, dx, dweight, dbias, workspace, workspace_bytes, stream};
  if (const int rc = bn_bwd_status(a, 8, dtype, false, nullptr, m, 1, 1, c)) return rc;
  return io16::with_dtype(dtype, [&](auto dt) {
    using Dy = DyMem16<decltype(dt)::value>;
    return bn_bwd_launch<Dy, kBnRedU>(a, Dy{(const uint16_t*)dy}, m, c);
  });
}

int mhaq_fq_maxpool3s2_fwd(const float* t, float* p, uint8_t* code, int64_t n, int64_t h, int64_t w, int64_t c,
                           void* stream) {
  if (const int rc = pool_fwd_status(t, p, code, 4, 0, n, h, w, c)) return rc;
  const PoolKernel<float> k = maxpool3s2_fwd_kernel<IoF32>;
  return pool_fwd_launch(k, t, p, code, n, h, w, c, stream);
}

int mhaq_fq_maxpool3s2_fwd_x16(const void* t, void* p, uint8_t* code, int64_t n, int64_t h, int64_t w, int64_t c, int dtype,
                               void* stream) {
  if (const int rc = pool_fwd_status(t, p, code, 8, dtype, n, h, w, c)) return rc;
  return io16::with_dtype(dtype, [&](auto dt) {
    const PoolKernel<uint16_t> k = maxpool3s2_fwd_kernel<Io16<decltype(dt)::value>>;
    return pool_fwd_launch(k, t, p, code, n, h, w, c, stream);
  });
}

int mhaq_fq_bn_norm_pool3s2_fwd_x16(const void* x, const float* mean, const float* invstd, const float* weight,
                                    const float* bias, void* p, uint8_t* code, int64_t n, int64_t h, int64_t w, int64_t c,
                                    int dtype, void* stream) {
  // mhaq_fq_maxpool3s2_fwd_x16's checks in its order, the statistics among the required pointers and the 4-byte rows last
  if (!mean || !invstd) return MHAQ_FQ_EINVAL;
  if (const int rc = pool_fwd_status(x, p, code, 8, dtype, n, h, w, c)) return rc;
  if (!bn_aligned(mean, 4) || !bn_aligned(invstd, 4) || !bn_aligned(weight, 4) || !bn_aligned(bias, 4)) return MHAQ_FQ_EALIGN;
  return io16::with_dtype(dtype, [&](auto dt) {
    const PoolKernel<uint16_t, const float*, const float*, const float*, const float*> k =
        maxpool3s2_fwd_kernel<Io16<decltype(dt)::value>, PoolOfNorm>;
    return pool_fwd_launch(k, x, p, code, n, h, w, c, stream, mean, invstd, weight, bias);
  });
}

int mhaq_fq_bn_pool_bwd(const float* x, const float* g, const uint8_t* code, const float* mean, const float* invstd,
                        const float* weight, float* dx, float* dweight, float* dbias, int64_t n, int64_t h, int64_t w,
                        int64_t c, void* workspace, size_t workspace_bytes, void* stream) {
  const BnCall a{x, g, mean, invstd, weight, dx, dweight, dbias, workspace, workspace_bytes, stream};
  if (const int rc = bn_bwd_status(a, 4, 0, true, code, n, h, w, c)) return rc;
  const DyPool src{g, code, (uint32_t)h, (uint32_t)w, (uint32_t)pool_out(h), (uint32_t)pool_out(w)};
  return bn_bwd_launch<DyPool, kBnPoolRedU>(a, src, n * h * w, c);
}

int mhaq_fq_bn_pool_bwd_x16(const void* x, const void* g, const uint8_t* code, const float* mean, const float* invstd,
                            const float* weight, void* dx, float* dweight, float* dbias, int64_t n, int64_t h, int64_t w,
                            int64_t c, int dtype, void* workspace, size_t workspace_bytes, void* stream) {
  const BnCall a{x, g, mean, invstd, weight, dx, dweight, dbias, workspace, workspace_bytes, stream};
  if (const int rc = bn_bwd_status(a, 8, dtype, true, code, n, h, w, c)) return rc;
  return io16::with_dtype(dtype, [&](auto dt) {
    using Dy = DyPool16<decltype(dt)::value>;
    const Dy src{(const uint16_t*)g, code, (uint32_t)h, (uint32_t)w, (uint32_t)pool_out(h), (uint32_t)pool_out(w),
                 h == 1 && w == 1};
    return bn_bwd_launch<Dy, kBnPool16RedU>(a, src, n * h * w, c);
  });
}

}  // extern "C"
