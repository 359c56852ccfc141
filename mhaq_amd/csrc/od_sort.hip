// The sort stage of the object-detection validation (mhaq_fq_od_sorted_keys, include/mhaq_fq.h): the candidates of every image
// are compacted out of the score rows and only they are sorted, by a segmented least-significant-digit radix sort.  The result
// is what a sort of mhaq_fq_od_keys' rows gives, cut to K = min(A * nc, max_nms) keys per image, on bits.
//
//   count    grid (anchor tiles of 256, images).  Thread t owns anchor a0 + t and walks the classes: every load is coalesced
//            along A.  It leaves its own candidate count and the workgroup the tile's.
//   offsets  one workgroup per image: exclusive scan of the tile counts in place, n_cand[b], and the INT64_MAX tail of the
//            image's output row (the positions no scatter of the last pass writes).
//   emit     the count kernel's tiling.  A block scan of the per-thread counts gives thread t its position; it writes its
//            candidates' keys in ascending class.  Threads and tiles are in anchor order, so the compacted row is ascending in
//            the key's LOW word (a * nc + c).  A stable sort by the 31 bits of the score word alone therefore yields the full
//            64-bit order: four passes of 8 bits where a sort of the whole key needs seven.
//   pass p   (p = 0..3, digit = bits 32 + 8p .. 39 + 8p of the key; image b's n_cand[b] keys in sort tiles of kSortTile)
//     hist     per sort tile, the 256 digit counts (LDS integer counters).
//     scan     one workgroup of 1024 per image, thread (digit d, slice q of the tiles): the counts become, in place, the
//              position of the tile's first key of digit d in the destination row -- (digit, tile) order, the order a stable
//              sort needs.
//     scatter  wavefront w of a tile takes its 64-key rows 4w .. 4w + 3 in turn (coalesced loads, order preserved).  The
//              rank of a lane among the equal digits of its row comes from wave-64 ballots: eight ballots, one per digit bit,
//              AND-ed to the set of peer lanes, then popcount(peers & lanes below); added to it the wavefront's running
//              counter of the digit in LDS, which starts at the tile's position plus the earlier wavefronts' counts.
//            The grids are launched for the worst case (every pair a candidate: the counts live on the device only); a tile at
//            or beyond ceil(n_cand[b] / kSortTile) leaves at once.  Keys ping-pong between two workspace rows; the last pass
//            writes only destination positions below K, into the output.
// No workgroup waits for another, no global atomics, every global word has one writer per launch: the same inputs give the
// same bits at every call.
#include "od_common.hpp"

namespace mhaq {

constexpr int kSortTile = 1024;                       // keys per sort tile (mhaq_fq_od_sort_tile): 4 per thread
constexpr int kSortRows = kSortTile / kBlock;         // 64-key rows per wavefront
constexpr int kSortWaves = kBlock / kWave;
constexpr int kRadix = 256, kRadixBits = 8, kSortPasses = 4;
constexpr int kScanBlock = 1024, kScanSlices = kScanBlock / kRadix;
static_assert(kRadix == kBlock, "thread d of a sort tile owns digit d");

// Exclusive scan of one int per thread over the workgroup (up to 16 wavefronts); `total` = the sum, to every thread.
// s_w: 16 ints of LDS.  Every thread of the workgroup calls it; two barriers.
__device__ __forceinline__ int block_excl_scan(int v, int* s_w, int& total) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, nw = ((int)blockDim.x + 63) >> 6;
  int incl = v;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int u = __shfl_up(incl, o, kWave);
    if (lane >= o) incl += u;
  }
  __syncthreads();                                            // an earlier call's reads of s_w are behind us
  if (lane == kWave - 1) s_w[wave] = incl;
  __syncthreads();
  int before = 0, sum = 0;
  for (int w = 0; w < nw; ++w) {
    const int c = s_w[w];
    before += w < wave ? c : 0;
    sum += c;
  }
  total = sum;
  return before + incl - v;
}

// ---------------------------------------------------------------- compaction
template <int DT>
__global__ __launch_bounds__(kBlock) void od_count_kernel(const void* __restrict__ pred, int A, int nc, float conf_thr,
                                                          int32_t* __restrict__ thread_cnt, int32_t* __restrict__ tile_cnt) {
  __shared__ int s_w[16];
  const int a = (int)(blockIdx.x * kBlock + threadIdx.x);
  const int64_t b = blockIdx.y;
  int n = 0;
  if (a < A) {
    const int64_t row0 = (b * (4 + nc) + 4) * A + a;
#pragma unroll 8                                              // eight rows' loads in flight: the walk is latency-bound
    for (int c = 0; c < nc; ++c) n += iox::ld1<DT>(pred, row0 + (int64_t)c * A) > conf_thr ? 1 : 0;      // false for a NaN
    *gptr(thread_cnt + b * A + a) = n;
  }
  int total;
  block_excl_scan(n, s_w, total);
  if (threadIdx.x == 0) *gptr(tile_cnt + b * gridDim.x + blockIdx.x) = total;
}

__global__ __launch_bounds__(kBlock) void od_offsets_kernel(int32_t* __restrict__ tile_cnt, int ntiles, int64_t K,
                                                            int32_t* __restrict__ n_cand, int64_t* __restrict__ skeys) {
  __shared__ int s_w[16];
  const int tid = (int)threadIdx.x;
  const int64_t b = blockIdx.x;
  int32_t* row = tile_cnt + b * ntiles;
  int carry = 0;
  for (int t0 = 0; t0 < ntiles; t0 += kBlock) {               // block-uniform trip count
    const int t = t0 + tid;
    const int v = t < ntiles ? *gptr(row + t) : 0;
    int total;
    const int ex = block_excl_scan(v, s_w, total);
    if (t < ntiles) *gptr(row + t) = carry + ex;
    carry += total;
  }
  if (tid == 0) *gptr(n_cand + b) = carry;
  for (int64_t i = (carry < K ? carry : K) + tid; i < K; i += kBlock) *gptr(skeys + b * K + i) = kOdNoKey;
}

template <int DT>
__global__ __launch_bounds__(kBlock) void od_emit_kernel(const void* __restrict__ pred, int A, int nc, float conf_thr,
                                                         const int32_t* __restrict__ thread_cnt,
                                                         const int32_t* __restrict__ tile_off, int64_t* __restrict__ keys) {
  __shared__ int s_w[16];
  const int a = (int)(blockIdx.x * kBlock + threadIdx.x);
  const int64_t b = blockIdx.y, N = (int64_t)A * nc;
  const int n = a < A ? *gptr(thread_cnt + b * A + a) : 0;
  int total;
  const int ex = block_excl_scan(n, s_w, total);
  if (n == 0) return;                                         // after the scan's barriers
  const int64_t row0 = (b * (4 + nc) + 4) * A + a;
  int64_t* out = keys + b * N + *gptr(tile_off + b * gridDim.x + blockIdx.x) + ex;
  int64_t* const end = out + n;                               // the count kernel saw n candidates; no write goes beyond them
  for (int c0 = 0; c0 < nc && out < end; c0 += 4) {           // four rows' loads in flight, then their keys in class order
    float s[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = c0 + k < nc ? iox::ld1<DT>(pred, row0 + (int64_t)(c0 + k) * A) : -1.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (s[k] > conf_thr && out < end) *gptr(out++) = od_key(s[k], a, nc, c0 + k);
  }
}

// ---------------------------------------------------------------- radix passes
__device__ __forceinline__ int od_digit(int64_t key, int shift) { return (int)((uint64_t)key >> shift) & (kRadix - 1); }

__global__ __launch_bounds__(kBlock) void od_sort_hist_kernel(const int64_t* __restrict__ src, int64_t N, int nst, int shift,
                                                              const int32_t* __restrict__ n_cand,
                                                              int32_t* __restrict__ hist) {
  __shared__ int s_h[kRadix];
  const int tid = (int)threadIdx.x;
  const int64_t b = blockIdx.y;
  const int n = *gptr(n_cand + b);
  const int64_t p0 = (int64_t)blockIdx.x * kSortTile;
  if (p0 >= n) return;                                        // block-uniform
  s_h[tid] = 0;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kSortRows; ++r) {
    const int64_t p = p0 + r * kBlock + tid;
    if (p < n) atomicAdd(&s_h[od_digit(*gptr(src + b * N + p), shift)], 1);
  }
  __syncthreads();
  *gptr(hist + (b * nst + blockIdx.x) * kRadix + tid) = s_h[tid];
}

__global__ __launch_bounds__(kScanBlock) void od_sort_scan_kernel(int32_t* __restrict__ hist, int nst,
                                                                  const int32_t* __restrict__ n_cand) {
  __shared__ int s_part[kScanSlices][kRadix];
  __shared__ int s_base[kRadix];
  __shared__ int s_w[16];
  const int tid = (int)threadIdx.x, d = tid & (kRadix - 1), q = tid >> kRadixBits;
  const int64_t b = blockIdx.x;
  const int n = *gptr(n_cand + b);
  const int nt = (int)(((int64_t)n + kSortTile - 1) / kSortTile);      // <= nst: n <= A * nc
  if (nt == 0) return;                                        // block-uniform
  const int per = (nt + kScanSlices - 1) / kScanSlices;
  const int t0 = q * per, t1 = (t0 + per < nt) ? t0 + per : nt;
  int32_t* col = hist + b * nst * kRadix + d;
  int sum = 0;
#pragma unroll 4
  for (int t = t0; t < t1; ++t) sum += *gptr(col + (int64_t)t * kRadix);
  s_part[q][d] = sum;
  __syncthreads();
  int mine = 0;
  if (q == 0) {
#pragma unroll
    for (int k = 0; k < kScanSlices; ++k) mine += s_part[k][d];
  }
  int total;
  int pos = block_excl_scan(mine, s_w, total);                // q == 0: keys of the image with a smaller digit
  if (q == 0) s_base[d] = pos;
  __syncthreads();
  pos = s_base[d];                                            // slice q starts at the digit's base + the slices before it
  for (int k = 0; k < q; ++k) pos += s_part[k][d];
#pragma unroll 4
  for (int t = t0; t < t1; ++t) {
    const int v = *gptr(col + (int64_t)t * kRadix);
    *gptr(col + (int64_t)t * kRadix) = pos;
    pos += v;
  }
}

__global__ __launch_bounds__(kBlock) void od_sort_scatter_kernel(const int64_t* __restrict__ src, int64_t N, int nst, int shift,
                                                                 const int32_t* __restrict__ n_cand,
                                                                 const int32_t* __restrict__ hist, int64_t* __restrict__ dst,
                                                                 int64_t dst_stride, int64_t dst_limit) {
  __shared__ int s_cnt[kSortWaves][kRadix];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.y;
  const int n = *gptr(n_cand + b);
  const int64_t p0 = (int64_t)blockIdx.x * kSortTile + wave * (kSortRows * kWave);
  if ((int64_t)blockIdx.x * kSortTile >= n) return;           // block-uniform
#pragma unroll
  for (int w = 0; w < kSortWaves; ++w) s_cnt[w][tid] = 0;
  __syncthreads();
  int64_t key[kSortRows];
  bool valid[kSortRows];
#pragma unroll
  for (int r = 0; r < kSortRows; ++r) {
    const int64_t p = p0 + r * kWave + lane;
    valid[r] = p < n;
    key[r] = valid[r] ? *gptr(src + b * N + p) : 0;
    if (valid[r]) atomicAdd(&s_cnt[wave][od_digit(key[r], shift)], 1);
  }
  __syncthreads();
  {                                                           // thread d: counts of digit d -> first positions, per wavefront
    int pos = *gptr(hist + (b * nst + blockIdx.x) * kRadix + tid);
#pragma unroll
    for (int w = 0; w < kSortWaves; ++w) {
      const int c = s_cnt[w][tid];
      s_cnt[w][tid] = pos;
      pos += c;
    }
  }
  __syncthreads();
  volatile int* cnt = s_cnt[wave];                            // this wavefront's running positions: read, then advanced, in
  int64_t* drow = dst + b * dst_stride;                       // program order (one wavefront's LDS accesses stay in order)
#pragma unroll
  for (int r = 0; r < kSortRows; ++r) {
    const int d = od_digit(key[r], shift);
    uint64_t peers = __ballot(valid[r]);
#pragma unroll
    for (int k = 0; k < kRadixBits; ++k) {
      const bool bit = (d >> k) & 1;
      const uint64_t m = __ballot(bit);
      peers &= bit ? m : ~m;
    }
    const int below = __popcll(peers & ((1ull << lane) - 1ull));
    if (valid[r]) {
      const int pos = cnt[d] + below;
      if (pos < dst_limit) *gptr(drow + pos) = key[r];
    }
    __builtin_amdgcn_wave_barrier();                          // every peer's read is issued before the leader's write
    if (valid[r] && below == 0) cnt[d] = cnt[d] + __popcll(peers);
    __builtin_amdgcn_wave_barrier();
  }
}

struct OdSortLayout {
  int64_t N, K;
  int nat, nst;                          // anchor tiles and sort tiles per image (worst case)
  size_t keys, thread_cnt, tile_cnt, hist, total;
};
inline OdSortLayout od_sort_layout(int64_t B, int64_t nc, int64_t A, int max_nms) {
  OdSortLayout l;
  l.N = A * nc;
  l.K = l.N < max_nms ? l.N : (int64_t)max_nms;
  l.nat = (int)((A + kBlock - 1) / kBlock);
  l.nst = (int)((l.N + kSortTile - 1) / kSortTile);
  l.keys = (size_t)B * l.N * 8;
  l.thread_cnt = od_r8((size_t)B * A * 4);
  l.tile_cnt = od_r8((size_t)B * l.nat * 4);
  l.hist = (size_t)B * l.nst * kRadix * 4;
  l.total = 2 * l.keys + l.thread_cnt + l.tile_cnt + l.hist;
  return l;
}

}  // namespace mhaq

using namespace mhaq;

extern "C" {

int mhaq_fq_od_sort_tile(void) { return kSortTile; }

size_t mhaq_fq_od_sorted_keys_workspace_bytes(int64_t B, int64_t nc, int64_t A, int max_nms) {
  if (B < 1 || nc < 1 || A < 1 || max_nms < 1 || !od_shape_supported(B, nc, A)) return 0;
  return od_sort_layout(B, nc, A, max_nms).total;
}

int mhaq_fq_od_sorted_keys(const void* pred, int pred_dtype, int64_t B, int64_t nc, int64_t A, float conf_thr, int max_nms,
                           int64_t* skeys, int32_t* n_cand, void* workspace, size_t workspace_bytes, void* stream) {
  if (!pred || !skeys || !n_cand || !workspace || !iox::known_dtype(pred_dtype) || B < 1 || nc < 1 || A < 1 || max_nms < 1)
    return MHAQ_FQ_EINVAL;
  if (!(conf_thr >= 0.f) || !od_finite(conf_thr)) return MHAQ_FQ_EINVAL;
  if (((uintptr_t)pred & (pred_dtype == MHAQ_FQ_DT_F32 ? 3 : 1)) || ((uintptr_t)skeys & 7) || ((uintptr_t)n_cand & 3) ||
      ((uintptr_t)workspace & 7))
    return MHAQ_FQ_EALIGN;
  if (!od_shape_supported(B, nc, A)) return MHAQ_FQ_EUNSUPPORTED;
  const OdSortLayout l = od_sort_layout(B, nc, A, max_nms);
  if (workspace_bytes < l.total) return MHAQ_FQ_EWORKSPACE;
  char* ws = static_cast<char*>(workspace);
  int64_t* buf[2] = {reinterpret_cast<int64_t*>(ws), reinterpret_cast<int64_t*>(ws + l.keys)};
  int32_t* thread_cnt = reinterpret_cast<int32_t*>(ws + 2 * l.keys);
  int32_t* tile_cnt = reinterpret_cast<int32_t*>(ws + 2 * l.keys + l.thread_cnt);
  int32_t* hist = reinterpret_cast<int32_t*>(ws + 2 * l.keys + l.thread_cnt + l.tile_cnt);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 agrid((unsigned)l.nat, (unsigned)B), sgrid((unsigned)l.nst, (unsigned)B);
  int rc = 0;
  iox::with_dtype(pred_dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    MHAQ_LAUNCH(od_count_kernel<DT>, agrid, dim3(kBlock), 0, st, pred, (int)A, (int)nc, conf_thr, thread_cnt, tile_cnt);
    if ((rc = launch_status()) != 0) return;
    MHAQ_LAUNCH(od_offsets_kernel, dim3((unsigned)B), dim3(kBlock), 0, st, tile_cnt, l.nat, l.K, n_cand, skeys);
    if ((rc = launch_status()) != 0) return;
    MHAQ_LAUNCH(od_emit_kernel<DT>, agrid, dim3(kBlock), 0, st, pred, (int)A, (int)nc, conf_thr,
                (const int32_t*)thread_cnt, (const int32_t*)tile_cnt, buf[0]);
    rc = launch_status();
  });
  for (int p = 0; p < kSortPasses && rc == 0; ++p) {
    const int shift = 32 + kRadixBits * p;
    const bool last = p == kSortPasses - 1;
    const int64_t* src = buf[p & 1];
    MHAQ_LAUNCH(od_sort_hist_kernel, sgrid, dim3(kBlock), 0, st, src, l.N, l.nst, shift, (const int32_t*)n_cand, hist);
    if ((rc = launch_status()) != 0) break;
    MHAQ_LAUNCH(od_sort_scan_kernel, dim3((unsigned)B), dim3(kScanBlock), 0, st, hist, l.nst, (const int32_t*)n_cand);
    if ((rc = launch_status()) != 0) break;
    MHAQ_LAUNCH(od_sort_scatter_kernel, sgrid, dim3(kBlock), 0, st, src, l.N, l.nst, shift, (const int32_t*)n_cand,
                (const int32_t*)hist, last ? skeys : buf[(p & 1) ^ 1], last ? l.K : l.N, last ? l.K : l.N);
    rc = launch_status();
  }
  return rc;
}

}  // extern "C"
