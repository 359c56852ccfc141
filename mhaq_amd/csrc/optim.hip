// One-pass RAdam: the update of every parameter tensor of a model in ONE launch (mhaq_fq_radam_step, include/mhaq_fq.h).
//
// torch.optim.RAdam in its foreach form walks the parameters in 9 op launches per ~24 tensors -- lerp, mul, addcmul, sqrt,
// add, div, reciprocal, add, addcmul --, 21 tensor-passes over the 11.7 M parameters of ResNet-18 and a 47 MB temporary.  The
// update needs 7 passes: read p, g, m, v; write p, m, v.  This kernel makes exactly those, with the arithmetic of the foreach
// chain line by line (fp32, every line rounded once), so that a training run keeps its bits.
//
// Geometry: a host-built work list maps block b to (tensor, chunk); a chunk is kRadamChunk consecutive elements of one tensor
// in memory order.  Where the chunk's four pointers are 16-byte aligned the block moves float4s and lanes 0..2 take the
// n % 4 tail as scalars; otherwise (a view at an odd offset) every lane walks dwords.  No atomics, no workspace, no LDS.
//
// Contraction.  The library is built with -ffp-contract=off.  The framework's device kernels are not: inside lerp and
// addcmul its compiler may fuse a multiply with the add behind it.  Each of the three ops is therefore written in both forms,
// and MHAQ_RADAM_FORM chooses (tests/test_gpu_fused_radam.py holds the choice to the framework's bits on the device):
//   bit 0   lerp      m + w * (g - m)          as fmaf(w, g - m, m)
//   bit 1   addcmul   v + w2 * (g * g)         as fmaf(w2, g * g, v)
//   bit 2   addcmul   p + one * (m * b)        as fmaf(one, m * b, p): the framework's addcmul multiplies by its `value`
//                                              argument, 1 here, at run time; fused or not the sum rounds the same, but
//                                              where p and m * b are both NaN the instruction decides whose bits survive
//   bit 3   the second moment's product as (w2 * g) * g instead of w2 * (g * g) (the framework's CPU kernel's order)
//   bit 4   lerp's second branch (|w| >= 0.5, beta1 <= 0.5), g - (g - m) * (1 - w), where bit 0 fuses it: the negation on
//           the weight, fmaf(g - m, -(1 - w), g), instead of on the difference, fmaf(-(g - m), 1 - w, g).  Every finite
//           value rounds the same; where g - m is NaN the negated operand hands its flipped sign on, and the framework's
//           instruction keeps the sign of g - m (tests/test_gpu_fused_radam_edges.py; the first branch has no negation)
// Cache policy (profiles/r19_fused_radam_micro.txt): every load is non-temporal, the stores take the
// default policy.  g is read once; p, m and v would fit the 256 MB Infinity Cache together, but a training step moves
// gigabytes between two optimizer steps, so nothing of them is left to hit: measured cold, non-temporal loads of all four
// streams are the fastest of the six policies (59-61 us against 64-70 us).  MHAQ_RADAM_G_NT / _LD_NT / _ST_NT force the
// policy of the gradient load, the state loads and the stores for A/B builds (tools/radam_bench.py).
#include <hip/hip_runtime.h>

#include "../../include/mhaq_fq.h"
#include "fq_common.hpp"

#ifndef MHAQ_RADAM_FORM
#define MHAQ_RADAM_FORM 23
#endif
#ifndef MHAQ_RADAM_G_NT
#define MHAQ_RADAM_G_NT 1
#endif
#ifndef MHAQ_RADAM_LD_NT
#define MHAQ_RADAM_LD_NT 1
#endif
#ifndef MHAQ_RADAM_ST_NT
#define MHAQ_RADAM_ST_NT 0
#endif

namespace mhaq {

constexpr int kRadamForm = MHAQ_RADAM_FORM;
constexpr bool kRadamGNt = MHAQ_RADAM_G_NT != 0, kRadamLdNt = MHAQ_RADAM_LD_NT != 0, kRadamStNt = MHAQ_RADAM_ST_NT != 0;
constexpr int kRadamU = 4;                                // float4s per lane and stream
constexpr int kRadamChunk = kBlock * 4 * kRadamU;         // 4096 elements: 16 KB per stream and block

struct RadamK {
  float w1, beta2, w2, eps, one, c1, c2;
};

// torch's lerp(a, b, w) (ATen/native/Lerp.h), then the chain of _multi_tensor_radam's non-capturable branch
__device__ __forceinline__ void radam_element(float& p, float g, float& m, float& v, const RadamK& k) {
  const float d = g - m;
  if (fabsf(k.w1) < 0.5f) {
    m = (kRadamForm & 1) ? fmaf(k.w1, d, m) : m + k.w1 * d;
  } else {
    const float u = 1.0f - k.w1;
    m = !(kRadamForm & 1) ? g - d * u : (kRadamForm & 16) ? fmaf(d, -u, g) : fmaf(-d, u, g);
  }
  v = v * k.beta2;
  float a, b;
  if (kRadamForm & 8) { a = k.w2 * g; b = g; } else { a = k.w2; b = g * g; }
  v = (kRadamForm & 2) ? fmaf(a, b, v) : v + a * b;
  float t = sqrtf(v);
  t = t + k.eps;
  t = t / k.c2;
  t = 1.0f / t;
  t = t + k.c1;
  const float mt = m * t;
  p = (kRadamForm & 4) ? fmaf(k.one, mt, p) : p + mt;
}

template <bool NT>
__device__ __forceinline__ vf4 radam_ld4(const float* q) {
  const vf4 MHAQ_GLOBAL_AS* a = gptr(reinterpret_cast<const vf4*>(q));
  return NT ? __builtin_nontemporal_load(a) : *a;
}
__device__ __forceinline__ void radam_st4(float* q, vf4 x) {
  vf4 MHAQ_GLOBAL_AS* a = gptr(reinterpret_cast<vf4*>(q));
  if constexpr (kRadamStNt) __builtin_nontemporal_store(x, a);
  else *a = x;
}

__global__ __launch_bounds__(kBlock) void radam_step_kernel(const mhaq_radam_desc* __restrict__ descs, int ntensors,
                                                            const mhaq_radam_work* __restrict__ work, float w1,
                                                            float beta2, float w2, float eps, float one) {
  const mhaq_radam_work wk = work[blockIdx.x];
  if (wk.tensor < 0 || wk.tensor >= ntensors || wk.chunk < 0) return;      // a malformed list touches no memory
  const mhaq_radam_desc t = descs[wk.tensor];
  const int64_t e0 = (int64_t)wk.chunk * kRadamChunk;
  if (e0 >= t.n) return;
  const int len = (int)(t.n - e0 < kRadamChunk ? t.n - e0 : kRadamChunk);
  float* __restrict__ p = t.p + e0;
  const float* __restrict__ g = t.g + e0;
  float* __restrict__ m = t.m + e0;
  float* __restrict__ v = t.v + e0;
  const RadamK k{w1, beta2, w2, eps, one, t.c1, t.c2};
  const int tid = (int)threadIdx.x;
  if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0) {
    const int nv = len >> 2;
    vf4 vp[kRadamU], vg[kRadamU], vm[kRadamU], vv[kRadamU];
#pragma unroll
    for (int u = 0; u < kRadamU; ++u) {
      const int i = tid + u * kBlock;
      if (i < nv) {
        vg[u] = radam_ld4<kRadamGNt>(g + 4 * i);
        vm[u] = radam_ld4<kRadamLdNt>(m + 4 * i);
        vv[u] = radam_ld4<kRadamLdNt>(v + 4 * i);
        vp[u] = radam_ld4<kRadamLdNt>(p + 4 * i);
      }
    }
#pragma unroll
    for (int u = 0; u < kRadamU; ++u) {
      const int i = tid + u * kBlock;
      if (i < nv) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float pj = vp[u][j], mj = vm[u][j], vj = vv[u][j];
          radam_element(pj, vg[u][j], mj, vj, k);
          vp[u][j] = pj; vm[u][j] = mj; vv[u][j] = vj;
        }
        radam_st4(m + 4 * i, vm[u]);
        radam_st4(v + 4 * i, vv[u]);
        radam_st4(p + 4 * i, vp[u]);
      }
    }
    const int i = (nv << 2) + tid;             // the n % 4 tail of the tensor's last chunk
    if (i < len) {
      float pj = ldg(p + i), mj = ldg(m + i), vj = ldg(v + i);
      radam_element(pj, ldg(g + i), mj, vj, k);
      stg(m + i, mj); stg(v + i, vj); stg(p + i, pj);
    }
  } else {
    for (int i = tid; i < len; i += kBlock) {
      float pj = ldg(p + i), mj = ldg(m + i), vj = ldg(v + i);
      radam_element(pj, ldg(g + i), mj, vj, k);
      stg(m + i, mj); stg(v + i, vj); stg(p + i, pj);
    }
  }
}

}  // namespace mhaq

using namespace mhaq;

extern "C" {

int64_t mhaq_fq_radam_chunk_elements(void) { return kRadamChunk; }

int mhaq_fq_radam_step(const mhaq_radam_desc* descs_device, int ntensors, const mhaq_radam_work* work_device,
                       int64_t nwork, float w1, float beta2, float w2, float eps, void* stream) {
  if (ntensors < 0 || nwork < 0) return MHAQ_FQ_EINVAL;
  if (nwork == 0) return 0;
  if (!descs_device || !work_device || ntensors == 0) return MHAQ_FQ_EINVAL;
  if (nwork > 0x7fffffff) return MHAQ_FQ_EUNSUPPORTED;
  if (((uintptr_t)descs_device & 7) || ((uintptr_t)work_device & 7)) return MHAQ_FQ_EALIGN;
  MHAQ_LAUNCH(radam_step_kernel, dim3((unsigned)nwork), dim3(kBlock), 0, (hipStream_t)stream, descs_device, ntensors,
              work_device, w1, beta2, w2, eps, 1.0f /* addcmul's `value`: a run-time operand, as in the framework */);
  return launch_status();
}

}  // extern "C"
