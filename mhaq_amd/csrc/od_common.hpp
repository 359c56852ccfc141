// What the object-detection sources share -- validation (od_nms.hip, od_sort.hip) and training (od_assign.hip, od_loss.hip):
// the box type, the key of a candidate, the reference's CIoU, the finite screen, and the host-side shape check and workspace
// rounding.  Element loads / stores and the dtype dispatch are fq_iox.hpp's (iox::ld1, iox::st1, iox::known_dtype,
// iox::with_dtype), which all four get through this header.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/mhaq_fq.h"
#include "fq_common.hpp"
#include "fq_iox.hpp"

namespace mhaq {

constexpr int64_t kOdNoKey = 0x7fffffffffffffffLL;

typedef float od_f4 __attribute__((ext_vector_type(4)));      // x1, y1, x2, y2

// the key of candidate (a, c) with score s > conf_thr >= 0: the bits of s are a positive int32
__device__ __forceinline__ int64_t od_key(float s, int a, int nc, int c) {
  return (int64_t)(((uint64_t)(uint32_t)(0x7fffffff - (int32_t)__float_as_uint(s)) << 32) | (uint32_t)(a * nc + c));
}

__host__ __device__ __forceinline__ bool od_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }      // false for a NaN

// compute_iou of the reference (CIoU) with box1 = p, box2 = g, in its order of operations.  od_loss.hip calls it with the
// prediction as box1 and the target as box2, od_assign.hip with the ground truth as box1 and the prediction as box2; the
// intermediates the loss's analytic gradient needs stay in the struct (dead stores where only .ciou is read).
struct OdCiou { float w1, h1, iw, ih, ix, iy, uni, iou, cw, ch, c2, dx, dy, rho2, da, al, ciou; };
__device__ __forceinline__ OdCiou od_ciou(od_f4 p, od_f4 g) {
  OdCiou c;
  const float eps = 1e-7f;
  c.w1 = p.z - p.x;
  c.h1 = (p.w - p.y) + eps;
  const float w2 = g.z - g.x, h2 = (g.w - g.y) + eps;
  c.ix = fminf(p.z, g.z) - fmaxf(p.x, g.x);
  c.iy = fminf(p.w, g.w) - fmaxf(p.y, g.y);
  c.iw = fmaxf(c.ix, 0.f);
  c.ih = fmaxf(c.iy, 0.f);
  const float inter = c.iw * c.ih;
  c.uni = ((c.w1 * c.h1 + w2 * h2) - inter) + eps;
  c.iou = inter / c.uni;
  c.cw = fmaxf(p.z, g.z) - fminf(p.x, g.x);
  c.ch = fmaxf(p.w, g.w) - fminf(p.y, g.y);
  c.c2 = (c.cw * c.cw + c.ch * c.ch) + eps;
  c.dx = ((g.x + g.z) - p.x) - p.z;
  c.dy = ((g.y + g.w) - p.y) - p.w;
  c.rho2 = (c.dx * c.dx + c.dy * c.dy) / 4.f;
  c.da = atanf(w2 / h2) - atanf(c.w1 / c.h1);
  const float v = 0.40528473456935109f * (c.da * c.da);        // 4 / pi^2
  c.al = v / ((v - c.iou) + 1.0000001f);
  c.ciou = c.iou - (c.rho2 / c.c2 + v * c.al);
  return c;
}

inline bool od_shape_supported(int64_t B, int64_t nc, int64_t A) {
  return B <= 65535 && nc <= 65535 && A <= 0x7fffffff && A * nc <= 0x7fffffff;
}
inline size_t od_r8(size_t n) { return (n + 7) & ~(size_t)7; }      // a workspace section's bytes, rounded up to 8

}  // namespace mhaq
