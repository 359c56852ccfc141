// Element I/O and dtype dispatch for the kernels whose tensors may be fp32, bf16 or fp16 (distill.hip, cls_head.hip,
// sr_metrics.hip and, through od_common.hpp, the od_*.hip sources): DT = MHAQ_FQ_DT_F32 / _BF16 / _F16.  Up is exact; down is
// ONE round to nearest-even with NaN kept (fq_io16.hpp's conversions).
#pragma once

#include "fq_io16.hpp"

namespace mhaq {
namespace iox {

template <int DT>
__device__ __forceinline__ float ld1(const void* p, int64_t i) {
  if constexpr (DT == MHAQ_FQ_DT_F32) return ldg(static_cast<const float*>(p) + i);
  else return io16::up1<DT>(*gptr(static_cast<const uint16_t*>(p) + i));
}
// elements 4 * g .. 4 * g + 3 of a row whose base is aligned to 4 elements (a 16-byte or an 8-byte load)
template <int DT>
__device__ __forceinline__ void ld4(const void* row, int g, float (&v)[4]) {
  if constexpr (DT == MHAQ_FQ_DT_F32) {
    ldvg<4>(static_cast<const float*>(row) + 4 * g, v);
  } else {
    const io16::vu2 w = *gptr(reinterpret_cast<const io16::vu2*>(static_cast<const uint16_t*>(row) + 4 * g));
    io16::up2<DT>(w.x, v[0], v[1]);
    io16::up2<DT>(w.y, v[2], v[3]);
  }
}
// elements i .. i + 7 of a row whose address at i is 16-byte aligned
template <int DT>
__device__ __forceinline__ void ld8(const void* row, int64_t i, float (&v)[8]) {
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
template <int DT>
__device__ __forceinline__ void st1(void* p, int64_t i, float v) {
  if constexpr (DT == MHAQ_FQ_DT_F32) stg(static_cast<float*>(p) + i, v);
  else *gptr(static_cast<uint16_t*>(p) + i) = io16::down1<DT>(v);
}
// elements 4 * g .. 4 * g + 3 of a tensor whose base is aligned to 4 elements
template <int DT>
__device__ __forceinline__ void st4(void* p, int64_t g, const float (&v)[4]) {
  if constexpr (DT == MHAQ_FQ_DT_F32) {
    stvg<4>(static_cast<float*>(p) + 4 * g, v);
  } else {
    const io16::vu2 w = {io16::down2<DT>(v[0], v[1]), io16::down2<DT>(v[2], v[3])};
    *gptr(reinterpret_cast<io16::vu2*>(static_cast<uint16_t*>(p) + 4 * g)) = w;
  }
}

// bytes per element, with the dtype as a template argument or as a value (the entry points' alignment checks; also
// sr_prepare_kernel, whose instruction stream is the one this form gives)
template <int DT>
__host__ __device__ constexpr int esize() { return DT == MHAQ_FQ_DT_F32 ? 4 : 2; }
__host__ __device__ constexpr int esize(int dt) { return dt == MHAQ_FQ_DT_F32 ? 4 : 2; }

// ---- host side: the dtype of an entry point, checked, and then as a template argument (f receives it as a
// std::integral_constant and its result, if it has one, is handed back; the entry points have checked the dtype before)
inline bool known_dtype(int dt) { return dt == MHAQ_FQ_DT_F32 || dt == MHAQ_FQ_DT_BF16 || dt == MHAQ_FQ_DT_F16; }
template <class F>
auto with_dtype(int dt, F f) {
  if (dt == MHAQ_FQ_DT_F32) return f(std::integral_constant<int, MHAQ_FQ_DT_F32>{});
  if (dt == MHAQ_FQ_DT_BF16) return f(std::integral_constant<int, MHAQ_FQ_DT_BF16>{});
  return f(std::integral_constant<int, MHAQ_FQ_DT_F16>{});
}

}  // namespace iox
}  // namespace mhaq
