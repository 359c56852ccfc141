// 16-bit (bf16 / fp16) element I/O shared by the kernels that stream 16-bit tensors (fq_io16.hip, bn_bwd.hip):
// 16 B per lane = 8 elements per access, exact conversion up, one round-to-nearest-even down.
#pragma once

#include <type_traits>

#include "fq_common.hpp"

namespace mhaq {
namespace io16 {

typedef uint32_t vu4 __attribute__((ext_vector_type(4)));
typedef float vf2 __attribute__((ext_vector_type(2)));
typedef __bf16 vbf2 __attribute__((ext_vector_type(2)));
typedef _Float16 vh2 __attribute__((ext_vector_type(2)));

// ---- conversions.  Up: exact.  Down: round to nearest-even, NaN stays NaN (v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32 on
// gfx950; a plain cast -- the integer-rounding trick would turn some NaNs into infinities).
template <int DT>
__device__ __forceinline__ float up1(uint16_t h) {
  if constexpr (DT == MHAQ_FQ_DT_BF16) return __uint_as_float((uint32_t)h << 16);
  else return (float)__builtin_bit_cast(_Float16, h);
}
template <int DT>
__device__ __forceinline__ void up2(uint32_t w, float& lo, float& hi) {
  if constexpr (DT == MHAQ_FQ_DT_BF16) {
    lo = __uint_as_float(w << 16);
    hi = __uint_as_float(w & 0xffff0000u);
  } else {
    const vh2 h = __builtin_bit_cast(vh2, w);
    lo = (float)h.x;
    hi = (float)h.y;
  }
}
template <int DT>
__device__ __forceinline__ uint16_t down1(float f) {
  if constexpr (DT == MHAQ_FQ_DT_BF16) return __builtin_bit_cast(uint16_t, (__bf16)f);
  else return __builtin_bit_cast(uint16_t, (_Float16)f);
}
template <int DT>
__device__ __forceinline__ uint32_t down2(float lo, float hi) {
  const vf2 v = {lo, hi};
  if constexpr (DT == MHAQ_FQ_DT_BF16) return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, vbf2));
  else return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, vh2));
}

template <bool NT>
__device__ __forceinline__ vu4 ld8(const uint16_t* p, int64_t vidx) {
  const vu4* q = reinterpret_cast<const vu4*>(p) + vidx;
  return NT ? __builtin_nontemporal_load(q) : *q;
}
template <bool NT>
__device__ __forceinline__ void st8(uint16_t* p, int64_t vidx, vu4 v) {
  vu4* q = reinterpret_cast<vu4*>(p) + vidx;
  if (NT) __builtin_nontemporal_store(v, q); else *q = v;
}

// ---- host side: the dtype of an *_x16 entry point, checked, and then as a template argument (f receives it as a
// std::integral_constant and its result is handed back; the entry points have checked the dtype before they get here)
inline bool known_dtype(int dt) { return dt == MHAQ_FQ_DT_BF16 || dt == MHAQ_FQ_DT_F16; }
template <class F>
auto with_dtype(int dtype, F f) {
  if (dtype == MHAQ_FQ_DT_BF16) return f(std::integral_constant<int, MHAQ_FQ_DT_BF16>{});
  return f(std::integral_constant<int, MHAQ_FQ_DT_F16>{});
}

}  // namespace io16
}  // namespace mhaq
