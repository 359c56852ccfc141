// What the object-detection validation sources (od_nms.hip, od_sort.hip) share: the element load with its exact conversion
// up, the key of a candidate, and the host-side argument checks.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/mhaq_fq.h"
#include "fq_common.hpp"
#include "fq_io16.hpp"

namespace mhaq {

constexpr int64_t kOdNoKey = 0x7fffffffffffffffLL;

template <int DT>
__device__ __forceinline__ float od_ld(const void* p, int64_t i) {
  if constexpr (DT == MHAQ_FQ_DT_F32) return ldg(static_cast<const float*>(p) + i);
  else return io16::up1<DT>(*gptr(static_cast<const uint16_t*>(p) + i));
}

// the key of candidate (a, c) with score s > conf_thr >= 0: the bits of s are a positive int32
__device__ __forceinline__ int64_t od_key(float s, int a, int nc, int c) {
  return (int64_t)(((uint64_t)(uint32_t)(0x7fffffff - (int32_t)__float_as_uint(s)) << 32) | (uint32_t)(a * nc + c));
}

__host__ __device__ __forceinline__ bool od_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }      // false for a NaN

template <class F>
void od_with_dtype(int dtype, F f) {
  if (dtype == MHAQ_FQ_DT_F32) f(std::integral_constant<int, MHAQ_FQ_DT_F32>{});
  else if (dtype == MHAQ_FQ_DT_BF16) f(std::integral_constant<int, MHAQ_FQ_DT_BF16>{});
  else f(std::integral_constant<int, MHAQ_FQ_DT_F16>{});
}
inline bool od_dtype_known(int dt) { return dt == MHAQ_FQ_DT_F32 || dt == MHAQ_FQ_DT_BF16 || dt == MHAQ_FQ_DT_F16; }
inline bool od_shape_supported(int64_t B, int64_t nc, int64_t A) {
  return B <= 65535 && nc <= 65535 && A <= 0x7fffffff && A * nc <= 0x7fffffff;
}

}  // namespace mhaq
