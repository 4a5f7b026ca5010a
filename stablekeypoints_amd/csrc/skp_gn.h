// The per-element arithmetic of the fused GroupNorm(+SiLU) forward, shared by every kernel that
// applies it (gn_apply_kernel in skp_groupnorm.hip, the Winograd input-transform pass in
// skp_conv.hip) so that they produce the same bits from the same (mean, rstd).
#pragma once
#include "skp_common.h"

namespace skp {

#ifndef SKP_GN_FAST
// 1: σ(z) through v_rcp_f32 (1 ulp) instead of the IEEE division sequence, and the channel of a
// group offset by a 32-bit division (the 64-bit one is a ≈40-instruction sequence per float4);
// 0: the r04 forms (A/B build)
#define SKP_GN_FAST 1
#endif
__device__ __forceinline__ float sigmoid_of(float z) {
#if SKP_GN_FAST
  return __builtin_amdgcn_rcpf(1.0f + __expf(-z));
#else
  return 1.0f / (1.0f + __expf(-z));
#endif
}
__device__ __forceinline__ float silu(float z) {
#if SKP_GN_FAST
  return z * sigmoid_of(z);
#else
  return z / (1.0f + __expf(-z));
#endif
}

// y = act((x + t)·ga + be) with ga = γ·rstd, be = β − mean·γ·rstd of the element's channel
struct GNCoef {
  float ga, be;
};
__device__ __forceinline__ GNCoef gn_coef(float gamma, float beta, float mean, float rstd) {
  return GNCoef{gamma * rstd, beta - mean * gamma * rstd};
}
template <bool ACT>
__device__ __forceinline__ float gn_elem(float x, float t, const GNCoef& k) {
  x += t;
  x = x * k.ga + k.be;
  return ACT ? silu(x) : x;
}

}  // namespace skp
