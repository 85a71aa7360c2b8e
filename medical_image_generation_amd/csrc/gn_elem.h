// Per-element arithmetic of the GroupNorm apply / backward-apply passes, shared by the kernels that evaluate it: groupnorm.hip
// (k_gn_apply, k_gn_bwd_partial, k_gn_bwd_apply) and the skip 1x1 conv of a ResnetBlock, which applies norm1 in its own pass over x
// (conv1x1.hip).  One definition, so both routes round alike.
#pragma once
#include "common.h"

// activation behind the affine: 0 none, 1 SiLU (UNet / AEKL), 2 LeakyReLU(0.2) (the PatchDiscriminator's BatchNorm layers)
template <int ACT>
__device__ __forceinline__ float act_f(float u) {
  if constexpr (ACT == 1) return silu_f(u);
  else if constexpr (ACT == 2) return u > 0.f ? u : 0.2f * u;
  else return u;
}
template <int ACT>
__device__ __forceinline__ float act_grad_f(float u) {
  if constexpr (ACT == 1) return silu_grad_f(u);
  else if constexpr (ACT == 2) return u > 0.f ? 1.f : 0.2f;
  else return 1.f;
}

// y = act(x * scale + shift)
template <int ACT>
__device__ __forceinline__ float gn_apply_elem(float x, float sc, float sh) {
  float u = x * sc + sh;
  return act_f<ACT>(u);
}

// dx = a * du + b * x + c with du = g * act'(x * scale + shift)  (the pending gradient branches are added by the caller, in its order)
template <int ACT>
__device__ __forceinline__ float gn_bwd_elem(float g, float x, float sc, float sh, float ca, float cb, float cc) {
  float du = g;
  if (ACT) du *= act_grad_f<ACT>(x * sc + sh);
  return ca * du + cb * x + cc;
}
