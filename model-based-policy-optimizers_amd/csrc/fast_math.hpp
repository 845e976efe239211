// fast_math.hpp — the hardware-transcendental helpers of the elementwise sections, in one place.
//
// The elementwise sections (NormalTanh sampling and log-probs, the BPTT log-prob gradient, hidden-layer activations) run on one or
// two waves while the rest of the workgroup waits at a barrier, and a lone wave issues one instruction per 4 cycles: libm's expf /
// log1pf / logf / tanhf (30-60 instructions each) were the sections' whole time.  These forms use v_exp_f32 (2^x), v_log_f32
// (log2 x) and v_rcp_f32 (~1 ulp each) instead.  Every kernel takes them from here, so a lean kernel and the generic kernel it
// replaces evaluate the same expressions and keep agreeing bit for bit.
//
// Accuracy (fp64 reference; tests/test_gpu_fastmath.py checks each through mbpo_debug_eval_fastmath, api.hip):
//   fm_softplus   relative error <= 1e-6 on [-80, 80]: collapsed policy stds (raw << 0) keep their relative accuracy
//   fm_tanh       relative error <= 1e-6 on 1e-6 <= |x| <= 15, exactly +-1 beyond, odd
//   fm_atanh      relative error <= 1e-6 on 1e-6 <= |a| <= 0.999, odd
//   fast_sigmoid  relative error <= 2e-6 on |v| <= 20
// BPTT (no floor under its std), PPO and SAC's layered path take fm_softplus / fm_tanh (BPTT also fm_atanh); the fused SAC kernels
// and the rollout take the plain fm_softplus_fast / fm_tanh_fast below.  tests/test_gpu_regimes.py measured PPO's policy gradient
// off by up to 0.6 % at collapsed stds and the layered SAC critic loss by 2e-5 relative with the plain forms.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ float fm_exp(float x) { return __builtin_amdgcn_exp2f(1.44269504088896340736f * x); }
__device__ __forceinline__ float fm_log(float x) { return 0.69314718055994530942f * __builtin_amdgcn_logf(x); }

// exp(x) with the rounding of x * log2(e) put back: fm_exp's relative error grows as |x| * 6e-8 (the product's rounding is an
// absolute error in the exponent), which is 5e-6 at |x| = 80.  h + l == x * log2(e) to ~2^-48 relative; 2^l = 1 + l ln 2.
__device__ __forceinline__ float fm_exp_acc(float x) {
  const float h = 1.44269504088896340736f * x;
  const float l = fmaf(x, 1.925963e-8f, fmaf(x, 1.44269502162933349609f, -h));   // log2(e) = 1.44269502162933349609 + 1.925963e-8
  const float e = __builtin_amdgcn_exp2f(h);
  return fmaf(e * l, 0.69314718055994530942f, e);
}

// log1p(t) for t > -1: rounding u = 1 + t loses t's low bits once t < 2^-24 * u; Goldberg's correction t / (u - 1) (u - 1 is exact)
// puts them back, so the result keeps t's relative accuracy (What Every Computer Scientist Should Know..., Theorem 4).
__device__ __forceinline__ float fm_log1p(float t) {
  const float u = 1.0f + t;
  return u == 1.0f ? t : fm_log(u) * (t * __builtin_amdgcn_rcpf(u - 1.0f));
}

// jax.nn.softplus(x) = max(x,0) + log1p(exp(-|x|)).  For x << 0 it is ~exp(x): both the log1p and the exp must keep relative
// accuracy there (the plain log(1 + exp(x)) is 0 below x = -17 and off by percents from x = -13).  The exponent is clamped at -104,
// where exp already rounds to 0, so that +-inf give inf and 0 (fm_exp_acc(-inf) is inf * 0); NaN still propagates.
__device__ __forceinline__ float fm_softplus(float x) {
  const float n = -fabsf(x);
  return fmaxf(x, 0.0f) + fm_log1p(fm_exp_acc(n < -104.0f ? -104.0f : n));
}

// tanh.  |x| < 0.5: an odd polynomial (x + x^3 p(x^2), fit to tanh on [0, 0.5]; (e - 1) / (e + 1) cancels as x -> 0).  Beyond:
// 1 - 2 / (e^{2|x|} + 1) with |x| clamped at 15, which rounds to exactly 1 once tanh does; the sign is put back.
__device__ __forceinline__ float fm_tanh(float x) {
  const float ax = fabsf(x);
  if (ax < 0.5f) {
    const float s = x * x;
    float p = -0.0069470033f;
    p = fmaf(p, s, 0.021472720f);
    p = fmaf(p, s, -0.053933788f);
    p = fmaf(p, s, 0.13333227f);
    p = fmaf(p, s, -0.33333331f);
    return x * fmaf(s, p, 1.0f);                      // (x * (...): tanh(-0) = -0)
  }
  const float e = fm_exp(2.0f * fminf(ax, 15.0f));
  return copysignf(1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f), x);
}

// atanh(a) = sign(a) 0.5 log1p(2|a| / (1 - |a|)) for |a| < 1: no cancellation as a -> 0, and 1 - |a| is exact near |a| = 1.
// Domain |a| < 1 only: +-1 gives NaN (log(inf) * (inf * rcp(inf))), not +-inf.  The caller (BPTT) clamps to +-0.999 first.
__device__ __forceinline__ float fm_atanh(float a) {
  const float aa = fabsf(a);
  return copysignf(0.5f * fm_log1p(2.0f * aa * __builtin_amdgcn_rcpf(1.0f - aa)), a);
}

// The plain forms, kept by the fused SAC kernels and the rollout (sac_shared.hpp, rollout_shared.hpp).  They keep the bits the
// SAC learning-rate measurements were taken on.  Accuracy (tests/test_gpu_fastmath.py):
//   fm_softplus_fast  absolute error <= 2e-7 + 1e-6 |softplus(x)|; it is exactly 0 below x ~ -17.3 (1 + exp(x) rounds to 1) and loses
//                     relative accuracy below x ~ -3.  Their policy std is softplus(raw) + 0.001: the floor bounds the error in
//                     sigma to <= 1e-4 relative (~6e-5 in the worst case).  tests/test_gpu_regimes.py runs SAC and the rollout at
//                     collapsed stds against the fp64 oracle.
//   fm_tanh_fast      absolute error <= 3e-7 on [-15, 15]; relative accuracy lost as x -> 0 ((e - 1) cancels); |result| may exceed 1
//                     by one ulp (v_rcp_f32's rounding).
__device__ __forceinline__ float fm_softplus_fast(float x) { return fmaxf(x, 0.0f) + fm_log(1.0f + fm_exp(-fabsf(x))); }
__device__ __forceinline__ float fm_tanh_fast(float x) {
  const float e = fm_exp(2.0f * fminf(fmaxf(x, -15.0f), 15.0f));
  return (e - 1.0f) * __builtin_amdgcn_rcpf(e + 1.0f);
}

// sigmoid: v_exp_f32 + v_rcp_f32, ~5 instructions against ~50 for libm expf and an IEEE division.  One wave evaluates 16
// activations per layer, so the libm form cost as much as the layer's MFMAs.
__device__ __forceinline__ float fast_sigmoid(float v) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504088896340736f * v));
}
