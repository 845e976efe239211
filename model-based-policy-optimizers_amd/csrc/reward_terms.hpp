// reward_terms.hpp — MBPO_REWARD_TERMS (include/mbpo_hip.h "term rewards"): the one device function that evaluates a term table.  The
// tile rollouts (csrc/rollout.hip), mbpo_reward_eval and BPTT's forward sweep (csrc/bptt.hip) all call reward_terms_eval, and it is
// written so that every call site yields the same bits: every product and sum is an explicit __fmul_rn / __fadd_rn / __fsub_rn (no
// contraction or reassociation is left to the surrounding code), terms and groups are walked in table order with one accumulator each,
// and the transcendentals are the accurate libm calls, not the hardware approximations of fast_math.hpp.
#pragma once
#include "common.hpp"

#define RT_GROUPS_OFF 4
#define RT_TERMS_OFF (4 + 4 * MBPO_REWARD_TERMS_MAX_GROUPS)

// a count or an index stored as a float, clamped to [0, hi] before the conversion (NaN -> 0)
__device__ __forceinline__ int rt_clamp_int(float v, int hi) { return (int)fminf(fmaxf(v, 0.f), (float)hi); }

// the x_next columns of z: the step's next state, or the pre-step state when any of its components is not finite
__device__ __forceinline__ const float *reward_terms_next(const float *xn, const float *x, int X) {
  if (!xn) return x;
  bool ok = true;
  for (int c = 0; c < X; ++c) ok &= fabsf(xn[c]) < __builtin_inff();      // (NaN fails the compare)
  return ok ? xn : x;
}

// f_k(v), and whether the id is known
__device__ __forceinline__ float rt_fn(int fn, float v) {
  switch (fn) {
    case MBPO_TERM_FN_IDENTITY: return v;
    case MBPO_TERM_FN_SQUARE: return __fmul_rn(v, v);
    case MBPO_TERM_FN_ABS: return fabsf(v);
    case MBPO_TERM_FN_RELU: return fmaxf(v, 0.f);
    case MBPO_TERM_FN_COS: return cosf(v);
    case MBPO_TERM_FN_SIN: return sinf(v);
  }
  return 0.f;
}

__device__ __forceinline__ float rt_link(int link, float s) {
  switch (link) {
    case MBPO_TERM_LINK_IDENTITY: return s;
    case MBPO_TERM_LINK_SQRT: return sqrtf(fmaxf(s, 0.f));
    case MBPO_TERM_LINK_EXP: return expf(s);
    case MBPO_TERM_LINK_TANH: return tanhf(s);
  }
  return 0.f;
}

// s_g of the group record gr (table `tab`, NT the header's clamped term count); z = [x (X) | u (UE) | xn (X)]
__device__ __forceinline__ float rt_group_sum(const float *tab, const float *gr, int NT, const float *x, const float *u, const float *xn,
                                              int X, int UE) {
  const int first = rt_clamp_int(gr[2], NT), cnt = rt_clamp_int(gr[3], NT - first);
  const float nz = (float)(2 * X + UE);
  float s = 0.f;
  for (int k = first; k < first + cnt; ++k) {
    const float *tr = tab + RT_TERMS_OFF + 4 * k;
    const float zi = tr[0], fid = tr[1];
    if (!(zi >= 0.f && zi < nz) || !(fid >= 0.f && fid <= (float)MBPO_TERM_FN_SIN)) continue;      // contributes 0 (NaN too)
    const int i = (int)zi;
    const float zv = i < X ? x[i] : (i < X + UE ? u[i - X] : xn[i - X - UE]);
    s = __fadd_rn(s, __fmul_rn(tr[2], rt_fn((int)fid, __fsub_rn(zv, tr[3]))));
  }
  return s;
}

// r of one row.  x [X], u [UE], xn [X] (what reward_terms_next returned); tab holds MBPO_REWARD_TERMS_FLOATS floats (global or LDS).
__device__ __forceinline__ float reward_terms_eval(const float *tab, const float *x, const float *u, const float *xn, int X, int UE) {
  const int NG = rt_clamp_int(tab[0], MBPO_REWARD_TERMS_MAX_GROUPS), NT = rt_clamp_int(tab[1], MBPO_REWARD_TERMS_MAX_TERMS);
  float r = tab[2];
  for (int g = 0; g < NG; ++g) {
    const float *gr = tab + RT_GROUPS_OFF + 4 * g;
    const float lid = gr[1];
    if (!(lid >= 0.f && lid <= (float)MBPO_TERM_LINK_TANH)) continue;
    r = __fadd_rn(r, __fmul_rn(gr[0], rt_link((int)lid, rt_group_sum(tab, gr, NT, x, u, xn, X, UE))));
  }
  return r;
}

// ---- the gradient, for BPTT (tables whose terms read x or u; a next-state term takes no gradient here) ----
// f_k'(v): abs and relu take the gradient torch takes at 0 (0)
__device__ __forceinline__ float rt_fn_grad(int fn, float v) {
  switch (fn) {
    case MBPO_TERM_FN_IDENTITY: return 1.f;
    case MBPO_TERM_FN_SQUARE: return 2.f * v;
    case MBPO_TERM_FN_ABS: return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f);
    case MBPO_TERM_FN_RELU: return v > 0.f ? 1.f : 0.f;
    case MBPO_TERM_FN_COS: return -sinf(v);
    case MBPO_TERM_FN_SIN: return cosf(v);
  }
  return 0.f;
}
// L_g'(s): the sqrt link has gradient 0 at s <= 0
__device__ __forceinline__ float rt_link_grad(int link, float s) {
  switch (link) {
    case MBPO_TERM_LINK_IDENTITY: return 1.f;
    case MBPO_TERM_LINK_SQRT: return s > 0.f ? 0.5f / sqrtf(s) : 0.f;
    case MBPO_TERM_LINK_EXP: return expf(s);
    case MBPO_TERM_LINK_TANH: { const float th = tanhf(s); return 1.f - th * th; }
  }
  return 0.f;
}
// d r / d z[comp] = sum_g w_g L_g'(s_g) sum_{k in g: i_k == comp} c_k f_k'(z[i_k] - t_k), comp < X + UE.  One (row, component) per
// thread: a group none of whose terms reads the component is skipped before its sum is formed.
__device__ __forceinline__ float reward_terms_grad_comp(const float *tab, const float *x, const float *u, int X, int UE, int comp) {
  const int NG = rt_clamp_int(tab[0], MBPO_REWARD_TERMS_MAX_GROUPS), NT = rt_clamp_int(tab[1], MBPO_REWARD_TERMS_MAX_TERMS);
  float acc = 0.f;
  for (int g = 0; g < NG; ++g) {
    const float *gr = tab + RT_GROUPS_OFF + 4 * g;
    const float lid = gr[1];
    if (!(lid >= 0.f && lid <= (float)MBPO_TERM_LINK_TANH)) continue;
    const int first = rt_clamp_int(gr[2], NT), cnt = rt_clamp_int(gr[3], NT - first);
    float inner = 0.f;
    bool any = false;
    for (int k = first; k < first + cnt; ++k) {
      const float *tr = tab + RT_TERMS_OFF + 4 * k;
      const float fid = tr[1];
      if (tr[0] != (float)comp || !(fid >= 0.f && fid <= (float)MBPO_TERM_FN_SIN)) continue;
      const float zv = comp < X ? x[comp] : u[comp - X];
      inner += tr[2] * rt_fn_grad((int)fid, zv - tr[3]);
      any = true;
    }
    if (any) acc += gr[0] * rt_link_grad((int)lid, rt_group_sum(tab, gr, NT, x, u, x, X, UE)) * inner;
  }
  return acc;
}
