// rollout_tile.hpp — what the two tile rollout kernels (k_model_rollout64: rollout64_kernel.hpp; k_model_rollout<128 | 256>:
// rollout_wide_kernel.hpp) and their host (rollout.hip) share: the reward selector, the hold of a time-adaptive rollout, the layout of the
// LDS behind s_rew, and the run-time flags a launch function turns into template arguments.
#pragma once
#include "common.hpp"
#include "rollout_shared.hpp"
#include "reward_terms.hpp"

// LR: how the reward is formed, three values (the learned reward and the term table exclude each other, so the third value adds half
// the instantiations, not double): FORMULA the Pendulum / quadratic reward picked by a run-time test of reward_kind, LEARNED
// MBPO_REWARD_LEARNED, TERMS MBPO_REWARD_TERMS (csrc/reward_terms.hpp).  Compile-time, so that the instantiations that existed before a
// value was added are emitted as they were (profiles/r14_term_reward_registers.txt).
#define RO_LR_FORMULA 0
#define RO_LR_LEARNED 1
#define RO_LR_TERMS 2
template <class F>
static int mbpo_with_lr(int lr, F &&f) {
  if (lr == RO_LR_TERMS) return f(std::integral_constant<int, RO_LR_TERMS>{});
  return lr == RO_LR_LEARNED ? f(std::integral_constant<int, RO_LR_LEARNED>{}) : f(std::integral_constant<int, RO_LR_FORMULA>{});
}
// TERMS: the reward reads the next state, so it is formed behind the barrier that follows the next-state write instead of in front of
// it, from the table staged in LDS (MBPO_REWARD_TERMS_FLOATS floats behind everything else: the host grows the block for this kind only)
// START: a start buffer is set (include/mbpo_hip.h "fresh starts").  A flag of its own: as a run-time test on start.rows it added 32 to
// 40 bytes of scratch per lane to every instantiation and two spilled registers to <128, false> (profiles/r09_fresh_starts_registers.txt)
// the controls the dynamics and the rewards see (u_env).  An expression, not a variable, and `if constexpr (HAL)` throughout: an
// instantiation with HAL = false is then emitted exactly as it was before the flag existed.  (With a local `UE` and run-time `if (HAL)`
// tests, all constant and all folded, seven existing k_model_rollout64 instantiations still came out with one to four SGPR spills more
// or fewer: profiles/r10_hallucinated_registers.txt.)
#define RO_UE (HAL ? U - X : (TA ? U - 1 : U))
// TA: a time-adaptive rollout (hold_max_steps > 0; include/mbpo_hip.h "time-adaptive rollouts").  A flag of its own, like HAL, with an
// argument block of its own.  The action is [u (U - 1) | tau]: the member chains and the rewards read the x + U - 1 leading columns
// of s_xu, tau sits where the padding was.  The hold is the action_repeat loop with a per-row count: the host hands these
// instantiations K in action_repeat (the descriptor's own must be 1), so every element index ((s * AR + ar) * N + env) is the
// documented one ((s * K + j) * N + env) without another formula; the rows' k, the steps they took and whether they terminated live
// in LDS (s_hold: [0, 16) k, [16, 32) inner steps taken, [32, 48) terminated, [48] the tile's largest k, which bounds the loop).  The
// member chains run on the whole tile; reward and next state are committed for the rows with j < k that have not terminated.
struct HoldArgs {
  int max_steps;                // K
  float min_time, max_time, dt, gamma, switch_cost;
};

// TA: the rows' hold counts, once per decision by the first wave (the action is in s_xu, a barrier behind its writers): k = 0 for the
// rows past the batch, which are then never committed.  The caller's barrier publishes s_hold.
template <class Args>
__device__ __forceinline__ void hold_setup(const Args &H, float *s_hold, const float *s_xu, int ld_xu, int tau_col, long long env0,
                                           long long N, int wave, int lane) {
  if (wave == 0) {
    int kk = 0;
    if (lane < 16 && env0 + lane < N) kk = hold_steps(s_xu[lane * ld_xu + tau_col], H.min_time, H.max_time, H.dt, H.max_steps);
    if (lane < 16) {
      s_hold[lane] = (float)kk;
      s_hold[16 + lane] = 0.f;
      s_hold[32 + lane] = 0.f;
    }
    for (int off = 8; off; off >>= 1) {
      const int o = __shfl_xor(kk, off);
      kk = o > kk ? o : kk;
    }
    if (lane == 0) s_hold[48] = (float)kk;
  }
}
// row r is still being stepped at inner step j
__device__ __forceinline__ bool hold_live(const float *s_hold, int r, int j) { return (float)j < s_hold[r] && s_hold[32 + r] == 0.f; }
// the tile's largest k: the inner loop's bound, uniform over the workgroup
__device__ __forceinline__ int hold_bound(const float *s_hold) { return __builtin_amdgcn_readfirstlane((int)s_hold[48]); }
// w_j = gamma^j as the running product forms it (w_0 = 1, w_{j+1} = w_j * gamma)
__device__ __forceinline__ float hold_weight(float gamma, int j) {
  float w = 1.f;
  for (int i = 0; i < j; ++i) w *= gamma;
  return w;
}
// TA: gamma of the hold (the argument blocks of the other instantiations have none)
template <bool TA, class Args>
__device__ __forceinline__ float hold_gamma(const Args &A) {
  if constexpr (TA) return A.hold.gamma;
  else return 1.f;
}
// A step's reward into the row's sum: the plain sum, or (TA) w_j * r, the product rounded on its own, then added (no fused multiply-add),
// for the rows still held.  The weight is the caller's: the two kernels derive it differently.
template <bool TA>
__device__ __forceinline__ void reward_accumulate(float *s_rew, const float *s_hold, int r, int j, float w, float rew) {
  if constexpr (TA) {
    const float wr = w * rew;
    if (hold_live(s_hold, r, j)) s_rew[r] += wr;
  } else {
    s_rew[r] += rew;
  }
}

// ------------------------------------------------------------------------------------------------
// The tile kernels' LDS behind the member outputs s_y, written once.  The host sizes the block from these functions; the kernels' own
// carves (k_model_rollout64: s_scr, s_rp, RO64_HOLD, RO64_TAB; k_model_rollout: s_hold, the `16 + ((X + 3) & ~3) + 64` of its table) keep
// their expressions, because a folded local has moved SGPR spills in these kernels before (the notes at RO_UE and RolloutArgs64TA), and
// must agree with them.  All figures are floats.
// ------------------------------------------------------------------------------------------------
struct RolloutTail {
  int scr, rp, hold, tab, end;  // offsets from s_rew (s_rew itself is [0, 16)); a region a kernel does not have is empty
};
__host__ __device__ inline int ro_up4(int v) { return (v + 3) & ~3; }
// k_model_rollout64: [scratch: next state, per-dim log-prob, the rows' SystemState.done | staged reward parameters (HAL: beta in their
// last X floats) | TA: the rows' hold state | TERMS: the staged table]
__host__ __device__ inline RolloutTail rollout64_tail(int X, int U, bool ta, bool terms) {
  RolloutTail t;
  t.scr = 16;
  t.rp = t.scr + ro_up4(16 * (X + U) + 16);
  t.hold = t.rp + ro_up4(2 * X + U + 4);
  t.tab = t.hold + (ta ? 64 : 0);
  t.end = t.tab + (terms ? MBPO_REWARD_TERMS_FLOATS : 0);
  return t;
}
// k_model_rollout<128 | 256>: [HAL: beta [X], or TA: the rows' hold state [49], in up4(X) + 64 floats | TERMS: the staged table]
__host__ __device__ inline RolloutTail rollout_wide_tail(int X, bool terms) {
  RolloutTail t;
  t.scr = t.rp = t.hold = 16;
  t.tab = t.hold + ro_up4(X) + 64;
  t.end = t.tab + (terms ? MBPO_REWARD_TERMS_FLOATS : 0);
  return t;
}
// everything in front of s_rew but the chains' ping-pong tiles: s_obs, s_first, s_pin, s_xu, s_y, the transition rows (`row_bufs` of
// them), the step counters (one set per row buffer) and s_done
__host__ __device__ inline size_t rollout_head_floats(int ld_x, int ld_xu, int ld_y, int n_out, int D, int row_bufs) {
  return 3ull * 16 * ld_x + 16ull * ld_xu + (size_t)n_out * 16 * ld_y + (size_t)row_bufs * 16 * ro_up4(D) + 16ull * row_bufs + 16;
}

// The run-time flags that a launch function (rollout64.hpp, rollout_wide.hpp) turns into template arguments.
struct RolloutFlags {
  bool wide, term, start, hal, ta;
};
// the two combinations that have no instantiation: TA with HAL (either kernel), TA with WIDE (k_model_rollout64)
static inline int rollout_refuse_ta(bool hal) {
  MBPO_REQUIRE(!hal, MBPO_ERR_ARG, "model_rollout: hold_max_steps and halluc_beta cannot both be set");
  MBPO_REQUIRE(false, MBPO_ERR_UNSUPPORTED,
               "model_rollout: hold_max_steps has no k_model_rollout64<WIDE> instantiation (64-wide networks with more than 16 inputs or outputs)");
  return MBPO_OK;
}
