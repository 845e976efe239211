// rollout64_kernel.hpp — R1-R8 fused model rollout, hidden width 64, on phase runners (see include/mbpo_hip.h and the note at
// RolloutArgs64, rollout64.hpp).  Included by the unit that instantiates it (rollout64.hip); the host reaches it through rollout64.hpp.
#pragma once
#include "common.hpp"
#include "chain_run.hpp"
#include "rollout64.hpp"

#define RO_STAMP(i)                                                                  \
  if (AA.stamps && blockIdx.x == 0 && s == 1 && tid_ == 0) {                           \
    unsigned long long t_;                                                           \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");       \
    AA.stamps[i] = t_;                                                               \
  }

// The thread id, re-derived where it is needed: wave id (an SGPR since the top of the kernel) * 64 + the lane's position from
// v_mbcnt.  Holding threadIdx.x itself across the step loop made hipcc park it in scratch (one of 168 VGPRs too many): 8 bytes
// per lane stored at the top of every launch — 1.6 MB of the 2.59 MB the PMC counters saw this kernel write for 0.98 MB of rows
// (profiles/r02_pmc_traffic.json).  volatile: not hoisted out of the loops, so nothing has to stay live for it.
__device__ __forceinline__ int ro_tid_now(int wave) {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return (wave << 6) | l;
}

// LR: MBPO_REWARD_LEARNED (section C reads the reward from the members' outputs; a flag of its own so the other instantiations stay
// as they were)
// TERM: a termination box is set (a flag of its own for the same reason: the run-time test cost the plain instantiation two spilled
// registers in the step loop; with it the step gains one barrier)
// START: a start buffer is set (a flag of its own, likewise): section D replaces the first_obs element it has just consumed
// HAL: hallucinated control (a flag of its own, likewise; see k_model_rollout): section C's 'mean' branch adds beta * sd * eta
// (the HAL instantiations' argument block, for the reason given at RolloutArgsHal)
struct RolloutArgs64Hal : RolloutArgs64 {
  const float *halluc_beta;     // [x_dim]
};
// TA: a time-adaptive rollout (a flag of its own, likewise; see k_model_rollout): section C commits the reward and the next state of
// the rows still held and re-emits the state of the others, so the scratch always holds every row's current state and section D reads
// it as before; a row's termination is decided after each of its inner steps, into s_hold, and copied to where section D reads it.
// Nothing here is a new local variable of the TA = false path (s_hold is the expression RO64_HOLD, the loop bound and the weight are
// re-derived where they are used): with locals, all dead and all folded, fourteen LR instantiations came out with one to ten SGPR
// spills more or fewer, as the note at RO_UE reports for HAL.  One barrier
// more per decision (the rows' k) and none per inner step.
struct RolloutArgs64TA : RolloutArgs64 {
  HoldArgs hold;
};
template <bool HAL, bool TA = false>
using RolloutArgs64For = typename std::conditional<TA, RolloutArgs64TA, typename std::conditional<HAL, RolloutArgs64Hal, RolloutArgs64>::type>::type;

template <bool WIDE, int LR, bool TERM, bool START, bool HAL, bool TA = false>
__global__ void __launch_bounds__(64 * RO64_WAVES) k_model_rollout64(RolloutArgs64For<HAL, TA> AA) {
  extern __shared__ __align__(16) float smem[];
  const RolloutArgs &A = AA.a;
  constexpr int HT = 4;
  const int tid_ = threadIdx.x, nthreads = 64 * RO64_WAVES;
  const int wave = __builtin_amdgcn_readfirstlane(tid_ >> 6);
  const int X = A.x_dim, U = A.u_dim, D = A.row_len;
  const int E = (A.system_kind == MBPO_SYS_ENSEMBLE) ? A.dyn.n_nets : 0;
  const long long N = A.n_envs;
  const int AR = A.action_repeat;
  const int ld_x = A.ld_x, ld_xu = A.ld_xu, ld_h = A.ld_h, ld_y = A.ld_y;
  const int T = 16 * ld_h;
  const int PL = A.actions ? 0 : AA.sh_pi.L, DL = AA.sh_dyn.L;

  // ---- LDS carve (floats) ----
  float *s_obs = smem;                           // [16][ld_x]  current raw obs
  float *s_first = s_obs + 16 * ld_x;            // [16][ld_x]
  float *s_pin = s_first + 16 * ld_x;            // [16][ld_x]  normalised obs (policy input)
  float *s_xu = s_pin + 16 * ld_x;               // [16][ld_xu] dynamics input [x,u]
  float *s_pp = s_xu + 16 * ld_xu;               // [n_chains][2] hidden tiles (ping-pong per chain)
  float *s_y = s_pp + A.n_chains * 2 * T;        // [n_out][16][ld_y]
  const int D4 = (D + 3) & ~3;
  float *s_rows = s_y + A.n_out * 16 * ld_y;     // [2][16][D]  transition rows, double-buffered over steps
  float *s_steps = s_rows + 2 * 16 * D4;         // [2][16]     double-buffered over steps
  float *s_done = s_steps + 32;                  // [16]
  float *s_rew = s_done + 16;                    // [16]
  float *s_scr = s_rew + 16;                     // [16 * max(X, U)] scratch: next state / per-dim log-prob
  const int SC = X > U ? X : U;
  (void)SC;
  // reward parameters staged once: section C read them from global memory inside a runtime-trip loop (one exposed scalar
  // load per term: ~1.5 k of that section's 3.6 k cycles)
  float *s_rp = s_scr + ((16 * (X + U) + 16 + 3) & ~3);   // [2X+U] quadratic (target, q, r) or [3] pendulum
  if (LR == RO_LR_FORMULA) {
    const int n_rp = (A.reward_kind == MBPO_REWARD_PENDULUM) ? 3 : 2 * X + RO_UE;
    for (int idx = tid_; idx < n_rp; idx += nthreads) s_rp[idx] = A.reward_params[idx];
  }
  // HAL: beta staged once per workgroup, in the X floats of s_rp that the reward's narrower control cost leaves free: s_rp[X + U + c]
  // (2X + UE == X + U)
  if constexpr (HAL)
    for (int idx = tid_; idx < X; idx += nthreads) s_rp[X + U + idx] = AA.halluc_beta[idx];
  // TA: the rows' k, inner steps taken and terminated flags, the tile's largest k (the host adds these 64 floats)
#define RO64_HOLD (s_rp + ((2 * X + U + 4 + 3) & ~3))
  // TERMS: the table staged once per workgroup, behind the hold state where there is one (the host adds MBPO_REWARD_TERMS_FLOATS floats
  // for this kind only; the tile load's barrier below orders it before its first use)
#define RO64_TAB (RO64_HOLD + (TA ? 64 : 0))
  if constexpr (LR == RO_LR_TERMS)
    for (int idx = tid_; idx < MBPO_REWARD_TERMS_FLOATS; idx += nthreads) RO64_TAB[idx] = A.reward_params[idx];

  const RngKey rk_ = rng_resolve(A.seed, A.offset, A.rng_dev);
  const unsigned long long rng_off = rk_.offset, rng_seed = rk_.seed;
  const long long n_tiles = (N + 15) >> 4;
  const int mchain = wave >> 1, msub = wave & 1;   // member-phase role of this wave
  // START: the true buffer's {sample_position, insert_position, head}
  const int sb_lo = START ? A.start.state[1] : 0, sb_hi = START ? A.start.state[0] : 0, sb_head = START ? A.start.state[2] : 0;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long env0 = tile * 16;
    {
      const int tid = ro_tid_now(wave);
      for (int idx = tid; idx < 16 * X; idx += nthreads) {
        const int r = idx & 15, c = idx >> 4;
        const long long env = env0 + r;
        float o = 0.f, f = 0.f;
        if (env < N) {
          o = A.obs[env * X + c];
          f = A.first_obs[env * X + c];
        }
        s_obs[r * ld_x + c] = o;
        s_first[r * ld_x + c] = f;
      }
      if (tid < 16) {
        const long long env = env0 + tid;
        s_steps[tid] = env < N ? A.steps[env] : 0.f;
        s_done[tid] = env < N ? A.done[env] : 0.f;
      }
    }
    __syncthreads();

#pragma nounroll
    for (int s = 0; s < A.n_steps; ++s) {
      const int tid = ro_tid_now(wave), lane = tid & 63;
      float *s_row = s_rows + (s & 1) * 16 * D4;
      float *steps_cur = s_steps + (s & 1) * 16, *steps_nxt = s_steps + ((s + 1) & 1) * 16;
      WSet<HT, 4> Rp;
      WSet<HT, 2> Rm;
      RO_STAMP(0);
      // ---- section A: policy input, obs into the dynamics input and the row; open-loop actions ----
      if (!A.actions && wave < 4) chain_fwd_prefetch<HT, 4, WIDE>(Rp, AA.sh_pi, A.policy.params, wave, lane);
      for (int idx = tid; idx < 16 * X; idx += nthreads) {
        const int r = idx & 15, c = idx >> 4;
        const float o = s_obs[r * ld_x + c];
        s_pin[r * ld_x + c] = A.norm_mean ? (o - A.norm_mean[c]) / A.norm_std[c] : o;   // running_statistics.normalize
        s_xu[r * ld_xu + c] = o;
        s_row[r * D + c] = o;                                                            // Transition.observation (acting.py:47)
      }
      if (A.actions) {
        // open-loop actions (rollout_actions, optimizer_utils.py:26-38): no policy
        for (int idx = tid; idx < 16 * U; idx += nthreads) {
          const int r = idx & 15, d = idx >> 4;
          const long long env = env0 + r;
          const float a = env < N ? A.actions[((long long)s * N + env) * U + d] : 0.f;
          s_xu[r * ld_xu + X + d] = a;
          s_row[r * D + X + d] = a;
        }
      }
      __syncthreads();
      RO_STAMP(1);
      // ---- policy chain -> logits in s_y[0] ----
      if (!A.actions) {
        if (wave < 4) chain_fwd_run<HT, 4, WIDE>(AA.sh_pi, A.policy.params, s_pin, ld_x, s_pp, s_pp + T, nullptr, nullptr, s_y, ld_y, ld_h, PL, wave, lane, Rp);
        else chain_idle_run(PL);
      }
      RO_STAMP(2);
      const bool mactive = (E > 0) && (mchain < A.n_chains) && (mchain < E);
      if (mactive) chain_fwd_prefetch<HT, 2, WIDE>(Rm, AA.sh_dyn, A.dyn.params + (long long)mchain * A.dyn.net_stride, msub, lane);
      // ---- section B: NormalTanh sample (parametric_distribution.py:97-124) + AutoReset pre-step (training.py:119-124) ----
      if (!A.actions) {
        for (int idx = tid; idx < 16 * U; idx += nthreads) {
          const int r = idx & 15, d = idx >> 4;
          const long long env = env0 + r;
          const float loc = s_y[r * ld_y + d], raw = s_y[r * ld_y + U + d];
          const float sigma = fm_softplus_fast(raw) + 0.001f;
          float eps = 0.f;
          if (!A.deterministic && env < N) {
            const long long nidx = ((long long)s * N + env) * U + d;
            eps = A.policy_noise ? A.policy_noise[nidx]
                                 : philox_normal(rng_seed, rng_off, MBPO_STREAM_POLICY_NOISE, (unsigned long long)nidx);
          }
          const float z = loc + sigma * eps;
          float a = fm_tanh_fast(z);
          if (A.action_clip > 0.f) a = fminf(fmaxf(a, -A.action_clip), A.action_clip);
          s_xu[r * ld_xu + X + d] = a;
          s_row[r * D + X + d] = a;
          if (A.ppo_extras) {
            // log N(z; loc, sigma) - log|d tanh/dz|, per action dim; summed in section D
            const float lp = -0.5f * eps * eps - fm_log(sigma) - 0.91893853320467274178f;
            const float ldj = 2.0f * (0.69314718055994530942f - z - fm_softplus_fast(-2.0f * z));
            s_row[r * D + 2 * X + U + 2 + 1 + d] = z;               // raw_action
            s_scr[16 * X + r * U + d] = lp - ldj;                   // per-dim log-prob (behind the next-state scratch)
          }
        }
      }
      if (tid < 16) {
        // AutoReset: steps <- 0 where previously done; done <- 0
        if (s_done[tid] != 0.f) steps_cur[tid] = 0.f;
        s_done[tid] = 0.f;
        s_rew[tid] = 0.f;
      }
      __syncthreads();
      RO_STAMP(3);
      if constexpr (TA) {
        hold_setup(AA.hold, RO64_HOLD, s_xu, ld_xu, X + U - 1, env0, N, wave, lane);
        __syncthreads();
      }

      // ---- EpisodeWrapper inner scan over action_repeat (training.py:91-97); TA: up to the tile's largest k ----
#pragma nounroll
      for (int ar = 0; ar < (TA ? hold_bound(RO64_HOLD) : AR); ++ar) {
        if (E > 0) {
#pragma nounroll
          for (int e0 = 0; e0 < E; e0 += A.n_chains) {
            const int e = e0 + mchain;
            const bool act = (mchain < A.n_chains) && (e < E);
            if (act && (e0 > 0 || ar > 0))
              chain_fwd_prefetch<HT, 2, WIDE>(Rm, AA.sh_dyn, A.dyn.params + (long long)e * A.dyn.net_stride, msub, lane);
            if (act)
              chain_fwd_run<HT, 2, WIDE>(AA.sh_dyn, A.dyn.params + (long long)e * A.dyn.net_stride, s_xu, ld_xu, s_pp + mchain * 2 * T,
                                   s_pp + mchain * 2 * T + T, nullptr, nullptr, s_y + e * 16 * ld_y, ld_y, ld_h, DL, msub, lane, Rm);
            else
              chain_idle_run(DL);
          }
        }
        RO_STAMP(4);
        // ---- section C: reward on the pre-step (x, u); next state into the scratch ----
        if (tid < 16) {
          const int r = tid;
          const float *xr = s_xu + r * ld_xu;
          if constexpr (LR != RO_LR_TERMS) {      // (TERMS: behind the barrier below, once the next state exists)
          float rew;
          if (LR == RO_LR_LEARNED) {
            rew = learned_reward(A, s_y, ld_y, E, r, env0 + r, ((long long)s * AR + ar) * N + env0 + r, rng_seed, rng_off);
          } else if (A.reward_kind == MBPO_REWARD_PENDULUM) {
            rew = pendulum_reward(xr, xr[X], s_rp);
          } else {
            // (the quadratic reward, as k_model_rollout, k_reward_eval and k_rollout_lean write it: a shared function moved SGPR spills)
            const float *tp = s_rp, *qp = tp + X, *rp = qp + X;
            float cx = 0.f, cu = 0.f;
            for (int c = 0; c < X; ++c) { float dd = xr[c] - tp[c]; cx += qp[c] * (dd * dd); }
            for (int d = 0; d < RO_UE; ++d) { float uu = xr[X + d]; cu += rp[d] * (uu * uu); }
            rew = -cx - cu;
          }
          reward_accumulate<TA>(s_rew, RO64_HOLD, r, ar, TA ? hold_weight(hold_gamma<TA>(AA), ar) : 1.f, rew);
          }
          if (A.system_kind == MBPO_SYS_PENDULUM) {
            float xn[3];
            pendulum_step(xr, xr[X], A.sys_params, xn);
            if constexpr (TA) {
              if (!hold_live(RO64_HOLD, r, ar)) { xn[0] = xr[0]; xn[1] = xr[1]; xn[2] = xr[2]; }
            }
            s_scr[r * X + 0] = xn[0];
            s_scr[r * X + 1] = xn[1];
            s_scr[r * X + 2] = xn[2];
          }
        }
        if (A.system_kind != MBPO_SYS_PENDULUM) {
          for (int idx = tid; idx < 16 * X; idx += nthreads) {
            const int r = idx & 15, c = idx >> 4;
            const long long env = env0 + r;
            const float base = A.ens_predict_delta ? s_xu[r * ld_xu + c] : 0.f;
            float v;
            if (A.ens_mode == MBPO_ENS_MEAN) {
              float acc = 0.f;
              for (int e = 0; e < E; ++e) acc += s_y[(e * 16 + r) * ld_y + c];
              if constexpr (HAL) {
                // x' = base + m + beta * sd * eta, sd the population std of the members' means (two passes over the E tiles in s_y)
                const float m = acc / (float)E;
                float q = 0.f;
                for (int e = 0; e < E; ++e) { const float dm = s_y[(e * 16 + r) * ld_y + c] - m; q += dm * dm; }
                const float sd = sqrtf(q / (float)E);
                v = base + m + s_rp[X + U + c] * sd * s_xu[r * ld_xu + U + c];      // eta: action columns UE .. UE + X, X + UE == U
              } else {
                v = base + acc / (float)E;
              }
            } else {
              int mem = 0;
              const long long eidx = ((long long)s * AR + ar) * N + env;
              if (env < N) {
                if (A.ens_mode == MBPO_ENS_TSINF) mem = (int)(env % E);
                else mem = A.member_idx ? A.member_idx[eidx]
                                        : philox_randint(rng_seed, rng_off, MBPO_STREAM_MEMBER, (unsigned long long)eidx, 0, E);
              }
              const float mu = s_y[(mem * 16 + r) * ld_y + c];
              v = base + mu;
              if (A.ens_sample_noise && env < N) {
                const float sg = softplus_f(s_y[(mem * 16 + r) * ld_y + X + c]) + A.ens_min_std;
                const long long nidx = eidx * X + c;
                const float eps = A.model_noise ? A.model_noise[nidx]
                                                : philox_normal(rng_seed, rng_off, MBPO_STREAM_MODEL_NOISE, (unsigned long long)nidx);
                v += sg * eps;
              }
            }
            if constexpr (TA) {
              if (!hold_live(RO64_HOLD, r, ar)) v = s_xu[r * ld_xu + c];      // a row that is not held any more keeps its state
            }
            s_scr[r * X + c] = v;
          }
        }
        __syncthreads();
        if constexpr (LR == RO_LR_TERMS) {
          // the reward on this inner step's (x, u, x'): x and u still in s_xu, x' in the scratch.  In front of the hold's bookkeeping
          // (the same 16 threads, in program order): whether a row was live is asked before this step can stop it.
          if (tid < 16) {
            const int r = tid;
            const float *xr = s_xu + r * ld_xu;
            const float rew = reward_terms_eval(RO64_TAB, xr, xr + X, reward_terms_next(s_scr + r * X, xr, X), X, RO_UE);
            reward_accumulate<TA>(s_rew, RO64_HOLD, r, ar, TA ? hold_weight(hold_gamma<TA>(AA), ar) : 1.f, rew);
          }
        }
        if constexpr (TA) {
          // the rows that took this step: count it, and stop a row whose new state leaves the box (the next reader of either is behind
          // a barrier: the one below, or the one in front of section D)
          if (tid < 16 && hold_live(RO64_HOLD, tid, ar)) {
            RO64_HOLD[16 + tid] += 1.f;
            if (TERM && term_row_done(A, s_scr + tid * X, X) != 0.f) RO64_HOLD[32 + tid] = 1.f;
          }
        }
        if (ar + 1 < (TA ? hold_bound(RO64_HOLD) : AR)) {   // the next inner step starts from the new state
          if constexpr (LR == RO_LR_TERMS) __syncthreads();      // (the term reward above still reads the pre-step x in s_xu)
          for (int idx = tid; idx < 16 * X; idx += nthreads) {
            const int r = idx & 15, c = idx >> 4;
            s_xu[r * ld_xu + c] = s_scr[r * X + c];
          }
          __syncthreads();
        }
      }

      // TERM: the rows' SystemState.done, once per row by 16 threads (the 16 floats behind the log-prob scratch), read by section D
      float *s_sd = s_scr + 16 * (X + U);
      if constexpr (TA) {
        if (TERM && tid < 16) s_sd[tid] = RO64_HOLD[32 + tid];      // the rows that left the box inside their hold
        __syncthreads();      // ... and the rows' step counts are complete
      } else
      if (TERM) {
        if (tid < 16) s_sd[tid] = term_row_done(A, s_scr + tid * X, X);
        __syncthreads();
      }
      RO_STAMP(5);
      // ---- section D: EpisodeWrapper / AutoReset post-step (training.py:98-107, 126-137) + Transition (acting.py:46-55) ----
      for (int idx = tid; idx < 16 * X; idx += nthreads) {
        const int r = idx & 15, c = idx >> 4;
        const float st = steps_cur[r] + (TA ? RO64_HOLD[16 + r] : (float)AR);
        const bool dn = st >= (float)A.episode_length || (TERM && s_sd[r] != 0.f);
        const float v = dn ? s_first[r * ld_x + c] : s_scr[r * X + c];
        s_obs[r * ld_x + c] = v;
        s_row[r * D + X + U + 2 + c] = v;  // next_observation = nstate.obs (post auto-reset)
        if (START && dn && env0 + r < N)     // the reset consumed the start state: the row's next one (read at its next reset)
          s_first[r * ld_x + c] = A.start.rows[start_draw_row(A.start, sb_lo, sb_hi, sb_head, rng_seed, rng_off, (long long)s * N + env0 + r) + c];
      }
      if (tid < 16) {
        const int r = tid;
        const float st = steps_cur[r] + (TA ? RO64_HOLD[16 + r] : (float)AR);   // TA: the inner steps the row took
        const float sys_done = TERM ? s_sd[r] : 0.f;  // SystemState.done: 0 (base_systems.py:25) or the termination box
        const float dn = (st >= (float)A.episode_length) ? 1.f : sys_done;
        const float trunc = (st >= (float)A.episode_length) ? (1.f - sys_done) : 0.f;
        steps_nxt[r] = st;
        s_done[r] = dn;
        if constexpr (TA) s_row[r * D + X + U] = s_rew[r] - AA.hold.switch_cost;
        else
        s_row[r * D + X + U] = s_rew[r];
        s_row[r * D + X + U + 1] = 1.f - dn;
        s_row[r * D + D - 1] = trunc;
        if (A.ppo_extras) {
          float lp = 0.f;
          for (int d = 0; d < U; ++d) lp += s_scr[16 * X + r * U + d];
          s_row[r * D + 2 * X + U + 2] = lp;  // log_prob (summed over action dims)
        }
      }
      __syncthreads();
      RO_STAMP(6);
      // ---- write the tile's 16 rows (the next step's section A works on the other row buffer) ----
      if (A.env_major) {
        for (int r = wave; r < 16; r += RO64_WAVES) {
          const long long env = env0 + r;
          if (env < N)
            for (int c = lane; c < D; c += 64) A.transitions[(env * A.n_steps + s) * D + c] = s_row[r * D + c];
        }
      } else {
        const long long nvalid = (N - env0 < 16 ? N - env0 : 16) * D;
        float *dst = A.transitions + ((long long)s * N + env0) * D;
        for (int idx = tid; idx < nvalid; idx += nthreads) dst[idx] = s_row[idx];
      }
      RO_STAMP(7);
    }
    __syncthreads();
    // ---- write back env state ----
    {
      const int tid = ro_tid_now(wave);
      const float *steps_fin = s_steps + (A.n_steps & 1) * 16;
      for (int idx = tid; idx < 16 * X; idx += nthreads) {
        const int r = idx & 15, c = idx >> 4;
        const long long env = env0 + r;
        if (env < N) A.obs[env * X + c] = s_obs[r * ld_x + c];
        if (START && env < N) A.first_obs[env * X + c] = s_first[r * ld_x + c];
      }
      if (tid < 16) {
        const long long env = env0 + tid;
        if (env < N) {
          A.steps[env] = steps_fin[tid];
          A.done[env] = s_done[tid];
        }
      }
    }
    __syncthreads();
  }
}
