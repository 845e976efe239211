// rollout_wide_kernel.hpp — R1-R8 fused model rollout, hidden widths 128 and 256 (see include/mbpo_hip.h).  Included by the units that
// instantiate it (rollout_wide_*.hip), one per reward selector; the host reaches them through rollout_wide.hpp.
//
// Decomposition (MI355X): one workgroup owns a tile of 16 envs for ALL steps of the rollout and ALL ensemble
// members, because every step ends in a reduction over members (mean / member pick) that feeds the next step's
// input.  Each wave walks a whole (tile, network) chain (wave_mlp.hpp): wave 0 the policy, then waves 0..E-1 one
// ensemble member each, with two workgroup barriers per step instead of one per layer.  Activations live in LDS,
// weights stream from L2 (flat params are ~0.2 MB, shared by every workgroup), the transition row is assembled in
// LDS and written to HBM as one contiguous block per step.
// Per (env, step) HBM traffic is one row write (row_len*4 B) — the kernel is MFMA/latency bound by design.
#pragma once
#include "common.hpp"
#include "chain_run.hpp"
#include "rollout_wide.hpp"

// HAL: hallucinated control (halluc_beta is set; include/mbpo_hip.h "hallucinated control").  A flag of its own, like the others: the
// instantiations without it compile to what they were (profiles/r10_hallucinated_registers.txt).  The action is [u (UE) | eta (X)]:
// the member chains read the x + UE leading columns of s_xu (every input-layer routine masks k >= dims[0] itself, none relies on zero
// pad columns, so eta may sit where the padding was), the rewards read the UE control columns, the combine section reads eta.
// Only the HAL instantiations take the argument block that carries beta (RolloutArgsHal): every other one keeps the kernel-argument
// type it had, and RolloutArgs — which k_rollout_lean embeds — its layout.
struct RolloutArgsHal : RolloutArgs {
  const float *halluc_beta;     // [x_dim]
};
// TA: the argument block of the time-adaptive instantiations (HoldArgs: rollout_tile.hpp)
struct RolloutArgsTA : RolloutArgs {
  HoldArgs hold;
};
template <bool HAL, bool TA = false>
using RolloutArgsFor = typename std::conditional<TA, RolloutArgsTA, typename std::conditional<HAL, RolloutArgsHal, RolloutArgs>::type>::type;

template <int H, int LR, bool START, bool HAL, bool TA = false>
__global__ void __launch_bounds__(512) k_model_rollout(RolloutArgsFor<HAL, TA> A) {
  extern __shared__ __align__(16) float smem[];
  constexpr int HT = H / 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x;
  const int X = A.x_dim, U = A.u_dim, D = A.row_len;
  const int E = (A.system_kind == MBPO_SYS_ENSEMBLE) ? A.dyn.n_nets : 0;
  const long long N = A.n_envs;
  const int AR = A.action_repeat;

  // ---- LDS carve (floats) ----
  float *s_obs = smem;                           // [16][ld_x]  current raw obs
  float *s_first = s_obs + 16 * A.ld_x;          // [16][ld_x]
  float *s_pin = s_first + 16 * A.ld_x;          // [16][ld_x]  normalised obs (policy input)
  float *s_xu = s_pin + 16 * A.ld_x;             // [16][ld_xu] dynamics input [x,u]
  const int T = 16 * A.ld_h;
  float *s_pp = s_xu + 16 * A.ld_xu;             // [n_chains][2] hidden tiles (ping-pong per chain)
  float *s_hA = s_pp;                            // also scratch between chains
  float *s_y = s_pp + A.n_chains * 2 * T;        // [n_out][16][ld_y]
  float *s_row = s_y + A.n_out * 16 * A.ld_y;    // [16][D4]
  float *s_steps = s_row + 16 * ((D + 3) & ~3);  // [16]
  float *s_done = s_steps + 16;                  // [16]
  float *s_rew = s_done + 16;                    // [16]
  // HAL: beta staged once per workgroup, [X] floats behind s_rew (the host sizes this region for k_model_rollout64's second row
  // buffer; the tile load's barrier below orders it before its first use)
  if constexpr (HAL)
    for (int idx = tid; idx < X; idx += nthreads) s_rew[16 + idx] = A.halluc_beta[idx];
  float *const s_hold = s_rew + 16;              // TA: [49] floats of the same region (never together with HAL)
  (void)s_hold;
  // TERMS: the table staged once per workgroup behind beta / the hold state (the tile load's barrier below orders it before its first use)
  if constexpr (LR == RO_LR_TERMS)
    for (int idx = tid; idx < MBPO_REWARD_TERMS_FLOATS; idx += nthreads) s_rew[16 + ((X + 3) & ~3) + 64 + idx] = A.reward_params[idx];

  const RngKey rk_ = rng_resolve(A.seed, A.offset, A.rng_dev);
  const unsigned long long rng_off = rk_.offset, rng_seed = rk_.seed;
  // START: the true buffer's {sample_position, insert_position, head}
  const int sb_lo = START ? A.start.state[1] : 0, sb_hi = START ? A.start.state[0] : 0, sb_head = START ? A.start.state[2] : 0;
  const long long n_tiles = (N + 15) >> 4;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long env0 = tile * 16;
    // ---- load env state ----
    for (int idx = tid; idx < 16 * X; idx += nthreads) {
      int r = idx / X, c = idx - r * X;
      long long env = env0 + r;
      float o = 0.f, f = 0.f;
      if (env < N) {
        o = A.obs[env * X + c];
        f = A.first_obs[env * X + c];
      }
      s_obs[r * A.ld_x + c] = o;
      s_first[r * A.ld_x + c] = f;
    }
    if (tid < 16) {
      long long env = env0 + tid;
      s_steps[tid] = env < N ? A.steps[env] : 0.f;
      s_done[tid] = env < N ? A.done[env] : 0.f;
    }
    __syncthreads();

    for (int s = 0; s < A.n_steps; ++s) {
      if (A.actions) {
        // open-loop actions (rollout_actions, optimizer_utils.py:26-38): no policy
        for (int idx = tid; idx < 16 * U; idx += nthreads) {
          int r = idx / U, d = idx - r * U;
          long long env = env0 + r;
          float a = env < N ? A.actions[((long long)s * N + env) * U + d] : 0.f;
          s_xu[r * A.ld_xu + X + d] = a;
          s_row[r * D + X + d] = a;
        }
      } else {
      // ---- policy input: running_statistics.normalize = (obs - mean) / std ----
      for (int idx = tid; idx < 16 * X; idx += nthreads) {
        int r = idx / X, c = idx - r * X;
        float o = s_obs[r * A.ld_x + c];
        s_pin[r * A.ld_x + c] = A.norm_mean ? (o - A.norm_mean[c]) / A.norm_std[c] : o;
      }
      __syncthreads();
      // ---- policy MLP -> logits in s_y[0]: waves 0..3 share the chain (column slices), one barrier per layer ----
      {
        FwdChain fc{&A.policy, A.policy.params, s_pin, A.ld_x, s_pp, s_pp + T, nullptr, nullptr, s_y};
        for (int l = 0; l < A.policy.n_layers; ++l) {
          if (wave < 4) group_fwd_step<HT, 4>(fc, l, A.ld_h, A.ld_y, wave, lane);
          __syncthreads();
        }
      }
      // ---- NormalTanh sample (parametric_distribution.py:97-124) + AutoReset pre-step (training.py:119-124) ----
      for (int idx = tid; idx < 16 * U; idx += nthreads) {
        int r = idx / U, d = idx - r * U;
        long long env = env0 + r;
        float loc = s_y[r * A.ld_y + d], raw = s_y[r * A.ld_y + U + d];
        float sigma = softplus_f(raw) + 0.001f;
        float eps = 0.f;
        if (!A.deterministic && env < N) {
          long long nidx = ((long long)s * N + env) * U + d;
          eps = A.policy_noise ? A.policy_noise[nidx]
                               : philox_normal(rng_seed, rng_off, MBPO_STREAM_POLICY_NOISE, (unsigned long long)nidx);
        }
        float z = loc + sigma * eps;
        float a = tanhf(z);
        if (A.action_clip > 0.f) a = fminf(fmaxf(a, -A.action_clip), A.action_clip);
        s_xu[r * A.ld_xu + X + d] = a;
        s_row[r * D + X + d] = a;
        if (A.ppo_extras) {
          // log N(z; loc, sigma) - log|d tanh/dz|, per action dim; summed below
          float lp = -0.5f * eps * eps - logf(sigma) - 0.91893853320467274178f;
          float ldj = 2.0f * (0.69314718055994530942f - z - softplus_f(-2.0f * z));
          s_row[r * D + 2 * X + U + 2 + 1 + d] = z;               // raw_action
          s_hA[r * U + d] = lp - ldj;                             // scratch: per-dim log-prob
        }
      }
      }
      for (int idx = tid; idx < 16 * X; idx += nthreads) {
        int r = idx / X, c = idx - r * X;
        float o = s_obs[r * A.ld_x + c];
        s_xu[r * A.ld_xu + c] = o;
        s_row[r * D + c] = o;  // Transition.observation = env_state.obs (acting.py:47)
      }
      if (tid < 16) {
        // AutoReset: steps <- 0 where previously done; done <- 0
        if (s_done[tid] != 0.f) s_steps[tid] = 0.f;
        s_done[tid] = 0.f;
        s_rew[tid] = 0.f;
      }
      __syncthreads();
      if (A.ppo_extras && tid < 16) {
        float lp = 0.f;
        for (int d = 0; d < U; ++d) lp += s_hA[tid * U + d];
        s_row[tid * D + 2 * X + U + 2] = lp;  // log_prob (summed over action dims)
      }
      if (A.ppo_extras) __syncthreads();
      float hold_w = 1.f;                        // TA: w_j
      if constexpr (TA) {
        hold_setup(A.hold, s_hold, s_xu, A.ld_xu, X + U - 1, env0, N, wave, lane);
        __syncthreads();
      }
      const int ARN = TA ? (int)s_hold[48] : AR; // TA: the tile's largest k (workgroup-uniform)

      // ---- EpisodeWrapper inner scan over action_repeat (training.py:91-97) ----
      for (int ar = 0; ar < ARN; ++ar) {
        if (A.system_kind == MBPO_SYS_ENSEMBLE) {
          // one wave per ensemble member chain (no barrier inside a chain), n_chains members side by side
          for (int e0 = 0; e0 < E; e0 += A.n_chains) {
            const int e = e0 + wave;
            if (wave < A.n_chains && e < E)
              wave_mlp_fwd<HT>(A.dyn, A.dyn.params + (long long)e * A.dyn.net_stride, s_xu, A.ld_xu, s_pp + wave * 2 * T,
                               s_pp + wave * 2 * T + T, nullptr, nullptr, A.ld_h, s_y + e * 16 * A.ld_y, A.ld_y, lane);
          }
          __syncthreads();
        }
        // reward uses the pre-step x and the action; next state from the system
        if (LR != RO_LR_TERMS && tid < 16) {
          const int r = tid;
          const float *xr = s_xu + r * A.ld_xu;
          float rew;
          if (LR == RO_LR_LEARNED) {
            rew = learned_reward(A, s_y, A.ld_y, E, r, env0 + r, ((long long)s * AR + ar) * N + env0 + r, rng_seed, rng_off);
          } else if (A.reward_kind == MBPO_REWARD_PENDULUM) {
            rew = pendulum_reward(xr, xr[X], A.reward_params);
          } else {
            // (the quadratic reward, as k_model_rollout64, k_reward_eval and k_rollout_lean write it: a shared function moved SGPR spills)
            const float *tp = A.reward_params, *qp = tp + X, *rp = qp + X;
            float cx = 0.f, cu = 0.f;
            for (int c = 0; c < X; ++c) { float dd = xr[c] - tp[c]; cx += qp[c] * (dd * dd); }
            for (int d = 0; d < RO_UE; ++d) { float uu = xr[X + d]; cu += rp[d] * (uu * uu); }
            rew = -cx - cu;
          }
          reward_accumulate<TA>(s_rew, s_hold, r, ar, hold_w, rew);
        }
        __syncthreads();
        if (A.system_kind == MBPO_SYS_PENDULUM) {
          if (tid < 16 && (!TA || hold_live(s_hold, tid, ar))) {
            float xn[3];
            pendulum_step(s_xu + tid * A.ld_xu, s_xu[tid * A.ld_xu + X], A.sys_params, xn);
            s_xu[tid * A.ld_xu + 0] = xn[0];
            s_xu[tid * A.ld_xu + 1] = xn[1];
            s_xu[tid * A.ld_xu + 2] = xn[2];
          }
        } else {
          for (int idx = tid; idx < 16 * X; idx += nthreads) {
            int r = idx / X, c = idx - r * X;
            long long env = env0 + r;
            float base = A.ens_predict_delta ? s_xu[r * A.ld_xu + c] : 0.f;
            float v;
            if (A.ens_mode == MBPO_ENS_MEAN) {
              float acc = 0.f;
              for (int e = 0; e < E; ++e) acc += s_y[(e * 16 + r) * A.ld_y + c];
              if constexpr (HAL) {
                // x' = base + m + beta * sd * eta, sd the population std of the members' means (two passes over the E tiles in s_y)
                const float m = acc / (float)E;
                float q = 0.f;
                for (int e = 0; e < E; ++e) { const float dm = s_y[(e * 16 + r) * A.ld_y + c] - m; q += dm * dm; }
                const float sd = sqrtf(q / (float)E);
                v = base + m + s_rew[16 + c] * sd * s_xu[r * A.ld_xu + U + c];      // eta: action columns UE .. UE + X, X + UE == U
              } else {
                v = base + acc / (float)E;
              }
            } else {
              int mem = 0;
              long long eidx = ((long long)s * AR + ar) * N + env;
              if (env < N) {
                if (A.ens_mode == MBPO_ENS_TSINF) mem = (int)(env % E);
                else mem = A.member_idx ? A.member_idx[eidx]
                                        : philox_randint(rng_seed, rng_off, MBPO_STREAM_MEMBER, (unsigned long long)eidx, 0, E);
              }
              float mu = s_y[(mem * 16 + r) * A.ld_y + c];
              v = base + mu;
              if (A.ens_sample_noise && env < N) {
                float sg = softplus_f(s_y[(mem * 16 + r) * A.ld_y + X + c]) + A.ens_min_std;
                long long nidx = eidx * X + c;
                float eps = A.model_noise ? A.model_noise[nidx]
                                          : philox_normal(rng_seed, rng_off, MBPO_STREAM_MODEL_NOISE, (unsigned long long)nidx);
                v += sg * eps;
              }
            }
            s_hA[r * X + c] = v;  // scratch (s_y must stay intact until every thread has read it)
          }
          __syncthreads();
          if constexpr (LR == RO_LR_TERMS) {
            // the reward on this inner step's (x, u, x'): x and u still in s_xu, x' in the scratch; the copy below waits for it
            if (tid < 16) {
              const int r = tid;
              const float *xr = s_xu + r * A.ld_xu;
              const float rew = reward_terms_eval(s_rew + 16 + ((X + 3) & ~3) + 64, xr, xr + X, reward_terms_next(s_hA + r * X, xr, X), X, RO_UE);
              reward_accumulate<TA>(s_rew, s_hold, r, ar, hold_w, rew);
            }
            __syncthreads();
          }
          for (int idx = tid; idx < 16 * X; idx += nthreads) {
            int r = idx / X, c = idx - r * X;
            if (!TA || hold_live(s_hold, r, ar)) s_xu[r * A.ld_xu + c] = s_hA[r * X + c];
          }
        }
        __syncthreads();
        if constexpr (TA) {
          // the rows that took this step: count it, and stop a row whose new state leaves the box
          if (tid < 16 && hold_live(s_hold, tid, ar)) {
            s_hold[16 + tid] += 1.f;
            if (term_row_done(A, s_xu + tid * A.ld_xu, X) != 0.f) s_hold[32 + tid] = 1.f;
          }
          hold_w *= A.hold.gamma;
          __syncthreads();
        }
      }

      // ---- EpisodeWrapper / AutoReset post-step (training.py:98-107, 126-137) + Transition (acting.py:46-55) ----
      if (tid < 16) {
        const int r = tid;
        float st = s_steps[r] + (TA ? s_hold[16 + r] : (float)AR);   // TA: the inner steps the row took
        // SystemState.done: 0 (base_systems.py:25) or the termination box (TA: on any inner step the row took)
        float sys_done = TA ? s_hold[32 + r] : term_row_done(A, s_xu + r * A.ld_xu, X);
        float dn = (st >= (float)A.episode_length) ? 1.f : sys_done;
        float trunc = (st >= (float)A.episode_length) ? (1.f - sys_done) : 0.f;
        s_steps[r] = st;
        s_done[r] = dn;
        if constexpr (TA) s_row[r * D + X + U] = s_rew[r] - A.hold.switch_cost;
        else
        s_row[r * D + X + U] = s_rew[r];
        s_row[r * D + X + U + 1] = 1.f - dn;
        s_row[r * D + D - 1] = trunc;
      }
      __syncthreads();
      for (int idx = tid; idx < 16 * X; idx += nthreads) {
        int r = idx / X, c = idx - r * X;
        float v = (s_done[r] != 0.f) ? s_first[r * A.ld_x + c] : s_xu[r * A.ld_xu + c];
        s_obs[r * A.ld_x + c] = v;
        s_row[r * D + X + U + 2 + c] = v;  // next_observation = nstate.obs (post auto-reset)
        if (START && s_done[r] != 0.f && env0 + r < N)      // the reset consumed the start state: the row's next one
          s_first[r * A.ld_x + c] = A.start.rows[start_draw_row(A.start, sb_lo, sb_hi, sb_head, rng_seed, rng_off, (long long)s * N + env0 + r) + c];
      }
      __syncthreads();
      // ---- write the tile's 16 rows ----
      for (int idx = tid; idx < 16 * D; idx += nthreads) {
        int r = idx / D, c = idx - r * D;
        long long env = env0 + r;
        if (env < N) {
          long long row = A.env_major ? (env * A.n_steps + s) : ((long long)s * N + env);
          A.transitions[row * D + c] = s_row[idx];
        }
      }
      __syncthreads();
    }

    // ---- write back env state ----
    for (int idx = tid; idx < 16 * X; idx += nthreads) {
      int r = idx / X, c = idx - r * X;
      long long env = env0 + r;
      if (env < N) A.obs[env * X + c] = s_obs[r * A.ld_x + c];
      if (START && env < N) A.first_obs[env * X + c] = s_first[r * A.ld_x + c];
    }
    if (tid < 16) {
      long long env = env0 + tid;
      if (env < N) {
        A.steps[env] = s_steps[tid];
        A.done[env] = s_done[tid];
      }
    }
    __syncthreads();
  }
}

// The launch of one reward selector's instantiations: H, START, HAL and TA become template arguments here.  TA with HAL has no
// instantiation (the host refuses it first; the guard keeps the nest from creating one).
template <int LR>
static int rollout_wide_launch_lr(int H, const RolloutFlags &f, const RolloutArgs &A, const float *halluc_beta, const HoldArgs *hold, int grid,
                                  int block, size_t lds, hipStream_t st) {
  return mbpo_with_bool(H == 256, [&](auto H256) {
    return mbpo_with_bool(f.start, [&](auto SB) {
      return mbpo_with_bool(f.hal, [&](auto HL) {
        return mbpo_with_bool(f.ta, [&](auto TA) {
          if constexpr (TA.value && HL.value) {
            return rollout_refuse_ta(true);
          } else {
            RolloutArgsFor<HL.value, TA.value> AH;
            static_cast<RolloutArgs &>(AH) = A;
            if constexpr (HL.value) AH.halluc_beta = halluc_beta;
            if constexpr (TA.value) AH.hold = *hold;
            rollout_note_kernel({RO_FAMILY_WIDE, H256.value ? 256 : 128, 0, 0, 0, LR, 0, f.term, SB.value, HL.value, TA.value});
            return mbpo_launch<k_model_rollout<H256.value ? 256 : 128, LR, SB.value, HL.value, TA.value>>(grid, block, lds, st, "model_rollout", AH);
          }
        });
      });
    });
  });
}
