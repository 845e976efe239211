/*
 * mbpo_hip.h — C-ABI of libmbpo_hip.so, the MI355X (gfx950) implementation of the
 * MBPO inner-loop hot path of lasgroup/Model-based-policy-optimizers.
 *
 * The reference has no FFI: its hot path is jax.numpy traced under jit/scan/vmap.  Each
 * entry point below replaces one traced computation; the "replaces" line cites the
 * reference file:line (relative to the reference repo root) whose arithmetic it computes.
 *
 * Conventions (all entry points):
 *   - plain pointers + sizes; every pointer is a DEVICE pointer unless named h_*;
 *   - the caller owns all memory; no entry point allocates, frees or synchronises;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - return value: MBPO_OK (0) or a negative MBPO_ERR_*; mbpo_last_error() gives text;
 *   - all floating point is IEEE fp32 (the reference's dtype: sac/sac.py:379,389);
 *     indices and positions are int32/int64 and bit-exact.
 *   - a `workspace` is caller-owned scratch of the stated size: unless its entry point says otherwise its content on entry does not
 *     matter (every word that is read was written earlier in the same call), it carries nothing from one call to the next, may be
 *     shared by calls that do not overlap in time, and nothing is written past the stated size.  INTEGRATION.md, "Scratch
 *     contract", lists every buffer of these entry points: outputs are overwritten in full (no element has to be zeroed first),
 *     while state, running sums and in/out buffers are read before they are written and must hold their documented initial values.
 *
 * Parameter layout of an MLP ("flat params"): for layer l = 0..n_layers-1
 *   W_l[dims[l]][dims[l+1]] row-major (flax Dense kernel layout [in,out]), then b_l[dims[l+1]].
 * n_nets networks of identical shape sit net_stride floats apart (ensemble members, twin critics).
 */
#ifndef MBPO_HIP_H
#define MBPO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MBPO_OK 0
#define MBPO_ERR_ARG (-1)         /* invalid argument / shape */
#define MBPO_ERR_UNSUPPORTED (-2) /* valid but outside what the kernels are built for */
#define MBPO_ERR_LAUNCH (-3)      /* HIP runtime error at launch */

#define MBPO_MAX_LAYERS 8

/* activation ids (reference default: flax.linen.swish — sac/sac.py:86-88, utils/network_utils.py:8) */
#define MBPO_ACT_SWISH 0
#define MBPO_ACT_RELU 1
#define MBPO_ACT_TANH 2

typedef struct mbpo_mlp_desc {
  const float *params;               /* flat params of net 0 */
  int64_t net_stride;                /* floats between consecutive nets */
  int32_t n_nets;                    /* >= 1 (ensemble members / critics) */
  int32_t n_layers;                  /* Dense layers incl. the output layer, 1..MBPO_MAX_LAYERS */
  int32_t dims[MBPO_MAX_LAYERS + 1]; /* dims[0] = input size, dims[n_layers] = output size */
  int32_t activation;                /* MBPO_ACT_*; applied after every layer except the last */
} mbpo_mlp_desc;

/* ---- library ---- */
int mbpo_version(void);
const char *mbpo_last_error(void);

/* ---- randomness ---------------------------------------------------------------------------------
 * The reference threads jax.random keys through every call and splits them (sac/sac.py:289,309-311; ppo/ppo.py:190-193).
 * JAX's threefry streams cannot be reproduced without JAX, so every drawing entry point here is keyed by
 * (seed, offset, stream id, element index) -> Philox4x32-10 (csrc/common.hpp; stream ids are fixed per consumer).
 * `rng_dev` (optional, device uint64[2] = {seed word, step counter}) is ADDED to the host-side (seed, offset):
 *   seed_eff = seed + rng_dev[0],   offset_eff = offset + rng_dev[1].
 * A training step captured into a hipGraph bakes its host-side seed/offset constants; everything that changes from step
 * to step lives in the two device words, so a replayed graph draws bit for bit what the eagerly issued step draws.
 * Convention used by the trainers: offset = (call-site id << 32), rng_dev = {epoch key, training-step index}.
 * mbpo_rng_advance: rng_dev[1] += inc (one tiny launch, graph-capturable). */
int mbpo_rng_advance(uint64_t *rng_dev, uint64_t inc, void *stream);
/* out[i] = standard normal of element (elem_base + i) of `stream` (1 = policy noise ... 10 = iCEM; csrc/common.hpp) under
 * (seed + rng_dev[0], offset + rng_dev[1]) — exactly the number a fused kernel draws for that element.  For host-side horizon
 * loops around a user-defined System (BPTT: the noise of jr.normal in act(), bptt_optimizer.py:305-325). */
int mbpo_philox_normal_fill(uint64_t seed, uint64_t offset, const uint64_t *rng_dev, uint32_t stream, uint64_t elem_base, int64_t n,
                            float *out, void *stream_);
/* out[i] = uniform integer in [lo, hi) of element (elem_base + i) of `stream`, keyed as above — exactly philox_randint on the device
 * (e.g. the MEMBER stream's draws of trajectory sampling, for the host-side BPTT horizon loop). */
int mbpo_philox_randint_fill(uint64_t seed, uint64_t offset, const uint64_t *rng_dev, uint32_t stream, uint64_t elem_base, int64_t n,
                             int32_t lo, int32_t hi, int32_t *out, void *stream_);

/* out[(s * n_problems + b) * group + j] = element (s * group + j) of `stream` under (seeds[b], offset), s < n_steps, j < group:
 * standard normals (as_int = 0, out float) or uniform integers in [lo, hi) (as_int = 1, out int32).  Problem b's numbers are the
 * ones a fused kernel draws for a rollout of its own `group`-element steps with seed = seeds[b]; the layout is that of one rollout
 * over all problems' envs.  seeds: device uint64[n_problems].  For the batched iCEM path (icem_optimizer.py:168-175 per problem):
 * member_idx [H][B NC P] (group = NC P, MEMBER stream) and model_noise [H][B NC P][x] (group = NC P x, MODEL_NOISE stream). */
int mbpo_philox_fill_grouped(const uint64_t *seeds, uint64_t offset, uint32_t stream, int32_t n_steps, int32_t n_problems, int64_t group,
                             int32_t as_int, int32_t lo, int32_t hi, void *out, void *stream_);

/* ---- R2: ensemble MLP forward -------------------------------------------------------------
 * replaces: the (new) learned Dynamics.next_state evaluated under vmap —
 *           mbpo/systems/dynamics/base_dynamics.py:15-20 called from
 *           mbpo/systems/pendulum_system.py:31-32 / brax_utils/training.py:71-74;
 *           MLP semantics: sac/networks.py:19-41, utils/network_utils.py:5-17.
 * x: [n_rows, dims[0]] if shared_input else [n_nets, n_rows, dims[0]];  y: [n_nets, n_rows, dims[n_layers]].
 */
int mbpo_ensemble_mlp_forward(const mbpo_mlp_desc *mlp, const float *x, int32_t shared_input,
                              float *y, int64_t n_rows, void *stream);

/* ---- R1-R8: fused model rollout -----------------------------------------------------------
 * replaces: SAC.get_experience's scan of acting.actor_step (sac/sac.py:283-296, sac/acting.py:35-55)
 *           and brax generate_unroll as used by PPO.training_step (ppo/ppo.py:194-208), i.e. per env and step:
 *           policy inference (sac_networks.py:58-73 / ppo_network.py:59-84, NormalTanh:
 *           sac/parametric_distribution.py:66-124), AutoReset/Episode bookkeeping
 *           (brax_utils/training.py:77-137), BraxWrapper.step -> System.step
 *           (systems/brax_wrapper.py:40-50, pendulum_system.py:18-39), Transition assembly.
 */
#define MBPO_SYS_PENDULUM 0 /* analytic PendulumDynamics (dynamics/pendulum_dynamics.py:29-63) */
#define MBPO_SYS_ENSEMBLE 1 /* learned ensemble MLP behind Dynamics.next_state */

#define MBPO_ENS_MEAN 0  /* x' = E_members[mean_e]  (what System.step consumes: .mean()) */
#define MBPO_ENS_TS1 1   /* member drawn per (env, step) — MBPO-style trajectory sampling */
#define MBPO_ENS_TSINF 2 /* env i bound to member i % E */

#define MBPO_REWARD_PENDULUM 0  /* rewards/pendulum_reward.py:27-42; params [angle_cost, control_cost, target_angle] */
#define MBPO_REWARD_QUADRATIC 1 /* -(sum q_d (x_d - t_d)^2) - sum r_d u_d^2; params [t[x], q[x], r[u]] */
/* Learned reward: the ensemble predicts it.  Needs MBPO_SYS_ENSEMBLE with member output [mu_x (x) | raw_x (x) | mu_r | raw_r]
 * (dout = 2x + 2; every state column keeps its offset).  The reward is the head at the pre-step (x, u), like the analytic rewards:
 *   MBPO_ENS_MEAN : r = mean_e mu_r,e
 *   TS1 / TSINF   : r = mu_r,m with m the member the state takes at that (env, step) (same member_idx entry / Philox MEMBER draw)
 * summed over action_repeat.  ens_sample_noise perturbs the state only: the reward carries no noise (raw_r is trained by
 * mbpo_ens_nll_grads and reported as the reward's std by the host API, never read by a rollout).  reward_params may be NULL.
 * The analytic rewards accept a 2x + 2 ensemble too and ignore its reward head. */
#define MBPO_REWARD_LEARNED 2
/* Term rewards (a known closed-form reward written as data.  Not in the reference tree; build-defined: THIS TEXT IS THE DEFINITION).
 * Needs MBPO_SYS_ENSEMBLE.  With UE the control width the dynamics see (u_dim, less x_dim with halluc_beta, less 1 with hold_max_steps:
 * eta and tau never enter a reward) and x' the next state the step produced (the members' mean, the drawn member plus its noise, or
 * the hallucinated state; before termination and auto-reset):
 *   z   = [x (x_dim) | u (UE) | x_next (x_dim)],   x_next = x' if every component of x' is finite, else x (the pre-step state)
 *   s_g = sum_{k in group g} c_k * f_k(z[i_k] - t_k)         k ascending from the group's first term, one accumulator from 0
 *   r   = bias + sum_g w_g * L_g(s_g)                        g ascending, one accumulator from bias
 * every product and every sum rounded to fp32 on its own (no fused multiply-add), with the accurate cosf / sinf / expf / tanhf / sqrtf.
 *   f: 0 identity v, 1 square v * v, 2 abs |v|, 3 relu max(v, 0), 4 cos, 5 sin             (MBPO_TERM_FN_*)
 *   L: 0 identity s, 1 sqrt(max(s, 0)), 2 exp, 3 tanh                                      (MBPO_TERM_LINK_*)
 * No product of two different columns exists.  reward_params is a table of MBPO_REWARD_TERMS_FLOATS fp32 values, always of its full
 * length, small integers stored as exact floats:
 *   [0, 4)                          header  [n_groups, n_terms, bias, 0]
 *   [4, 4 + 4 * MAX_GROUPS)         group g [w, link, first_term, n_terms]
 *   [4 + 4 * MAX_GROUPS, FLOATS)    term k  [z_index, fn, c, t]
 * The kernels clamp n_groups to [0, MAX_GROUPS], the header's n_terms to [0, MAX_TERMS], a group's first_term to [0, n_terms] and its
 * count to [0, n_terms - first_term]; a term whose z_index lies outside [0, 2 * x_dim + UE) or whose fn is unknown contributes 0, and so
 * does a group whose link is unknown: whatever the vector holds, no read leaves it or the row.  The reward of an inner step
 * (action_repeat, or a time-adaptive hold) is formed from that inner step's (x_j, u, x_{j+1}) and accumulated as the other kinds are.
 * The non-finite rule keeps the reward of a diverged (then terminal) row finite.  The tile kernels (64 / 128 / 256 wide) run it; the
 * kernel specialised for the benchmark networks never takes it.  mbpo_bptt_actor_grads (MBPO_SYS_ENSEMBLE) takes tables whose terms
 * all read x or u (z_index < x_dim + u_dim): d r / d z_c = sum_g w_g L_g'(s_g) sum_{k in g: i_k = c} c_k f_k'(z_c - t_k), abs and relu
 * with gradient 0 at 0 (torch's), the sqrt link with gradient 0 at s <= 0.  The gradient through next-state terms is not built: there
 * a next-state column reads x and takes no gradient, and the host API (BPTTOptimizer) refuses such a table before any launch. */
#define MBPO_REWARD_TERMS 3
#define MBPO_REWARD_TERMS_MAX_GROUPS 16
#define MBPO_REWARD_TERMS_MAX_TERMS 128
#define MBPO_REWARD_TERMS_FLOATS (4 + 4 * MBPO_REWARD_TERMS_MAX_GROUPS + 4 * MBPO_REWARD_TERMS_MAX_TERMS)
#define MBPO_TERM_FN_IDENTITY 0
#define MBPO_TERM_FN_SQUARE 1
#define MBPO_TERM_FN_ABS 2
#define MBPO_TERM_FN_RELU 3
#define MBPO_TERM_FN_COS 4
#define MBPO_TERM_FN_SIN 5
#define MBPO_TERM_LINK_IDENTITY 0
#define MBPO_TERM_LINK_SQRT 1
#define MBPO_TERM_LINK_EXP 2
#define MBPO_TERM_LINK_TANH 3

/* Termination (SystemState.done of the fused systems, base_systems.py:25; MBPO's termination functions): a box on the step's
 * pre-auto-reset next state x', term_low / term_high [x_dim] (unbounded dimensions carry -inf / +inf; the bounds are closed):
 *   violated_d = !(low_d <= x'_d && x'_d <= high_d) || isinf(x'_d)        (NaN fails the compares, so it is violated)
 *   sys_done   = any_d violated_d ? 1 : 0
 *   over = steps >= episode_length;  done = over ? 1 : sys_done;  truncation = over ? 1 - sys_done : 0
 *   obs <- first_obs where done;  discount = 1 - done;  next_observation = the post-reset obs
 * (EpisodeWrapper / AutoReset, brax_utils/training.py:98-107, 126-137, given a System that reports done.)  Both system kinds, every
 * ensemble mode and reward kind, with a policy or open-loop `actions`.  With action_repeat > 1 sys_done comes from the LAST inner
 * step: the inner steps keep stepping and the reward is summed over all of them.  The reward is unchanged (evaluated at the
 * pre-step (x, u)).  With a termination set a non-finite next state is done = 1 and a reset to first_obs: it never reaches
 * next_observation or the carried obs.  Without one (both pointers NULL) sys_done = 0 and every kernel runs as before.
 *
 * Fresh starts (MBPO's branched rollouts: every round of k-step model rollouts starts from a new batch of real states.  Not in the
 * reference tree, whose AutoReset returns to the same first_obs every time — restated from the MBPO paper's procedure as remembered,
 * unverified against its code).  first_obs[env] is the state the env's next reset goes to.  With a start buffer set (start_rows,
 * start_max_size, start_row_len, start_state: a ring of mbpo_replay_insert, normally the true buffer, with its device state
 * {insert_position, sample_position, head, ...}), when env's step s of this launch ends with done = 1:
 *   the reset uses the current first_obs[env], exactly as above;  immediately after it
 *   idx = randint(sample_position, insert_position) from Philox(seed_eff, offset_eff, stream START = 11, element s * n_envs + env)
 *   first_obs[env] <- start_logical[wrap(idx)][0 .. x_dim)     (a bit copy through the ring's head, as mbpo_replay_gather reads it)
 * The draw shares the launch's (seed, offset, rng_dev) and, having a stream id of its own, collides with no other consumer.  An empty
 * range (insert_position == sample_position) yields idx = sample_position, as mbpo_replay_sample does.  One draw per env step
 * whatever action_repeat is.  The updated first_obs is written back at the end of the launch (the field is in/out with a start
 * buffer, read-only without), so across launches and hipGraph replays an env walks one chain of start states.  Everything else
 * about the row — discount, truncation, next_observation = the post-reset obs, the termination rules, the reward — is unchanged.
 * Both system kinds, every ensemble mode and reward kind, with or without a termination box, with a policy or open-loop `actions`.
 * All four start_* fields zero (a zero-initialised descriptor): off, every kernel runs what it ran before.  MBPO_ERR_ARG, checked
 * before any device use: rows without state or state without rows, start_row_len < x_dim, start_max_size outside (0, 2^31 - 1).
 *
 * Hallucinated control (optimistic exploration in the style of H-UCRL: the policy also picks the next state inside the ensemble's
 * epistemic confidence set.  Not in the reference tree; build-defined).  A rollout is hallucinated when halluc_beta ([x_dim], device)
 * is non-NULL.  Then:
 *   action width   u_dim stays the width the policy emits, the rows carry and SAC's critics see: A = u_env + x_dim.  An action is
 *                  [u (u_env) | eta (x_dim)], both parts whatever the policy or the open-loop `actions` give; the kernel adds no clip
 *                  of its own beyond action_clip.
 *   dynamics input the dynamics read [x, u] only: dynamics.dims[0] == x_dim + u_env == u_dim.
 *   next state     with mu_e,c member e's mean head at (x, u):
 *                    m_c  = (sum_e mu_e,c) / E           e ascending: the MBPO_ENS_MEAN sum, unchanged
 *                    q_c  = sum_e (mu_e,c - m_c)^2       e ascending
 *                    sd_c = sqrtf(q_c / E)               population std (EnsembleDynamics.next_state's var(unbiased=False))
 *                    x'_c = base_c + m_c + beta_c * sd_c * eta_c          base = x when ens_predict_delta
 *   action_repeat  > 1: eta is held and sd is recomputed at every inner step.
 *   elites         the members are the elites (the kernels see E = n_elites).
 *   member outputs x_dim (mean only) is accepted, like 2x and 2x + 2.
 *   reward         evaluated at the pre-step (x, u); eta never enters it.  Pendulum reward: x_dim == 3 && u_env == 1.  Quadratic
 *                  reward: params stay [t[x], q[x], r[u_env]], the control cost runs over the u_env columns.  Learned reward: the
 *                  mean over members of the reward head, as in MBPO_ENS_MEAN.
 *   unchanged      termination (the box on x'), resets, fresh starts, ppo_extras (log_prob summed over all A dims), env_major, the
 *                  normaliser, the Philox streams, the row layout (at action width A).
 * MBPO_ERR_ARG, checked before any device use, when halluc_beta is set with system_kind != MBPO_SYS_ENSEMBLE, ens_mode !=
 * MBPO_ENS_MEAN, u_dim <= x_dim, or a dynamics input width other than u_dim.  NULL (a zero-initialised descriptor): off, every kernel
 * runs what it ran before.
 *
 * Time-adaptive rollouts (the environment side of non_equidistant_time, lasgroup's "when to sense and control" setting: the policy
 * also chooses how long its control is held.  The reference tree carries the loss side only — sac/losses.py:90-96,
 * ppo/losses_new.py:105-112 — its wrapper lives elsewhere and is restated here as remembered, unverified: THIS TEXT IS THE
 * DEFINITION, as for hallucinated control).  A rollout is time-adaptive when hold_max_steps = K > 0.  Then:
 *   action width   u_dim stays the width the policy emits, the rows carry and the critics see: A = u_env + 1.  An action is
 *                  [u (u_env) | tau], both parts whatever the policy or the open-loop `actions` give after action_clip.
 *   dynamics input the dynamics and every reward read [x, u] only: dynamics.dims[0] == x_dim + u_env == x_dim + u_dim - 1.  Pendulum
 *                  dynamics and reward: x_dim == 3 && u_env == 1.  Quadratic reward: params stay [t[x], q[x], r[u_env]].
 *   hold           t = (hold_max_time - hold_min_time) / 2 * tau + (hold_max_time + hold_min_time) / 2      (one fused multiply-add)
 *                  k = clamp((int) floor_divide(t, hold_dt), 1, K)
 *                  with floor_divide jnp.floor_divide on floats (mod = fmodf(t, dt); div = (t - mod) / dt; div -= 1 where mod != 0
 *                  and its sign differs from dt's; roundf(div)).  These are the operations, in their order, of the losses' per-sample
 *                  discount exp(-continuous_discounting * floor_divide(t, env_dt) * env_dt): the time a row is discounted by is the
 *                  time its control was held.  The clamp to 1 is the rollout's alone: where the floor gives 0 (tau = -1 to rounding,
 *                  with hold_min_time == hold_dt) the loss discounts by exp(0) while the control is held for one hold_dt; a floor above
 *                  K (hold_max_time beyond K * hold_dt) is cut to K likewise.
 *   inner steps    j = 0 .. k - 1 with u held: r_j is the reward at the pre-step (x_j, u), x_{j+1} the system's step — every ensemble
 *                  mode, ens_sample_noise, the learned reward, the Pendulum — exactly as an action_repeat inner step.  The model stays
 *                  a model of one hold_dt.
 *   reward         R = (sum_j w_j r_j) - hold_switch_cost, w_0 = 1, w_{j+1} = w_j * hold_gamma, every product rounded to fp32 before
 *                  it is added, j ascending from 0.  The caller passes hold_gamma = exp(-continuous_discounting * env_dt) (formed in
 *                  float64, rounded once); at 1 the sum is the plain sum action_repeat forms, bit for bit.
 *   termination    with a box set it is checked after EVERY inner step: a row whose x_{j+1} is violated stops there — its state
 *                  freezes, it takes no further reward, sys_done = 1 (so done = 1 and, unless the episode also ran out, truncation =
 *                  0).  Without a box nothing is checked.
 *   bookkeeping    steps += k_eff, the inner steps the row took (k, or fewer where it terminated); done / truncation / discount /
 *                  the reset / fresh starts (one draw per decision, element s * n_envs + env) keep their formulas; next_observation is
 *                  the post-reset obs.  episode_length counts model steps (an episode is episode_length * hold_dt of time) and may be
 *                  overshot by less than one hold, as action_repeat overshoots it.
 *   randomness     the member / model-noise / learned-reward element index is ((s * K + j) * n_envs + env): action_repeat's with K
 *                  in its place, whatever k the row has.  Explicit model_noise is [S, K, N, x_dim], member_idx [S, K, N].
 *   unchanged      the policy's sampling, action_clip, ppo_extras (log_prob summed over all A dims), env_major, the normaliser, the
 *                  row layout (at action width A).
 * MBPO_ERR_ARG, checked before any device use, when hold_max_steps is set and: it lies outside [1, 64]; action_repeat != 1; halluc_beta
 * is set; u_dim < 2; the dynamics input width is not x_dim + u_dim - 1; hold_dt <= 0; hold_min_time > hold_max_time; hold_gamma outside
 * (0, 1]; hold_switch_cost < 0.  MBPO_ERR_UNSUPPORTED for 64-wide networks with more than 16 inputs or outputs (no such instantiation).
 * All six fields zero (a zero-initialised descriptor): off, every kernel runs what it ran before.  The kernel specialised for the
 * benchmark networks and mbpo_episode_step never see the option. */
typedef struct mbpo_rollout_desc {
  mbpo_mlp_desc policy;   /* [x_dim] -> [2*u_dim] */
  mbpo_mlp_desc dynamics; /* [x_dim+u_dim] -> [2*x_dim] (mean, raw std) or [2*x_dim+2] (+ reward mean, raw std: MBPO_REWARD_LEARNED);
                             ignored for MBPO_SYS_PENDULUM.  With halluc_beta: [u_dim] -> ... (u_dim = x_dim + the control width) */
  int32_t x_dim, u_dim;
  int64_t n_envs;          /* N */
  int32_t n_steps;         /* S = num_env_steps_between_updates (SAC) or unroll_length (PPO) */
  int32_t episode_length;  /* model-env horizon H (EpisodeWrapper) */
  int32_t action_repeat;   /* EpisodeWrapper.action_repeat */
  int32_t system_kind;     /* MBPO_SYS_* */
  int32_t ens_mode;        /* MBPO_ENS_* */
  int32_t ens_predict_delta; /* 1: x' = x + f(x,u) */
  int32_t ens_sample_noise;  /* 1 (TS modes): x' += sigma_e * eps */
  float ens_min_std;         /* sigma = softplus(raw) + ens_min_std */
  int32_t reward_kind;       /* MBPO_REWARD_* */
  const float *reward_params;
  const float *sys_params;   /* pendulum: [max_speed, max_torque, dt, g, m, l] */
  const float *norm_mean;    /* [x_dim] or NULL (normalize_observations=False) */
  const float *norm_std;     /* [x_dim] or NULL */
  int32_t deterministic;     /* 1: action = tanh(loc) (mode) */
  int32_t ppo_extras;        /* 1: rows carry log_prob and raw_action (ppo_network.py:72-80) */
  int32_t env_major;         /* 0: row = s*N + i (SAC concat order, sac.py:296); 1: row = i*S + s (PPO [B*M,T]) */
  float action_clip;         /* > 0: action = clip(tanh(z), +-action_clip) — BPTT's squash_action (bptt_optimizer.py:313-317) */
  const float *actions;        /* optional [S, N, u_dim] open-loop actions: the policy is skipped (`policy` may be zeroed) —
                                  rollout_actions (utils/optimizer_utils.py:11-59) and, with S=1, System.step itself */
  /* randomness: explicit tensors when non-NULL, else counter-based Philox4x32-10 keyed by (seed, offset) */
  const float *policy_noise;   /* [S, N, u_dim] standard normal */
  const float *model_noise;    /* [S, action_repeat, N, x_dim] standard normal */
  const int32_t *member_idx;   /* [S, action_repeat, N] in [0, E) for MBPO_ENS_TS1 */
  uint64_t seed, offset;
  const uint64_t *rng_dev;     /* optional device uint64[2] {seed word, step counter} added to (seed, offset): see "randomness" */
  /* env state, updated in place (brax State.obs / info['steps'] / done / info['first_obs']) */
  float *obs;             /* [N, x_dim] */
  float *first_obs;       /* [N, x_dim]; in/out with a start buffer (see "fresh starts"), read-only without */
  float *steps;           /* [N] (float flags, as in the reference) */
  float *done;            /* [N] */
  /* output: flattened Transition rows (brax UniformSamplingQueue ravel order)
   *   [obs(x), action(u), reward, discount, next_obs(x), {log_prob, raw_action(u)}, truncation] */
  float *transitions;     /* [S*N, row_len] */
  int32_t row_len;        /* 2x+u+3 (+1+u with ppo_extras) */
  /* hallucinated control (see above): NULL = off */
  const float *halluc_beta;    /* [x_dim] */
  /* fresh starts (see above): all four zero = off.  (They sit in front of the termination pair, which closes the descriptor.) */
  const float *start_rows;     /* [start_max_size, start_row_len] ring storage; the start state is columns 0 .. x_dim of a row */
  int64_t start_max_size;
  int32_t start_row_len;       /* >= x_dim */
  const int32_t *start_state;  /* device int32[>= 3] {insert_position, sample_position, head, ...} */
  /* time-adaptive rollouts (see above): hold_max_steps 0 = off.  (They too sit in front of the termination pair.) */
  int32_t hold_max_steps;      /* K in [1, 64] */
  float hold_min_time, hold_max_time, hold_dt;   /* tau in [-1, 1] -> [hold_min_time, hold_max_time]; hold_dt = env_dt > 0 */
  float hold_gamma;            /* exp(-continuous_discounting * env_dt) in (0, 1] */
  float hold_switch_cost;      /* >= 0, charged once per decision */
  /* termination (see above): each [x_dim], both NULL = none (a zero-initialised descriptor), exactly one NULL = MBPO_ERR_ARG */
  const float *term_low, *term_high;
} mbpo_rollout_desc;

int mbpo_model_rollout(const mbpo_rollout_desc *d, void *stream);

/* steps_out[i] = the k a time-adaptive rollout holds the control of actions[i] for ("time-adaptive rollouts" above, from the last of
 * its action_dim columns; the same device function, one thread per row): for host code that applies an action to the true system
 * for as long as the model held it.  actions [n, action_dim], steps_out int32 [n], both on the device.  MBPO_ERR_ARG before any device
 * use: n < 0, action_dim < 1, env_dt <= 0, min_time > max_time, max_steps outside [1, 64], a NULL pointer with n > 0. */
int mbpo_hold_steps(const float *actions, int64_t n, int32_t action_dim, float min_time, float max_time, float env_dt,
                    int32_t max_steps, int32_t *steps_out, void *stream);

/* out[i] = the reward of row i as the rollout kernels form it, one thread per row, by the same device function: for
 * Reward.__call__ on the host side and for tests.  MBPO_REWARD_TERMS ("term rewards" above; u_dim is the control width UE) and
 * MBPO_REWARD_QUADRATIC; every other kind is MBPO_ERR_UNSUPPORTED.  x [n, x_dim], u [n, u_dim], x_next [n, x_dim] or NULL, out [n], all
 * on the device.  x_next == NULL makes the x_next columns of z read x — for a table the caller knows to be free of next-state terms;
 * a row of x_next with a non-finite component reads x likewise.  The quadratic reward ignores x_next.  No workspace; capturable.
 * MBPO_ERR_ARG before any device use: n < 0, x_dim < 1, u_dim < 1, or with n > 0 a NULL reward_params, x, u or out. */
int mbpo_reward_eval(int32_t reward_kind, const float *reward_params, const float *x, const float *u, const float *x_next, int64_t n,
                     int32_t x_dim, int32_t u_dim, float *out, void *stream);

/* ---- R1/R4-R7 for a USER-DEFINED System: the non-fused env step ------------------------------------
 * replaces: the same reference lines as mbpo_model_rollout, split at the reference's own plug-in seam — System.step
 *           (systems/base_systems.py:40-52 -> Dynamics.next_state, dynamics/base_dynamics.py:15-20 / Reward.__call__,
 *           rewards/base_rewards.py:15-21) stays the caller's code (a batched torch function on the device); per env step the
 *           host issues  mbpo_policy_act -> System.step (x action_repeat) -> mbpo_episode_step.
 * mbpo_policy_act   : make_inference_fn (sac_networks.py:58-73 / ppo_network.py:59-84): logits = MLP(normalize(obs)),
 *                     NormalTanh sample / mode (sac/parametric_distribution.py:66-124); raw_action [n,u] and log_prob [n] are
 *                     optional (PPO's policy extras).  Noise: explicit [n,u] or Philox(seed, offset [+ rng_dev], stream 1,
 *                     element elem_base + i*u + d) — with elem_base = s*N*u this IS the fused kernel's stream at step s.
 *                     workspace: n * (x_dim + 2*u_dim) floats (normalised obs, logits); need not be initialised.
 * mbpo_episode_step : EpisodeWrapper.step + AutoResetWrapper.step bookkeeping (brax_utils/training.py:91-137) and the
 *                     Transition row of actor_step (sac/acting.py:46-55) for step `step_index` of an unroll of `n_steps`;
 *                     `reward` is already summed over action_repeat, `sys_done` (optional) is SystemState.done.
 *                     Updates obs/steps/done in place, exactly like mbpo_model_rollout.  With a start buffer (the start_* fields,
 *                     "fresh starts" above) an env that comes out done has its first_obs replaced by the draw of element
 *                     step_index * n_envs + env of stream START under (seed, offset [+ rng_dev]): a host loop over the steps draws
 *                     bit for bit what the fused launch draws. */
int mbpo_policy_act(const mbpo_mlp_desc *policy, const float *obs, int64_t n, const float *norm_mean, const float *norm_std,
                    int32_t deterministic, float action_clip, const float *noise, uint64_t seed, uint64_t offset,
                    const uint64_t *rng_dev, uint64_t elem_base, float *action, float *raw_action, float *log_prob,
                    float *workspace, void *stream);

typedef struct mbpo_episode_step_desc {
  int32_t x_dim, u_dim;
  int64_t n_envs;
  int32_t episode_length, action_repeat;
  int32_t ppo_extras, env_major;   /* as in mbpo_rollout_desc */
  int32_t step_index, n_steps;     /* s and S: the row is s*N + i (or i*S + s with env_major) */
  const float *action;             /* [N, u] */
  const float *raw_action;         /* [N, u] (ppo_extras) */
  const float *log_prob;           /* [N]    (ppo_extras) */
  const float *reward;             /* [N] */
  const float *x_next;             /* [N, x] */
  const float *sys_done;           /* [N] or NULL (= 0) */
  float *first_obs;                /* [N, x]; in/out with a start buffer */
  float *obs, *steps, *done;       /* env state, updated in place */
  float *transitions;              /* [S*N, row_len] */
  int32_t row_len;
  /* fresh starts: all four start_* zero = off (seed, offset, rng_dev are then unused) */
  const float *start_rows;
  int64_t start_max_size;
  int32_t start_row_len;
  const int32_t *start_state;
  uint64_t seed, offset;
  const uint64_t *rng_dev;         /* optional device uint64[2], see "randomness" */
} mbpo_episode_step_desc;

int mbpo_episode_step(const mbpo_episode_step_desc *d, void *stream);

/* ---- R9: replay buffer (brax UniformSamplingQueue semantics, INT32-exact) --------------------
 * replaces: replay_buffer.insert / .sample as called at sac/sac.py:303,318 and systems/brax_wrapper.py:29,
 *           bptt_optimizer.py:459,479 ([3P] brax.training.replay_buffers.UniformSamplingQueue; field use
 *           evidenced by bptt_optimizer.py:447-456).
 * The logical array data[max_size][row_len] of the reference is stored as a ring: logical row i lives at
 * physical row (i + head) % max_size, so the reference's jnp.roll on overflow is an O(1) head move.
 * state (device, int32[4]) = {insert_position, sample_position, head, total_inserted_low32}.
 */
int mbpo_replay_insert(float *data, int64_t max_size, int32_t row_len, int32_t *state, const float *rows,
                       int64_t n_rows, void *stream);
/* out[j] = data_logical[wrap(idx[j])]   (jnp.take(..., mode='wrap')); idx are LOGICAL indices */
int mbpo_replay_gather(const float *data, int64_t max_size, int32_t row_len, const int32_t *state, const int32_t *idx,
                       int64_t n, float *out, void *stream);
/* idx[j] = randint(sample_position, insert_position) from Philox(seed, offset, stream=REPLAY, j), then gather.
 * idx_out may be NULL; rng_dev (optional device uint64[2], see "randomness") is added to (seed, offset) at run time.
 * Fused sample+gather: sac/sac.py:318 (UniformSamplingQueue.sample). */
int mbpo_replay_sample(const float *data, int64_t max_size, int32_t row_len, const int32_t *state, uint64_t seed,
                       uint64_t offset, const uint64_t *rng_dev, int64_t n, int32_t *idx_out, float *out, void *stream);
/* MBPO's mixed minibatches (its real_ratio; not in the reference tree, which has no model loop — restated from the MBPO paper's
 * procedure, unverified against its code): ONE launch fills out [n, row_len], n = minibatch * G rows in the MODEL buffer's layout,
 * from two rings.  replaces: the mbpo_replay_sample launch of a SAC training step (sac/sac.py:318) when real_ratio > 0.
 * Row j is position p = j % minibatch of minibatch j / minibatch; real rows come first:
 *   p <  n_real: idx[j] = randint(real sample_position, real insert_position) from Philox(seed, real_offset, stream=REPLAY, j),
 *                out[j] = [real_logical[wrap(idx[j])][0 .. real_row_len) | 0.0f ...]   (real_row_len <= row_len: a real transition
 *                [obs | action | reward | discount | next_obs] shares the model row's column prefix; the rest — truncation — is 0)
 *   p >= n_real: idx[j] and out[j] are exactly mbpo_replay_sample's at the same j under (seed, offset): same draw, same row.
 * The element index is j in both draws; positions, head and max_size are each buffer's own.  An empty range (insert_position ==
 * sample_position) yields idx = sample_position, as mbpo_replay_sample does.  idx_out (may be NULL) receives the LOGICAL index in
 * whichever buffer served row j.  rng_dev is added to (seed, offset) and to (seed, real_offset).  n == 0 launches nothing.
 * MBPO_ERR_ARG: a null buffer/state (or out with n > 0), minibatch <= 0, n not a multiple of minibatch, n_real outside
 * [0, minibatch], real_row_len outside (0, row_len], either max_size outside (0, 2^31 - 1). */
int mbpo_replay_sample_mixed(const float *data, int64_t max_size, int32_t row_len, const int32_t *state, const float *real_data,
                             int64_t real_max_size, int32_t real_row_len, const int32_t *real_state, uint64_t seed, uint64_t offset,
                             uint64_t real_offset, const uint64_t *rng_dev, int64_t n, int32_t minibatch, int32_t n_real,
                             int32_t *idx_out, float *out, void *stream);

/* perm = stable argsort of key_i = Philox(seed, offset [+ rng_dev], stream PERM, i).word0, i in [0, n): the ONE shared
 * permutation of PPO.sgd_step (ppo/ppo.py:166-171: jr.permutation with the same key for every leaf); gather whole
 * trajectories with mbpo_replay_gather(idx = perm).  workspace: n uint32 of scratch (keys for n > 16384; word 0 is an overflow flag of
 * the bucketed sort for 1024 < n <= 16384 — its initial value does not matter, it is left at 0).  The whole workspace need not be initialised; perm is written in full.  n <= 2^20. */
int mbpo_philox_permutation(uint64_t seed, uint64_t offset, const uint64_t *rng_dev, int64_t n, int32_t *perm,
                            uint32_t *workspace, void *stream);

/* ---- R8: running_statistics.update ([3P] brax.training.acme.running_statistics; call sites
 * sac/sac.py:298-301, ppo/ppo.py:216-219), in the reference's own two-pass form, split so that a multi-GPU
 * host can all-reduce `sums` after each pass (the live form of `pmap_axis_name`'s two psums):
 *   pass 0: sums[0] = n, sums[1..x] = sum(d),  d = obs - mean_old  over rows[:, col_off : col_off+x_dim]
 *   pass 1: sums[1+x..1+2x) = sum(d * (d - upd)),  upd = sums[1..x] / (count + sums[0])
 *   apply : count += n; mean += sum_d/count; summed_variance += pass-1 sums;
 *           std = clip(sqrt(max(summed_variance,0)/count), std_min, std_max)   (brax: 1e-6, 1e6)
 * The same update IS BPTT's Normalizer.update (bptt_optimizer.py:52-67) with summed_variance = std^2 * size:
 *   sum (x - new_mean)^2 + size*(mean - new_mean)^2 == sum d*(d - upd); its floor is std_min = 1e-8, no ceiling.
 * stats (device, fp32) = [count, mean[x], summed_variance[x], std[x]];
 * workspace >= mbpo_running_stats_workspace_floats(x_dim) floats (one partial per workgroup, column and pass); need not be initialised.
 * `sums` [1 + 2 x_dim]: pass 0 writes [0, 1 + x_dim) and pass 1 reads those and writes the rest; mbpo_running_stats_update writes all of it.
 * `stats` is state (read and updated).
 */
int64_t mbpo_running_stats_workspace_floats(int32_t x_dim);
int mbpo_running_stats_reduce(const float *rows, int64_t n_rows, int32_t row_len, int32_t col_off, int32_t x_dim,
                              const float *stats, float *sums, float *workspace, int32_t pass, void *stream);
int mbpo_running_stats_apply(float *stats, const float *sums, int32_t x_dim, float std_min, float std_max, void *stream);
/* The same update for a SINGLE rank (nothing to all-reduce between the passes) in three launches instead of five: pass 0, then a
 * pass 1 whose workgroups add the first pass's partials up themselves, then one workgroup that sums the second pass and applies.
 * Bit-identical to reduce(pass 0) -> reduce(pass 1) -> apply; `sums` receives the same values. */
int mbpo_running_stats_update(const float *rows, int64_t n_rows, int32_t row_len, int32_t col_off, int32_t x_dim, float *stats,
                              float *sums, float *workspace, float std_min, float std_max, void *stream);

/* ---- P4: GAE (ppo/losses.py:128-184) and B2: lambda-return (utils/optimizer_utils.py:119-152) -------
 * Reverse first-order linear recurrences evaluated as wavefront-shuffle segmented scans.
 * Layout: time_major=1 -> arrays are [T,B] (the reference's layout after its swapaxes, losses.py:79);
 *         time_major=0 -> [B,T] (PPO's native data layout, ppo.py:210-213; no transpose needed).
 * gae:  vs, adv (both stop_gradient in the reference) from truncation, termination, rewards, values, bootstrap[B].
 * lambda_return: returns[t] = r_t + gamma*(1-lam)*v'_t + gamma*lam*returns[t+1], returns[T] = v'_{T-1}.
 */
int mbpo_gae_scan(const float *truncation, const float *termination, const float *rewards, const float *values,
                  const float *bootstrap, float *vs, float *advantages, int64_t B, int32_t T, float gamma,
                  float lam, int32_t time_major, void *stream);
int mbpo_lambda_return_scan(const float *rewards, const float *next_values, float *returns, int64_t B, int32_t T,
                            float gamma, float lam, int32_t time_major, void *stream);
/* N1: GAE with a per-element discount array (same layout as rewards) — the non_equidistant_time form of compute_gae
 * (ppo/losses_new.py:181-226): gamma is replaced element-wise in deltas, in the scan coefficient and in the advantages. */
int mbpo_gae_scan_discounts(const float *truncation, const float *termination, const float *rewards, const float *values,
                            const float *bootstrap, const float *discounts, float *vs, float *advantages, int64_t B,
                            int32_t T, float lam, int32_t time_major, void *stream);

/* ---- S3-S8: SAC sgd_step (sac/sac.py:227-281) -------------------------------------------------
 * replaces: SAC.sgd_step = alpha_update + critic_update + actor_update (all three evaluated at the OLD
 *           (alpha, policy, q) parameters, sac.py:234-258) + Polyak target update (sac.py:260-261);
 *           losses sac/losses.py:61-125; gradient_update_fn + optax chain(clip_by_global_norm, adamw)
 *           sac/utils.py:36-63, sac/sac.py:175-186.
 *
 * Flat train state (device, fp32), NP = P + 2*Q + 1 with P = policy params, Q = params of one critic:
 *   params   [NP] = [ policy | critic 0 | critic 1 | log_alpha ]
 *   target_q [2Q];  adam_m [NP];  adam_v [NP];  step_count [1] (optax's count, kept as a float: it only feeds Adam's bias
 *                   corrections 1 - b^count, which are exactly 1.0f long before a float stops counting at 2^24; it plays NO part
 *                   in the random streams)
 *                   SATURATION: every optimizer here (this one, mbpo_ppo_*, mbpo_adamw_step) advances its count as a float32
 *                   `count + 1.0f`, so the stored count reaches 16 777 216 = 2^24 and stays there: 2^24 + 1 rounds back to 2^24.
 *                   optax's int32 count saturates at 2^31 - 1 instead.  The update is the same on both sides of 2^24 (both
 *                   corrections are exactly 1.0f from count ~ 17 000 on: 0.999^count < 2^-25), so only the NUMBER read back
 *                   differs: a caller that needs the true number of steps beyond 2^24 keeps an integer of its own
 *                   (tests/test_gpu_optimizer_trained_state.py pins the stored value and the update across 2^24).
 *   grads    [NP]   written by mbpo_sac_grads, read by mbpo_sac_apply (all-reduce it in between for N>1 ranks —
 *                   the live form of the reference's dead jax.lax.pmean, sac/utils.py:29-33)
 * Three entry points so that the multi-GPU exchange sits at the reference's pmean position:
 *   mbpo_sac_grads      : per-sample forward/backward of the three losses on one minibatch -> grads, metrics[0..2]
 *                         (critic_loss, actor_loss, alpha_loss); also bumps step_count (at the start of the forward/backward
 *                         launch) and leaves per-group
 *                         sum-of-squares partials of `grads` in the workspace.
 *   mbpo_sac_grad_norms : recompute those partials from `grads` (call after an all-reduce changed it).
 *   mbpo_sac_apply      : grads *= grad_scale; clip_by_global_norm per optimizer; AdamW; target <- (1-tau) target + tau q_new;
 *                         metrics[3] = exp(new log_alpha).
 * Noise: explicit standard-normal tensors [B,u] or NULL -> Philox(seed, offset [+ rng_dev]), streams 5/6/7: the caller
 *        advances `offset` (or the device counter) between sgd_steps.
 * Network shapes (sac.py:84-88 takes any tuple): policy and critics with hidden layers of ONE common width in {64, 128} whose 16-row
 *        tile fits the LDS run on the fused wave-chain kernel; every other shape (any hidden sizes, up to MBPO_MAX_LAYERS Dense layers)
 *        runs its forward/backward layer by layer — one GEMM launch per Dense layer — behind the same entry points, with the same
 *        results contract (mbpo_sac_step == mbpo_sac_grads + mbpo_sac_apply bit for bit).
 */
typedef struct mbpo_sac_desc {
  int32_t x_dim, u_dim;
  int32_t policy_layers;                     /* Dense layers of the policy: dims policy_dims[0..policy_layers] */
  int32_t policy_dims[MBPO_MAX_LAYERS + 1];  /* [x_dim, hidden..., 2*u_dim] */
  int32_t q_layers;
  int32_t q_dims[MBPO_MAX_LAYERS + 1];       /* [x_dim+u_dim, hidden..., 1] */
  int32_t policy_activation, q_activation;   /* MBPO_ACT_* */
  float *params, *target_q, *adam_m, *adam_v, *step_count, *grads;
  float *workspace;                          /* >= mbpo_sac_workspace_floats() floats */
  float *metrics;                            /* [4] critic_loss, actor_loss, alpha_loss, alpha */
  float *metrics_accum;                      /* optional [5]: running sums of the four metrics + step count, for the
                                                epoch means of sac/sac.py:360 without a host round trip per step */
  const float *batch;                        /* [batch_size, row_len] SAC transition rows (2x+u+3) */
  int32_t batch_size, row_len;
  const float *norm_mean, *norm_std;         /* [x_dim] or NULL */
  const float *noise_alpha, *noise_critic, *noise_actor; /* [batch_size, u_dim] or NULL */
  uint64_t seed, offset;
  const uint64_t *rng_dev;                   /* optional device uint64[2], see "randomness" */
  float discounting, reward_scaling, target_entropy, tau;
  float lr_policy, lr_q, lr_alpha, wd_policy, wd_q, wd_alpha, max_grad_norm;
  float grad_scale;                          /* 1/world_size when grads were all-reduced with SUM, else 1 */
  /* N1 (sac/losses.py:90-98): per-sample discount exp(-continuous_discounting * t), t = the switch time encoded in the last
   * action component, affinely mapped to [min,max]_time_between_switches and floored to a multiple of env_dt */
  int32_t non_equidistant_time;
  float continuous_discounting, min_time_between_switches, max_time_between_switches, env_dt;
} mbpo_sac_desc;

int64_t mbpo_sac_workspace_floats(const mbpo_sac_desc *d);
/* Offset (in floats) inside `workspace` of the 16-word control block the optimizer launches keep (uint32 words unless noted):
 * [0] two-launch steps issued, [1] two-launch steps whose clip check is resolved, [13] clip events = optimizer steps in which
 * clip_by_global_norm actually scaled some group (sac.py:218-225 'optax.clip_by_global_norm'), counted by every path
 * (mbpo_sac_apply, the next mbpo_sac_step, mbpo_sac_finalize).  The other words are private.  A host reads [13] between epochs
 * to choose between the two- and the three-launch step: a step that clips costs the two-launch path a second pass (see
 * INTEGRATION.md, "Gradient clipping").  Negative: error code. */
int64_t mbpo_sac_control_offset(const mbpo_sac_desc *d);
int mbpo_sac_grads(const mbpo_sac_desc *d, void *stream);
/* measurement hook: run only part of mbpo_sac_grads — phase_mask bit0 = forward/backward kernel (k_sac_fwd_bwd),
 * bit1 = slab reduce (k_sac_reduce).  mbpo_sac_grads == phase_mask 3.  Used by bench.py to time the dominant kernel. */
int mbpo_sac_grads_phase(const mbpo_sac_desc *d, int32_t phase_mask, void *stream);
int mbpo_sac_grad_norms(const mbpo_sac_desc *d, void *stream);
int mbpo_sac_apply(const mbpo_sac_desc *d, void *stream);
/* The default path — ONE sgd_step in TWO launches (mbpo_sac_grads + mbpo_sac_apply is three):
 *   mbpo_sac_step     : the forward/backward kernel, then ONE launch that reduces the per-tile slabs and applies the optimizer step
 *                       UNCLIPPED, saving the previous (params, adam_m, adam_v, target_q) in an undo log inside `workspace`.
 *                       clip_by_global_norm needs the global gradient norm, i.e. every block's partial: instead of a device-wide
 *                       meeting point inside the launch (measured slower than the kernel boundary it removes), the check is done
 *                       by the NEXT consumer of the parameters — the prologue of the next mbpo_sac_step / mbpo_sac_grads launch, or
 *                       mbpo_sac_finalize — which, if a group's norm reached max_grad_norm, recomputes that group's step from the
 *                       undo log with the clipped gradient: bit-identical to mbpo_sac_grads + mbpo_sac_apply in every case.
 *   mbpo_sac_finalize : resolves the pending check when no further mbpo_sac_step follows (end of training_step's scan of
 *                       sgd_steps, sac/sac.py:324; before anything else reads params / target_q / adam state).  Idempotent.
 * metrics[3] ('alpha') of a step becomes valid when its check has been resolved.  `workspace` must be zero before the first call. */
int mbpo_sac_step(const mbpo_sac_desc *d, void *stream);
int mbpo_sac_finalize(const mbpo_sac_desc *d, void *stream);
/* mbpo_sac_finalize and mbpo_rng_advance(rng_dev, inc) in ONE launch: the end of a training step (sac.py:306-327 — after the scan
 * of sgd_steps the step's randomness is used up and the device counter moves on). */
int mbpo_sac_finalize_advance(const mbpo_sac_desc *d, uint64_t *rng_dev, uint64_t inc, void *stream);

/* ---- P1-P3: PPO minibatch update (ppo/ppo.py:142-156, ppo/losses.py:56-126; ppo/ppo_brax_env.py + losses_new.py) ----------
 * replaces: PPO.minibatch_step = value_and_grad(PPOLoss.loss) + the optimizer over {policy, value}, in either of the reference's
 *           two variants:
 *             ppo.py            optax.adamw(lr, wd), constant discount (ppo.py:128,139-140)          max_grad_norm <= 0, non_equidistant_time = 0
 *             ppo_brax_env.py   optax.chain(clip_by_global_norm(max_grad_norm), adamw(lr, wd))      max_grad_norm > 0 (:137-141)
 *                               and, with non_equidistant_time, a per-sample discount (losses_new.py:105-120,181-226)
 *           A zero-filled tail (max_grad_norm = 0, non_equidistant_time = 0) is the ppo.py variant.
 *           Inside the loss: policy logits and value baseline on [B,T] samples, bootstrap value, compute_gae (stop-gradient),
 *           advantage normalisation over the whole minibatch (losses.py:101-102), clipped surrogate, 0.5*MSE value loss, entropy bonus
 *           with a fresh NormalTanh sample.
 * Flat state: params [P+V] = [ policy | value ]; adam_m/adam_v [P+V]; step_count [1] (a float32 that stops at 2^24: see the
 *             SATURATION note at mbpo_sac_desc's step_count); grads [P+V].
 *   mbpo_ppo_grads : grads, metrics[0..3] = total_loss, policy_loss, v_loss, entropy_loss (losses.py:121-126); bumps step_count
 *   mbpo_ppo_apply : grads *= grad_scale; [clip_by_global_norm over the whole [P+V] gradient;] AdamW.  All-reduce `grads` in
 *                    between for N>1 ranks (ppo.py:149-154's pmean): the clip norm is that of the reduced, scaled gradient.
 * N1 discount: d = exp(-continuous_discounting * t), t = (tu - tl)/2 * a + (tu + tl)/2 floored to a multiple of env_dt, where
 *       a = the last action component of the row and [tl, tu] = [min, max]_time_between_switches; d replaces `discounting` in the
 *       deltas, the scan coefficient and the advantages.  non_equidistant_time with env_dt <= 0 -> MBPO_ERR_ARG.
 * data: one minibatch [batch_size, unroll_length, row_len] of PPO rows (row_len = 2x+2u+4), i.e. the rollout kernel's
 *       env_major output after the permutation gather.  entropy_noise [B,T,u] or NULL -> Philox(seed, offset [+ rng_dev], stream 9).
 * Network shapes (ppo.py:60-63 takes any tuple): as for SAC — one common hidden width in {64, 128} -> fused kernels, anything else
 *       (e.g. experiments/train_inverted_pendulum/exp_ppo.py's 256x5 critic) -> layer by layer behind the same entry points.
 */
typedef struct mbpo_ppo_desc {
  int32_t x_dim, u_dim;
  int32_t policy_layers;
  int32_t policy_dims[MBPO_MAX_LAYERS + 1];  /* [x_dim, hidden..., 2*u_dim] */
  int32_t value_layers;
  int32_t value_dims[MBPO_MAX_LAYERS + 1];   /* [x_dim, hidden..., 1] */
  int32_t policy_activation, value_activation;
  float *params, *adam_m, *adam_v, *step_count, *grads;
  float *workspace;                          /* >= mbpo_ppo_workspace_floats() floats; need not be initialised (every region — values,
                                                GAE arrays, moments, per-sample discounts, slabs, norm partials, the layer-by-layer
                                                buffers — is written before it is read in each mbpo_ppo_grads / _apply / _step) */
  float *metrics;                            /* [4], overwritten (as `grads` is, in full, by mbpo_ppo_grads and mbpo_ppo_step) */
  float *metrics_accum;                      /* optional [5]: running sums of the four metrics + count (state: start it at zero) */
  const float *data;
  int32_t batch_size, unroll_length, row_len;
  const float *norm_mean, *norm_std;         /* [x_dim] or NULL */
  const float *entropy_noise;                /* [B,T,u] or NULL */
  uint64_t seed, offset;
  const uint64_t *rng_dev;                   /* optional device uint64[2], see "randomness" */
  float entropy_cost, discounting, reward_scaling, gae_lambda, clipping_epsilon;
  int32_t normalize_advantage;
  float lr, wd, grad_scale;
  float max_grad_norm;            /* > 0: optax.clip_by_global_norm before AdamW (ppo_brax_env.py:137-141); <= 0: no clip (ppo.py) */
  int32_t non_equidistant_time;   /* losses_new.py:105-112: per-sample discount from the last action component (see above) */
  float continuous_discounting, min_time_between_switches, max_time_between_switches, env_dt;
} mbpo_ppo_desc;

int64_t mbpo_ppo_workspace_floats(const mbpo_ppo_desc *d);
int mbpo_ppo_grads(const mbpo_ppo_desc *d, void *stream);
int mbpo_ppo_apply(const mbpo_ppo_desc *d, void *stream);
/* mbpo_ppo_grads + mbpo_ppo_apply with no seam for a collective between them (a single rank): the launch that sums the gradient
 * also applies AdamW to it — the same bits, one launch less per minibatch_step (ppo/ppo.py:142-156).  With max_grad_norm > 0 that
 * launch leaves the norm's partial sums instead and one more launch clips and applies (the same bits as grads + apply). */
int mbpo_ppo_step(const mbpo_ppo_desc *d, void *stream);

/* ---- B1-B5: BPTT actor gradient (bptt_optimizer.py:327-378) -----------------------------------------
 * replaces: value_and_grad(vmap(actor_loss)) of BPTTOptimizer._train_step, i.e. rollout_policy with stop_grads=True
 *           (utils/optimizer_utils.py:62-116) through System.step, target-critic min(v1,v2) on the normalised next states,
 *           lambda_return (:119-152), discount cumprod, Actor.get_log_prob (:144-152), and the backward pass through ALL of
 *           it with respect to the actor parameters (gradient flows a -> x' -> ... through the model and the target
 *           critic; the policy's own observation input is stop-gradiented when acting but NOT inside get_log_prob).
 * One launch: forward rollout (checkpoints x_t, a_t, eps_t in `workspace`), lambda-returns, reverse sweep with per-step
 * recomputation of the activations in LDS.  Outputs: actor `grads` [P]; the simulated transitions
 * [n*horizon, 2x+u+2] = [obs, action, reward(raw), discount=1, next_obs] (what :478-479 inserts into the sampling buffer);
 * lambda_values [n*horizon] (the critic targets of :385-419); metrics = {actor_loss, entropy_loss}.
 * Log-prob for u_dim > 1 uses sum_A logN - sum_A log(1-a^2) per step (identical to the reference at u_dim = 1).
 * Ensemble model: every mode of mbpo_model_rollout.  The reference's actor loss threads SystemParams.key through rollout_policy
 * (utils/optimizer_utils.py:81-97) and the optimizer splits a fresh system key each train step (bptt_optimizer.py:357-363, :435-436),
 * so a stochastic System is differentiated by reparameterisation.  For trajectory i and step t:
 *   MBPO_ENS_MEAN : x' = base + mean_e mu_e                         (ens_sample_noise has no effect, as in the rollout)
 *   MBPO_ENS_TS1  : m = member_idx[i, t], or Philox(seed, offset [+ rng_dev], stream MEMBER, i*H + t) in [0, E)
 *   MBPO_ENS_TSINF: m = i % E
 *   TS modes      : x' = base + mu_m (+ (softplus(raw_m) + ens_min_std) * eps with ens_sample_noise; eps = model_noise[i, t, c],
 *                   or Philox(..., stream MODEL_NOISE, (i*H + t)*x + c)),  base = x if ens_predict_delta else 0.
 * The gradient is the pathwise one: only member m receives dL/dmu_m = dL/dx' (and dL/draw_m = dL/dx' * eps * sigmoid(raw_m));
 * the member draw itself is not differentiated.  member_idx values in [0, E) are the caller's contract.
 * MBPO_REWARD_LEARNED: r_t is read from the reward head (column 2x) as mbpo_model_rollout reads it, and dL/dr_t enters the member
 * output gradient at that column (divided by E in MBPO_ENS_MEAN; the selected member alone in the TS modes).
 */
typedef struct mbpo_bptt_desc {
  int32_t x_dim, u_dim, horizon;
  int32_t actor_layers;
  int32_t actor_dims[MBPO_MAX_LAYERS + 1];   /* [x_dim, features..., 2*u_dim] */
  int32_t critic_layers;
  int32_t critic_dims[MBPO_MAX_LAYERS + 1];  /* [x_dim, features..., 1] */
  int32_t actor_activation, critic_activation;
  float init_stddev;                         /* Actor.init_stddev (:127) */
  const float *actor_params;                 /* [P] */
  const float *target_critic_params;         /* [2*C] = [critic_1 | critic_2] */
  int32_t system_kind;                       /* MBPO_SYS_* */
  mbpo_mlp_desc dynamics;                    /* ensemble ([x+u] -> [x] or [2x] = [mu, raw std], or [2x+2] with the reward head of
                                                MBPO_REWARD_LEARNED), ignored for MBPO_SYS_PENDULUM */
  int32_t ens_predict_delta;
  int32_t reward_kind;                       /* MBPO_REWARD_* */
  const float *reward_params, *sys_params;
  const float *state_mean, *state_std;       /* [x_dim] state normaliser */
  const float *reward_mean_std;              /* [2] reward normaliser {mean, std} */
  const float *init_states;                  /* [n, x_dim] */
  int64_t n;
  const float *act_noise;                    /* [n, horizon, u_dim] or NULL -> Philox(seed, offset [+ rng_dev], stream 1) */
  uint64_t seed, offset;
  const uint64_t *rng_dev;                   /* optional device uint64[2], see "randomness" */
  float discount, lambda_, ent_coef;
  float *transitions, *lambda_values, *grads, *metrics;
  float *workspace;                          /* >= mbpo_bptt_workspace_floats() floats; need not be initialised (the forward sweep writes
                                                every checkpoint — states, actions, noise, rewards, values, the drawn members, the z store —
                                                before the reverse sweep reads it); transitions, lambda_values, grads and metrics are
                                                overwritten in full */
  int32_t ens_mode;                          /* MBPO_ENS_*; TS1 / TSINF need MBPO_SYS_ENSEMBLE */
  int32_t ens_sample_noise;                  /* 1 (TS modes): x' += sigma_m * eps; needs dynamics outputs >= 2*x_dim */
  float ens_min_std;                         /* sigma = softplus(raw) + ens_min_std */
  const int32_t *member_idx;                 /* [n, horizon] in [0, E) or NULL -> Philox (MBPO_ENS_TS1) */
  const float *model_noise;                  /* [n, horizon, x_dim] standard normal or NULL -> Philox */
} mbpo_bptt_desc;

int64_t mbpo_bptt_workspace_floats(const mbpo_bptt_desc *d);
int mbpo_bptt_actor_grads(const mbpo_bptt_desc *d, void *stream);

/* ---- B4: twin-V critic regression (bptt_optimizer.py:385-419) ----------------------------------------
 * replaces: value_and_grad(critic_loss_fn) of update_critic: loss = 0.5*(mean l2(v1, lamb) + mean l2(v2, lamb)), l2 = 0.5(.)^2,
 *           on a minibatch gathered (with replacement) from the flattened simulated transitions:
 *           obs_j = transitions[idx[j], 0:x_dim] (normalised with the state normaliser), target_j = lambda_values[idx[j]].
 * grads [2*C] in the [critic_1 | critic_2] layout; metrics[0] = critic loss (both overwritten).  workspace >=
 * mbpo_critic_workspace_floats() floats (gradient slabs and loss partials); need not be initialised.
 */
int64_t mbpo_critic_workspace_floats(int32_t x_dim, int32_t critic_layers, const int32_t *critic_dims, int64_t batch);
int mbpo_critic_grads(const float *critic_params, int32_t x_dim, int32_t critic_layers, const int32_t *critic_dims,
                      int32_t activation, const float *transitions, int32_t row_len, const float *lambda_values,
                      const int32_t *idx, int64_t batch, const float *state_mean, const float *state_std, float *grads,
                      float *metrics, float *workspace, void *stream);

/* ---- B1/B3 around a USER-DEFINED System: vector-Jacobian product of one or two 64-wide MLPs ------------------------
 * replaces: the reverse-mode pieces of value_and_grad(vmap(actor_loss)) (bptt_optimizer.py:361-372) that are NOT the user's
 *           System.step when the horizon loop of rollout_policy (utils/optimizer_utils.py:62-116) has to run on the host:
 *           the actor MLP (weights only: act(stop_gradient(obs)), :85-86) and the twin target critics on the next state
 *           (input only: bptt_optimizer.py:342-343).  MLP semantics: utils/network_utils.py:5-17.
 * For every net k < n_nets (1 or 2; shared input):  y_k = MLP_k((x - norm_mean) / norm_std)   [norm_* NULL: y_k = MLP_k(x)]
 *   dx[k][j][:] = d <dy[k][j], y_k[j]> / d x[j]        (optional, [n_nets][n][dims[0]], with respect to the RAW x)
 *   dw[k][:]    = sum_j d <dy[k][j], y_k[j]> / d params_k   (optional, [n_nets][params per net]; needs net_stride == params per net)
 *   y[k][j][:]  = the recomputed outputs (optional, [n_nets][n][dims[n_layers]])
 * dy: [n_nets][n][dims[n_layers]].  Hidden layers 64 wide, input / output width <= 32.  workspace (only for dw)
 * >= mbpo_mlp_vjp_workspace_floats(mlp, n) floats (weight-gradient slabs); need not be initialised.  y, dx and dw are overwritten
 * in full.  Fixed-order reductions: bit-reproducible.
 */
int64_t mbpo_mlp_vjp_workspace_floats(const mbpo_mlp_desc *mlp, int64_t n);
int mbpo_mlp_vjp(const mbpo_mlp_desc *mlp, const float *x, int64_t n, const float *norm_mean, const float *norm_std,
                 const float *dy, float *y, float *dx, float *dw, float *workspace, void *stream);

/* The same contract for ANY hidden sizes (bptt_optimizer.py:183-186 `actor_features` / `critic_features` accept any tuple; the fused
 * kernel above is built for 64-wide hidden layers): one fp32-MFMA GEMM launch per Dense layer over all n rows (csrc/layered.hip),
 * forward recomputed with its pre-activations kept in `workspace`, then input and weight gradients layer by layer.
 *   x: [n][dims[0]], ALREADY normalised (shared by the nets);  dy: [n_nets][n][dims[n_layers]] or NULL (forward only -> y);
 *   y (optional with dy): [n_nets][n][dims[n_layers]];  dx (optional): [n_nets][n][dims[0]] with respect to the x given;
 *   dw (optional): [n_nets][params per net].  workspace >= mbpo_mlp_layered_workspace_floats(mlp, n) floats (activations, ping-pong
 *   deltas, the split row ranges' partials beyond 1024 rows); need not be initialised.  Fixed-order sums. */
int64_t mbpo_mlp_layered_workspace_floats(const mbpo_mlp_desc *mlp, int64_t n);
int mbpo_mlp_layered_vjp(const mbpo_mlp_desc *mlp, const float *x, int64_t n, const float *dy, float *y, float *dx, float *dw,
                         float *workspace, void *stream);

/* ---- generic optimizer step: [optax.apply_if_finite(] optax.adamw(lr, wd) [)] + optional Polyak target ----------------
 * replaces: actor_optimizer.update/apply_updates (bptt_optimizer.py:218-225, 374-378), critic_optimizer + soft_update
 *           (:406-410; utils/optimizer_utils.py:155-161).
 * grads *= grad_scale; if apply_if_finite and any gradient is non-finite the whole update (params, moments, count) is
 * skipped; count (device scalar, a float32 that stops at 2^24: the SATURATION note at mbpo_sac_desc's step_count) advances by one
 * otherwise; grad_norm_out (optional) = optax.global_norm(grads), +inf when a finite gradient's square overflows (the step is then
 * taken: v = +inf there and that parameter moves by its weight decay alone, as optax in float32);
 * target (optional) <- (1 - tau) * target + tau * new_params.   workspace >= 2 * ceil(n / 256) + 4 floats (sum-of-squares and
 * non-finite counts per block); need not be initialised.  grad_norm_out is overwritten; params, moments, count and target are state.
 */
int mbpo_adamw_step(float *params, const float *grads, float *adam_m, float *adam_v, float *step_count, int64_t n, float lr,
                    float wd, float grad_scale, int32_t apply_if_finite, float *target, float tau, float *grad_norm_out,
                    float *workspace, void *stream);

/* soft_update alone (utils/optimizer_utils.py:155-161): out = (1 - tau) * target + tau * online; out may alias target. */
int mbpo_soft_update(const float *target, const float *online, float *out, int64_t n, float tau, void *stream);

/* ---- N3: ensemble model learning (the step before the rollout path) ------------------------------------
 * Not in the reference (its model would come from the external `bsm` package, setup.py:22).  Gradient of every member's
 * Gaussian negative log-likelihood on its own minibatch of true transitions, with exactly the parameterisation the rollout
 * kernel consumes: (mu, raw) = MLP_e([x, u]); mean = mu (+ x if predict_delta); sigma = softplus(raw) + min_std;
 *   loss_e = mean_b sum_d [ 0.5 ((x'_d - mean_d)/sigma_d)^2 + log sigma_d ].
 * rows: [R, row_len] transitions (x at column 0, u at x_dim, next_obs at next_obs_off); idx: [E, batch] row indices (one
 * bootstrapped minibatch per member); grads [E * n_params] in the dynamics' flat layout; metrics [E] = loss_e.
 * reward_off >= 0 (a [x+u] -> [2x+2] ensemble, MBPO_REWARD_LEARNED): the reward head is fitted too; the target r = row[reward_off]
 * (never delta-encoded), sigma_r = softplus(raw_r) + min_std, and loss_e gains mean_b [ 0.5 ((r - mu_r)/sigma_r)^2 + log sigma_r ].
 * reward_off = -1: no reward term (a 2x + 2 ensemble then gets zero gradient on its reward head).
 * Apply with mbpo_adamw_step on the whole flat vector (members are independent, AdamW is elementwise).
 * Any hidden sizes.  Hidden layers all 64 wide whose 16-row tile fits 160 KiB of LDS: the fused kernel (two launches).  Any other
 * shape (other widths, unequal widths, deeper or wider-output 64 stacks): a layer-by-layer path (gather, one GEMM launch per Dense
 * layer, NLL head, backward GEMM levels writing grads directly), the same loss and gradient, deterministic.  The workspace size
 * depends on the path; mbpo_ens_nll_workspace_floats needs no device.  The workspace need not be initialised on either path; grads
 * (every parameter of every member, an unfitted reward head's as zeros) and metrics are overwritten in full. */
typedef struct mbpo_ens_train_desc {
  int32_t x_dim, u_dim;
  mbpo_mlp_desc dynamics;
  const float *rows;
  int32_t row_len, next_obs_off;
  const int32_t *idx;
  int64_t batch;
  int32_t predict_delta;
  float min_std;
  float *grads, *metrics, *workspace;
  /* Callers MUST set reward_off: a zero-initialised descriptor asks for the reward from column 0 (an error on a 2x net, a wrong
   * target on a 2x+2 net).  Set -1 for no reward head. */
  int32_t reward_off;     /* column of the reward target in rows, or -1: no reward head fitted */
} mbpo_ens_train_desc;

int64_t mbpo_ens_nll_workspace_floats(const mbpo_ens_train_desc *d);
int mbpo_ens_nll_grads(const mbpo_ens_train_desc *d, void *stream);

/* ---- N3b: ensemble model selection (MBPO's model-training procedure — Janner et al. 2019, "When to Trust Your Model" — not the
 * reference's, which has no learned model): held-out loss of every member, per-member best snapshot, elite members.
 * mbpo_ens_eval: forward only, every member on the SAME rows idx[0..n):
 *   metrics[0][e] = mbpo_ens_nll_grads's loss_e on those rows (the same per-element terms; a row's state terms summed first, the
 *                   reward term last);
 *   metrics[1][e] = mean_b [ sum_d (t_d - mu_d)^2 (+ (r - mu_r)^2 when reward_off >= 0) ], t the regression target (delta-encoded
 *                   when predict_delta): MBPO's selection metric, non-negative and independent of the std head.
 * The two paths of mbpo_ens_nll_grads, selected the same way: fused (hidden layers all 64 wide: one workgroup = (member, slot)
 * walks 16-row tiles through the forward chain, two partials per (member, slot), fixed-order reduce — no atomics, deterministic
 * for a fixed slot count) or layered (the shared [x, u] and target gathered once, one GEMM launch per Dense layer over the E nets,
 * a head kernel).  Rows beyond n in the last tile contribute zero.  The shape checks are mbpo_ens_nll_grads's; n > 0; idx,
 * metrics and workspace must not be NULL.  mbpo_ens_eval_workspace_floats needs no device.  The workspace need not be initialised
 * (a larger one left by another shape or path serves as well); metrics [2][E] is overwritten in full. */
typedef struct mbpo_ens_eval_desc {
  int32_t x_dim, u_dim;
  mbpo_mlp_desc dynamics;              /* [x+u] -> [2x] or [2x+2], as mbpo_ens_train_desc */
  const float *rows;
  int32_t row_len, next_obs_off, reward_off;   /* reward_off -1: no reward term */
  const int32_t *idx;                  /* ONE index list [n], shared by all members */
  int64_t n;
  int32_t predict_delta;
  float min_std;
  float *metrics;                      /* [2][E]: row 0 mean NLL, row 1 mean squared error */
  float *workspace;
} mbpo_ens_eval_desc;
int64_t mbpo_ens_eval_workspace_floats(const mbpo_ens_eval_desc *d);
int mbpo_ens_eval(const mbpo_ens_eval_desc *d, void *stream);

/* Per-member best snapshot (MBPO's early stopping), decided and copied on the device: params / best_params [n_members][n_params].
 *   improved_e = isfinite(score_e) && score_e < best_score_e * (1 - rel_tol)      (best_score starts at +inf; scores are >= 0)
 *   improved members: best_params[e] <- params[e] (bit copy), best_score_e <- score_e; the others are untouched.
 *   state (device int32[2]): state[0] <- any improved ? 0 : state[0] + 1 (evaluations since an improvement);  state[1] += 1.
 * Two launches: the decision (it stages the copy map in workspace, int32[n_members]) and the member copy, which reads the map
 * only — nothing reads best_score after it was overwritten.  The workspace need not be initialised: the decision writes all
 * n_members entries of the map before the copy reads them.  best_params, best_score and state are state. */
int mbpo_ens_keep_best(const float *params, float *best_params, int64_t n_params, int32_t n_members, const float *score,
                       float *best_score, float rel_tol, int32_t *state, int32_t *workspace, void *stream);
/* elite_idx[j] = the member of rank j under the total order (score ascending, NaN last, ties by lower index) — the order
 * mbpo_icem_update ranks by;  elite_params[j] <- params[elite_idx[j]] (bit copy), j < n_elites <= n_members.  Two launches (rank,
 * member copy).  The member copy of both calls: destination member j takes source member map[j], 16-byte accesses where source
 * and destination are equally aligned; n_params need not be a multiple of 4.  elite_idx and elite_params are overwritten in full
 * (no workspace: the ranks are a permutation, so every elite_idx entry is written before the copy reads it). */
int mbpo_ens_pick_elites(const float *params, int64_t n_params, int32_t n_members, const float *score, int32_t n_elites,
                         int32_t *elite_idx, float *elite_params, void *stream);

/* ---- N3c: input scaler of the ensemble (MBPO fits one on the training inputs [x, u]; restated from its procedure, unverified against
 * its code; the reference has no model).  Only the inputs are scaled, never the targets.  No kernel above changes: training runs
 * mbpo_ens_nll_grads / mbpo_ens_eval on a matrix prepared once per fit, and every consumer runs on parameters whose first Dense layer
 * has the scaler folded in — ((v - m) / s) W + b == v (diag(1/s) W) + (b - (diag(1/s) W)^T m).
 * Rows are selected the same way in both row calls: row k = rows[idx[k]], k < n, or rows[k] with idx == NULL (then n <= n_rows); an
 * idx entry outside [0, n_rows) is clamped into it.  in_dim = x_dim + u_dim <= 256, else MBPO_ERR_UNSUPPORTED.
 *
 * mbpo_ens_scaler_fit: scaler[0][c] = mean_c, scaler[1][c] = std_c of column c < in_dim over the selected rows, two passes in fp64:
 *   mean_c = (sum_k d_kc) / n;  var_c = (sum_k (d_kc - mean_c)^2) / n  (population variance);  std_c = (float)sqrt(var_c), and
 *   std_c < std_floor -> exactly 1.0f (a constant column, or n = 1, stays unscaled).
 * Three launches (partial sums per workgroup, partial squared deviations per workgroup — each workgroup adds the first pass's
 * partials itself —, one workgroup that finishes).  No atomics; the number of workgroups and each one's rows depend on (n, in_dim)
 * only and every sum runs in a fixed order, so two calls give the same bits.  workspace: mbpo_ens_scaler_workspace_floats(n, in_dim)
 * floats (fp64 partials: 8-byte aligned), no device needed for the query; need not be initialised.  scaler [2][in_dim] is overwritten.
 * MBPO_ERR_ARG: a null rows / scaler / workspace, n_rows, row_len or n <= 0, in_dim outside [1, row_len], n > n_rows without idx,
 * std_floor < 0 (or NaN), a misaligned workspace. */
int64_t mbpo_ens_scaler_workspace_floats(int64_t n, int32_t in_dim);
int mbpo_ens_scaler_fit(const float *rows, int64_t n_rows, int32_t row_len, const int32_t *idx, int64_t n, int32_t in_dim,
                        float std_floor, float *scaler, float *workspace, void *stream);
/* One launch: out[n][2 x_dim + u_dim + 1], the matrix mbpo_ens_nll_grads / mbpo_ens_eval then read with predict_delta = 0,
 * reward_off = x_dim + u_dim (or -1) and next_obs_off = x_dim + u_dim + 1:
 *   out[k][c]               = (row[c] - mean_c) * inv_c,  c < in_dim,  inv_c = 1.0f / std_c (fp32, once per column)
 *   out[k][in_dim]          = row[reward_off], or 0.0f when reward_off < 0
 *   out[k][in_dim + 1 + d]  = row[next_obs_off + d] - row[d] when predict_delta, else row[next_obs_off + d]   (raw values), d < x_dim
 * The output is written 16 bytes per lane when `out` is 16-byte aligned, as dwords otherwise; the source rows are read as dwords.
 * MBPO_ERR_ARG: as above, and a null scaler / out, x_dim <= 0, u_dim < 0, next_obs_off < 0 or next_obs_off + x_dim > row_len,
 * reward_off >= row_len. */
int mbpo_ens_scaler_prepare(const float *rows, int64_t n_rows, int32_t row_len, const int32_t *idx, int64_t n, int32_t x_dim,
                            int32_t u_dim, int32_t next_obs_off, int32_t reward_off, int32_t predict_delta, const float *scaler,
                            float *out, void *stream);
/* One launch: out_params[e] = params[e] with the scaler folded into the first Dense layer, e < n_members (members n_params apart, the
 * stored — padded — layout: W_0[dims0][dims1] row-major, then b_0[dims1]; dims0 = in_dim):
 *   W'[i][j] = W[i][j] * inv_i,  inv_i = 1.0f / std_i
 *   b'[j]    = b[j] - s_j,  s_j = fma(W'[i][j], mean_i, s_j) over i ascending from 0.0f
 * every other float is a bit copy.  A zero-padded hidden column j (W[.][j] = b[j] = +0) comes out exactly +0.  16-byte accesses when
 * n_params and dims1 are multiples of 4 and both vectors are 16-byte aligned, dwords otherwise.
 * MBPO_ERR_ARG: a null pointer, n_members outside [1, 65535], n_params <= 0, a first layer that does not fit n_params, out_params
 * overlapping params (the bias sum reads the unfolded weights). */
int mbpo_ens_fold_scaler(const float *params, int64_t n_params, int32_t n_members, int32_t dims0, int32_t dims1, const float *scaler,
                         float *out_params, void *stream);

/* ---- N3d: calibration of the ensemble's spread on held-out rows (the statistical-model package the reference declares — `bsm`, in
 * setup.py, never imported — recalibrates after every fit; restated from its procedure as remembered, unverified against its code,
 * so the definition below is the authority; the reference has no model).  Per output dimension c one factor calibration[c] is picked
 * from a grid so that the intervals built from calibration[c] * sd_c, sd the population std of the members' means (the sd the
 * hallucinated rollouts form), cover the held-out targets as often as a Gaussian's would at P levels.  No kernel above changes: the
 * result reaches the rollouts as halluc_beta = beta * calibration, formed by the caller.
 * Inputs: y[e][k][c], e < n_members, k < n, c < x_dim: the members' mean heads, dense [n_members][n][y_stride], y_stride >= x_dim (the
 * columns past x_dim are never read).  Row k is rows[idx[k]] of rows[n_rows][row_len], or rows[k] with idx == NULL (then n <= n_rows);
 * an idx entry outside [0, n_rows) is clamped into it.  alphas[n_alphas]: the candidate factors; level_q[n_levels]: the thresholds
 * of the levels, strictly increasing (the caller's contract: for the equispaced levels p_j = j / (P + 1), j = 1..P, level_q[j - 1] =
 * 2 erfinv(p_j)^2, the chi-square(1) quantile; no kernel evaluates a quantile function); scale[x_dim] or NULL (all ones).
 * Statistic of (k, c), every operation a single rounded fp32 operation (no fused multiply-add):
 *   t  = row[next_obs_off + c] - (predict_delta ? row[c] : 0)
 *   m  = (sum_e y[e][k][c]) / n_members, summed in member order from 0.0f
 *   v  = (sum_e (y[e][k][c] - m)^2) / n_members     (two-pass; the square of the rollouts' sd, no square root taken)
 *   d2 = (t - m)^2
 * counts[c][a][j] = #{k : d2 <= (((alphas[a] * scale[c])^2) * level_q[j]) * v}, an IEEE comparison: a NaN on either side is "not
 * covered", and v == 0 covers only d2 == 0 (and nothing where the factor in front of it overflowed to inf).  int32 [x_dim][A][P].
 * Selection, exact in int64:  S[c][a] = sum_{j = 1..P} (counts[c][a][j - 1] * (P + 1) - j * n)^2;  best_idx[c] = argmin_a S[c][a],
 * ties to the lower index;  calibration[c] = alphas[best_idx[c]] * scale[c].
 * One memset and two launches on the stream, capturable into a hipGraph.  The entry point zeroes counts itself and accumulates in it
 * with integer atomics, whose sum does not depend on their order: two calls give the same bits.  It takes no caller-owned scratch.
 * counts, best_idx [x_dim] and calibration [x_dim] are overwritten in full.
 * MBPO_ERR_ARG, before any device use: a null pointer (idx and scale may be NULL), n, n_rows, row_len, n_members, n_alphas, n_levels
 * or x_dim <= 0, y_stride < x_dim, next_obs_off < 0 or next_obs_off + x_dim > row_len, n > n_rows without idx, and
 * n * (n_levels + 1) > 2^28 (so that S cannot overflow).  MBPO_ERR_UNSUPPORTED: n_levels > 127, x_dim > 65535, n_alphas * n_levels >
 * 2^24 or x_dim * n_alphas * n_levels > 2^29. */
int mbpo_ens_calibrate(const float *y, int32_t n_members, int64_t n, int32_t y_stride, const float *rows, int64_t n_rows,
                       int32_t row_len, const int32_t *idx, int32_t x_dim, int32_t next_obs_off, int32_t predict_delta,
                       const float *alphas, int32_t n_alphas, const float *level_q, int32_t n_levels, const float *scale,
                       int32_t *counts, int32_t *best_idx, float *calibration, void *stream);

/* ---- N4: iCEM trajectory optimizer, device side (trajectory_optimizers/icem_optimizer.py:135-252) ---------------------
 * One iteration = mbpo_icem_sample -> mbpo_model_rollout(actions = the sampled sequences) -> mbpo_icem_update.
 * mbpo_icem_sample: coloured noise (utils/general_utils.py:81-208, powerlaw_psd_gaussian, as a direct inverse real DFT; Philox
 *   stream ICEM) per (sample, action dim) series of length horizon; candidate = clip(mean + noise*std, u_min, u_max) (:186-187);
 *   the n_prev previous elites are appended (:190); every candidate is replicated over n_particles envs:
 *   actions [horizon][(n_samples+n_prev)*n_particles][u_dim] (env = candidate*n_particles + particle),
 *   candidates [(n_samples+n_prev)][horizon][u_dim].  u_min/u_max are [u_dim] device vectors.
 * mbpo_icem_update: values[c] = mean (use_max: max) over particles of mean_t reward (:146-163) from the rollout's step-major
 *   transition rows; elites = the n_elites best in np.argsort order; mean <- alpha*mean + (1-alpha)*elite mean, std likewise on
 *   the population variance (:199-209); best_value/best_sequence keep the best elite seen (:212-221); the n_prev best elites
 *   go to prev_elites (:227).  workspace: n_candidates int32 (every candidate's rank, written before any is read); need not be
 *   initialised.  values [n_candidates] and prev_elites [n_prev][horizon*u_dim] are overwritten in full; mean, std, best_value and
 *   best_sequence are state.  State vectors are [horizon*u_dim] device floats. */
int mbpo_icem_sample(const float *mean, const float *std, const float *prev_elites, const float *u_min, const float *u_max,
                     int32_t n_samples, int32_t n_prev, int32_t horizon, int32_t u_dim, int32_t n_particles, float exponent,
                     uint64_t seed, uint64_t offset, const uint64_t *rng_dev, float *actions, float *candidates, void *stream);
int mbpo_icem_update(const float *rows, int32_t row_len, int32_t reward_col, int32_t n_candidates, int32_t n_particles,
                     int32_t horizon, int32_t u_dim, const float *candidates, int32_t n_elites, int32_t n_prev, float alpha,
                     int32_t use_max, float *mean, float *std, float *best_value, float *best_sequence, float *prev_elites,
                     float *values, int32_t *workspace, void *stream);
/* The same with the reference's constraint term (icem_optimizer.py:99,157-166): particle_cost[c * n_particles + p] = the user's
 * cost_fn on the trajectory of candidate c, particle p (evaluated by the host between the rollout and this launch — a Python
 * callable cannot run in a kernel — or written by mbpo_traj_cost_eval, "term costs" below, for a cost given as a term table);
 * objective[c] = reward[c] - lambda_constraint * relu(cost[c]), cost[c] = mean (cost_use_max:
 * max, `use_pessimism`) over the particles.  particle_cost NULL: mbpo_icem_update. */
int mbpo_icem_update_constrained(const float *rows, int32_t row_len, int32_t reward_col, int32_t n_candidates, int32_t n_particles,
                                 int32_t horizon, int32_t u_dim, const float *candidates, int32_t n_elites, int32_t n_prev, float alpha,
                                 int32_t use_max, const float *particle_cost, float lambda_constraint, int32_t cost_use_max, float *mean,
                                 float *std, float *best_value, float *best_sequence, float *prev_elites, float *values,
                                 int32_t *workspace, void *stream);

/* Batched MPC: n_problems independent iCEM problems in one launch chain (icem_optimizer.py:135-252 vmapped over states).
 * Problem b's state sits at mean/std/best_sequence + b*horizon*u_dim, best_value + b, prev_elites + b*n_prev*horizon*u_dim,
 * candidates + b*(n_samples+n_prev)*horizon*u_dim; values/workspace + b*n_candidates.  Its envs are (b*NC + c)*n_particles + p of
 * actions [horizon][n_problems*NC*n_particles][u_dim] and of the rollout rows (NC = n_samples + n_prev = n_candidates).
 * mbpo_icem_sample_batched: problem b draws with seed = seeds[b] (device uint64[n_problems]) at the shared `offset` — bit for bit
 *   mbpo_icem_sample(seed = seeds[b], offset, rng_dev = NULL) on problem b's slices.  n_problems <= 65535.
 * mbpo_icem_update_batched: one workgroup per problem, bit for bit mbpo_icem_update_constrained on problem b's slices
 *   (particle_cost [n_problems*NC*n_particles] or NULL).  workspace: n_problems*n_candidates int32; need not be initialised. */
int mbpo_icem_sample_batched(const float *mean, const float *std, const float *prev_elites, const float *u_min, const float *u_max,
                             int32_t n_samples, int32_t n_prev, int32_t horizon, int32_t u_dim, int32_t n_particles, float exponent,
                             int32_t n_problems, const uint64_t *seeds, uint64_t offset, float *actions, float *candidates, void *stream);
int mbpo_icem_update_batched(const float *rows, int32_t row_len, int32_t reward_col, int32_t n_problems, int32_t n_candidates,
                             int32_t n_particles, int32_t horizon, int32_t u_dim, const float *candidates, int32_t n_elites, int32_t n_prev,
                             float alpha, int32_t use_max, const float *particle_cost, float lambda_constraint, int32_t cost_use_max,
                             float *mean, float *std, float *best_value, float *best_sequence, float *prev_elites, float *values,
                             int32_t *workspace, void *stream);

/* ---- term costs: a trajectory constraint written as a term table, evaluated on the rollout's rows -------------------------------
 * replaces: vmap(cost_fn)(observation, action) between the rollout and the update (icem_optimizer.py:99,161-166) for a cost that can
 *           be written as data (mbpo.systems.TermCost).  Not in the reference tree; build-defined: THIS TEXT IS THE DEFINITION.
 * table is a term table ("term rewards" above: the same MBPO_REWARD_TERMS_FLOATS floats, read by the same device function).  rows is
 * what mbpo_model_rollout writes with open-loop actions, step-major: row t * n_traj + i of row_len floats holds step t of trajectory
 * i, obs at column 0, the action at column x_dim, the next state at column next_off (iCEM: row_len = 2 x_dim + A + 3 and next_off =
 * x_dim + A + 2 with A the action width; u_dim <= A is the control width the dynamics see — an eta or tau column never enters).
 *   c_t     = the table on z = [obs_t (x_dim) | action_t[:u_dim] | next_t (x_dim)], next_t reading obs_t where a component of the
 *             row's next state is not finite (the term rewards' rule)
 *   cost[i] = sum_t c_t    reduce 0: one fp32 accumulator from 0 in ascending t, every sum rounded on its own — bit for bit the
 *                          sequential fp32 sum of mbpo_reward_eval over the trajectory's rows
 *           = max_t c_t    reduce 1: from c_0 in ascending t; a NaN c_t makes cost[i] NaN (as torch.max, not fmaxf)
 * Positive means violated (mbpo_icem_update_constrained applies relu).  One thread per trajectory, no atomics; rows need no alignment.
 * cost [n_traj] is overwritten in full; nothing else is written.  No workspace, no allocation, no host read-back; capturable.
 * MBPO_ERR_ARG before any device use: n_steps < 1, n_traj < 0, x_dim < 1, u_dim < 1, next_off + x_dim > row_len, x_dim + u_dim >
 * next_off, reduce not 0 or 1, or with n_traj > 0 a NULL table, rows or cost.  n_traj == 0: MBPO_OK, nothing is launched. */
int mbpo_traj_cost_eval(const float *table, const float *rows, int32_t row_len, int32_t next_off, int32_t n_steps, int64_t n_traj,
                        int32_t x_dim, int32_t u_dim, int32_t reduce, float *cost, void *stream);

/* ---- plan rewards: reward parameters per planned problem and per planned step, evaluated on the rollout's rows -------------------
 * replaces: the vmapped reward_params of jax.vmap(iCemTO.optimize) over a batch of plans, and a reward whose parameters move along the
 *           horizon (mbpo.systems.PlanRewardParams).  Not in the reference tree; build-defined: THIS TEXT IS THE DEFINITION.
 * A plan reward is a reward kind and a parameter array params [PB][PH][param_len], PB in {1, n_problems}, PH in {1, n_steps}; an axis
 * of size 1 is broadcast.  rows is what mbpo_model_rollout writes with open-loop actions over n_problems * group envs, step-major: row
 * (t, b, j) — step t, problem b, env j of the problem — lies at rows + ((t * n_problems + b) * group + j) * row_len, obs at column 0,
 * the action at column x_dim, the next state at column next_off (iCEM: row_len = 2 x_dim + A + 3, next_off = x_dim + A + 2, A the
 * action width; u_dim <= A is the control width the dynamics see — on an optimistic system the eta columns lie between x_dim + u_dim
 * and the reward column and are never read).  With episode_length = 2^30 and no termination the row's next state is the step's own.
 *   r(t, b, j) = R_kind(params[PB > 1 ? b : 0][PH > 1 ? t : 0]; x = row[0 .. x_dim), u = row[x_dim .. x_dim + u_dim),
 *                       x_next = row[next_off .. next_off + x_dim))
 *   MBPO_REWARD_TERMS      the term table ("term rewards" above) through the one device function every other site calls, x_next reading
 *                          x where a component of it is not finite; param_len >= MBPO_REWARD_TERMS_FLOATS.  Bit for bit mbpo_reward_eval.
 *   MBPO_REWARD_QUADRATIC  [target (x_dim) | q (x_dim) | r (u_dim)], mbpo_reward_eval's expressions in their order, bit for bit;
 *                          param_len >= 2 x_dim + u_dim
 *   MBPO_REWARD_PENDULUM   [angle_cost, control_cost, target_angle] on x = [cos, sin, thetadot] and u[0], the rollout kernels' function;
 *                          x_dim == 3, u_dim == 1, param_len >= 3
 *   MBPO_REWARD_LEARNED    MBPO_ERR_UNSUPPORTED: the head is not a function of the row
 * out[((t * n_problems + b) * group + j) * out_stride] = r(t, b, j).  Dense: out_stride = 1 into a buffer of its own, which the update
 * kernels take as (rows = out, row_len = 1, reward_col = 0).  In place: out = rows + reward_col, out_stride = row_len; this aliasing is
 * legal — a thread reads only the obs, control and next-state columns of its row and writes only that row's reward column, which no
 * thread reads.  Every row's output is written; nothing else is written.  One thread per row, no atomics; rows and params need no
 * alignment.  No workspace, no allocation, no host read-back; capturable.  params is read by the launch: a table refilled in place
 * between two launches (or two replays of a captured one) is honoured.
 * MBPO_ERR_ARG before any device use: an unknown kind, n_steps < 1, n_problems < 1, group < 0, x_dim < 1, u_dim < 1, param_problems not
 * in {1, n_problems}, param_steps not in {1, n_steps}, param_len smaller than the kind reads, the Pendulum kind at other widths than
 * 3 / 1, x_dim + u_dim > next_off, next_off + x_dim > row_len, out_stride < 1, an index product (n_steps * n_problems * group * row_len
 * or * out_stride, param_problems * param_steps * param_len) that overflows int64, more than (2^31 - 1) * 256 rows, or with group > 0
 * a NULL params, rows or out.  group == 0: MBPO_OK, nothing is launched. */
int mbpo_plan_reward_eval(int32_t reward_kind, const float *params, int32_t param_problems, int32_t param_steps, int32_t param_len,
                          const float *rows, int32_t row_len, int32_t next_off, int32_t n_steps, int32_t n_problems, int64_t group,
                          int32_t x_dim, int32_t u_dim, float *out, int64_t out_stride, void *stream);

/* ---- terminal values: a learned critic at the end of the planned horizon, evaluated on the rollout's rows ------------------------------
 * replaces: nothing in the reference tree, whose iCEM objective is the sum of the horizon's rewards and nothing else.  Build-defined
 *           (mbpo.optimizers.TerminalValue): THIS TEXT IS THE DEFINITION.
 * For row i, x(i) = x + i * x_stride is a state of x_dim floats (iCEM: the next-state columns of trajectory i's last-step row, x_stride =
 * row_len).  With n(x) = (x - norm_mean) / norm_std, a true division, or n(x) = x when both pointers are NULL:
 *   kind V (action_dim == 0)  v(i) = min_k V_k(n(x(i))), k < critic.n_nets in {1, 2}; networks [x_dim] -> [1] (BPTT's twin target critic;
 *                             PPO's value network with one net)
 *   kind Q (action_dim  > 0)  a = tanh(loc(policy(n(x)))), loc the first action_dim of the policy's 2 action_dim outputs (the mode of
 *                             SAC's NormalTanh policy), tanhf the accurate one;  v(i) = min(Q_1, Q_2)([n(x) | a]); critic.n_nets == 2,
 *                             networks [x_dim + action_dim] -> [1].  action_dim is the policy's action width: on an optimistic system
 *                             u_dim + x_dim, the critics having been trained on [u | eta].
 *   bonus(i) = fl(weight * v(i))                                   the product rounded on its own (__fmul_rn)
 *   out[i * out_stride] = bonus(i)                                 accumulate 0
 *                       = fl(out[i * out_stride] + bonus(i))       accumulate 1: the sum rounded on its own (__fadd_rn)
 *                       = -inf                                     either mode, where a component of x(i) is not finite: a store, not an
 *                                                                  add, so a diverged trajectory ranks below every finite one and carries
 *                                                                  no NaN into a ranking; the other rows of its tile keep their bits
 * The minimum is torch.minimum's (a NaN wins).  There is no entropy term, no discounting and no reward un-scaling: weight is the caller's
 * (typically gamma^H / reward_scaling for SAC's critics, r_std * gamma^H for BPTT's normalised critic); a constant shift of v changes no
 * ranking and is not offered.  The value of a row depends on that row alone — not on n, its tile or its position.
 * In iCEM: one launch with accumulate 1 between the reward source and mbpo_icem_update*, x = rows + ((H - 1) n_traj) row_len + next_off,
 * x_stride = row_len, out = the last step's n_traj rewards of whichever source the update reads (the rows' reward column, out_stride =
 * row_len; a plan reward's dense buffer, out_stride = 1), n = n_traj: the objective becomes J_i = sum_{t<H} r_t(i) + bonus(i) (the update
 * ranks J_i / H, the reference's mean over steps).  Only those n_traj floats are touched; the update kernels are unchanged.
 * One workgroup per tile of 16 rows, persistent; each out element is written by exactly one thread (no atomics); x needs no alignment.
 * Nothing but out[i * out_stride], i < n, is written.  No workspace, no allocation, no host read-back; capturable.  The parameters and
 * the normaliser are read by the launch: tensors refreshed in place between two launches (or two replays) are honoured.
 * MBPO_ERR_ARG before any device use: x_dim < 1, action_dim < 0, n < 0, accumulate not 0 or 1, a network with bad sizes
 * (mbpo_mlp_desc's rules), critic.n_nets outside {1, 2} or kind Q with one critic, critic.dims[0] != x_dim + action_dim, a critic that
 * does not end in one output, kind Q with policy.n_nets != 1, policy.dims[0] != x_dim or a policy that does not end in 2 action_dim
 * outputs, exactly one of norm_mean / norm_std set, x_stride < x_dim, out_stride < 1, n * x_stride or n * out_stride overflowing
 * int64, or with n > 0 a NULL critic.params, policy.params (kind Q), x or out.  MBPO_ERR_UNSUPPORTED (the message says so by name):
 * hidden layers of a network that do not share one width in {64, 128, 256} (what the wave chains take, as mbpo_ensemble_mlp_forward's
 * generic kernel), action_dim > 64, or shapes whose tiles do not fit the LDS.  Policy and critics may differ in width; the kernel is
 * built for the larger one.  n == 0: MBPO_OK, nothing is launched. */
typedef struct mbpo_terminal_value_desc {
  int32_t x_dim, action_dim;            /* action_dim == 0: kind V */
  mbpo_mlp_desc critic;                 /* n_nets 1 or 2 (kind Q: 2); [x_dim + action_dim] -> [1] */
  mbpo_mlp_desc policy;                 /* kind Q: [x_dim] -> [2*action_dim]; ignored for kind V */
  const float *norm_mean, *norm_std;    /* [x_dim], both or neither */
  const float *x;  int64_t x_stride;    /* terminal state of row i at x + i*x_stride (floats); no alignment assumed */
  float *out;      int64_t out_stride;  /* out[i*out_stride] */
  int64_t n;  float weight;  int32_t accumulate;   /* 1: out += bonus, 0: out = bonus */
} mbpo_terminal_value_desc;
int mbpo_terminal_value_eval(const mbpo_terminal_value_desc *d, void *stream);

/* ---- policy priors: a learned policy's closed-loop action sequences among iCEM's candidates -------------------------------------------
 * replaces: nothing in the reference tree, whose iCEM samples every candidate around (mean, std).  Build-defined
 *           (mbpo.optimizers.PolicyPrior; TD-MPC's policy trajectories among the CEM samples, LOOP's actor prior): THIS TEXT IS THE DEFINITION.
 * Proposals.  Once per `optimize`, before the first iteration, the policy is rolled closed-loop through the model: for every problem b, K
 * proposals of H steps from x0[b],
 *   a_t = squash(loc(pi(n(x_t))) + noise_scale * scale * eps)          the rollout kernels' own NormalTanh path (tanh, optional action_clip,
 *                                                                      the trainer's normaliser n), through ONE mbpo_model_rollout over
 *                                                                      B K envs with a policy and an explicit policy_noise; no new rollout
 *                                                                      kernel, whichever kernel the dispatch picks for the descriptor
 * under the system's descriptor without termination and with episode_length = 2^30, as iCEM's candidate rollouts run.  A stochastic
 * ensemble (ts1 / tsinf, or sample_noise) runs its proposals in MBPO_ENS_MEAN without model noise: proposals are action sequences, their
 * only randomness is the policy's.  The optimistic mode already is ENS_MEAN plus halluc_beta and runs unchanged at action width u + x.  A
 * plan reward is taken out of the parameters as for the candidate rollouts; the proposal rollout's reward column is never read.
 *   eps [H][B K][A] = mbpo_philox_fill_grouped(seeds = prior_key[b], offset 0, MBPO_STREAM_POLICY_NOISE, n_steps H, n_problems B,
 *                     group K A), times noise_scale where that is not 1; with include_mode, eps of proposal k = 0 is zeroed: the policy's
 *                     mode sequence.  prior_key = split(optimizer_key, 3)[2]; split(k, 3)[:2] == split(k, 2), so the key chain of a run
 *                     without a prior, and every number it draws, is untouched.  The single path is the same call with n_problems = 1:
 *                     problem b of a batched call equals its single call by construction.
 * Seeding.  In iteration it (every iteration, TD-MPC's scheme; or only it = 0), after mbpo_icem_sample[_batched] and before the candidate
 * rollout, one launch of mbpo_icem_seed_candidates overwrites the sampled slots [0, K) of every problem with the clipped proposals; with
 * init_mean (LOOP's scheme) a launch before the first sample launch writes the clipped proposal 0 into mean[b] in place of the warm start.
 *   p(b, k, t, a) = src[t * src_step_stride + (b * n_seed + k) * src_traj_stride + a]      k < n_seed = K, t < horizon = H, a < u_dim = A
 *                   (iCEM: src = proposal rows + x_dim, src_traj_stride = row_len, src_step_stride = B K row_len — the action columns of
 *                   the step-major rows mbpo_model_rollout wrote; no dense copy in between)
 *   v             = fminf(fmaxf(p, u_min[a]), u_max[a])                                    mbpo_icem_sample's clip expression
 *   finite(b, k)  = every one of the H A elements p(b, k, ., .) is finite (neither NaN nor an infinity)
 * Where finite(b, k), with NC = n_candidates, P = n_particles, B = n_problems, and only when actions / candidates are set:
 *   candidates[((b NC + k) H + t) A + a]               = v
 *   actions[(t (B NC P) + (b NC + k) P + p) A + a]     = v     for every p < P   (the rollout's [H][B NC P][A] layout)
 * and, where mean != NULL, k == 0 and finite(b, 0):
 *   mean[(b H + t) A + a]                              = v
 * Nothing else is written: a proposal with a non-finite element (a diverged model state fed the policy a NaN) is DROPPED, not repaired —
 * its slot keeps the sampled candidate, mean[b] keeps the warm start — and the slots [n_seed, NC) keep their bits.  The Philox element
 * of a sampled slot does not depend on the other slots, so in iteration 0 the slots [K, num_samples) equal those of a run without a prior.
 * actions and candidates are both NULL (the mean-only call) or both set; at least one of (actions, mean) is set.  src must not overlap an
 * output.  No alignment is assumed anywhere (the rows' stride is odd).  One wave per (b, k): a wave-wide vote on "any element not
 * finite", then plain vector stores.  No workspace, no allocation, no atomics, no host read-back; capturable.  src and the bounds are
 * read by the launch: refilled in place between two launches (or two replays) they are honoured.
 * MBPO_ERR_ARG before any device use: n_problems < 1, n_seed < 1, n_seed > n_candidates, horizon < 1, u_dim < 1, n_particles < 1,
 * horizon * u_dim overflowing int32, a stride smaller than u_dim, strides under which steps and trajectories overlap — neither
 * src_step_stride >= (n_problems n_seed - 1) src_traj_stride + u_dim (step-major, iCEM's) nor src_traj_stride >= (horizon - 1)
 * src_step_stride + u_dim (trajectory-major) —, an index product (horizon * src_step_stride + n_problems * n_seed * src_traj_stride, horizon *
 * n_problems * n_candidates * n_particles * u_dim) that overflows int64, a NULL src, u_min or u_max, exactly one of actions / candidates
 * set, actions and mean both NULL, more than 2^31 - 1 workgroups of four proposals.  The grid is flat over (b, k): n_problems has no
 * bound of its own. */
int mbpo_icem_seed_candidates(const float *src, int64_t src_step_stride, int64_t src_traj_stride, int32_t n_problems, int32_t n_seed,
                              int32_t n_candidates, int32_t horizon, int32_t u_dim, int32_t n_particles, const float *u_min,
                              const float *u_max, float *actions, float *candidates, float *mean, void *stream);

/* ---- one-shot all-reduce over xGMI peer memory (multi-GPU SAC gradient exchange) ------------------------
 * replaces: the live form of the reference's jax.lax.pmean(grad) (sac/utils.py:29-33) for vectors small enough that a
 *           collective is pure latency.  Every rank owns an exchange REGION (mbpo_p2p_alloc -> 64-byte IPC handle, passed to
 *           the other ranks out of band, mbpo_p2p_open there); a producer kernel stores its vector into slot[rank] of every
 *           rank's region and publishes per-block arrival counts; the consumer waits for all ranks (bounded spin) and adds the
 *           slots in rank order, so every rank holds bit-identical sums.  Regions are zero-initialised by mbpo_p2p_alloc.
 * regions[r] : base of rank r's region as mapped in THIS process (regions[rank] is the own allocation);
 * n_max      : floats per slot the region was sized for (mbpo_p2p_region_bytes).
 * mbpo_p2p_all_reduce_sum: buf[0..n) <- sum over ranks, in place (3 small launches; every rank must call it the same number
 *   of times).  On a consumer timeout buf is filled with NaN and mbpo_p2p_status reports 1 — nothing hangs.
 */
#define MBPO_P2P_MAX_RANKS 16
typedef struct mbpo_p2p_desc {
  int32_t world, rank;
  int64_t n_max;
  void *regions[MBPO_P2P_MAX_RANKS];
} mbpo_p2p_desc;

int64_t mbpo_p2p_region_bytes(int32_t world, int64_t n_max);
int mbpo_p2p_alloc(int64_t bytes, void **ptr, void *handle64);
int mbpo_p2p_open(const void *handle64, int32_t peer_device, void **ptr);   /* peer_device < 0: same device */
int mbpo_p2p_close(void *ptr);
int mbpo_p2p_free(void *ptr);
int mbpo_p2p_all_reduce_sum(const mbpo_p2p_desc *d, float *buf, int64_t n, void *stream);
/* SAC sgd_step over N ranks without a collective launch:  mbpo_sac_grads_p2p (= mbpo_sac_grads whose reduction kernel also
 * stores the rank's gradient into every rank's exchange region)  ->  mbpo_sac_gather_p2p (waits for all ranks, grads <- sum
 * over ranks in rank order, clip-norm partials)  ->  mbpo_sac_apply (grad_scale = 1/N).  n_max >= NP. */
int mbpo_sac_grads_p2p(const mbpo_sac_desc *d, const mbpo_p2p_desc *x, void *stream);
int mbpo_sac_gather_p2p(const mbpo_sac_desc *d, const mbpo_p2p_desc *x, void *stream);
/* The same exchange in ONE reduction launch (= mbpo_sac_grads_p2p + mbpo_sac_gather_p2p): the reduction kernel stores the rank's
 * gradient into every region, waits inside the kernel for every rank's arrivals and leaves grads = sum over ranks and the
 * clip-norm partials.  Then mbpo_sac_apply (grad_scale = 1/N).  Needs the reduction's workgroups (NP/256) co-resident. */
int mbpo_sac_grads_exchange_p2p(const mbpo_sac_desc *d, const mbpo_p2p_desc *x, void *stream);
/* mbpo_sac_step over N ranks: the second launch also exchanges (stores the rank's gradient into every region, waits for every rank,
 * sums the world slots in rank order) before the unclipped optimizer step (grad_scale = 1/N); mbpo_sac_finalize as above. */
int mbpo_sac_step_p2p(const mbpo_sac_desc *d, const mbpo_p2p_desc *x, void *stream);
int mbpo_p2p_status(const mbpo_p2p_desc *d, int32_t *status_out);

#ifdef __cplusplus
}
#endif
#endif /* MBPO_HIP_H */
