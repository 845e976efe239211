// rollout.hip — R1-R8 fused model rollout (see include/mbpo_hip.h): the host half of mbpo_model_rollout, which validates the descriptor,
// plans the LDS block and picks one of four kernels, and the small kernels that need no tile (open-loop Pendulum, hold steps, reward
// evaluation).  The tile kernels live behind launch headers, in translation units of their own, so that they compile side by side:
//   rollout64.hpp      k_model_rollout64 (hidden width 64)          rollout64_kernel.hpp, rollout64.hip
//   rollout_wide.hpp   k_model_rollout<128 | 256>                   rollout_wide_kernel.hpp, rollout_wide_{formula,learned,terms}.hip
//   rollout_lean.hpp   k_rollout_lean (the benchmark networks)      rollout_lean.hip
// What the two tile kernels share is in rollout_tile.hpp; the ensemble forward (R2) is ens_forward.hpp, compiled with rollout64.hip.
#include "common.hpp"
#include "chain_run.hpp"
#include "rollout_shared.hpp"
#include "rollout_tile.hpp"
#include "rollout_lean.hpp"
#include "rollout64.hpp"
#include "rollout_wide.hpp"
#include "reward_terms.hpp"
#include <stdlib.h>
#include <string.h>

static unsigned long long *g_ro_stamps = nullptr;
// Diagnostic switch (not part of include/mbpo_hip.h): 0 the generic 64-wide rollout kernel, 1 the specialised one, 2 / 3 the specialised one
// with two tiles in flight per workgroup forced on / off, -1 = default.
extern "C" int mbpo_debug_set_rollout_lean(int mode) { return mbpo_knob_set_override(KNOB_ROLLOUT_LEAN, mode); }
extern "C" int mbpo_debug_set_rollout_stamps(void *buf) {
  g_ro_stamps = (unsigned long long *)buf;
  return MBPO_OK;
}

// Test hook (not part of include/mbpo_hip.h): which kernel mbpo_model_rollout launched last, as the launch sites recorded it
// (RolloutKernelId, rollout_shared.hpp) — out[0 .. 11) = {family, H, X, PEND, PIPE, LR, W, TM, SB, HL, TA}; family 0: none yet.
static RolloutKernelId g_ro_last = {RO_FAMILY_NONE, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
void rollout_note_kernel(const RolloutKernelId &id) { g_ro_last = id; }
extern "C" int mbpo_debug_last_rollout_kernel(int32_t *out, int32_t n) {
  MBPO_REQUIRE(out && n >= 11, MBPO_ERR_ARG, "debug_last_rollout_kernel: needs room for 11 ints");
  const int v[11] = {g_ro_last.family, g_ro_last.h, g_ro_last.x, g_ro_last.pend, g_ro_last.pipe, g_ro_last.lr,
                     g_ro_last.wide, g_ro_last.term, g_ro_last.start, g_ro_last.hal, g_ro_last.ta};
  for (int i = 0; i < 11; ++i) out[i] = v[i];
  return MBPO_OK;
}

// ------------------------------------------------------------------------------------------------
// Open-loop rollout of the analytic Pendulum system (rollout_actions, utils/optimizer_utils.py:26-38 — the iCEM planner's candidate
// evaluation, icem_optimizer.py:146-160): no network, so a 16-env tile on a 768-thread workgroup has 16 busy lanes per step (the
// tile kernels spent 130 us on 5500 envs x 20 steps).  Here one THREAD owns an env for all steps: the sections of k_model_rollout64 —
// reward on the pre-step (x, u), the step, EpisodeWrapper / AutoReset bookkeeping, the Transition row — with the same device functions
// in the same order: the same rows bit for bit (tests/test_gpu_icem.py).
// ------------------------------------------------------------------------------------------------
// START: a start buffer is set (a compile-time flag: the run-time test cost the plain kernel two registers)
template <bool START>
__global__ void __launch_bounds__(256) k_openloop_pendulum(RolloutArgs A) {
  const long long env = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long N = A.n_envs;
  if (env >= N) return;
  constexpr int X = 3, U = 1;
  const int D = A.row_len, AR = A.action_repeat;
  float o[3], f[3];
#pragma unroll
  for (int c = 0; c < X; ++c) {
    o[c] = A.obs[env * X + c];
    f[c] = A.first_obs[env * X + c];
  }
  float steps = A.steps[env], done = A.done[env];
  const float rp[3] = {A.reward_params[0], A.reward_params[1], A.reward_params[2]};
  // START (fresh starts, include/mbpo_hip.h): the key of the draw and the true buffer's {sample_position, insert_position, head}
  const RngKey rk = START ? rng_resolve(A.seed, A.offset, A.rng_dev) : RngKey{0ull, 0ull};
  const int sb_lo = START ? A.start.state[1] : 0, sb_hi = START ? A.start.state[0] : 0, sb_head = START ? A.start.state[2] : 0;
  for (int s = 0; s < A.n_steps; ++s) {
    float *row = A.transitions + (A.env_major ? (env * A.n_steps + s) : ((long long)s * N + env)) * D;
    const float a = A.actions[((long long)s * N + env) * U];
#pragma unroll
    for (int c = 0; c < X; ++c) row[c] = o[c];
    row[X] = a;
    if (done != 0.f) steps = 0.f;      // AutoReset pre-step (training.py:119-124)
    done = 0.f;
    float rew = 0.f;
    float xu[4] = {o[0], o[1], o[2], a};
    for (int ar = 0; ar < AR; ++ar) {   // EpisodeWrapper inner scan over action_repeat (training.py:91-97)
      rew += (A.reward_kind == MBPO_REWARD_PENDULUM) ? pendulum_reward(xu, a, rp) : 0.f;
      float xn[3];
      pendulum_step(xu, a, A.sys_params, xn);
      xu[0] = xn[0]; xu[1] = xn[1]; xu[2] = xn[2];
    }
    const float st = steps + (float)AR;
    const bool over = st >= (float)A.episode_length;
    const float sys_done = term_row_done(A, xu, X);      // SystemState.done: 0 (base_systems.py:25) or the termination box
    const bool dn = over || sys_done != 0.f;
#pragma unroll
    for (int c = 0; c < X; ++c) {
      const float v = dn ? f[c] : xu[c];
      o[c] = v;
      row[X + U + 2 + c] = v;          // next_observation = nstate.obs (post auto-reset)
    }
    if (START && dn) {                 // the reset consumed the start state: the env's next one
      const float *nf = A.start.rows + start_draw_row(A.start, sb_lo, sb_hi, sb_head, rk.seed, rk.offset, (long long)s * N + env);
#pragma unroll
      for (int c = 0; c < X; ++c) f[c] = nf[c];
    }
    row[X + U] = rew;
    row[X + U + 1] = 1.f - (dn ? 1.f : 0.f);
    row[D - 1] = over ? 1.f - sys_done : 0.f;      // truncation
    steps = st;
    done = dn ? 1.f : 0.f;
  }
#pragma unroll
  for (int c = 0; c < X; ++c) A.obs[env * X + c] = o[c];
  if (START) {
#pragma unroll
    for (int c = 0; c < X; ++c) A.first_obs[env * X + c] = f[c];
  }
  A.steps[env] = steps;
  A.done[env] = done;
}

// ------------------------------------------------------------------------------------------------
// mbpo_model_rollout, host half: validate the descriptor, plan the launch, dispatch it.
// ------------------------------------------------------------------------------------------------
// What the descriptor alone decides.
struct RolloutReq {
  RolloutArgs A;          // everything but the LDS geometry, which the plan fills
  HoldArgs hold;
  int H, E, dyn_out;      // the networks' common hidden width; member networks (0: the analytic Pendulum system) and their outputs
  int lr;                 // RO_LR_*
  bool has_policy;
  RolloutFlags f;         // (wide is the plan's: it reads the networks' shapes)
};

// Every check that reads only the descriptor, in the order callers and tests know (the first failing check decides the message), then the
// descriptor's fields into q->A.
static int rollout_validate(const mbpo_rollout_desc *d, RolloutReq *q) {
  MBPO_REQUIRE(d, MBPO_ERR_ARG, "model_rollout: null descriptor");
  MBPO_REQUIRE(d->x_dim > 0 && d->u_dim > 0, MBPO_ERR_ARG, "model_rollout: x_dim/u_dim must be positive");
  MBPO_REQUIRE(d->n_envs >= 0 && d->n_steps >= 0, MBPO_ERR_ARG, "model_rollout: negative n_envs/n_steps");
  MBPO_REQUIRE(d->episode_length > 0 && d->action_repeat > 0, MBPO_ERR_ARG,
               "model_rollout: episode_length and action_repeat must be positive");
  const bool empty = (d->n_envs == 0 || d->n_steps == 0);  // empty tensors carry NULL data pointers
  MBPO_REQUIRE(empty || (d->obs && d->first_obs && d->steps && d->done && d->transitions), MBPO_ERR_ARG,
               "model_rollout: null state/output pointer");
  MBPO_REQUIRE((d->norm_mean == nullptr) == (d->norm_std == nullptr), MBPO_ERR_ARG,
               "model_rollout: norm_mean and norm_std must both be set or both NULL");
  MBPO_REQUIRE((d->term_low == nullptr) == (d->term_high == nullptr), MBPO_ERR_ARG,
               "model_rollout: term_low and term_high must both be set or both NULL");
  MBPO_REQUIRE(d->reward_params || d->reward_kind == MBPO_REWARD_LEARNED, MBPO_ERR_ARG, "model_rollout: reward_params is NULL");
  const int X = d->x_dim, U = d->u_dim;
  // hallucinated control: the action is [u (UE) | eta (x_dim)], the dynamics and the rewards see the UE leading columns
  const bool hal = d->halluc_beta != nullptr;
  MBPO_REQUIRE(!hal || d->system_kind == MBPO_SYS_ENSEMBLE, MBPO_ERR_ARG, "model_rollout: halluc_beta needs system_kind ENSEMBLE");
  MBPO_REQUIRE(!hal || d->ens_mode == MBPO_ENS_MEAN, MBPO_ERR_ARG, "model_rollout: halluc_beta needs ens_mode MEAN");
  MBPO_REQUIRE(!hal || U > X, MBPO_ERR_ARG, "model_rollout: halluc_beta needs u_dim > x_dim (the action is [u | eta], eta [x_dim]); got u_dim %d, x_dim %d", U, X);
  // time-adaptive: the action is [u (UE) | tau], the dynamics and the rewards see the UE leading columns
  const bool ta = d->hold_max_steps != 0;
  if (ta) {
    MBPO_REQUIRE(d->hold_max_steps >= 1 && d->hold_max_steps <= 64, MBPO_ERR_ARG, "model_rollout: hold_max_steps %d outside [1, 64]", d->hold_max_steps);
    MBPO_REQUIRE(d->action_repeat == 1, MBPO_ERR_ARG, "model_rollout: hold_max_steps needs action_repeat 1 (the hold is the repeat); got %d", d->action_repeat);
    MBPO_REQUIRE(!hal, MBPO_ERR_ARG, "model_rollout: hold_max_steps and halluc_beta cannot both be set");
    MBPO_REQUIRE(U >= 2, MBPO_ERR_ARG, "model_rollout: hold_max_steps needs u_dim >= 2 (the action is [u | tau]); got u_dim %d", U);
    MBPO_REQUIRE(d->hold_dt > 0.f, MBPO_ERR_ARG, "model_rollout: hold_dt must be positive");
    MBPO_REQUIRE(d->hold_min_time <= d->hold_max_time, MBPO_ERR_ARG, "model_rollout: hold_min_time > hold_max_time");
    MBPO_REQUIRE(d->hold_gamma > 0.f && d->hold_gamma <= 1.f, MBPO_ERR_ARG, "model_rollout: hold_gamma outside (0, 1]");
    MBPO_REQUIRE(d->hold_switch_cost >= 0.f, MBPO_ERR_ARG, "model_rollout: hold_switch_cost is negative");
  }
  const int UE = hal ? U - X : (ta ? U - 1 : U);
  int rc = mbpo_check_start_buffer(d->start_rows, d->start_max_size, d->start_row_len, d->start_state, X, "model_rollout");
  if (rc != MBPO_OK) return rc;
  const int want_row = 2 * X + U + 3 + (d->ppo_extras ? 1 + U : 0);
  MBPO_REQUIRE(d->row_len == want_row, MBPO_ERR_ARG, "model_rollout: row_len %d != expected %d", d->row_len, want_row);
  MBPO_REQUIRE(d->reward_kind == MBPO_REWARD_PENDULUM || d->reward_kind == MBPO_REWARD_QUADRATIC || d->reward_kind == MBPO_REWARD_LEARNED ||
                   d->reward_kind == MBPO_REWARD_TERMS,
               MBPO_ERR_ARG, "model_rollout: unknown reward_kind %d", d->reward_kind);
  MBPO_REQUIRE(d->reward_kind != MBPO_REWARD_TERMS || d->system_kind == MBPO_SYS_ENSEMBLE, MBPO_ERR_ARG,
               "model_rollout: the term reward needs system_kind ENSEMBLE");
  MBPO_REQUIRE(d->reward_kind != MBPO_REWARD_LEARNED || d->system_kind == MBPO_SYS_ENSEMBLE, MBPO_ERR_ARG,
               "model_rollout: the learned reward needs system_kind ENSEMBLE");
  MBPO_REQUIRE(d->reward_kind != MBPO_REWARD_PENDULUM || (X == 3 && UE == 1), MBPO_ERR_ARG,
               "model_rollout: pendulum reward needs x_dim=3,u_dim=1 (with halluc_beta: u_dim = 1 + x_dim; with hold_max_steps: u_dim = 2)");
  RolloutArgs &A = q->A;
  int H = 64;
  const bool has_policy = (d->actions == nullptr);
  MBPO_REQUIRE(has_policy || !d->ppo_extras, MBPO_ERR_ARG, "model_rollout: ppo_extras needs a policy (actions must be NULL)");
  if (has_policy) {
    rc = mbpo_make_mlp_dev(&d->policy, &A.policy, "model_rollout.policy");
    if (rc != MBPO_OK) return rc;
    MBPO_REQUIRE(A.policy.n_nets == 1, MBPO_ERR_ARG, "model_rollout: policy.n_nets must be 1");
    MBPO_REQUIRE(A.policy.dims[0] == X && A.policy.dims[A.policy.n_layers] == 2 * U, MBPO_ERR_ARG,
                 "model_rollout: policy must map [x_dim] -> [2*u_dim]");
    H = hidden_width(A.policy);
  }
  int E = 0;
  int dyn_out = 0;
  if (d->system_kind == MBPO_SYS_ENSEMBLE) {
    rc = mbpo_make_mlp_dev(&d->dynamics, &A.dyn, "model_rollout.dynamics");
    if (rc != MBPO_OK) return rc;
    E = A.dyn.n_nets;
    dyn_out = A.dyn.dims[A.dyn.n_layers];
    MBPO_REQUIRE(hal || ta || A.dyn.dims[0] == X + U, MBPO_ERR_ARG, "model_rollout: dynamics input must be x_dim+u_dim");
    MBPO_REQUIRE(!ta || A.dyn.dims[0] == X + U - 1, MBPO_ERR_ARG,
                 "model_rollout: with hold_max_steps the dynamics input must be x_dim + u_dim - 1 (the dynamics read [x, u] only); got %d, x_dim %d, u_dim %d",
                 A.dyn.dims[0], X, U);
    MBPO_REQUIRE(!hal || A.dyn.dims[0] == U, MBPO_ERR_ARG,
                 "model_rollout: with halluc_beta the dynamics input must be u_dim = x_dim + the control width (the dynamics read [x, u] only); got %d, u_dim %d",
                 A.dyn.dims[0], U);
    MBPO_REQUIRE(dyn_out == 2 * X || dyn_out == 2 * X + 2 || (dyn_out == X && !(d->ens_sample_noise && d->ens_mode != MBPO_ENS_MEAN)),
                 MBPO_ERR_ARG, "model_rollout: dynamics output must be 2*x_dim (mean, raw std), 2*x_dim+2 (+ reward mean, raw std) or "
                 "x_dim (mean only, no sampling)");
    MBPO_REQUIRE(d->reward_kind != MBPO_REWARD_LEARNED || dyn_out == 2 * X + 2, MBPO_ERR_ARG,
                 "model_rollout: the learned reward needs dynamics output 2*x_dim+2 (got %d)", dyn_out);
    MBPO_REQUIRE(d->ens_mode >= 0 && d->ens_mode <= 2, MBPO_ERR_ARG, "model_rollout: unknown ens_mode");
    int Hd = hidden_width(A.dyn);
    if (!has_policy || A.policy.n_layers == 1) H = Hd;
    MBPO_REQUIRE(Hd == H || A.dyn.n_layers == 1, MBPO_ERR_UNSUPPORTED,
                 "model_rollout: policy and dynamics hidden widths must match (got %d vs %d)", H, Hd);
  } else if (d->system_kind == MBPO_SYS_PENDULUM) {
    MBPO_REQUIRE(X == 3 && UE == 1, MBPO_ERR_ARG, "model_rollout: pendulum system needs x_dim=3,u_dim=1 (with hold_max_steps: u_dim = 2)");
    MBPO_REQUIRE(d->sys_params, MBPO_ERR_ARG, "model_rollout: sys_params is NULL");
    memset(&A.dyn, 0, sizeof(A.dyn));  // unused
  } else {
    MBPO_REQUIRE(false, MBPO_ERR_ARG, "model_rollout: unknown system_kind %d", d->system_kind);
  }
  MBPO_REQUIRE(H == 64 || H == 128 || H == 256, MBPO_ERR_UNSUPPORTED,
               "model_rollout: hidden layers must share one width in {64,128,256}");

  A.x_dim = X; A.u_dim = U; A.n_envs = d->n_envs; A.n_steps = d->n_steps;
  A.episode_length = d->episode_length;
  A.action_repeat = ta ? d->hold_max_steps : d->action_repeat;      // TA: K, the stride of the inner-step element indices
  A.system_kind = d->system_kind; A.ens_mode = d->ens_mode; A.ens_predict_delta = d->ens_predict_delta;
  A.ens_sample_noise = d->ens_sample_noise; A.ens_min_std = d->ens_min_std;
  A.reward_kind = d->reward_kind; A.reward_params = d->reward_params; A.sys_params = d->sys_params;
  A.norm_mean = d->norm_mean; A.norm_std = d->norm_std;
  A.deterministic = d->deterministic; A.ppo_extras = d->ppo_extras; A.env_major = d->env_major;
  A.actions = d->actions;
  A.action_clip = d->action_clip;
  if (!has_policy) memset(&A.policy, 0, sizeof(A.policy));
  A.policy_noise = d->policy_noise; A.model_noise = d->model_noise; A.member_idx = d->member_idx;
  A.seed = d->seed; A.offset = d->offset; A.rng_dev = (const unsigned long long *)d->rng_dev;
  A.obs = d->obs; A.first_obs = d->first_obs; A.steps = d->steps; A.done = d->done;
  A.transitions = d->transitions; A.row_len = d->row_len;
  A.term_low = d->term_low; A.term_high = d->term_high;
  A.start = StartBuf{d->start_rows, (long long)d->start_max_size, d->start_row_len, d->start_state};
  q->hold = HoldArgs{d->hold_max_steps, d->hold_min_time, d->hold_max_time, d->hold_dt, d->hold_gamma, d->hold_switch_cost};
  q->H = H; q->E = E; q->dyn_out = dyn_out; q->has_policy = has_policy;
  q->lr = d->reward_kind == MBPO_REWARD_TERMS ? RO_LR_TERMS : (d->reward_kind == MBPO_REWARD_LEARNED ? RO_LR_LEARNED : RO_LR_FORMULA);
  q->f = RolloutFlags{false, A.term_low != nullptr, A.start.rows != nullptr, hal, ta};
  return MBPO_OK;
}

enum RolloutPath { RO_PATH_OPENLOOP, RO_PATH_LEAN, RO_PATH_64, RO_PATH_WIDE };
struct RolloutPlan {
  RolloutPath path;
  size_t lds;
  int grid, block;        // of the tile kernels (the other two paths size their own launches)
  long long n_tiles;
  RolloutArgs64 AA;       // RO_PATH_64
};

// The LDS geometry into q->A, the block's size, the grid, and which kernel runs.
static int rollout_plan(const mbpo_rollout_desc *d, RolloutReq *q, RolloutPlan *pl) {
  RolloutArgs &A = q->A;
  const int X = A.x_dim, U = A.u_dim, E = q->E;
  A.n_out = E > 1 ? E : 1;
  A.ld_x = up4(X) + 4;
  A.ld_xu = up4(X + U) + 4;
  A.ld_h = q->H + 4;
  int ymax = 2 * U > q->dyn_out ? 2 * U : q->dyn_out;
  A.ld_y = up4(ymax) + 4;
  // One size for both tile kernels, k_model_rollout64's: two row buffers and its tail (rollout_tile.hpp), and 16 floats that nothing
  // uses, kept so that the block, and with it pick_chains' answer, is what it has always been.
  const bool terms = q->lr == RO_LR_TERMS;
  const size_t fixed_f = rollout_head_floats(A.ld_x, A.ld_xu, A.ld_y, A.n_out, d->row_len, 2) + rollout64_tail(X, U, q->f.ta, terms).end + 16;
  // k_model_rollout has one row buffer and a shorter tail: it fits inside the same block
  MBPO_REQUIRE(rollout_head_floats(A.ld_x, A.ld_xu, A.ld_y, A.n_out, d->row_len, 1) + rollout_wide_tail(X, terms).end <= fixed_f, MBPO_ERR_UNSUPPORTED,
               "model_rollout: k_model_rollout's LDS tail does not fit the block sized for k_model_rollout64");
  A.n_chains = pick_chains(E, fixed_f, A.ld_h);
  MBPO_REQUIRE(A.n_chains >= 1, MBPO_ERR_UNSUPPORTED, "model_rollout: shapes do not fit 160 KiB of LDS");
  pl->lds = (fixed_f + 2ull * A.n_chains * 16 * A.ld_h) * sizeof(float);
  const int n_waves = A.n_chains > 4 ? A.n_chains : 4;  // the policy chain is shared by waves 0..3
  pl->block = n_waves * 64;
  pl->n_tiles = (d->n_envs + 15) >> 4;
  pl->grid = (int)(pl->n_tiles < 4LL * mbpo_num_cus() ? pl->n_tiles : 4LL * mbpo_num_cus());
  if (!q->f.ta && !q->has_policy && d->system_kind == MBPO_SYS_PENDULUM && d->reward_kind == MBPO_REWARD_PENDULUM && !d->ppo_extras &&
      mbpo_knob_override(KNOB_ROLLOUT_LEAN) != 0) {      // (mbpo_debug_set_rollout_lean(0), not the environment: the tile kernel, for the A/B test)
    pl->path = RO_PATH_OPENLOOP;
    return MBPO_OK;
  }
  if (q->H != 64) {
    pl->path = RO_PATH_WIDE;
    return MBPO_OK;
  }
  // the kernel specialised for the benchmark networks (rollout_lean.hip): MBPO_ROLLOUT_LEAN=0 / mbpo_debug_set_rollout_lean(0) keep the
  // generic one
  // (k_rollout_lean never sees hallucinated control: rollout_lean_supports refuses u_dim != 1, and halluc_beta needs u_dim > x_dim)
  // (nor a time-adaptive one: hold_max_steps needs u_dim >= 2)
  if (mbpo_knob(KNOB_ROLLOUT_LEAN) != 0 && !q->f.ta && rollout_lean_supports(A, q->has_policy, E)) {
    pl->path = RO_PATH_LEAN;
    return MBPO_OK;
  }
  pl->path = RO_PATH_64;
  RolloutArgs64 &AA = pl->AA;
  AA.a = A;
  AA.stamps = g_ro_stamps;
  if (q->has_policy) AA.sh_pi = net_shape(A.policy);
  else AA.sh_pi = NetShape{X, 0, 2 * U, 0};
  if (E > 0) AA.sh_dyn = net_shape(A.dyn);
  else AA.sh_dyn = NetShape{X + U, 0, X, 0};
  if (AA.a.n_chains > RO64_WAVES / 2) AA.a.n_chains = RO64_WAVES / 2;   // member chains of 2 waves side by side
  if (AA.a.n_chains < 1) AA.a.n_chains = 1;
  pl->lds = (fixed_f + 2ull * (AA.a.n_chains > 1 ? AA.a.n_chains : 1) * 16 * A.ld_h) * sizeof(float);
  pl->block = 64 * RO64_WAVES;
  q->f.wide = net_is_wide(AA.sh_pi) || net_is_wide(AA.sh_dyn);
  return MBPO_OK;
}

// One call per path.
static int rollout_dispatch(const mbpo_rollout_desc *d, const RolloutReq &q, const RolloutPlan &pl, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  const RolloutArgs &A = q.A;
  switch (pl.path) {
  case RO_PATH_OPENLOOP: {
    const dim3 ogrid((unsigned)((d->n_envs + 255) / 256));
    rollout_note_kernel({RO_FAMILY_OPENLOOP, 0, 3, 1, 0, 0, 0, A.term_low != nullptr, A.start.rows != nullptr, 0, 0});
    if (A.start.rows) hipLaunchKernelGGL(k_openloop_pendulum<true>, ogrid, dim3(256), 0, st, A);
    else hipLaunchKernelGGL(k_openloop_pendulum<false>, ogrid, dim3(256), 0, st, A);
    return MBPO_OK;
  }
  case RO_PATH_LEAN: {
    const int lean_mode = (int)mbpo_knob(KNOB_ROLLOUT_LEAN);      // 1 lean, 2 lean + two tiles in flight forced, 3 lean without
    RoLeanArgs L;
    L.a = A;
    L.E = q.E;
    L.n_dyn_out = q.dyn_out;
    L.stamps = g_ro_stamps;
    // two tiles in flight per workgroup once every CU has at least two (MBPO_ROLLOUT_PIPE=0/1 forces it off / on)
    const int pipe_force = lean_mode == 2 ? 1 : (lean_mode == 3 ? 0 : (int)mbpo_knob(KNOB_ROLLOUT_PIPE));
    const bool pipe = q.E > 0 && (pipe_force >= 0 ? pipe_force != 0 : pl.n_tiles >= 2LL * mbpo_num_cus());
    const long long units = pipe ? (pl.n_tiles + 1) / 2 : pl.n_tiles;
    const int lgrid = (int)(units < (long long)mbpo_num_cus() ? units : (long long)mbpo_num_cus());
    return rollout_lean_launch(L, lgrid, pipe, stream);
  }
  case RO_PATH_64:
    return rollout64_launch(q.lr, q.f, pl.AA, d->halluc_beta, &q.hold, pl.grid, pl.block, pl.lds, st);
  case RO_PATH_WIDE:
    if (q.lr == RO_LR_TERMS) return rollout_wide_launch_terms(q.H, q.f, A, d->halluc_beta, &q.hold, pl.grid, pl.block, pl.lds, st);
    if (q.lr == RO_LR_LEARNED) return rollout_wide_launch_learned(q.H, q.f, A, d->halluc_beta, &q.hold, pl.grid, pl.block, pl.lds, st);
    return rollout_wide_launch_formula(q.H, q.f, A, d->halluc_beta, &q.hold, pl.grid, pl.block, pl.lds, st);
  }
  return MBPO_OK;
}

extern "C" int mbpo_model_rollout(const mbpo_rollout_desc *d, void *stream) {
  RolloutReq q;
  int rc = rollout_validate(d, &q);
  if (rc != MBPO_OK) return rc;
  if (d->n_envs == 0 || d->n_steps == 0) return MBPO_OK;
  RolloutPlan pl;
  rc = rollout_plan(d, &q, &pl);
  if (rc != MBPO_OK) return rc;
  rc = rollout_dispatch(d, q, pl, stream);
  if (rc != MBPO_OK) return rc;
  MBPO_CHECK_LAUNCH("model_rollout");
  return MBPO_OK;
}

// ------------------------------------------------------------------------------------------------
// mbpo_hold_steps: the k of a time-adaptive rollout (hold_steps, common.hpp) for n actions, one thread per row — for host code that
// applies an action to the true system for as long as the model held it.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_hold_steps(const float *actions, long long n, int A, float tl, float tu, float dt, int K, int *out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = hold_steps(actions[i * A + A - 1], tl, tu, dt, K);
}

extern "C" int mbpo_hold_steps(const float *actions, int64_t n, int32_t action_dim, float min_time, float max_time, float env_dt,
                               int32_t max_steps, int32_t *steps_out, void *stream) {
  MBPO_REQUIRE(n >= 0, MBPO_ERR_ARG, "hold_steps: n < 0");
  MBPO_REQUIRE(action_dim >= 1, MBPO_ERR_ARG, "hold_steps: action_dim must be positive");
  MBPO_REQUIRE(env_dt > 0.f, MBPO_ERR_ARG, "hold_steps: env_dt must be positive");
  MBPO_REQUIRE(min_time <= max_time, MBPO_ERR_ARG, "hold_steps: min_time > max_time");
  MBPO_REQUIRE(max_steps >= 1 && max_steps <= 64, MBPO_ERR_ARG, "hold_steps: max_steps %d outside [1, 64]", max_steps);
  if (n == 0) return MBPO_OK;
  MBPO_REQUIRE(actions && steps_out, MBPO_ERR_ARG, "hold_steps: null pointer");
  MBPO_REQUIRE(n <= 256LL * 2147483647LL, MBPO_ERR_ARG, "hold_steps: n too large");
  hipLaunchKernelGGL(k_hold_steps, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, actions, (long long)n, action_dim, min_time,
                     max_time, env_dt, max_steps, steps_out);
  MBPO_CHECK_LAUNCH("hold_steps");
  return MBPO_OK;
}

// ------------------------------------------------------------------------------------------------
// mbpo_reward_eval: the reward of n rows as the rollout kernels form it, one thread per row — the term table through the kernels' own
// reward_terms_eval (read from global memory: every lane of a wave walks the same records), the quadratic reward in section C's
// expressions.  For Reward.__call__ on the host side and for the tests that pin the rollouts' reward column bit for bit.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_reward_eval(int kind, const float *rp, const float *x, const float *u, const float *x_next, long long n,
                                                     int X, int U, float *out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float *xr = x + i * X, *ur = u + i * U;
  if (kind == MBPO_REWARD_TERMS) {
    out[i] = reward_terms_eval(rp, xr, ur, reward_terms_next(x_next ? x_next + i * X : nullptr, xr, X), X, U);
  } else {
    const float *tp = rp, *qp = tp + X, *rr = qp + X;
    float cx = 0.f, cu = 0.f;
    for (int c = 0; c < X; ++c) { float dd = xr[c] - tp[c]; cx += qp[c] * (dd * dd); }
    for (int d = 0; d < U; ++d) { float uu = ur[d]; cu += rr[d] * (uu * uu); }
    out[i] = -cx - cu;
  }
}

extern "C" int mbpo_reward_eval(int32_t reward_kind, const float *reward_params, const float *x, const float *u, const float *x_next, int64_t n,
                                int32_t x_dim, int32_t u_dim, float *out, void *stream) {
  MBPO_REQUIRE(reward_kind == MBPO_REWARD_TERMS || reward_kind == MBPO_REWARD_QUADRATIC, MBPO_ERR_UNSUPPORTED,
               "reward_eval: reward_kind %d is not evaluated here (MBPO_REWARD_TERMS and MBPO_REWARD_QUADRATIC are)", reward_kind);
  MBPO_REQUIRE(n >= 0, MBPO_ERR_ARG, "reward_eval: n < 0");
  MBPO_REQUIRE(x_dim >= 1 && u_dim >= 1, MBPO_ERR_ARG, "reward_eval: x_dim and u_dim must be positive");
  if (n == 0) return MBPO_OK;
  MBPO_REQUIRE(reward_params && x && u && out, MBPO_ERR_ARG, "reward_eval: null pointer");
  MBPO_REQUIRE(n <= 256LL * 2147483647LL, MBPO_ERR_ARG, "reward_eval: n too large");
  hipLaunchKernelGGL(k_reward_eval, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (int)reward_kind, reward_params, x, u,
                     x_next, (long long)n, (int)x_dim, (int)u_dim, out);
  MBPO_CHECK_LAUNCH("reward_eval");
  return MBPO_OK;
}
