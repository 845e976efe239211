// rollout_shared.hpp — what the rollout kernels share (csrc/rollout64_kernel.hpp, csrc/rollout_wide_kernel.hpp and csrc/rollout.hip: the
// generic kernels; csrc/rollout_lean.hip: the kernel specialised for the benchmark networks): the argument block, the analytic Pendulum
// step / reward, the hardware-transcendental helpers, the host's plan helpers.
#pragma once
#include "common.hpp"

// The true buffer a reset draws its next start state from (mbpo_rollout_desc.start_*): the ring of mbpo_replay_insert.
struct StartBuf {
  const float *rows;       // [max_size][row_len], the start state in columns 0 .. x_dim
  long long max_size;
  int row_len;
  const int *state;        // {insert_position, sample_position, head, ...}
};

// host: the start_* fields of a descriptor — all zero (off), or a well-formed ring whose rows hold at least x_dim columns
static inline int mbpo_check_start_buffer(const float *rows, long long max_size, int row_len, const int *state, int x_dim, const char *who) {
  if (!rows && !state && max_size == 0 && row_len == 0) return MBPO_OK;
  MBPO_REQUIRE(rows && state, MBPO_ERR_ARG, "%s: start_rows and start_state must both be set or both NULL", who);
  MBPO_REQUIRE(row_len >= x_dim, MBPO_ERR_ARG, "%s: start_row_len %d < x_dim %d", who, row_len, x_dim);
  MBPO_REQUIRE(max_size > 0 && max_size < 2147483647LL, MBPO_ERR_ARG, "%s: start_max_size outside (0, 2^31 - 1)", who);
  return MBPO_OK;
}

// host: plan helpers of the generic tile kernels (the rollouts and the ensemble forward, ens_forward.hip)
static inline int hidden_width(const MlpDev &m) {
  // all hidden layers must share one width H in {64,128,256}; a 1-layer MLP (no hidden) uses the 64 build.
  if (m.n_layers == 1) return 64;
  int H = m.dims[1];
  for (int l = 2; l < m.n_layers; ++l)
    if (m.dims[l] != H) return -1;
  return H;
}

// how many chains (waves) a workgroup runs side by side: one per member, capped at 8 waves (512 threads: two waves per
// SIMD keep 256 VGPRs each) and by the LDS that the per-chain ping-pong tiles need next to `fixed_floats` of other
// buffers; larger ensembles run in rounds of n_chains members
static inline int pick_chains(int n_members, size_t fixed_floats, int ld_h) {
  int c = n_members < 1 ? 1 : (n_members > 8 ? 8 : n_members);
  while (c >= 1 && (fixed_floats + 2ull * c * 16 * ld_h) * sizeof(float) > 160 * 1024) --c;
  return c;
}

struct RolloutArgs {
  MlpDev policy, dyn;
  int x_dim, u_dim;
  long long n_envs;
  int n_steps, episode_length, action_repeat;
  int system_kind, ens_mode, ens_predict_delta, ens_sample_noise;
  float ens_min_std;
  int reward_kind;
  const float *reward_params, *sys_params, *norm_mean, *norm_std;
  int deterministic, ppo_extras, env_major;
  float action_clip;
  const float *actions;
  const float *policy_noise, *model_noise;
  const int *member_idx;
  unsigned long long seed, offset;
  const unsigned long long *rng_dev;
  float *obs;
  float *first_obs;                       // in/out with a start buffer (written back at the end of the launch), read-only without
  float *steps, *done;
  float *transitions;
  int row_len;
  // LDS geometry
  int ld_x, ld_xu, ld_h, ld_y, n_chains, n_out;
  const float *term_low, *term_high;      // [x_dim] each, or both NULL: no termination
  StartBuf start;                         // rows == NULL: no start buffer (first_obs stays what the caller set)
};

// Which kernel mbpo_model_rollout launched last, for the tests (mbpo_debug_last_rollout_kernel, rollout.hip): every launch site stores the
// template arguments it instantiates the kernel with, next to its mbpo_launch.  Host only; a field a family does not have is 0.
#define RO_FAMILY_NONE 0
#define RO_FAMILY_64 1          // k_model_rollout64
#define RO_FAMILY_WIDE 2        // k_model_rollout<128 | 256> (term: the run-time box flag)
#define RO_FAMILY_LEAN 3        // k_rollout_lean
#define RO_FAMILY_OPENLOOP 4    // k_openloop_pendulum
struct RolloutKernelId {
  int family, h, x, pend, pipe, lr, wide, term, start, hal, ta;
};
void rollout_note_kernel(const RolloutKernelId &id);

// Fresh starts (include/mbpo_hip.h): the physical row of the true buffer that env `env` takes as its next start state after a reset at
// the launch's step s: idx = randint(sample_position, insert_position) of element s * N + env of stream START, wrapped and moved
// through the ring's head as k_replay_gather does.  An empty range yields sample_position (span 0), as mbpo_replay_sample does.
__device__ __forceinline__ long long start_draw_row(const StartBuf &B, int lo, int hi, int head, unsigned long long rng_seed,
                                                    unsigned long long rng_off, long long elem) {
  const long long li = philox_randint(rng_seed, rng_off, MBPO_STREAM_START, (unsigned long long)elem, lo, hi);
  long long w = li % B.max_size;      // jnp.take(mode='wrap'): python-style modulo
  if (w < 0) w += B.max_size;
  return ((w + head) % B.max_size) * B.row_len;
}

// Termination (include/mbpo_hip.h): one element of the next state against its closed interval.  NaN fails both compares and an
// infinity is violated whatever the bounds (an unbounded dimension carries -inf / +inf, which +-inf would pass).
__device__ __forceinline__ bool term_violated(float v, float lo, float hi) {
  return !(lo <= v && v <= hi) || fabsf(v) == __builtin_inff();
}

// SystemState.done of row r from its next state xn[0..X): 1 if any element is violated; 0 without a termination.
__device__ __forceinline__ float term_row_done(const RolloutArgs &A, const float *xn, int X) {
  if (!A.term_low) return 0.f;
  bool bad = false;
  for (int c = 0; c < X; ++c) bad |= term_violated(xn[c], A.term_low[c], A.term_high[c]);
  return bad ? 1.f : 0.f;
}

// PendulumDynamics.next_state (dynamics/pendulum_dynamics.py:29-63), fp32, same operation order.
__device__ __forceinline__ void pendulum_step(const float *x, float u, const float *sp, float *xn) {
  const float max_speed = sp[0], max_torque = sp[1], dt = sp[2], g = sp[3], mm = sp[4], l = sp[5];
  const float th = atan2f(x[1], x[0]);
  const float thdot = x[2];
  const float uc = fminf(fmaxf(u, -1.0f), 1.0f) * max_torque;
  const float thdd = (3.0f * g) / (2.0f * l) * sinf(th) + 3.0f / (mm * (l * l)) * uc;
  float nthdot = thdot + thdd * dt;
  nthdot = fminf(fmaxf(nthdot, -max_speed), max_speed);
  const float nth = th + nthdot * dt;  // dx[0] = clipped newthdot (ode :61-63)
  float nthdot2 = thdot + thdd * dt;   // dx[-1] = newthddot (:41)
  nthdot2 = fminf(fmaxf(nthdot2, -max_speed), max_speed);
  xn[0] = cosf(nth);
  xn[1] = sinf(nth);
  xn[2] = nthdot2;
}

// PendulumReward.__call__ (rewards/pendulum_reward.py:32-41): uses pre-step x and the unclipped action.
__device__ __forceinline__ float pendulum_reward(const float *x, float u, const float *rp) {
  const float angle_cost = rp[0], control_cost = rp[1], target = rp[2];
  const float PI_F = 3.14159265358979323846f, TWO_PI_F = 6.28318530717958647692f;
  const float theta = atan2f(x[1], x[0]), omega = x[2];
  float d = theta - target;
  float t = d + PI_F;
  float mpy = fmodf(t, TWO_PI_F);  // python/jnp % : result takes the sign of the divisor
  if (mpy < 0.0f) mpy += TWO_PI_F;
  d = mpy - PI_F;
  return -(angle_cost * (d * d) + 0.1f * (omega * omega)) - control_cost * (u * u);
}

// MBPO_REWARD_LEARNED: the reward of row r (env `env`, member-draw index eidx = (s * action_repeat + ar) * N + env) from the members'
// outputs s_y = [E][16][ld_y], reward head at column 2X: the mean over members, or in the TS modes the member the row's state takes
// (the same member_idx entry or Philox MEMBER draw as the state's section).
__device__ __forceinline__ float learned_reward(const RolloutArgs &A, const float *s_y, int ld_y, int E, int r, long long env, long long eidx,
                                                unsigned long long rng_seed, unsigned long long rng_off) {
  const int c = 2 * A.x_dim;
  if (A.ens_mode == MBPO_ENS_MEAN) {
    float acc = 0.f;
    for (int e = 0; e < E; ++e) acc += s_y[(e * 16 + r) * ld_y + c];
    return acc / (float)E;
  }
  int mem = 0;
  if (env < A.n_envs) {
    if (A.ens_mode == MBPO_ENS_TSINF) mem = (int)(env % E);
    else mem = A.member_idx ? A.member_idx[eidx] : philox_randint(rng_seed, rng_off, MBPO_STREAM_MEMBER, (unsigned long long)eidx, 0, E);
  }
  return s_y[(mem * 16 + r) * ld_y + c];
}
