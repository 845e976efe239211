// plan_reward.hip — plan rewards (include/mbpo_hip.h "plan rewards"): the reward column of an open-loop rollout's rows, evaluated again
// under parameters that differ per problem and per step.  iCEM's batched and single paths issue one launch of mbpo_plan_reward_eval
// between mbpo_model_rollout and the update, which then reads the rewards this launch wrote.  A compile unit of its own: a caller added
// to rollout.hip or icem.hip moves the register and spill figures of the kernels already there.
//
// One thread per row, neighbouring lanes on neighbouring rows of one step.  Rows carry no alignment promise: every column is a scalar
// load.  The parameters of (b, t) lie at params + ((PB > 1 ? b : 0) * PH + (PH > 1 ? t : 0)) * param_len.
//   k_plan_reward_grouped (group >= 256, the planner's sizes: 5150 rows per problem and step at the reference's defaults): the grid is
//     (tiles of the group, problem, step), so a workgroup's 256 rows belong to ONE (b, t) and no thread divides anything.  A term table
//     is staged in LDS once per workgroup — the header, the group records and the header's (clamped) count of term records, not all 2320
//     bytes; reward_terms_eval reads no term record past that count — and all lanes walk the same records: broadcast reads.  The last
//     tile of a group is partly idle (30 of 256 lanes at 5150).
//   k_plan_reward_flat (smaller groups, or more than 65535 problems or steps): 256 consecutive rows of the flat step-major index, which
//     span up to 256 pairs.  A tile's first pair q0 = i0 / group is a workgroup-uniform 64-bit division; a lane's pair is q0 + (tile-local
//     row) / group, a 32-bit division of a number below 511 (0 or 1 from group 256 on).  Each lane walks its own table in global memory:
//     lanes diverge, L2 serves it.
//   QUADRATIC, PENDULUM: a handful of floats, read from global memory where they are used (one address per wave in the grouped kernel).
// The arithmetic is reward_terms_eval, k_reward_eval's quadratic expressions in their order, and pendulum_reward.  A thread reads the
// obs, control and next-state columns of its row and writes one float, out[i * out_stride]; with out = rows + reward_col and out_stride =
// row_len that float is the row's own reward column, which no thread reads.  The grids are not capped (nothing strides): the host
// refuses more than 2^31 - 1 tiles.  No atomics, no workspace.
#include "common.hpp"
#include "reward_terms.hpp"
#include "rollout_shared.hpp"

#define PLAN_REWARD_BLOCK 256
#define PLAN_REWARD_GROUPED_MIN_GROUP PLAN_REWARD_BLOCK
#define PLAN_REWARD_GRID_YZ_MAX 65535

// r of row `r` under the parameters at `rp` (a term table: at `tab`, which may be its copy in LDS)
__device__ __forceinline__ float plan_reward_row(int kind, const float *tab, const float *rp, const float *r, int next_off, int X, int UE) {
  if (kind == MBPO_REWARD_TERMS) return reward_terms_eval(tab, r, r + X, reward_terms_next(r + next_off, r, X), X, UE);
  if (kind == MBPO_REWARD_PENDULUM) return pendulum_reward(r, r[X], rp);
  // (the quadratic reward, as k_reward_eval writes it)
  const float *xr = r, *ur = r + X;
  const float *tp = rp, *qp = tp + X, *rr = qp + X;
  float cx = 0.f, cu = 0.f;
  for (int c = 0; c < X; ++c) { float dd = xr[c] - tp[c]; cx += qp[c] * (dd * dd); }
  for (int d = 0; d < UE; ++d) { float uu = ur[d]; cu += rr[d] * (uu * uu); }
  return -cx - cu;
}

// grid (tiles of the group, n_problems, n_steps)
__global__ void __launch_bounds__(PLAN_REWARD_BLOCK) k_plan_reward_grouped(int kind, const float *params, int PB, int PH, int P, const float *rows,
                                                                           int row_len, int next_off, long long G, int X, int UE, float *out,
                                                                           long long out_stride) {
  __shared__ float s_tab[MBPO_REWARD_TERMS_FLOATS];
  const int b = blockIdx.y, t = blockIdx.z;
  const float *rp = params + ((long long)(PB > 1 ? b : 0) * PH + (PH > 1 ? t : 0)) * P;
  if (kind == MBPO_REWARD_TERMS) {      // (a kernel argument: every thread takes the barrier or none does)
    const int n = RT_TERMS_OFF + 4 * rt_clamp_int(rp[1], MBPO_REWARD_TERMS_MAX_TERMS);
    for (int idx = threadIdx.x; idx < n; idx += PLAN_REWARD_BLOCK) s_tab[idx] = rp[idx];
    __syncthreads();
  }
  const long long j = (long long)blockIdx.x * PLAN_REWARD_BLOCK + threadIdx.x;
  if (j >= G) return;
  const long long i = ((long long)t * gridDim.y + b) * G + j;
  out[i * out_stride] = plan_reward_row(kind, s_tab, rp, rows + i * row_len, next_off, X, UE);
}

// grid (tiles of the flat row index)
__global__ void __launch_bounds__(PLAN_REWARD_BLOCK) k_plan_reward_flat(int kind, const float *params, int PB, int PH, int P, const float *rows,
                                                                        int row_len, int next_off, long long n_rows, int B, long long G, int X,
                                                                        int UE, float *out, long long out_stride) {
  const long long base = (long long)blockIdx.x * PLAN_REWARD_BLOCK;
  const long long q0 = base / G, rem0 = base - q0 * G, t0 = q0 / B;      // (workgroup-uniform)
  const unsigned b0 = (unsigned)(q0 - t0 * B);
  const long long i = base + threadIdx.x, r0 = rem0 + threadIdx.x;       // (r0 < G + 256)
  if (i >= n_rows) return;
  const unsigned dq = G >= PLAN_REWARD_BLOCK ? (r0 >= G ? 1u : 0u) : (unsigned)r0 / (unsigned)G;      // this row's pair is q0 + dq
  const unsigned bd = b0 + dq, dt = bd / (unsigned)B;                     // ... step t0 + (b0 + dq) / B, problem (b0 + dq) % B
  const long long t = t0 + dt, b = bd - dt * (unsigned)B;
  const float *rp = params + ((PB > 1 ? b : 0) * PH + (PH > 1 ? t : 0)) * P;
  out[i * out_stride] = plan_reward_row(kind, rp, rp, rows + i * row_len, next_off, X, UE);
}

static bool plan_reward_mul_fits(long long a, long long b) { return a == 0 || b <= 0x7fffffffffffffffLL / a; }

// Test hook (not part of include/mbpo_hip.h): 1 = k_plan_reward_flat also for groups of 256 rows and more, where the dispatch picks
// k_plan_reward_grouped unless there are more than 65535 problems or steps — sizes no test can afford; 0 or -1 = the default dispatch.
// tests/test_gpu_plan_reward.py runs the large-group shapes under it and compares the bits.
extern "C" int mbpo_debug_set_plan_reward_flat(int mode) {
  MBPO_REQUIRE(mode >= -1 && mode <= 1, MBPO_ERR_ARG, "debug_set_plan_reward_flat: mode must be -1, 0 or 1");
  return mbpo_knob_set_override(KNOB_PLAN_REWARD_FLAT, mode);
}

extern "C" int mbpo_plan_reward_eval(int32_t reward_kind, const float *params, int32_t param_problems, int32_t param_steps, int32_t param_len,
                                     const float *rows, int32_t row_len, int32_t next_off, int32_t n_steps, int32_t n_problems, int64_t group,
                                     int32_t x_dim, int32_t u_dim, float *out, int64_t out_stride, void *stream) {
  MBPO_REQUIRE(reward_kind != MBPO_REWARD_LEARNED, MBPO_ERR_UNSUPPORTED,
               "plan_reward_eval: the learned reward is not a function of the row (MBPO_REWARD_TERMS, _QUADRATIC and _PENDULUM are evaluated here)");
  MBPO_REQUIRE(reward_kind == MBPO_REWARD_TERMS || reward_kind == MBPO_REWARD_QUADRATIC || reward_kind == MBPO_REWARD_PENDULUM, MBPO_ERR_ARG,
               "plan_reward_eval: unknown reward_kind %d", reward_kind);
  MBPO_REQUIRE(n_steps >= 1, MBPO_ERR_ARG, "plan_reward_eval: n_steps=%d < 1", n_steps);
  MBPO_REQUIRE(n_problems >= 1, MBPO_ERR_ARG, "plan_reward_eval: n_problems=%d < 1", n_problems);
  MBPO_REQUIRE(group >= 0, MBPO_ERR_ARG, "plan_reward_eval: group < 0");
  MBPO_REQUIRE(x_dim >= 1 && u_dim >= 1, MBPO_ERR_ARG, "plan_reward_eval: x_dim and u_dim must be positive");
  MBPO_REQUIRE(param_problems == 1 || param_problems == n_problems, MBPO_ERR_ARG,
               "plan_reward_eval: param_problems=%d is neither 1 nor n_problems=%d", param_problems, n_problems);
  MBPO_REQUIRE(param_steps == 1 || param_steps == n_steps, MBPO_ERR_ARG, "plan_reward_eval: param_steps=%d is neither 1 nor n_steps=%d",
               param_steps, n_steps);
  if (reward_kind == MBPO_REWARD_PENDULUM)
    MBPO_REQUIRE(x_dim == 3 && u_dim == 1, MBPO_ERR_ARG, "plan_reward_eval: the Pendulum reward needs x_dim 3 and u_dim 1, got %d and %d", x_dim,
                 u_dim);
  const long long need = reward_kind == MBPO_REWARD_TERMS ? MBPO_REWARD_TERMS_FLOATS
                                                          : (reward_kind == MBPO_REWARD_PENDULUM ? 3 : 2LL * x_dim + u_dim);
  MBPO_REQUIRE(param_len >= need, MBPO_ERR_ARG, "plan_reward_eval: param_len=%d, this kind reads %lld floats", param_len, need);
  MBPO_REQUIRE(next_off >= 0 && (long long)next_off + x_dim <= row_len, MBPO_ERR_ARG,
               "plan_reward_eval: next_off=%d + x_dim=%d leaves the row (row_len=%d)", next_off, x_dim, row_len);
  MBPO_REQUIRE((long long)x_dim + u_dim <= next_off, MBPO_ERR_ARG, "plan_reward_eval: x_dim=%d + u_dim=%d overlaps next_off=%d", x_dim, u_dim,
               next_off);
  MBPO_REQUIRE(out_stride >= 1, MBPO_ERR_ARG, "plan_reward_eval: out_stride < 1");
  const long long n_pairs = (long long)n_steps * n_problems;
  MBPO_REQUIRE(plan_reward_mul_fits(n_pairs, group) && plan_reward_mul_fits(n_pairs * group, row_len) &&
                   plan_reward_mul_fits(n_pairs * group, out_stride) && plan_reward_mul_fits((long long)param_problems * param_steps, param_len),
               MBPO_ERR_ARG, "plan_reward_eval: n_steps * n_problems * group * row_len (or out_stride) overflows int64");
  if (group == 0) return MBPO_OK;
  MBPO_REQUIRE(params && rows && out, MBPO_ERR_ARG, "plan_reward_eval: null pointer");
  const long long n_rows = n_pairs * group, tiles = (n_rows + PLAN_REWARD_BLOCK - 1) / PLAN_REWARD_BLOCK;
  MBPO_REQUIRE(tiles <= 2147483647LL, MBPO_ERR_ARG, "plan_reward_eval: more than 2^31 - 1 tiles of %d rows", PLAN_REWARD_BLOCK);
  const hipStream_t st = (hipStream_t)stream;
  if (group >= PLAN_REWARD_GROUPED_MIN_GROUP && n_problems <= PLAN_REWARD_GRID_YZ_MAX && n_steps <= PLAN_REWARD_GRID_YZ_MAX &&
      mbpo_knob_override(KNOB_PLAN_REWARD_FLAT) != 1) {
    const long long gt = (group + PLAN_REWARD_BLOCK - 1) / PLAN_REWARD_BLOCK;      // (<= tiles: it fits a grid's x)
    hipLaunchKernelGGL(k_plan_reward_grouped, dim3((unsigned)gt, (unsigned)n_problems, (unsigned)n_steps), dim3(PLAN_REWARD_BLOCK), 0, st,
                       (int)reward_kind, params, (int)param_problems, (int)param_steps, (int)param_len, rows, (int)row_len, (int)next_off,
                       (long long)group, (int)x_dim, (int)u_dim, out, (long long)out_stride);
  } else {
    hipLaunchKernelGGL(k_plan_reward_flat, dim3((unsigned)tiles), dim3(PLAN_REWARD_BLOCK), 0, st, (int)reward_kind, params, (int)param_problems,
                       (int)param_steps, (int)param_len, rows, (int)row_len, (int)next_off, n_rows, (int)n_problems, (long long)group, (int)x_dim,
                       (int)u_dim, out, (long long)out_stride);
  }
  MBPO_CHECK_LAUNCH("plan_reward_eval");
  return MBPO_OK;
}
