// icem_seed.hip — policy priors (include/mbpo_hip.h "policy priors"): a learned policy's closed-loop action sequences put where iCEM's
// launches read their candidates.  iCEM rolls the policy through the model once per `optimize` (mbpo_model_rollout, unchanged) and issues
// one launch of mbpo_icem_seed_candidates per seeded iteration, between mbpo_icem_sample[_batched] and the candidate rollout.  A compile
// unit of its own: a caller added to icem.hip moves the register and spill figures of the kernels already there.
//
// One wave per proposal (b, k), four waves to a workgroup.  The decision "is every element finite" is per trajectory, so the wave's lanes
// stride over its H * A elements twice: a first pass ORs "not finite" per lane and one wave-wide vote (__any) settles it — a wave that
// votes "drop" returns having written nothing — and a second pass reads the elements again (a few hundred floats, L2-resident), clips
// them with mbpo_icem_sample's expression and stores the candidate, its P replicas in the rollout's action layout and, for k == 0 with a
// mean pointer, the mean.  The source is addressed by two strides and carries no alignment promise (iCEM passes the action columns of the
// rollout's rows, whose stride is odd): every access is a scalar load or store.  The exit of a wave past the last proposal and the vote's
// early return are wave-uniform; no barrier, no LDS, no atomics, no workspace.
#include "common.hpp"

#define ICEM_SEED_BLOCK 256
#define ICEM_SEED_WAVES (ICEM_SEED_BLOCK / 64)

struct IcemSeedArgs {
  const float *src;
  long long step_stride, traj_stride;
  long long n_traj;      // n_problems * n_seed
  int B, K, NC, H, A, P;
  const float *u_min, *u_max;
  float *actions, *candidates, *mean;
};

// (the exponent bits, not isfinite: the answer must not depend on what the compiler may assume about floats)
__device__ __forceinline__ bool icem_seed_not_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

__global__ void __launch_bounds__(ICEM_SEED_BLOCK) k_icem_seed(IcemSeedArgs S) {
  const long long w = (long long)blockIdx.x * ICEM_SEED_WAVES + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (w >= S.n_traj) return;                                            // (wave-uniform)
  const long long b = w / S.K;
  const int k = (int)(w - b * S.K);
  const float *s = S.src + w * S.traj_stride;
  const int HA = S.H * S.A;
  bool bad = false;
  for (int e = lane; e < HA; e += 64) {
    const int t = e / S.A, a = e - t * S.A;
    bad |= icem_seed_not_finite(s[(long long)t * S.step_stride + a]);
  }
  if (__any(bad)) return;                                               // dropped: the slot keeps the sampled candidate
  const long long c = b * S.NC + k, n_all = (long long)S.B * S.NC * S.P;
  const bool to_mean = S.mean != nullptr && k == 0;
  for (int e = lane; e < HA; e += 64) {
    const int t = e / S.A, a = e - t * S.A;
    float v = s[(long long)t * S.step_stride + a];
    v = fminf(fmaxf(v, S.u_min[a]), S.u_max[a]);                        // (mbpo_icem_sample's clip)
    if (S.candidates) {
      S.candidates[(c * S.H + t) * S.A + a] = v;
      float *act = S.actions + ((long long)t * n_all + c * S.P) * S.A + a;
      for (int p = 0; p < S.P; ++p) act[(long long)p * S.A] = v;
    }
    if (to_mean) S.mean[(b * S.H + t) * S.A + a] = v;
  }
}

static bool icem_seed_mul_fits(long long a, long long b) { return a == 0 || b <= 0x7fffffffffffffffLL / a; }

extern "C" int mbpo_icem_seed_candidates(const float *src, int64_t src_step_stride, int64_t src_traj_stride, int32_t n_problems, int32_t n_seed,
                                         int32_t n_candidates, int32_t horizon, int32_t u_dim, int32_t n_particles, const float *u_min,
                                         const float *u_max, float *actions, float *candidates, float *mean, void *stream) {
  MBPO_REQUIRE(n_problems >= 1, MBPO_ERR_ARG, "icem_seed_candidates: n_problems=%d < 1", n_problems);
  MBPO_REQUIRE(n_seed >= 1, MBPO_ERR_ARG, "icem_seed_candidates: n_seed=%d < 1", n_seed);
  MBPO_REQUIRE(n_seed <= n_candidates, MBPO_ERR_ARG, "icem_seed_candidates: n_seed=%d > n_candidates=%d", n_seed, n_candidates);
  MBPO_REQUIRE(horizon >= 1, MBPO_ERR_ARG, "icem_seed_candidates: horizon=%d < 1", horizon);
  MBPO_REQUIRE(u_dim >= 1, MBPO_ERR_ARG, "icem_seed_candidates: u_dim=%d < 1", u_dim);
  MBPO_REQUIRE(n_particles >= 1, MBPO_ERR_ARG, "icem_seed_candidates: n_particles=%d < 1", n_particles);
  const long long B = n_problems, K = n_seed, NC = n_candidates, H = horizon, A = u_dim, P = n_particles, n_traj = B * K;
  MBPO_REQUIRE(H * A <= 0x7fffffffLL, MBPO_ERR_ARG, "icem_seed_candidates: horizon * u_dim overflows int32");
  MBPO_REQUIRE(src_step_stride >= A && src_traj_stride >= A, MBPO_ERR_ARG,
               "icem_seed_candidates: src_step_stride=%lld or src_traj_stride=%lld is smaller than u_dim=%d", (long long)src_step_stride,
               (long long)src_traj_stride, u_dim);
  MBPO_REQUIRE(icem_seed_mul_fits(n_traj, src_traj_stride) && icem_seed_mul_fits(H, src_step_stride) &&
                   n_traj * src_traj_stride <= 0x7fffffffffffffffLL - H * src_step_stride,
               MBPO_ERR_ARG, "icem_seed_candidates: horizon * src_step_stride + n_problems * n_seed * src_traj_stride overflows int64");
  // the two axes must not interleave: steps outside the trajectories (step-major, iCEM's rows) or trajectories outside the steps
  MBPO_REQUIRE(src_step_stride >= (n_traj - 1) * src_traj_stride + A || src_traj_stride >= (H - 1) * src_step_stride + A, MBPO_ERR_ARG,
               "icem_seed_candidates: src_step_stride=%lld and src_traj_stride=%lld make steps and trajectories overlap (%lld trajectories, "
               "%d steps of %d floats)", (long long)src_step_stride, (long long)src_traj_stride, n_traj, horizon, u_dim);
  MBPO_REQUIRE(icem_seed_mul_fits(B * NC, P) && icem_seed_mul_fits(B * NC * P, H) && icem_seed_mul_fits(B * NC * P * H, A), MBPO_ERR_ARG,
               "icem_seed_candidates: horizon * n_problems * n_candidates * n_particles * u_dim overflows int64");
  MBPO_REQUIRE(src && u_min && u_max, MBPO_ERR_ARG, "icem_seed_candidates: null pointer (src, u_min or u_max)");
  MBPO_REQUIRE((actions == nullptr) == (candidates == nullptr), MBPO_ERR_ARG,
               "icem_seed_candidates: actions and candidates must both be set or both NULL");
  MBPO_REQUIRE(actions || mean, MBPO_ERR_ARG, "icem_seed_candidates: nothing to write (actions, candidates and mean are all NULL)");
  const long long blocks = (n_traj + ICEM_SEED_WAVES - 1) / ICEM_SEED_WAVES;
  MBPO_REQUIRE(blocks <= 2147483647LL, MBPO_ERR_ARG, "icem_seed_candidates: more than 2^31 - 1 workgroups");
  IcemSeedArgs S{src, (long long)src_step_stride, (long long)src_traj_stride, n_traj, (int)n_problems, (int)n_seed, (int)n_candidates,
                 (int)horizon, (int)u_dim, (int)n_particles, u_min, u_max, actions, candidates, mean};
  hipLaunchKernelGGL(k_icem_seed, dim3((unsigned)blocks), dim3(ICEM_SEED_BLOCK), 0, (hipStream_t)stream, S);
  MBPO_CHECK_LAUNCH("icem_seed_candidates");
  return MBPO_OK;
}
