// N3d: calibration of the ensemble's spread on held-out rows (include/mbpo_hip.h, "N3d").  One entry point, mbpo_ens_calibrate, run
// once per fit and never on a per-step path, so it is written for plainness, not latency: a memset and two stream-ordered launches.
//   k_ens_cal_count  a workgroup owns one output dimension c and CAL_CHUNK consecutive rows.  Phase 1: thread t forms (d2, v) of its
//                    rows and parks them in LDS.  Phase 2: thread t owns the cells (a, j) = t, t + 256, ... of the [A][P] table, walks
//                    the parked rows (every lane reads the same LDS word: a broadcast) and counts the covered ones in a register —
//                    the definition's comparison, cell by cell, with no assumption that coverage is monotone in j (a threshold that
//                    overflows to inf against v == 0 is NaN and covers nothing, whatever the level below it did).  The workgroup
//                    then adds its non-zero cells to counts[c] with one global integer atomic each; neighbouring lanes hold
//                    neighbouring cells, so a wave's atomics are one contiguous run.  Integer adds commute: the result does not
//                    depend on the order the workgroups arrive in, and no ordering protocol exists.
//   k_ens_cal_pick   one workgroup per dimension: S[c][a] in int64, argmin over a (ties to the lower index), calibration[c].
// No caller-owned scratch: the only cross-workgroup state is `counts` itself, zeroed here on the stream.
#include <hip/hip_runtime.h>

#include "common.hpp"

#define CAL_CHUNK 512             // rows a counting workgroup owns: two per thread
#define CAL_MAX_LEVELS 127        // P <= 127: S is a sum of P squares, each at most 2^56
#define CAL_MAX_X 65535           // one grid row per output dimension

__device__ __forceinline__ long long cal_row(const int *idx, long long k, long long n_rows) {
  long long r = idx ? (long long)idx[k] : k;
  return r < 0 ? 0 : (r >= n_rows ? n_rows - 1 : r);      // (an index outside the matrix is clamped into it: never an access outside)
}

// Every product and sum below is written as a single rounded operation (no contraction into fma), so that the counts are those of the
// definition evaluated in plain fp32 anywhere.
__global__ void __launch_bounds__(256) k_ens_cal_count(const float *y, int n_members, long long n, int y_stride,
                                                       const float *rows, long long n_rows, int row_len, const int *idx, int next_obs_off,
                                                       int predict_delta, const float *alphas, int n_alphas, const float *level_q,
                                                       int n_levels, const float *scale, int *counts) {
  __shared__ float s_d2[CAL_CHUNK], s_v[CAL_CHUNK];
  const int t = threadIdx.x, c = blockIdx.y;
  const long long k0 = (long long)blockIdx.x * CAL_CHUNK;
  const int n_here = (int)((n - k0 < CAL_CHUNK) ? n - k0 : CAL_CHUNK);
  const float members = (float)n_members;
  const long long member_stride = n * y_stride;      // y is dense: [E][n][y_stride]
  for (int r = t; r < n_here; r += 256) {
    const long long k = k0 + r;
    const float *row = rows + cal_row(idx, k, n_rows) * row_len;
    const float target = predict_delta ? __fsub_rn(row[next_obs_off + c], row[c]) : row[next_obs_off + c];
    const float *yk = y + k * y_stride + c;
    float sum = 0.0f;
    for (int e = 0; e < n_members; ++e) sum = __fadd_rn(sum, yk[e * member_stride]);
    const float m = __fdiv_rn(sum, members);
    float sq = 0.0f;
    for (int e = 0; e < n_members; ++e) {
      const float d = __fsub_rn(yk[e * member_stride], m);
      sq = __fadd_rn(sq, __fmul_rn(d, d));
    }
    const float dt = __fsub_rn(target, m);
    s_d2[r] = __fmul_rn(dt, dt);
    s_v[r] = __fdiv_rn(sq, members);
  }
  __syncthreads();
  const float sc = scale ? scale[c] : 1.0f;
  const int n_cells = n_alphas * n_levels;
  int *out = counts + (long long)c * n_cells;
  for (int cell = t; cell < n_cells; cell += 256) {
    const int a = cell / n_levels, j = cell - a * n_levels;
    const float as = __fmul_rn(alphas[a], sc);
    const float tq = __fmul_rn(__fmul_rn(as, as), level_q[j]);
    int covered = 0;
    for (int r = 0; r < n_here; ++r) covered += (s_d2[r] <= __fmul_rn(tq, s_v[r])) ? 1 : 0;      // false for a NaN on either side
    if (covered) atomicAdd(out + cell, covered);
  }
}

// S[c][a] = sum_j (counts[c][a][j] * (P + 1) - j * n)^2, j = 1..P, in int64; (S, a) minimal in lexicographic order wins.
__global__ void __launch_bounds__(256) k_ens_cal_pick(const int *counts, long long n, const float *alphas, int n_alphas, int n_levels,
                                                      const float *scale, int *best_idx, float *calibration) {
  __shared__ long long s_best[256];
  __shared__ int s_arg[256];
  const int t = threadIdx.x, c = blockIdx.x;
  const int *cnt = counts + (long long)c * n_alphas * n_levels;
  long long best = -1;          // (S >= 0: -1 marks a thread that saw no alpha)
  int arg = 0;
  for (int a = t; a < n_alphas; a += 256) {
    long long s = 0;
    for (int j = 1; j <= n_levels; ++j) {
      const long long d = (long long)cnt[(long long)a * n_levels + (j - 1)] * (n_levels + 1) - (long long)j * n;
      s += d * d;
    }
    if (best < 0 || s < best) { best = s; arg = a; }      // a ascending within a thread: the first minimum stays
  }
  s_best[t] = best;
  s_arg[t] = arg;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) {
      const long long ob = s_best[t + w];
      const int oa = s_arg[t + w];
      if (ob >= 0 && (s_best[t] < 0 || ob < s_best[t] || (ob == s_best[t] && oa < s_arg[t]))) {
        s_best[t] = ob;
        s_arg[t] = oa;
      }
    }
    __syncthreads();
  }
  if (t == 0) {
    best_idx[c] = s_arg[0];
    calibration[c] = __fmul_rn(alphas[s_arg[0]], scale ? scale[c] : 1.0f);
  }
}

extern "C" int mbpo_ens_calibrate(const float *y, int32_t n_members, int64_t n, int32_t y_stride, const float *rows,
                                  int64_t n_rows, int32_t row_len, const int32_t *idx, int32_t x_dim, int32_t next_obs_off,
                                  int32_t predict_delta, const float *alphas, int32_t n_alphas, const float *level_q, int32_t n_levels,
                                  const float *scale, int32_t *counts, int32_t *best_idx, float *calibration, void *stream) {
  MBPO_REQUIRE(y && rows && alphas && level_q, MBPO_ERR_ARG, "ens_calibrate: null y / rows / alphas / level_q");
  MBPO_REQUIRE(counts && best_idx && calibration, MBPO_ERR_ARG, "ens_calibrate: null counts / best_idx / calibration");
  MBPO_REQUIRE(n > 0 && n_rows > 0 && row_len > 0, MBPO_ERR_ARG, "ens_calibrate: n, n_rows and row_len must be positive (n = %lld)",
               (long long)n);
  MBPO_REQUIRE(n_members > 0 && n_alphas > 0 && n_levels > 0, MBPO_ERR_ARG,
               "ens_calibrate: n_members, n_alphas and n_levels must be positive (E = %d, A = %d, P = %d)", n_members, n_alphas, n_levels);
  MBPO_REQUIRE(x_dim > 0 && y_stride >= x_dim, MBPO_ERR_ARG, "ens_calibrate: y_stride = %d below x_dim = %d (or x_dim <= 0)", y_stride,
               x_dim);
  MBPO_REQUIRE(next_obs_off >= 0 && (int64_t)next_obs_off + x_dim <= row_len && x_dim <= row_len, MBPO_ERR_ARG,
               "ens_calibrate: next_obs_off %d + x_dim %d outside the row (row_len %d)", next_obs_off, x_dim, row_len);
  MBPO_REQUIRE(idx || n <= n_rows, MBPO_ERR_ARG, "ens_calibrate: n = %lld rows without idx, the matrix has %lld", (long long)n,
               (long long)n_rows);
  MBPO_REQUIRE(n <= (1LL << 28) / ((int64_t)n_levels + 1), MBPO_ERR_ARG,
               "ens_calibrate: n * (n_levels + 1) = %lld * %d above 2^28 (the selection sums squares of it in int64)", (long long)n,
               n_levels + 1);
  MBPO_REQUIRE(n_levels <= CAL_MAX_LEVELS, MBPO_ERR_UNSUPPORTED, "ens_calibrate: n_levels = %d above %d", n_levels, CAL_MAX_LEVELS);
  MBPO_REQUIRE(x_dim <= CAL_MAX_X, MBPO_ERR_UNSUPPORTED, "ens_calibrate: x_dim = %d above %d", x_dim, CAL_MAX_X);
  const long long cells = (long long)n_alphas * n_levels;
  MBPO_REQUIRE(cells <= (1LL << 24) && cells * x_dim <= (1LL << 29), MBPO_ERR_UNSUPPORTED,
               "ens_calibrate: a counts table of %d x %d x %d cells is too large", x_dim, n_alphas, n_levels);
  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)(cells * x_dim), st);
  MBPO_REQUIRE(e == hipSuccess, MBPO_ERR_LAUNCH, "ens_calibrate: zeroing counts: %s", hipGetErrorString(e));
  const unsigned n_chunks = (unsigned)((n + CAL_CHUNK - 1) / CAL_CHUNK);
  hipLaunchKernelGGL(k_ens_cal_count, dim3(n_chunks, (unsigned)x_dim), dim3(256), 0, st, y, n_members,
                     (long long)n, y_stride, rows, (long long)n_rows, row_len, idx, next_obs_off, predict_delta, alphas, n_alphas, level_q,
                     n_levels, scale, counts);
  MBPO_CHECK_LAUNCH("ens_calibrate.count");
  hipLaunchKernelGGL(k_ens_cal_pick, dim3((unsigned)x_dim), dim3(256), 0, st, (const int *)counts, (long long)n, alphas, n_alphas, n_levels,
                     scale, best_idx, calibration);
  MBPO_CHECK_LAUNCH("ens_calibrate.pick");
  return MBPO_OK;
}
