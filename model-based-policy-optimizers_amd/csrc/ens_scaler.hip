// N3c: the dynamics ensemble's input scaler (MBPO's model training fits one on the training inputs [x, u]; the reference has no model).
// Three one-shot calls per fit, none of them on a per-step path (include/mbpo_hip.h, "N3c"):
//   mbpo_ens_scaler_fit     per-column mean and std of the selected rows' inputs, fp64 two-pass, fixed-order reduction
//   mbpo_ens_scaler_prepare gather + normalise the inputs + delta-encode the target into the training matrix the NLL / eval kernels read
//   mbpo_ens_fold_scaler    the scaler folded into every member's first Dense layer, so that every consumer runs its existing kernel on
//                           raw inputs
// All three are HBM / latency bound (a few MB at most): the work is spread over enough workgroups to cover the latency, the dense
// outputs are written 16 bytes per lane where their alignment allows it, and the gathered source rows (row_len is arbitrary, the
// rows are picked by idx) are read as dwords that neighbouring lanes share through L1 / L2.
#include <hip/hip_runtime.h>

#include "common.hpp"

#define SCALER_MAX_IN 256          // x_dim + u_dim: one thread per column in a 256-thread workgroup
#define SCALER_MAX_WG 512          // workgroups of a statistics pass
#define SCALER_ROW_PASSES 8        // row passes a statistics workgroup makes at least, before more workgroups are used

// ------------------------------------------------------------------------------------------------ statistics
// Geometry of a statistics pass: a function of (n, in_dim) only, so that two calls reduce in the same order.
struct ScalerGeom {
  int rows_per_pass;     // rows a workgroup covers at once: thread t is (row t / in_dim, column t % in_dim)
  int n_wg;
  long long chunk;       // consecutive k a workgroup owns
};

static ScalerGeom scaler_geom(long long n, int in_dim) {
  ScalerGeom g;
  g.rows_per_pass = 256 / in_dim;
  const long long per_wg = (long long)g.rows_per_pass * SCALER_ROW_PASSES;
  long long wg = (n + per_wg - 1) / per_wg;
  wg = wg < 1 ? 1 : (wg > SCALER_MAX_WG ? SCALER_MAX_WG : wg);
  g.chunk = (n + wg - 1) / wg;
  g.n_wg = (int)((n + g.chunk - 1) / g.chunk);
  return g;
}

__device__ __forceinline__ long long scaler_row(const int *idx, long long k, long long n_rows) {
  long long r = idx ? (long long)idx[k] : k;
  return r < 0 ? 0 : (r >= n_rows ? n_rows - 1 : r);      // (an index outside the matrix is clamped into it: never an access outside)
}

// sum over g (ascending) of part[g][c]
__device__ __forceinline__ double scaler_partial_sum(const double *part, int n_wg, int in_dim, int c) {
  double s = 0.0;
  for (int g = 0; g < n_wg; ++g) s += part[(long long)g * in_dim + c];
  return s;
}

// PASS 0: part0[wg][c] = sum over the workgroup's rows of d;  PASS 1: part1[wg][c] = sum of (d - mean_c)^2, mean_c from part0.
// A thread adds its rows in ascending k; the workgroup adds its threads' sums per column in ascending thread row.
template <int PASS>
__global__ void __launch_bounds__(256) k_ens_scaler_partial(const float *rows, long long n_rows, int row_len, const int *idx, long long n,
                                                            int in_dim, int rows_per_pass, long long chunk, int n_wg, double *part0,
                                                            double *part1) {
  __shared__ double s_acc[256];
  __shared__ double s_mean[SCALER_MAX_IN];
  const int t = threadIdx.x, r = t / in_dim, c = t - r * in_dim;
  if (PASS == 1) {
    if (t < in_dim) s_mean[t] = scaler_partial_sum(part0, n_wg, in_dim, t) / (double)n;
    __syncthreads();
  }
  const long long k0 = (long long)blockIdx.x * chunk, k1 = (k0 + chunk < n) ? k0 + chunk : n;
  double acc = 0.0;
  if (r < rows_per_pass) {
    const double mean = PASS == 1 ? s_mean[c] : 0.0;
    for (long long k = k0 + r; k < k1; k += rows_per_pass) {
      const double d = (double)rows[scaler_row(idx, k, n_rows) * row_len + c] - mean;
      acc += PASS == 1 ? d * d : d;
    }
  }
  s_acc[t] = acc;
  __syncthreads();
  if (t < in_dim) {
    double s = 0.0;
    for (int q = 0; q < rows_per_pass; ++q) s += s_acc[q * in_dim + t];
    (PASS == 1 ? part1 : part0)[(long long)blockIdx.x * in_dim + t] = s;
  }
}

// One workgroup: scaler[0][c] = mean, scaler[1][c] = std (population), a std below the floor replaced by exactly 1.
__global__ void __launch_bounds__(256) k_ens_scaler_finish(const double *part0, const double *part1, int n_wg, int in_dim, long long n,
                                                           float std_floor, float *scaler) {
  const int c = threadIdx.x;
  if (c >= in_dim) return;
  const double mean = scaler_partial_sum(part0, n_wg, in_dim, c) / (double)n;
  const double var = scaler_partial_sum(part1, n_wg, in_dim, c) / (double)n;
  const float sd = (float)sqrt(var);
  scaler[c] = (float)mean;
  scaler[in_dim + c] = sd < std_floor ? 1.0f : sd;
}

static int scaler_rows_check(const char *what, const float *rows, long long n_rows, int row_len, const int32_t *idx, long long n, int in_dim) {
  MBPO_REQUIRE(rows, MBPO_ERR_ARG, "%s: null rows", what);
  MBPO_REQUIRE(n_rows > 0 && row_len > 0 && n > 0, MBPO_ERR_ARG, "%s: n_rows, row_len and n must be positive (n = %lld)", what, n);
  MBPO_REQUIRE(in_dim > 0 && in_dim <= row_len, MBPO_ERR_ARG, "%s: x_dim + u_dim = %d outside [1, row_len = %d]", what, in_dim, row_len);
  MBPO_REQUIRE(in_dim <= SCALER_MAX_IN, MBPO_ERR_UNSUPPORTED, "%s: x_dim + u_dim = %d above %d", what, in_dim, SCALER_MAX_IN);
  MBPO_REQUIRE(idx || n <= n_rows, MBPO_ERR_ARG, "%s: n = %lld rows without idx, the matrix has %lld", what, n, n_rows);
  return MBPO_OK;
}

extern "C" int64_t mbpo_ens_scaler_workspace_floats(int64_t n, int32_t in_dim) {
  MBPO_REQUIRE(n > 0 && in_dim > 0, MBPO_ERR_ARG, "ens_scaler_workspace: n and in_dim must be positive");
  MBPO_REQUIRE(in_dim <= SCALER_MAX_IN, MBPO_ERR_UNSUPPORTED, "ens_scaler_workspace: in_dim = %d above %d", in_dim, SCALER_MAX_IN);
  const ScalerGeom g = scaler_geom(n, in_dim);
  return 2LL * 2 * g.n_wg * in_dim;      // two passes of [n_wg][in_dim] doubles
}

extern "C" int mbpo_ens_scaler_fit(const float *rows, int64_t n_rows, int32_t row_len, const int32_t *idx, int64_t n, int32_t in_dim,
                                   float std_floor, float *scaler, float *workspace, void *stream) {
  int rc = scaler_rows_check("ens_scaler_fit", rows, n_rows, row_len, idx, n, in_dim);
  if (rc != MBPO_OK) return rc;
  MBPO_REQUIRE(scaler && workspace, MBPO_ERR_ARG, "ens_scaler_fit: null scaler / workspace");
  MBPO_REQUIRE(((uintptr_t)workspace & 7) == 0, MBPO_ERR_ARG, "ens_scaler_fit: the workspace must be 8-byte aligned (fp64 partials)");
  MBPO_REQUIRE(std_floor >= 0.0f, MBPO_ERR_ARG, "ens_scaler_fit: std_floor must be >= 0");
  const ScalerGeom g = scaler_geom(n, in_dim);
  double *part0 = reinterpret_cast<double *>(workspace), *part1 = part0 + (long long)g.n_wg * in_dim;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_ens_scaler_partial<0>, dim3(g.n_wg), dim3(256), 0, st, rows, (long long)n_rows, row_len, idx, (long long)n, in_dim,
                     g.rows_per_pass, g.chunk, g.n_wg, part0, part1);
  MBPO_CHECK_LAUNCH("ens_scaler_fit.mean");
  hipLaunchKernelGGL(k_ens_scaler_partial<1>, dim3(g.n_wg), dim3(256), 0, st, rows, (long long)n_rows, row_len, idx, (long long)n, in_dim,
                     g.rows_per_pass, g.chunk, g.n_wg, part0, part1);
  MBPO_CHECK_LAUNCH("ens_scaler_fit.var");
  hipLaunchKernelGGL(k_ens_scaler_finish, dim3(1), dim3(256), 0, st, (const double *)part0, (const double *)part1, g.n_wg, in_dim,
                     (long long)n, std_floor, scaler);
  MBPO_CHECK_LAUNCH("ens_scaler_fit.finish");
  return MBPO_OK;
}

// ------------------------------------------------------------------------------------------------ prepare
struct PrepArgs {
  const float *rows;
  long long n_rows, n;
  int row_len, x_dim, u_dim, next_obs_off, reward_off, predict_delta;
  const int *idx;
  const float *scaler;
  float *out;
};

// out[k][col]: col < x+u the normalised input, col == x+u the reward, above it the target.
__device__ __forceinline__ float prep_elem(const PrepArgs &a, long long f, int out_len, const float *s_mean, const float *s_inv) {
  const long long k = f / out_len;
  const int col = (int)(f - k * out_len), in_dim = a.x_dim + a.u_dim;
  const float *row = a.rows + scaler_row(a.idx, k, a.n_rows) * a.row_len;
  if (col < in_dim) return (row[col] - s_mean[col]) * s_inv[col];
  if (col == in_dim) return a.reward_off >= 0 ? row[a.reward_off] : 0.0f;
  const int d = col - in_dim - 1;
  const float nx = row[a.next_obs_off + d];
  return a.predict_delta ? nx - row[d] : nx;
}

// VEC: a thread forms four consecutive floats of the dense output and stores them as 16 bytes (out 16-byte aligned); the last
// (n * out_len) % 4 floats, and every float without VEC, go as dwords.
template <bool VEC>
__global__ void __launch_bounds__(256) k_ens_scaler_prepare(PrepArgs a) {
  __shared__ float s_mean[SCALER_MAX_IN], s_inv[SCALER_MAX_IN];
  const int in_dim = a.x_dim + a.u_dim, out_len = in_dim + 1 + a.x_dim;
  if ((int)threadIdx.x < in_dim) {
    s_mean[threadIdx.x] = a.scaler[threadIdx.x];
    s_inv[threadIdx.x] = 1.0f / a.scaler[in_dim + threadIdx.x];
  }
  __syncthreads();
  const long long total = a.n * out_len, i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (VEC) {
    const long long n_vec = total >> 2;
    if (i < n_vec) {
      float4 v;
      v.x = prep_elem(a, 4 * i + 0, out_len, s_mean, s_inv);
      v.y = prep_elem(a, 4 * i + 1, out_len, s_mean, s_inv);
      v.z = prep_elem(a, 4 * i + 2, out_len, s_mean, s_inv);
      v.w = prep_elem(a, 4 * i + 3, out_len, s_mean, s_inv);
      reinterpret_cast<float4 *>(a.out)[i] = v;
    } else if (i - n_vec < (total & 3)) {
      const long long f = 4 * n_vec + (i - n_vec);
      a.out[f] = prep_elem(a, f, out_len, s_mean, s_inv);
    }
  } else if (i < total) {
    a.out[i] = prep_elem(a, i, out_len, s_mean, s_inv);
  }
}

extern "C" int mbpo_ens_scaler_prepare(const float *rows, int64_t n_rows, int32_t row_len, const int32_t *idx, int64_t n, int32_t x_dim,
                                       int32_t u_dim, int32_t next_obs_off, int32_t reward_off, int32_t predict_delta,
                                       const float *scaler, float *out, void *stream) {
  MBPO_REQUIRE(x_dim > 0 && u_dim >= 0, MBPO_ERR_ARG, "ens_scaler_prepare: x_dim must be positive, u_dim >= 0");
  int rc = scaler_rows_check("ens_scaler_prepare", rows, n_rows, row_len, idx, n, x_dim + u_dim);
  if (rc != MBPO_OK) return rc;
  MBPO_REQUIRE(scaler && out, MBPO_ERR_ARG, "ens_scaler_prepare: null scaler / out");
  MBPO_REQUIRE(next_obs_off >= 0 && next_obs_off + x_dim <= row_len, MBPO_ERR_ARG,
               "ens_scaler_prepare: next_obs_off %d + x_dim %d outside the row (row_len %d)", next_obs_off, x_dim, row_len);
  MBPO_REQUIRE(reward_off < row_len, MBPO_ERR_ARG, "ens_scaler_prepare: reward_off %d outside the row (row_len %d)", reward_off, row_len);
  const int out_len = 2 * x_dim + u_dim + 1;
  MBPO_REQUIRE(n <= ((1LL << 40) / out_len), MBPO_ERR_ARG, "ens_scaler_prepare: n too large");
  PrepArgs a;
  a.rows = rows; a.n_rows = n_rows; a.n = n; a.row_len = row_len; a.x_dim = x_dim; a.u_dim = u_dim;
  a.next_obs_off = next_obs_off; a.reward_off = reward_off; a.predict_delta = predict_delta; a.idx = idx; a.scaler = scaler; a.out = out;
  const long long total = (long long)n * out_len;
  hipStream_t st = (hipStream_t)stream;
  if (((uintptr_t)out & 15) == 0) {
    const long long threads = (total >> 2) + (total & 3);
    hipLaunchKernelGGL(k_ens_scaler_prepare<true>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL(k_ens_scaler_prepare<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
  }
  MBPO_CHECK_LAUNCH("ens_scaler_prepare");
  return MBPO_OK;
}

// ------------------------------------------------------------------------------------------------ fold
// Float i of a member with the first Dense layer folded; everything past the layer is the source word.
__device__ __forceinline__ float fold_elem(const float *src, long long i, int d0, int d1, const float *s_mean, const float *s_inv) {
  const long long nw = (long long)d0 * d1;
  if (i >= nw + d1) return src[i];
  if (i < nw) return src[i] * s_inv[i / d1];
  const int j = (int)(i - nw);
  float s = 0.0f;
  for (int q = 0; q < d0; ++q) s = __fmaf_rn(src[(long long)q * d1 + j] * s_inv[q], s_mean[q], s);     // W'[q][j] as it is stored, q ascending
  return src[i] - s;
}

// Member blockIdx.y.  VEC (n_params and d1 multiples of 4, both members 16-byte aligned): 16-byte loads and stores; four consecutive
// floats then lie in one row of W_0, or in b_0, or past the layer, so the first float's region is all four's.
template <bool VEC>
__global__ void __launch_bounds__(256) k_ens_fold_scaler(const float *params, float *out_params, long long n_params, int d0, int d1,
                                                         const float *scaler) {
  __shared__ float s_mean[SCALER_MAX_IN], s_inv[SCALER_MAX_IN];
  if ((int)threadIdx.x < d0) {
    s_mean[threadIdx.x] = scaler[threadIdx.x];
    s_inv[threadIdx.x] = 1.0f / scaler[d0 + threadIdx.x];
  }
  __syncthreads();
  const float *src = params + (long long)blockIdx.y * n_params;
  float *dst = out_params + (long long)blockIdx.y * n_params;
  const long long i0 = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
  const long long layer = (long long)d0 * d1 + d1;
  if (VEC) {
    const float4 *s4 = reinterpret_cast<const float4 *>(src);
    float4 *d4 = reinterpret_cast<float4 *>(dst);
    for (long long v = i0; v < (n_params >> 2); v += stride) {
      float4 w;
      if (4 * v >= layer) {
        w = s4[v];
      } else {
        w.x = fold_elem(src, 4 * v + 0, d0, d1, s_mean, s_inv);
        w.y = fold_elem(src, 4 * v + 1, d0, d1, s_mean, s_inv);
        w.z = fold_elem(src, 4 * v + 2, d0, d1, s_mean, s_inv);
        w.w = fold_elem(src, 4 * v + 3, d0, d1, s_mean, s_inv);
      }
      d4[v] = w;
    }
  } else {
    for (long long i = i0; i < n_params; i += stride) dst[i] = fold_elem(src, i, d0, d1, s_mean, s_inv);
  }
}

extern "C" int mbpo_ens_fold_scaler(const float *params, int64_t n_params, int32_t n_members, int32_t dims0, int32_t dims1,
                                    const float *scaler, float *out_params, void *stream) {
  MBPO_REQUIRE(params && scaler && out_params, MBPO_ERR_ARG, "ens_fold_scaler: null pointer");
  MBPO_REQUIRE(n_members > 0 && n_members <= 65535 && n_params > 0, MBPO_ERR_ARG, "ens_fold_scaler: n_members must be in [1, 65535], n_params positive");
  MBPO_REQUIRE(dims0 > 0 && dims1 > 0 && (long long)dims0 * dims1 + dims1 <= n_params, MBPO_ERR_ARG,
               "ens_fold_scaler: the first layer [%d][%d] + bias does not fit n_params = %lld", dims0, dims1, (long long)n_params);
  MBPO_REQUIRE(dims0 <= SCALER_MAX_IN, MBPO_ERR_UNSUPPORTED, "ens_fold_scaler: dims0 = %d above %d", dims0, SCALER_MAX_IN);
  const long long total = (long long)n_members * n_params;
  MBPO_REQUIRE(out_params + total <= params || params + total <= out_params, MBPO_ERR_ARG,
               "ens_fold_scaler: out_params overlaps params (the bias sum reads the layer's unfolded weights)");
  const bool vec = (n_params & 3) == 0 && (dims1 & 3) == 0 && (((uintptr_t)params | (uintptr_t)out_params) & 15) == 0;
  long long bx = ((vec ? n_params / 4 : n_params) + 255) / 256;
  bx = bx < 1 ? 1 : (bx > 1024 ? 1024 : bx);
  hipStream_t st = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL(k_ens_fold_scaler<true>, dim3((unsigned)bx, (unsigned)n_members), dim3(256), 0, st, params, out_params,
                       (long long)n_params, dims0, dims1, scaler);
  else
    hipLaunchKernelGGL(k_ens_fold_scaler<false>, dim3((unsigned)bx, (unsigned)n_members), dim3(256), 0, st, params, out_params,
                       (long long)n_params, dims0, dims1, scaler);
  MBPO_CHECK_LAUNCH("ens_fold_scaler");
  return MBPO_OK;
}
