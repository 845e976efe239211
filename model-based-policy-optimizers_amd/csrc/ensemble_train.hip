// ensemble_train.hip — N3: the model-learning step that feeds the rollout path — Gaussian negative
// log-likelihood gradients of every ensemble member on its own (bootstrapped) minibatch of true transitions.
// Not in the reference (its model would come from the external `bsm` package, setup.py:22): semantics are this build's,
// chosen to be the exact inverse of what the rollout kernel consumes (EnsembleDynamics.next_state):
//     (mu, raw) = MLP_e([x, u]);  mean = mu (+ x if predict_delta);  sigma = softplus(raw) + min_std
//     loss_e = mean_b sum_d [ 0.5 ((x'_d - mean_d) / sigma_d)^2 + log sigma_d ]          (+ const)
// With a reward head (reward_off >= 0, outputs [mu | raw | mu_r | raw_r]) the loss gains the same term for r = row[reward_off] at
// output columns 2X, 2X + 1 (staged as target column X); its loss element is summed after the state's.
// Two paths, the same loss and gradient:
//  * fused (hidden layers all 64 wide, and the 16-row tile's stored activations fit 160 KiB of LDS): one workgroup = (member,
//    16-row tile): forward chain with stored activations, elementwise output gradient, then a dgrad and a wgrad chain side by side
//    (chain_run.hpp); a workgroup walks tiles and accumulates into its slab; fixed-order reduce.  Two launches.
//  * layered (every other shape: any hidden sizes, e.g. MBPO's 4 x 200, or a 64-wide stack too deep for the LDS plan): gather the
//    members' minibatches, the forward as one GEMM launch per Dense layer (layered.hpp, E nets with per-net inputs), the NLL head
//    (output gradient, per-member loss in a fixed order), the backward's GEMM levels straight into `grads` ([W | b] per layer).
//    About 2L + 2 launches, no atomics, deterministic.
// fp32 MFMA; algorithmic work per (member, sample): 3 * 2M FLOP, HBM 4*(2x+u) B gathered.
#include "common.hpp"
#include "chain_run.hpp"
#include "layered.hpp"

struct EnsTrainArgs {
  NetShape sh;
  const float *params;
  long long net_stride;
  int n_params, E, X, U, D, noff, roff;   // roff: reward target column, or -1
  const float *rows;
  const int *idx;
  long long batch;
  int predict_delta;
  float min_std;
  float *slabs, *extras;
  int n_slots, ld_xu, ld_h, ld_y, LH;
};

template <int SP, bool WIDE>
__global__ void __launch_bounds__(128 * SP) k_ens_nll_fwd_bwd(EnsTrainArgs A) {
  extern __shared__ __align__(16) float smem[];
  constexpr int HT = 4;
  const int tid_ = threadIdx.x, nthreads = 128 * SP;
  const int wave = __builtin_amdgcn_readfirstlane(tid_ >> 6);
  const int chain = wave / SP, sub = wave % SP;    // chain 0: forward, then dgrad; chain 1: wgrad
  const int e = blockIdx.x / A.n_slots, slot = blockIdx.x - e * A.n_slots;
  const int X = A.X, U = A.U, ld_xu = A.ld_xu, ld_h = A.ld_h, ld_y = A.ld_y, LH = A.LH;
  const int T = 16 * ld_h;
  float *s_xu = smem;                       // [16][ld_xu]  [x, u]
  float *s_t = s_xu + 16 * ld_xu;           // [16][ld_y]   regression target (X state columns, then the reward), loss elements from X + 1
  float *s_y = s_t + 16 * ld_y;             // [16][ld_y]   (mu, raw)
  float *s_dy = s_y + 16 * ld_y;            // [16][ld_y]
  float *s_st = s_dy + 16 * ld_y;           // 2*LH tiles: z, h
  float *s_pp = s_st + 2 * LH * T;          // 2 delta tiles
  float *s_ls = s_pp + 2 * T;               // [16] loss partials
  const float *params = A.params + (long long)e * A.net_stride;
  const int L = A.sh.L;
  const float invB = 1.0f / (float)A.batch;
  float *slab = A.slabs + ((long long)e * A.n_slots + slot) * A.n_params;
  const int *idx = A.idx + (long long)e * A.batch;
  float loss = 0.f;
  bool first = true;
  const long long n_tiles = (A.batch + 15) >> 4;
#pragma nounroll
  for (long long tile = slot; tile < n_tiles; tile += A.n_slots, first = false) {
    const int tid = opaque(tid_), lane = tid & 63;
    const long long j0 = tile * 16;
    WSet<HT, SP> R;
    if (chain == 0) chain_fwd_prefetch<HT, SP, WIDE>(R, A.sh, params, sub, lane);
    for (int i2 = tid; i2 < 16 * (X + U); i2 += nthreads) {
      const int r = i2 & 15, c = i2 >> 4;
      const long long j = j0 + r;
      s_xu[r * ld_xu + c] = (j < A.batch) ? A.rows[(long long)idx[j] * A.D + c] : 0.f;
    }
    for (int i2 = tid; i2 < 16 * X; i2 += nthreads) {
      const int r = i2 & 15, c = i2 >> 4;
      const long long j = j0 + r;
      float t = 0.f;
      if (j < A.batch) {
        const float *row = A.rows + (long long)idx[j] * A.D;
        t = row[A.noff + c] - (A.predict_delta ? row[c] : 0.f);
      }
      s_t[r * ld_y + c] = t;
    }
    if (A.roff >= 0 && tid < 16) {
      const long long j = j0 + tid;
      s_t[tid * ld_y + X] = (j < A.batch) ? A.rows[(long long)idx[j] * A.D + A.roff] : 0.f;
    }
    __syncthreads();
    if (chain == 0) chain_fwd_run<HT, SP, WIDE>(A.sh, params, s_xu, ld_xu, nullptr, nullptr, s_st, s_st + LH * T, s_y, ld_y, ld_h, L, sub, lane, R);
    else chain_idle_run(L);
    if (chain == 0) chain_dgrad_prefetch<HT, SP, WIDE>(R, A.sh, params, sub, lane);
    // d loss / d(mu, raw) per element, loss partial per row
    for (int i2 = tid; i2 < 16 * X; i2 += nthreads) {
      const int r = i2 & 15, c = i2 >> 4;
      const bool ok = j0 + r < A.batch;
      const float mu = s_y[r * ld_y + c], raw = s_y[r * ld_y + X + c];
      const float sg = softplus_f(raw) + A.min_std;
      const float q = (s_t[r * ld_y + c] - mu) / sg;
      s_dy[r * ld_y + c] = ok ? -(q / sg) * invB : 0.f;
      s_dy[r * ld_y + X + c] = ok ? ((1.f - q * q) / sg) * sigmoid_f(raw) * invB : 0.f;
      s_t[r * ld_y + X + 1 + c] = ok ? 0.5f * q * q + logf(sg) : 0.f;      // per-element loss, summed below
    }
    if (A.sh.N_out > 2 * X && tid < 16) {       // the reward head: its term, or zero gradient when it is not fitted
      const int r = tid;
      const bool ok = j0 + r < A.batch && A.roff >= 0;
      const float mu = s_y[r * ld_y + 2 * X], raw = s_y[r * ld_y + 2 * X + 1];
      const float sg = softplus_f(raw) + A.min_std;
      const float q = (s_t[r * ld_y + X] - mu) / sg;
      s_dy[r * ld_y + 2 * X] = ok ? -(q / sg) * invB : 0.f;
      s_dy[r * ld_y + 2 * X + 1] = ok ? ((1.f - q * q) / sg) * sigmoid_f(raw) * invB : 0.f;
      s_t[r * ld_y + 2 * X + 1] = ok ? 0.5f * q * q + logf(sg) : 0.f;
    }
    __syncthreads();
    if (tid < 16) {
      float a = 0.f;
      for (int c = 0; c < X; ++c) a += s_t[tid * ld_y + X + 1 + c];
      if (A.roff >= 0) a += s_t[tid * ld_y + 2 * X + 1];
      s_ls[tid] = a;
    }
    if (chain == 0) chain_dgrad_run<HT, SP, WIDE>(A.sh, params, s_dy, ld_y, s_st, s_pp, s_pp + T, nullptr, ld_xu, ld_h, L, sub, lane, R);
    else chain_wgrad_run<HT, SP, WIDE>(A.sh, s_xu, ld_xu, s_st + LH * T, s_dy, ld_y, s_pp, s_pp + T, slab, !first, ld_h, L, sub, lane);
    if (tid == 0)
      for (int i = 0; i < 16; ++i) loss += s_ls[i];
    __syncthreads();
  }
  if (tid_ == 0) A.extras[(long long)e * A.n_slots + slot] = loss;
}

__global__ void __launch_bounds__(256) k_ens_reduce(const float *slabs, const float *extras, int n_slots, int n_params, long long batch,
                                                     float *grads, float *metrics) {
  const int e = blockIdx.y;
  const int i = blockIdx.x * 64 + (threadIdx.x & 63);
  const float gsum = slab_sum_wg64(slabs + (long long)e * n_slots * n_params, n_params, n_slots, i, i < n_params);
  if (threadIdx.x < 64 && i < n_params) grads[(long long)e * n_params + i] = gsum;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const float a = slab_sum<16>(extras + (long long)e * n_slots, 1, n_slots, 0);
    metrics[e] = a / (float)batch;
  }
}

// ------------------------------------------------------------------------------------------------ layered path
// xu [E][B][X+U] = rows[idx[e][b]][0 : X+U];  t [E][B][X+1] = the regression targets (the state's X, then the reward or 0)
__global__ void __launch_bounds__(256) k_ens_gather(const float *rows, const int *idx, int D, int X, int U, int noff, int roff,
                                                    int predict_delta, long long n_rows, float *xu, float *t) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;     // (member, row) = e * B + b
  if (i >= n_rows) return;
  const float *row = rows + (long long)idx[i] * D;
  float *o = xu + i * (X + U);
  for (int c = 0; c < X + U; ++c) o[c] = row[c];
  float *tt = t + i * (X + 1);
  for (int c = 0; c < X; ++c) tt[c] = row[noff + c] - (predict_delta ? row[c] : 0.f);
  tt[X] = roff >= 0 ? row[roff] : 0.f;
}

// One workgroup per member: dy [E][B][dout] and the member's loss.  The formulas are k_ens_nll_fwd_bwd's: the same per-element
// terms, the row's state terms summed first and the reward last; a thread adds its rows b = tid, tid + 256, ... in order, then a
// fixed tree over the threads.
__global__ void __launch_bounds__(256) k_ens_nll_head(const float *y, const float *t, int X, int dout, int roff, int B, float min_std,
                                                      float *dy, float *metrics) {
  __shared__ float s_red[256];
  const int e = blockIdx.x, tid = threadIdx.x;
  const float invB = 1.0f / (float)B;
  float acc = 0.f;
  for (int b = tid; b < B; b += 256) {
    const long long r = (long long)e * B + b;
    const float *yr = y + r * dout, *tr = t + r * (X + 1);
    float *dr = dy + r * dout;
    float a = 0.f;
    for (int c = 0; c < X; ++c) {
      const float mu = yr[c], raw = yr[X + c];
      const float sg = softplus_f(raw) + min_std;
      const float q = (tr[c] - mu) / sg;
      dr[c] = -(q / sg) * invB;
      dr[X + c] = ((1.f - q * q) / sg) * sigmoid_f(raw) * invB;
      a += 0.5f * q * q + logf(sg);
    }
    if (dout > 2 * X) {                         // the reward head: its term, or zero gradient when it is not fitted
      const bool ok = roff >= 0;
      const float mu = yr[2 * X], raw = yr[2 * X + 1];
      const float sg = softplus_f(raw) + min_std;
      const float q = (tr[X] - mu) / sg;
      dr[2 * X] = ok ? -(q / sg) * invB : 0.f;
      dr[2 * X + 1] = ok ? ((1.f - q * q) / sg) * sigmoid_f(raw) * invB : 0.f;
      if (ok) a += 0.5f * q * q + logf(sg);
    }
    acc += a;
  }
  s_red[tid] = acc;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) s_red[tid] += s_red[tid + h];
    __syncthreads();
  }
  if (tid == 0) metrics[e] = s_red[0] / (float)B;
}

struct EnsPlan {
  MlpDev dyn;
  bool layered;
  int n_slots, ld_xu, ld_h, ld_y, LH;
  size_t lds;
  long long total;
  // layered path: workspace offsets (floats)
  long long off_xu, off_t, off_z[MBPO_MAX_LAYERS + 1], off_h[MBPO_MAX_LAYERS + 1], off_y, off_dy, off_tmp0, off_tmp1, off_part;
};

static int ens_plan(const mbpo_ens_train_desc *d, EnsPlan *pl, bool need_ptrs) {
  MBPO_REQUIRE(d, MBPO_ERR_ARG, "ens_nll: null descriptor");
  MBPO_REQUIRE(d->x_dim > 0 && d->u_dim > 0 && d->batch > 0, MBPO_ERR_ARG, "ens_nll: x_dim/u_dim/batch must be positive");
  mbpo_mlp_desc md = d->dynamics;
  if (!md.params) md.params = (const float *)16;
  int rc = mbpo_make_mlp_dev(&md, &pl->dyn, "ens_nll.dynamics");
  if (rc != MBPO_OK) return rc;
  const int X = d->x_dim, U = d->u_dim, L = pl->dyn.n_layers;
  MBPO_REQUIRE(pl->dyn.dims[0] == X + U && (pl->dyn.dims[L] == 2 * X || pl->dyn.dims[L] == 2 * X + 2), MBPO_ERR_ARG,
               "ens_nll: dynamics must map [x+u] -> [2x] (mean, raw std) or [2x+2] (+ reward mean, raw std)");
  MBPO_REQUIRE(d->reward_off >= -1 && d->reward_off < d->row_len, MBPO_ERR_ARG, "ens_nll: reward_off %d outside the row", d->reward_off);
  MBPO_REQUIRE(d->reward_off < 0 || pl->dyn.dims[L] == 2 * X + 2, MBPO_ERR_ARG, "ens_nll: reward_off needs a [x+u] -> [2x+2] ensemble");
  MBPO_REQUIRE(L >= 2, MBPO_ERR_ARG, "ens_nll: the member networks need at least one hidden layer");
  MBPO_REQUIRE(d->row_len >= d->next_obs_off + X && d->next_obs_off >= X + U, MBPO_ERR_ARG, "ens_nll: bad row_len / next_obs_off");
  bool all64 = true;
  for (int l = 1; l < L; ++l) all64 = all64 && pl->dyn.dims[l] == 64;
  pl->LH = L - 1;
  pl->ld_xu = up4(X + U) + 4;
  pl->ld_h = 68;
  pl->ld_y = up4(pl->dyn.dims[L]) + 4;
  pl->lds = sizeof(float) * (16ull * pl->ld_xu + 3ull * 16 * pl->ld_y + (size_t)(2 * pl->LH + 2) * 16 * pl->ld_h + 16);
  const int E = pl->dyn.n_nets;
  pl->layered = !all64 || pl->lds > 160 * 1024;
  if (!pl->layered) {
    const long long tiles = (d->batch + 15) / 16;
    long long cap = (2LL * mbpo_num_cus() + E - 1) / E;
    if (cap < 1) cap = 1;
    pl->n_slots = (int)(tiles < cap ? tiles : cap);
    pl->total = (long long)E * pl->n_slots * pl->dyn.n_params + (((long long)E * pl->n_slots + 3) & ~3LL);
  } else {
    MBPO_REQUIRE(d->batch < (1LL << 24), MBPO_ERR_ARG, "ens_nll: batch must be below 2^24 on the layered path");
    const long long EB = (long long)E * d->batch;
    const LayeredNet net = layered_net(pl->dyn, nullptr, pl->dyn.n_params, E);
    long long off = 0;
    auto take = [&](long long n) { const long long o = off; off += (n + 3) & ~3LL; return o; };
    pl->off_xu = take(EB * (X + U));
    pl->off_t = take(EB * (X + 1));
    for (int l = 1; l < L; ++l) {
      pl->off_z[l] = take(EB * pl->dyn.dims[l]);
      pl->off_h[l] = take(EB * pl->dyn.dims[l]);
    }
    pl->off_y = take(EB * pl->dyn.dims[L]);
    pl->off_dy = take(EB * pl->dyn.dims[L]);
    const long long mh = layered_max_hidden(net);
    pl->off_tmp0 = take(EB * mh);
    pl->off_tmp1 = take(EB * mh);
    pl->off_part = take(layered_part_floats(net, (int)d->batch));
    pl->total = off;
  }
  if (need_ptrs)
    MBPO_REQUIRE(d->dynamics.params && d->rows && d->idx && d->grads && d->metrics && d->workspace, MBPO_ERR_ARG, "ens_nll: null pointer");
  return MBPO_OK;
}

extern "C" int64_t mbpo_ens_nll_workspace_floats(const mbpo_ens_train_desc *d) {
  EnsPlan pl;
  int rc = ens_plan(d, &pl, false);
  if (rc != MBPO_OK) return rc;
  return pl.total;
}

static int ens_nll_layered(const mbpo_ens_train_desc *d, const EnsPlan &pl, hipStream_t st) {
  const int L = pl.dyn.n_layers, E = pl.dyn.n_nets, X = d->x_dim, U = d->u_dim, dout = pl.dyn.dims[L];
  const int B = (int)d->batch;
  const long long EB = (long long)E * B;
  float *ws = d->workspace;
  float *xu = ws + pl.off_xu, *t = ws + pl.off_t, *y = ws + pl.off_y, *dy = ws + pl.off_dy;
  float *Z[MBPO_MAX_LAYERS + 1], *H[MBPO_MAX_LAYERS + 1];
  for (int l = 0; l <= MBPO_MAX_LAYERS; ++l) Z[l] = H[l] = nullptr;
  for (int l = 1; l < L; ++l) {
    Z[l] = ws + pl.off_z[l];
    H[l] = ws + pl.off_h[l];
  }
  hipLaunchKernelGGL(k_ens_gather, dim3((unsigned)((EB + 255) / 256)), dim3(256), 0, st, d->rows, d->idx, d->row_len, X, U,
                     d->next_obs_off, d->reward_off, d->predict_delta, EB, xu, t);
  MBPO_CHECK_LAUNCH("ens_nll_grads.gather");
  const LayeredNet net = layered_net(pl.dyn, d->dynamics.params, pl.dyn.net_stride, E);
  int rc = layered_forward(net, xu, (long long)B * (X + U), B, Z, H, y, st);
  if (rc != MBPO_OK) return rc;
  hipLaunchKernelGGL(k_ens_nll_head, dim3(E), dim3(256), 0, st, (const float *)y, (const float *)t, X, dout, d->reward_off, B, d->min_std,
                     dy, d->metrics);
  MBPO_CHECK_LAUNCH("ens_nll_grads.head");
  // every weight and bias of every member is written: the bias gradient is the last row of its layer's [K + 1][N] block
  return layered_backward(net, xu, (long long)B * (X + U), B, Z, H, dy, d->grads, pl.dyn.n_params, nullptr, ws + pl.off_tmp0,
                          ws + pl.off_tmp1, ws + pl.off_part, st);
}

extern "C" int mbpo_ens_nll_grads(const mbpo_ens_train_desc *d, void *stream) {
  EnsPlan pl;
  int rc = ens_plan(d, &pl, true);
  if (rc != MBPO_OK) return rc;
  if (pl.layered) return ens_nll_layered(d, pl, (hipStream_t)stream);
  EnsTrainArgs A;
  const int E = pl.dyn.n_nets;
  A.sh = net_shape(pl.dyn);
  A.params = d->dynamics.params; A.net_stride = pl.dyn.net_stride; A.n_params = pl.dyn.n_params; A.E = E;
  A.X = d->x_dim; A.U = d->u_dim; A.D = d->row_len; A.noff = d->next_obs_off; A.roff = d->reward_off;
  A.rows = d->rows; A.idx = d->idx; A.batch = d->batch; A.predict_delta = d->predict_delta; A.min_std = d->min_std;
  A.slabs = d->workspace; A.extras = d->workspace + (long long)E * pl.n_slots * pl.dyn.n_params;
  A.n_slots = pl.n_slots; A.ld_xu = pl.ld_xu; A.ld_h = pl.ld_h; A.ld_y = pl.ld_y; A.LH = pl.LH;
  hipStream_t st = (hipStream_t)stream;
  rc = mbpo_with_bool(net_is_wide(A.sh), [&](auto W) { return mbpo_launch<k_ens_nll_fwd_bwd<4, W.value>>(E * pl.n_slots, 512, pl.lds, st, "ens_nll_grads", A); });
  if (rc != MBPO_OK) return rc;
  hipLaunchKernelGGL(k_ens_reduce, dim3((pl.dyn.n_params + 63) / 64, E), dim3(256), 0, st, (const float *)A.slabs, (const float *)A.extras,
                     pl.n_slots, pl.dyn.n_params, (long long)d->batch, d->grads, d->metrics);
  MBPO_CHECK_LAUNCH("ens_nll_grads");
  return MBPO_OK;
}
