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

// Kernel arguments of both fused kernels (training step and evaluation).
struct EnsArgs {
  NetShape sh;
  const float *params;
  long long net_stride;
  int n_params, E, X, U, D, noff, roff;   // roff: reward target column, or -1
  const float *rows;
  const int *idx;                         // training: [E][n], a minibatch per member; evaluation: [n], shared by the members
  long long n;                            // rows per member
  int predict_delta;
  float min_std;
  float *slabs, *extras;                  // training: gradient slabs, loss partials [E][n_slots]; evaluation: extras = [2][E][n_slots]
  int n_slots, ld_xu, ld_h, ld_y, LH;
};

// One output element of the Gaussian NLL, the one place its terms are written: sigma = softplus(raw) + min_std, q = (t - mu) / sigma,
// the loss term 0.5 q^2 + log sigma and the squared error (t - mu)^2.  Padded rows and an unfitted reward head are masked by the callers.
struct NllTerm {
  float sg, q, nll, se;
};
__device__ __forceinline__ NllTerm ens_nll_term(float t, float mu, float raw, float min_std) {
  NllTerm o;
  o.sg = softplus_f(raw) + min_std;
  o.q = (t - mu) / o.sg;
  o.nll = 0.5f * o.q * o.q + logf(o.sg);
  const float d = t - mu;
  o.se = d * d;
  return o;
}
// ... and its gradient: d(nll * invB) / d mu and / d raw
__device__ __forceinline__ NllTerm ens_nll_grad(float t, float mu, float raw, float min_std, float invB, float *dmu, float *draw) {
  const NllTerm o = ens_nll_term(t, mu, raw, min_std);
  *dmu = -(o.q / o.sg) * invB;
  *draw = ((1.f - o.q * o.q) / o.sg) * sigmoid_f(raw) * invB;
  return o;
}

// Stage rows j0 .. j0 + 15 of the index list `idx` ([n]; zeros beyond n): s_xu [16][ld_xu] = [x, u], s_t [16][ld_y] = the regression
// target (X state columns, delta-encoded with predict_delta; then the reward at column X when roff >= 0).  No barrier.
__device__ __forceinline__ void ens_stage_tile(const EnsArgs &A, const int *idx, long long j0, float *s_xu, float *s_t, int tid,
                                               int nthreads) {
  const int X = A.X, U = A.U, ld_xu = A.ld_xu, ld_y = A.ld_y;
  for (int i2 = tid; i2 < 16 * (X + U); i2 += nthreads) {
    const int r = i2 & 15, c = i2 >> 4;
    const long long j = j0 + r;
    s_xu[r * ld_xu + c] = (j < A.n) ? A.rows[(long long)idx[j] * A.D + c] : 0.f;
  }
  for (int i2 = tid; i2 < 16 * X; i2 += nthreads) {
    const int r = i2 & 15, c = i2 >> 4;
    const long long j = j0 + r;
    float t = 0.f;
    if (j < A.n) {
      const float *row = A.rows + (long long)idx[j] * A.D;
      t = row[A.noff + c] - (A.predict_delta ? row[c] : 0.f);
    }
    s_t[r * ld_y + c] = t;
  }
  if (A.roff >= 0 && tid < 16) {
    const long long j = j0 + tid;
    s_t[tid * ld_y + X] = (j < A.n) ? A.rows[(long long)idx[j] * A.D + A.roff] : 0.f;
  }
}

template <int SP, bool WIDE>
__global__ void __launch_bounds__(128 * SP) k_ens_nll_fwd_bwd(EnsArgs A) {
  extern __shared__ __align__(16) float smem[];
  constexpr int HT = 4;
  const int tid_ = threadIdx.x, nthreads = 128 * SP;
  const int wave = __builtin_amdgcn_readfirstlane(tid_ >> 6);
  const int chain = wave / SP, sub = wave % SP;    // chain 0: forward, then dgrad; chain 1: wgrad
  const int e = blockIdx.x / A.n_slots, slot = blockIdx.x - e * A.n_slots;
  const int X = A.X, ld_xu = A.ld_xu, ld_h = A.ld_h, ld_y = A.ld_y, LH = A.LH;
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
  const float invB = 1.0f / (float)A.n;
  float *slab = A.slabs + ((long long)e * A.n_slots + slot) * A.n_params;
  const int *idx = A.idx + (long long)e * A.n;
  float loss = 0.f;
  bool first = true;
  const long long n_tiles = (A.n + 15) >> 4;
#pragma nounroll
  for (long long tile = slot; tile < n_tiles; tile += A.n_slots, first = false) {
    const int tid = opaque(tid_), lane = tid & 63;
    const long long j0 = tile * 16;
    WSet<HT, SP> R;
    if (chain == 0) chain_fwd_prefetch<HT, SP, WIDE>(R, A.sh, params, sub, lane);
    ens_stage_tile(A, idx, j0, s_xu, s_t, tid, nthreads);
    __syncthreads();
    if (chain == 0) chain_fwd_run<HT, SP, WIDE>(A.sh, params, s_xu, ld_xu, nullptr, nullptr, s_st, s_st + LH * T, s_y, ld_y, ld_h, L, sub, lane, R);
    else chain_idle_run(L);
    if (chain == 0) chain_dgrad_prefetch<HT, SP, WIDE>(R, A.sh, params, sub, lane);
    // d loss / d(mu, raw) per element, loss partial per row
    for (int i2 = tid; i2 < 16 * X; i2 += nthreads) {
      const int r = i2 & 15, c = i2 >> 4;
      const bool ok = j0 + r < A.n;
      float dmu, draw;
      const NllTerm el = ens_nll_grad(s_t[r * ld_y + c], s_y[r * ld_y + c], s_y[r * ld_y + X + c], A.min_std, invB, &dmu, &draw);
      s_dy[r * ld_y + c] = ok ? dmu : 0.f;
      s_dy[r * ld_y + X + c] = ok ? draw : 0.f;
      s_t[r * ld_y + X + 1 + c] = ok ? el.nll : 0.f;      // per-element loss, summed below
    }
    if (A.sh.N_out > 2 * X && tid < 16) {       // the reward head: its term, or zero gradient when it is not fitted
      const int r = tid;
      const bool ok = j0 + r < A.n && A.roff >= 0;
      float dmu, draw;
      const NllTerm el = ens_nll_grad(s_t[r * ld_y + X], s_y[r * ld_y + 2 * X], s_y[r * ld_y + 2 * X + 1], A.min_std, invB, &dmu, &draw);
      s_dy[r * ld_y + 2 * X] = ok ? dmu : 0.f;
      s_dy[r * ld_y + 2 * X + 1] = ok ? draw : 0.f;
      s_t[r * ld_y + 2 * X + 1] = ok ? el.nll : 0.f;
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

// The layered path's head, one workgroup per member over y [E][B][dout] and the targets t [B][X + 1] at t + e * t_stride (training:
// a minibatch per member, t_stride = B * (X + 1); evaluation: shared, 0).  The terms and their order are the fused kernels': the row's
// state terms summed first and the reward last; a thread adds its rows b = tid, tid + 256, ... in order, then a fixed tree over the
// threads.  GRAD (training): dy [E][B][dout] and metrics[e] = the member's loss; otherwise (evaluation) metrics[e] and, at
// metrics[E + e], the mean squared error.
template <bool GRAD>
__global__ void __launch_bounds__(256) k_ens_head(const float *y, const float *t, long long t_stride, int X, int dout, int roff, int B,
                                                  int E, float min_std, float *dy, float *metrics) {
  __shared__ float s_red[GRAD ? 1 : 2][256];
  const int e = blockIdx.x, tid = threadIdx.x;
  const float invB = 1.0f / (float)B;
  float acc = 0.f, acc2 = 0.f;
  for (int b = tid; b < B; b += 256) {
    const long long r = (long long)e * B + b;
    const float *yr = y + r * dout, *tr = t + e * t_stride + (long long)b * (X + 1);
    float *dr = GRAD ? dy + r * dout : nullptr;
    float a = 0.f, a2 = 0.f, dmu, draw;
    for (int c = 0; c < X; ++c) {
      const NllTerm el = ens_nll_grad(tr[c], yr[c], yr[X + c], min_std, invB, &dmu, &draw);
      if constexpr (GRAD) {
        dr[c] = dmu;
        dr[X + c] = draw;
      }
      a += el.nll;
      a2 += el.se;
    }
    if (dout > 2 * X) {                         // the reward head: its term, or zero gradient when it is not fitted
      const bool ok = roff >= 0;
      const NllTerm el = ens_nll_grad(tr[X], yr[2 * X], yr[2 * X + 1], min_std, invB, &dmu, &draw);
      if constexpr (GRAD) {
        dr[2 * X] = ok ? dmu : 0.f;
        dr[2 * X + 1] = ok ? draw : 0.f;
      }
      if (ok) {
        a += el.nll;
        a2 += el.se;
      }
    }
    acc += a;
    acc2 += a2;
  }
  s_red[0][tid] = acc;
  if constexpr (!GRAD) s_red[1][tid] = acc2;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) {
      s_red[0][tid] += s_red[0][tid + h];
      if constexpr (!GRAD) s_red[1][tid] += s_red[1][tid + h];
    }
    __syncthreads();
  }
  if (tid == 0) {
    metrics[e] = s_red[0][0] / (float)B;
    if constexpr (!GRAD) metrics[E + e] = s_red[1][0] / (float)B;
  }
}

struct EnsPlan {
  MlpDev dyn;
  bool layered;
  int n_slots, ld_xu, ld_h, ld_y, LH;
  size_t lds;
  long long total;
  // layered path: workspace offsets (floats); evaluation keeps no z / h / dy / part and ping-pongs its hidden layers through tmp0 / tmp1
  long long off_xu, off_t, off_z[MBPO_MAX_LAYERS + 1], off_h[MBPO_MAX_LAYERS + 1], off_y, off_dy, off_tmp0, off_tmp1, off_part;
};

// What the training and the evaluation plans share: the shape checks, the tile geometry and the choice of path.  `what` prefixes the
// messages; batch = rows per member.
static int ens_plan_shape(const char *what, int X, int U, const mbpo_mlp_desc &dynamics, int row_len, int noff, int roff, long long batch,
                          EnsPlan *pl) {
  MBPO_REQUIRE(X > 0 && U > 0 && batch > 0, MBPO_ERR_ARG, "%s: x_dim/u_dim/batch must be positive", what);
  mbpo_mlp_desc md = dynamics;
  if (!md.params) md.params = (const float *)16;
  char name[48];
  snprintf(name, sizeof name, "%s.dynamics", what);
  int rc = mbpo_make_mlp_dev(&md, &pl->dyn, name);
  if (rc != MBPO_OK) return rc;
  const int L = pl->dyn.n_layers;
  MBPO_REQUIRE(pl->dyn.dims[0] == X + U && (pl->dyn.dims[L] == 2 * X || pl->dyn.dims[L] == 2 * X + 2), MBPO_ERR_ARG,
               "%s: dynamics must map [x+u] -> [2x] (mean, raw std) or [2x+2] (+ reward mean, raw std)", what);
  MBPO_REQUIRE(roff >= -1 && roff < row_len, MBPO_ERR_ARG, "%s: reward_off %d outside the row", what, roff);
  MBPO_REQUIRE(roff < 0 || pl->dyn.dims[L] == 2 * X + 2, MBPO_ERR_ARG, "%s: reward_off needs a [x+u] -> [2x+2] ensemble", what);
  MBPO_REQUIRE(L >= 2, MBPO_ERR_ARG, "%s: the member networks need at least one hidden layer", what);
  MBPO_REQUIRE(row_len >= noff + X && noff >= X + U, MBPO_ERR_ARG, "%s: bad row_len / next_obs_off", what);
  bool all64 = true;
  for (int l = 1; l < L; ++l) all64 = all64 && pl->dyn.dims[l] == 64;
  pl->LH = L - 1;
  pl->ld_xu = up4(X + U) + 4;
  pl->ld_h = 68;
  pl->ld_y = up4(pl->dyn.dims[L]) + 4;
  // (the training tile decides for both: one shape, one path)
  pl->lds = sizeof(float) * (16ull * pl->ld_xu + 3ull * 16 * pl->ld_y + (size_t)(2 * pl->LH + 2) * 16 * pl->ld_h + 16);
  pl->layered = !all64 || pl->lds > 160 * 1024;
  if (!pl->layered) {
    const long long tiles = (batch + 15) / 16;
    long long cap = (2LL * mbpo_num_cus() + pl->dyn.n_nets - 1) / pl->dyn.n_nets;
    if (cap < 1) cap = 1;
    pl->n_slots = (int)(tiles < cap ? tiles : cap);
  } else {
    MBPO_REQUIRE(batch < (1LL << 24), MBPO_ERR_ARG, "%s: batch must be below 2^24 on the layered path", what);
  }
  return MBPO_OK;
}

// The fused kernels' arguments that both entry points fill alike, from the members the two public descriptors share (n = rows per
// member); slabs / extras are the caller's.
static EnsArgs ens_args(const EnsPlan &pl, const mbpo_mlp_desc &dynamics, int X, int U, const float *rows, int row_len, int noff, int roff,
                        const int *idx, long long n, int predict_delta, float min_std) {
  EnsArgs A;
  A.sh = net_shape(pl.dyn);
  A.params = dynamics.params; A.net_stride = pl.dyn.net_stride; A.n_params = pl.dyn.n_params; A.E = pl.dyn.n_nets;
  A.X = X; A.U = U; A.D = row_len; A.noff = noff; A.roff = roff;
  A.rows = rows; A.idx = idx; A.n = n; A.predict_delta = predict_delta; A.min_std = min_std;
  A.slabs = A.extras = nullptr;
  A.n_slots = pl.n_slots; A.ld_xu = pl.ld_xu; A.ld_h = pl.ld_h; A.ld_y = pl.ld_y; A.LH = pl.LH;
  return A;
}

static int ens_plan(const mbpo_ens_train_desc *d, EnsPlan *pl, bool need_ptrs) {
  MBPO_REQUIRE(d, MBPO_ERR_ARG, "ens_nll: null descriptor");
  int rc = ens_plan_shape("ens_nll", d->x_dim, d->u_dim, d->dynamics, d->row_len, d->next_obs_off, d->reward_off, d->batch, pl);
  if (rc != MBPO_OK) return rc;
  const int X = d->x_dim, U = d->u_dim, L = pl->dyn.n_layers, E = pl->dyn.n_nets;
  if (!pl->layered) {
    pl->total = (long long)E * pl->n_slots * pl->dyn.n_params + (((long long)E * pl->n_slots + 3) & ~3LL);
  } else {
    const long long EB = (long long)E * d->batch;
    const LayeredNet net = layered_net(pl->dyn, nullptr, pl->dyn.n_params, E);
    Carve c;
    pl->off_xu = c.take(EB * (X + U));
    pl->off_t = c.take(EB * (X + 1));
    for (int l = 1; l < L; ++l) {
      pl->off_z[l] = c.take(EB * pl->dyn.dims[l]);
      pl->off_h[l] = c.take(EB * pl->dyn.dims[l]);
    }
    pl->off_y = c.take(EB * pl->dyn.dims[L]);
    pl->off_dy = c.take(EB * pl->dyn.dims[L]);
    const long long mh = layered_max_hidden(net);
    pl->off_tmp0 = c.take(EB * mh);
    pl->off_tmp1 = c.take(EB * mh);
    pl->off_part = c.take(layered_part_floats(net, (int)d->batch));
    pl->total = c.off;
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
  hipLaunchKernelGGL(k_ens_head<true>, dim3(E), dim3(256), 0, st, (const float *)y, (const float *)t, (long long)B * (X + 1), X, dout,
                     d->reward_off, B, E, d->min_std, dy, d->metrics);
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
  const int E = pl.dyn.n_nets;
  EnsArgs A = ens_args(pl, d->dynamics, d->x_dim, d->u_dim, d->rows, d->row_len, d->next_obs_off, d->reward_off, d->idx, d->batch,
                       d->predict_delta, d->min_std);
  A.slabs = d->workspace; A.extras = d->workspace + (long long)E * pl.n_slots * pl.dyn.n_params;
  hipStream_t st = (hipStream_t)stream;
  rc = mbpo_with_bool(net_is_wide(A.sh), [&](auto W) { return mbpo_launch<k_ens_nll_fwd_bwd<4, W.value>>(E * pl.n_slots, 512, pl.lds, st, "ens_nll_grads", A); });
  if (rc != MBPO_OK) return rc;
  hipLaunchKernelGGL(k_ens_reduce, dim3((pl.dyn.n_params + 63) / 64, E), dim3(256), 0, st, (const float *)A.slabs, (const float *)A.extras,
                     pl.n_slots, pl.dyn.n_params, (long long)d->batch, d->grads, d->metrics);
  MBPO_CHECK_LAUNCH("ens_nll_grads");
  return MBPO_OK;
}

// ================================================================================================ model selection
// MBPO's model-training procedure (held-out loss per member, per-member best snapshot, elite members) — not the reference's, which
// has no learned model.  mbpo_ens_eval is the forward half of the step above on ONE index list shared by the members: the same
// per-element terms (ens_nll_term), the row's state terms summed first and the reward last, plus the squared error of the mean head.

// One workgroup = (member, slot), four waves = one forward chain; hidden activations ping-pong through two tiles (nothing is kept
// for a backward pass).  Partials to A.extras [2][E][n_slots].
template <bool WIDE>
__global__ void __launch_bounds__(256) k_ens_eval(EnsArgs A) {
  extern __shared__ __align__(16) float smem[];
  constexpr int HT = 4, SP = 4;
  const int tid_ = threadIdx.x, nthreads = 256;
  const int sub = __builtin_amdgcn_readfirstlane(tid_ >> 6);
  const int e = blockIdx.x / A.n_slots, slot = blockIdx.x - e * A.n_slots;
  const int X = A.X, ld_xu = A.ld_xu, ld_h = A.ld_h, ld_y = A.ld_y;
  const int T = 16 * ld_h;
  float *s_xu = smem;                       // [16][ld_xu]  [x, u]
  float *s_t = s_xu + 16 * ld_xu;           // [16][ld_y]   regression target: X state columns, then the reward
  float *s_y = s_t + 16 * ld_y;             // [16][ld_y]   (mu, raw)
  float *s_el = s_y + 16 * ld_y;            // [16][ld_y]   per-element NLL terms at [0, X], squared errors at [X + 1, 2X + 1]
  float *s_pp = s_el + 16 * ld_y;           // 2 hidden tiles
  float *s_ls = s_pp + 2 * T;               // [2][16] row sums
  const float *params = A.params + (long long)e * A.net_stride;
  const int L = A.sh.L;
  float loss = 0.f, sqe = 0.f;
  const long long n_tiles = (A.n + 15) >> 4;
#pragma nounroll
  for (long long tile = slot; tile < n_tiles; tile += A.n_slots) {
    const int tid = opaque(tid_), lane = tid & 63;
    const long long j0 = tile * 16;
    WSet<HT, SP> R;
    chain_fwd_prefetch<HT, SP, WIDE>(R, A.sh, params, sub, lane);
    ens_stage_tile(A, A.idx, j0, s_xu, s_t, tid, nthreads);
    __syncthreads();
    chain_fwd_run<HT, SP, WIDE>(A.sh, params, s_xu, ld_xu, s_pp, s_pp + T, nullptr, nullptr, s_y, ld_y, ld_h, L, sub, lane, R);
    for (int i2 = tid; i2 < 16 * X; i2 += nthreads) {
      const int r = i2 & 15, c = i2 >> 4;
      const bool ok = j0 + r < A.n;
      const NllTerm el = ens_nll_term(s_t[r * ld_y + c], s_y[r * ld_y + c], s_y[r * ld_y + X + c], A.min_std);
      s_el[r * ld_y + c] = ok ? el.nll : 0.f;
      s_el[r * ld_y + X + 1 + c] = ok ? el.se : 0.f;
    }
    if (A.roff >= 0 && tid < 16) {
      const int r = tid;
      const bool ok = j0 + r < A.n;
      const NllTerm el = ens_nll_term(s_t[r * ld_y + X], s_y[r * ld_y + 2 * X], s_y[r * ld_y + 2 * X + 1], A.min_std);
      s_el[r * ld_y + X] = ok ? el.nll : 0.f;
      s_el[r * ld_y + 2 * X + 1] = ok ? el.se : 0.f;
    }
    __syncthreads();
    if (tid < 32) {                          // threads 0..15: the rows' NLL, 16..31: their squared error
      const int r = tid & 15;
      const float *el = s_el + r * ld_y + (tid < 16 ? 0 : X + 1);
      float a = 0.f;
      for (int c = 0; c < X; ++c) a += el[c];
      if (A.roff >= 0) a += el[X];
      s_ls[tid] = a;
    }
    __syncthreads();
    if (tid == 0)
      for (int i = 0; i < 16; ++i) {
        loss += s_ls[i];
        sqe += s_ls[16 + i];
      }
  }
  if (tid_ == 0) {
    A.extras[(long long)e * A.n_slots + slot] = loss;
    A.extras[((long long)A.E + e) * A.n_slots + slot] = sqe;
  }
}

// metrics[m][e] = (sum over slots, in slot order) / n
__global__ void __launch_bounds__(64) k_ens_eval_reduce(const float *part, int n_slots, int n_out, long long n, float *metrics) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n_out) metrics[i] = slab_sum<16>(part + (long long)i * n_slots, 1, n_slots, 0) / (float)n;
}

static int ens_eval_plan(const mbpo_ens_eval_desc *d, EnsPlan *pl, bool need_ptrs) {
  MBPO_REQUIRE(d, MBPO_ERR_ARG, "ens_eval: null descriptor");
  int rc = ens_plan_shape("ens_eval", d->x_dim, d->u_dim, d->dynamics, d->row_len, d->next_obs_off, d->reward_off, d->n, pl);
  if (rc != MBPO_OK) return rc;
  const int X = d->x_dim, U = d->u_dim, L = pl->dyn.n_layers, E = pl->dyn.n_nets;
  Carve c;
  if (!pl->layered) {
    pl->lds = sizeof(float) * (16ull * pl->ld_xu + 3ull * 16 * pl->ld_y + 2ull * 16 * pl->ld_h + 32);
    c.take(2LL * E * pl->n_slots);
  } else {
    const LayeredNet net = layered_net(pl->dyn, nullptr, pl->dyn.n_params, E);
    const long long mh = layered_max_hidden(net);
    pl->off_xu = c.take(d->n * (X + U));
    pl->off_t = c.take(d->n * (X + 1));
    pl->off_tmp0 = c.take((long long)E * d->n * mh);
    pl->off_tmp1 = c.take((long long)E * d->n * mh);
    pl->off_y = c.take((long long)E * d->n * pl->dyn.dims[L]);
  }
  pl->total = c.off;
  if (need_ptrs)
    MBPO_REQUIRE(d->dynamics.params && d->rows && d->idx && d->metrics && d->workspace, MBPO_ERR_ARG, "ens_eval: null pointer");
  return MBPO_OK;
}

extern "C" int64_t mbpo_ens_eval_workspace_floats(const mbpo_ens_eval_desc *d) {
  EnsPlan pl;
  int rc = ens_eval_plan(d, &pl, false);
  if (rc != MBPO_OK) return rc;
  return pl.total;
}

extern "C" int mbpo_ens_eval(const mbpo_ens_eval_desc *d, void *stream) {
  EnsPlan pl;
  int rc = ens_eval_plan(d, &pl, true);
  if (rc != MBPO_OK) return rc;
  const int L = pl.dyn.n_layers, E = pl.dyn.n_nets, X = d->x_dim, U = d->u_dim;
  hipStream_t st = (hipStream_t)stream;
  if (pl.layered) {
    const int n = (int)d->n;
    float *ws = d->workspace;
    float *xu = ws + pl.off_xu, *t = ws + pl.off_t, *y = ws + pl.off_y;
    float *H[MBPO_MAX_LAYERS + 1];
    for (int l = 0; l <= MBPO_MAX_LAYERS; ++l) H[l] = ws + ((l & 1) ? pl.off_tmp1 : pl.off_tmp0);     // layer l reads H[l], writes H[l + 1]
    // the members share the rows: one gather (k_ens_gather with a single "member")
    hipLaunchKernelGGL(k_ens_gather, dim3((unsigned)((d->n + 255) / 256)), dim3(256), 0, st, d->rows, d->idx, d->row_len, X, U,
                       d->next_obs_off, d->reward_off, d->predict_delta, (long long)d->n, xu, t);
    MBPO_CHECK_LAUNCH("ens_eval.gather");
    const LayeredNet net = layered_net(pl.dyn, d->dynamics.params, pl.dyn.net_stride, E);
    rc = layered_forward(net, xu, 0, n, nullptr, H, y, st);
    if (rc != MBPO_OK) return rc;
    hipLaunchKernelGGL(k_ens_head<false>, dim3(E), dim3(256), 0, st, (const float *)y, (const float *)t, 0LL, X, pl.dyn.dims[L],
                       d->reward_off, n, E, d->min_std, (float *)nullptr, d->metrics);
    MBPO_CHECK_LAUNCH("ens_eval.head");
    return MBPO_OK;
  }
  EnsArgs A = ens_args(pl, d->dynamics, X, U, d->rows, d->row_len, d->next_obs_off, d->reward_off, d->idx, d->n, d->predict_delta,
                       d->min_std);
  A.extras = d->workspace;
  rc = mbpo_with_bool(net_is_wide(A.sh), [&](auto W) { return mbpo_launch<k_ens_eval<W.value>>(E * pl.n_slots, 256, pl.lds, st, "ens_eval", A); });
  if (rc != MBPO_OK) return rc;
  hipLaunchKernelGGL(k_ens_eval_reduce, dim3((2 * E + 63) / 64), dim3(64), 0, st, (const float *)A.extras, pl.n_slots, 2 * E, (long long)d->n,
                     d->metrics);
  MBPO_CHECK_LAUNCH("ens_eval");
  return MBPO_OK;
}

// ------------------------------------------------------------------------------------------------ snapshot and elites
// The member copy both calls end in: destination member j = blockIdx.y takes source member map[j], or is skipped when map[j] < 0.
// Bit copy (integer words).  16-byte accesses over the part of the member where source and destination are equally aligned (members
// are n_params floats apart, not necessarily a multiple of 4: the aligned part starts up to 3 words in), single words elsewhere.
__global__ void __launch_bounds__(256) k_ens_member_copy(const uint32_t *src, uint32_t *dst, long long n_params, const int *map) {
  const int j = blockIdx.y, m = map[j];
  if (m < 0) return;
  const uint32_t *s = src + (long long)m * n_params;
  uint32_t *d = dst + (long long)j * n_params;
  const long long i0 = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
  if ((((uintptr_t)s ^ (uintptr_t)d) & 15) != 0) {
    for (long long i = i0; i < n_params; i += stride) d[i] = s[i];
    return;
  }
  long long head = (long long)(((16 - ((uintptr_t)d & 15)) & 15) >> 2);
  if (head > n_params) head = n_params;
  const long long n_vec = (n_params - head) >> 2, tail = head + 4 * n_vec;
  const uint4 *s4 = reinterpret_cast<const uint4 *>(s + head);
  uint4 *d4 = reinterpret_cast<uint4 *>(d + head);
  for (long long v = i0; v < n_vec; v += stride) d4[v] = s4[v];
  if (i0 < head) d[i0] = s[i0];
  if (tail + i0 < n_params) d[tail + i0] = s[tail + i0];      // (at most 3 words; i0 < 256 reaches them in workgroup 0)
}

static int ens_member_copy(const float *src, float *dst, long long n_params, const int *map, int n_dst, hipStream_t st, const char *what) {
  long long bx = (n_params / 4 + 255) / 256;
  bx = bx < 1 ? 1 : (bx > 1024 ? 1024 : bx);
  hipLaunchKernelGGL(k_ens_member_copy, dim3((unsigned)bx, (unsigned)n_dst), dim3(256), 0, st, reinterpret_cast<const uint32_t *>(src),
                     reinterpret_cast<uint32_t *>(dst), n_params, map);
  MBPO_CHECK_LAUNCH(what);
  return MBPO_OK;
}

// One workgroup: the decision of mbpo_ens_keep_best.  Every member's test reads its own best_score entry before writing it.
__global__ void __launch_bounds__(64) k_ens_keep_decide(const float *score, float *best_score, int E, float rel_tol, int *state, int *map) {
  int any = 0;
  for (int e = threadIdx.x; e < E; e += 64) {
    const float s = score[e];
    const bool improved = isfinite(s) && s < best_score[e] * (1.0f - rel_tol);
    map[e] = improved ? e : -1;
    if (improved) best_score[e] = s;
    any |= improved ? 1 : 0;
  }
  any = __syncthreads_or(any);
  if (threadIdx.x == 0) {
    state[0] = any ? 0 : state[0] + 1;
    state[1] += 1;
  }
}

extern "C" int mbpo_ens_keep_best(const float *params, float *best_params, int64_t n_params, int32_t n_members, const float *score,
                                  float *best_score, float rel_tol, int32_t *state, int32_t *workspace, void *stream) {
  MBPO_REQUIRE(n_members > 0 && n_members <= 65535 && n_params > 0, MBPO_ERR_ARG, "ens_keep_best: n_members must be in [1, 65535], n_params positive");
  MBPO_REQUIRE(params && best_params && score && best_score && state && workspace, MBPO_ERR_ARG, "ens_keep_best: null pointer");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_ens_keep_decide, dim3(1), dim3(64), 0, st, score, best_score, n_members, rel_tol, state, workspace);
  MBPO_CHECK_LAUNCH("ens_keep_best.decide");
  return ens_member_copy(params, best_params, n_params, workspace, n_members, st, "ens_keep_best.copy");
}

// One workgroup: elite_idx[rank of member e] = e for the ranks below n_elites (the ranks are a permutation: rank_before is total)
__global__ void __launch_bounds__(64) k_ens_rank(const float *score, int E, int n_elites, int *elite_idx) {
  for (int e = threadIdx.x; e < E; e += 64) {
    const float v = score[e];
    int r = 0;
    for (int j = 0; j < E; ++j) r += rank_before(score[j], j, v, e) ? 1 : 0;
    if (r < n_elites) elite_idx[r] = e;
  }
}

extern "C" int mbpo_ens_pick_elites(const float *params, int64_t n_params, int32_t n_members, const float *score, int32_t n_elites,
                                    int32_t *elite_idx, float *elite_params, void *stream) {
  MBPO_REQUIRE(n_members > 0 && n_members <= 65535 && n_params > 0, MBPO_ERR_ARG, "ens_pick_elites: n_members must be in [1, 65535], n_params positive");
  MBPO_REQUIRE(n_elites > 0 && n_elites <= n_members, MBPO_ERR_ARG, "ens_pick_elites: n_elites %d outside [1, n_members = %d]", n_elites, n_members);
  MBPO_REQUIRE(params && score && elite_idx && elite_params, MBPO_ERR_ARG, "ens_pick_elites: null pointer");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_ens_rank, dim3(1), dim3(64), 0, st, score, n_members, n_elites, elite_idx);
  MBPO_CHECK_LAUNCH("ens_pick_elites.rank");
  return ens_member_copy(params, elite_params, n_params, elite_idx, n_elites, st, "ens_pick_elites.copy");
}
