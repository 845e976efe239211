// terminal_value.hip — terminal values (include/mbpo_hip.h "terminal values"): a learned critic evaluated at the terminal state of every
// planned trajectory, weighted and stored or added into the reward the planner's update reads.  iCEM's single and batched paths issue
// one launch of mbpo_terminal_value_eval between the reward source and the update, and only when a TerminalValue was given.  A compile
// unit of its own: a caller added to rollout.hip or icem.hip moves the register and spill figures of the kernels already there.
//
// Decomposition, as k_ensemble_forward's (ens_forward.hpp): one workgroup owns a tile of 16 terminal states and walks tiles persistently
// (tile += gridDim.x); activations live in LDS, weights stream from L2 (a policy and two critics of 64x3 are ~0.1 MB, shared by every
// workgroup); one wave walks a whole (tile, network) chain (wave_mlp.hpp), the critics side by side on waves 0 and 1.
//   1  gather: the 16 states through x_stride (no alignment promise: scalar loads), normalised into s_in[:, 0 .. X).  Threads 0 .. 15 also
//      read their row's raw components again (the loads are independent and in flight together, the lines are the ones the gather just
//      touched) and keep the row's finiteness in a register until phase 5: no LDS flag, no barrier for one.
//   2  kind Q: wave 0 walks the policy chain into s_pol                                   (wave 1 waits at the barrier)
//   3  kind Q: tanh (the accurate tanhf) of the loc half, written behind the normalised state: s_in[:, X .. X + A)
//   4  wave k < n_critics walks critic k on s_in into s_q[k]
//   5  threads 0 .. 15: the minimum over critics, fl(weight * v), then the strided store or fl(out + .); a row whose state was not
//      finite stores -inf.  Each out element is written by exactly one thread: no atomics.
// A NaN or infinity in row r of the MFMA's A operand reaches only row r of its result, so a bad row leaves its tile-mates' bits alone.
// No barrier closes the tile loop: phase 5 reads s_q and registers only, and the next tile's writes to s_q lie behind its own barriers.
// The kernel is instantiated per hidden width H in {64, 128, 256}: H is the larger of the policy's and the critics' width, and a network
// of the smaller width runs wave_dense_fwd's partial-tile paths (correct, not the fast path).
#include "common.hpp"
#include "wave_mlp.hpp"
#include "rollout_shared.hpp"

struct TermValueArgs {
  MlpDev critic, policy;
  int X, A;                              // A == 0: kind V
  const float *norm_mean, *norm_std;     // both or neither
  const float *x;
  long long x_stride;
  float *out;
  long long out_stride;
  long long n;
  float weight;
  int accumulate;
  int ld_in, ld_h, ld_pol, ld_q;         // LDS row strides (floats, multiples of 4)
};

#define TERM_VALUE_LD_Q 8

// (two waves per SIMD, k_ensemble_forward's budget of 256 registers a lane: left alone the compiler takes accumulation registers on top of
// 227 and halves the occupancy; at three waves the 64-wide chain spills)
template <int H>
__global__ void __launch_bounds__(128, 2) k_terminal_value(TermValueArgs T) {
  extern __shared__ __align__(16) float smem[];
  constexpr int HT = H / 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x;
  const int X = T.X, A = T.A, K = T.critic.n_nets;
  const int tile_h = 16 * T.ld_h;
  float *s_in = smem;                                // [16][ld_in]: n(x), then tanh(loc) for kind Q
  float *s_pol = s_in + 16 * T.ld_in;                // [16][ld_pol]: the policy's output layer (kind Q)
  float *s_q = s_pol + 16 * T.ld_pol;                // [2][16][ld_q]: the critics' outputs, column 0
  float *s_pp = s_q + 2 * 16 * T.ld_q;               // [waves][2] hidden ping-pong tiles
  float *pp0 = s_pp + wave * 2 * tile_h, *pp1 = pp0 + tile_h;
  const long long n_tiles = (T.n + 15) >> 4;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long row0 = tile * 16;
    // 1 — gather and normalise; rows past n read nothing and carry zeros
    bool bad = false;
    if (tid < 16 && row0 + tid < T.n) {
      const float *xr = T.x + (row0 + tid) * T.x_stride;
      for (int c = 0; c < X; ++c) {
        const float v = xr[c];
        bad |= !(fabsf(v) < __builtin_inff());       // (NaN fails the compare too)
      }
    }
    for (int idx = tid; idx < 16 * X; idx += nthreads) {
      const int r = idx / X, c = idx - r * X;
      const long long row = row0 + r;
      float v = 0.f;
      if (row < T.n) {
        v = T.x[row * T.x_stride + c];
        if (T.norm_mean) v = (v - T.norm_mean[c]) / T.norm_std[c];
      }
      s_in[r * T.ld_in + c] = v;
    }
    __syncthreads();
    if (A > 0) {      // (a kernel argument: every thread takes the barriers or none does)
      // 2 — a = tanh(loc(pi(n(x))))
      if (wave == 0) wave_mlp_fwd<HT>(T.policy, T.policy.params, s_in, T.ld_in, pp0, pp1, nullptr, nullptr, T.ld_h, s_pol, T.ld_pol, lane);
      __syncthreads();
      // 3
      for (int idx = tid; idx < 16 * A; idx += nthreads) {
        const int r = idx / A, c = idx - r * A;
        s_in[r * T.ld_in + X + c] = tanhf(s_pol[r * T.ld_pol + c]);
      }
      __syncthreads();
    }
    // 4 — the critics, one wave each
    if (wave < K)
      wave_mlp_fwd<HT>(T.critic, T.critic.params + (long long)wave * T.critic.net_stride, s_in, T.ld_in, pp0, pp1, nullptr, nullptr, T.ld_h,
                       s_q + wave * 16 * T.ld_q, T.ld_q, lane);
    __syncthreads();
    // 5 — min, product, store or add
    if (tid < 16 && row0 + tid < T.n) {
      float v = s_q[tid * T.ld_q];
      if (K > 1) {
        const float v1 = s_q[(16 + tid) * T.ld_q];
        v = (v1 < v || v1 != v1) ? v1 : v;           // (torch.minimum: a NaN wins)
      }
      const float bonus = __fmul_rn(T.weight, v);
      float *o = T.out + (row0 + tid) * T.out_stride;
      float res = bonus;
      if (T.accumulate) res = __fadd_rn(*o, bonus);
      *o = bad ? -__builtin_inff() : res;
    }
  }
}

// a descriptor whose params may still be NULL (n == 0 asks for nothing): shapes are validated against a placeholder
static int term_value_mlp(const mbpo_mlp_desc *d, MlpDev *out, const char *name) {
  mbpo_mlp_desc md = *d;
  if (!md.params) md.params = (const float *)16;
  const int rc = mbpo_make_mlp_dev(&md, out, name);
  out->params = d->params;
  if (rc == MBPO_OK && out->n_nets == 1) out->net_stride = out->n_params;
  return rc;
}

static bool term_value_mul_fits(long long a, long long b) { return a == 0 || b <= 0x7fffffffffffffffLL / a; }

extern "C" int mbpo_terminal_value_eval(const mbpo_terminal_value_desc *d, void *stream) {
  MBPO_REQUIRE(d != nullptr, MBPO_ERR_ARG, "terminal_value_eval: null descriptor");
  MBPO_REQUIRE(d->x_dim >= 1, MBPO_ERR_ARG, "terminal_value_eval: x_dim=%d < 1", d->x_dim);
  MBPO_REQUIRE(d->action_dim >= 0, MBPO_ERR_ARG, "terminal_value_eval: action_dim=%d < 0", d->action_dim);
  MBPO_REQUIRE(d->n >= 0, MBPO_ERR_ARG, "terminal_value_eval: n < 0");
  MBPO_REQUIRE(d->accumulate == 0 || d->accumulate == 1, MBPO_ERR_ARG, "terminal_value_eval: accumulate=%d is neither 0 nor 1", d->accumulate);
  const int X = d->x_dim, A = d->action_dim;
  TermValueArgs T;
  int rc = term_value_mlp(&d->critic, &T.critic, "terminal_value_eval.critic");
  if (rc != MBPO_OK) return rc;
  MBPO_REQUIRE(T.critic.n_nets == 1 || T.critic.n_nets == 2, MBPO_ERR_ARG, "terminal_value_eval: critic.n_nets=%d is neither 1 nor 2",
               T.critic.n_nets);
  MBPO_REQUIRE(A == 0 || T.critic.n_nets == 2, MBPO_ERR_ARG, "terminal_value_eval: kind Q (action_dim=%d) needs critic.n_nets=2, got %d", A,
               T.critic.n_nets);
  MBPO_REQUIRE((long long)T.critic.dims[0] == (long long)X + A, MBPO_ERR_ARG,
               "terminal_value_eval: critic.dims[0]=%d is not x_dim + action_dim = %d + %d", T.critic.dims[0], X, A);
  MBPO_REQUIRE(T.critic.dims[T.critic.n_layers] == 1, MBPO_ERR_ARG, "terminal_value_eval: critic.dims[%d]=%d, a critic ends in one output",
               T.critic.n_layers, T.critic.dims[T.critic.n_layers]);
  if (A > 0) {
    rc = term_value_mlp(&d->policy, &T.policy, "terminal_value_eval.policy");
    if (rc != MBPO_OK) return rc;
    MBPO_REQUIRE(T.policy.n_nets == 1, MBPO_ERR_ARG, "terminal_value_eval: policy.n_nets=%d, one policy", T.policy.n_nets);
    MBPO_REQUIRE(T.policy.dims[0] == X, MBPO_ERR_ARG, "terminal_value_eval: policy.dims[0]=%d is not x_dim=%d", T.policy.dims[0], X);
    MBPO_REQUIRE((long long)T.policy.dims[T.policy.n_layers] == 2LL * A, MBPO_ERR_ARG,
                 "terminal_value_eval: policy.dims[%d]=%d is not 2 * action_dim = %d", T.policy.n_layers, T.policy.dims[T.policy.n_layers], 2 * A);
  } else {
    T.policy = T.critic;      // (never walked)
  }
  MBPO_REQUIRE((d->norm_mean == nullptr) == (d->norm_std == nullptr), MBPO_ERR_ARG,
               "terminal_value_eval: norm_mean and norm_std must both be set or both NULL");
  MBPO_REQUIRE(d->x_stride >= X, MBPO_ERR_ARG, "terminal_value_eval: x_stride=%lld < x_dim=%d", (long long)d->x_stride, X);
  MBPO_REQUIRE(d->out_stride >= 1, MBPO_ERR_ARG, "terminal_value_eval: out_stride=%lld < 1", (long long)d->out_stride);
  MBPO_REQUIRE(term_value_mul_fits(d->n, d->x_stride) && term_value_mul_fits(d->n, d->out_stride), MBPO_ERR_ARG,
               "terminal_value_eval: n * x_stride (or out_stride) overflows int64");
  const int Hc = hidden_width(T.critic), Hp = A > 0 ? hidden_width(T.policy) : Hc;
  MBPO_REQUIRE(Hc == 64 || Hc == 128 || Hc == 256, MBPO_ERR_UNSUPPORTED,
               "terminal_value_eval: MBPO_ERR_UNSUPPORTED: the critic's hidden layers must share one width in {64,128,256}");
  MBPO_REQUIRE(Hp == 64 || Hp == 128 || Hp == 256, MBPO_ERR_UNSUPPORTED,
               "terminal_value_eval: MBPO_ERR_UNSUPPORTED: the policy's hidden layers must share one width in {64,128,256}");
  MBPO_REQUIRE(A <= 64, MBPO_ERR_UNSUPPORTED, "terminal_value_eval: MBPO_ERR_UNSUPPORTED: action_dim=%d > 64 (the policy's output tile)", A);
  if (d->n == 0) return MBPO_OK;
  MBPO_REQUIRE(d->critic.params != nullptr, MBPO_ERR_ARG, "terminal_value_eval: critic.params is NULL");
  MBPO_REQUIRE(A == 0 || d->policy.params != nullptr, MBPO_ERR_ARG, "terminal_value_eval: policy.params is NULL");
  MBPO_REQUIRE(d->x != nullptr, MBPO_ERR_ARG, "terminal_value_eval: x is NULL");
  MBPO_REQUIRE(d->out != nullptr, MBPO_ERR_ARG, "terminal_value_eval: out is NULL");
  const int H = Hc > Hp ? Hc : Hp;
  T.X = X; T.A = A;
  T.norm_mean = d->norm_mean; T.norm_std = d->norm_std;
  T.x = d->x; T.x_stride = d->x_stride;
  T.out = d->out; T.out_stride = d->out_stride;
  T.n = d->n; T.weight = d->weight; T.accumulate = d->accumulate;
  T.ld_in = up4(X + A) + 4;
  T.ld_h = H + 4;
  T.ld_pol = A > 0 ? up4(2 * A) + 4 : 4;
  T.ld_q = TERM_VALUE_LD_Q;
  const int n_waves = T.critic.n_nets;
  const size_t lds = sizeof(float) * (16ull * T.ld_in + 16ull * T.ld_pol + 2ull * 16 * T.ld_q + 2ull * n_waves * 16 * T.ld_h);
  const long long n_tiles = (d->n + 15) >> 4, cap = 8LL * mbpo_num_cus();
  const int grid = (int)(n_tiles < cap ? n_tiles : cap);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 block(64 * n_waves);
  if (H == 64) rc = mbpo_launch<k_terminal_value<64>>(grid, block, lds, st, "terminal_value_eval", T);
  else if (H == 128) rc = mbpo_launch<k_terminal_value<128>>(grid, block, lds, st, "terminal_value_eval", T);
  else rc = mbpo_launch<k_terminal_value<256>>(grid, block, lds, st, "terminal_value_eval", T);
  if (rc != MBPO_OK) return rc;
  MBPO_CHECK_LAUNCH("terminal_value_eval");
  return MBPO_OK;
}
