// ppo.hip — P1-P3: one PPO minibatch update (see include/mbpo_hip.h).
//
//   k_ppo_values    V(obs) on all B*T samples + the bootstrap V(next_obs[:, T-1]); also splits the row columns the
//                   GAE scan needs (truncation, termination, scaled reward) into [B,T] arrays.            [fp32 MFMA]
//   mbpo_gae_scan   vs, advantages (scan.hip; batch-major, wavefront-shuffle scan)                         [HBM]
//   k_ppo_values_gae  both of the above and the moments' first stage in one launch, where a workgroup's LDS holds whole trajectories:
//                   values, GAE and {n, mean, M2} partials of the advantages, which k_ppo_moments_combine merges.  [fp32 MFMA]
//   k_moments_*     mean / population std of the advantages over the whole minibatch after the separate launches: k_moments_fused
//                   (one workgroup, up to PPO_MOM_FUSED_MAX elements), else k_moments_partial / k_moments_final, two passes.  [HBM]
//   k_ppo_fwd_bwd   policy and value forward + hand-written backward of the clipped-surrogate / value / entropy losses;
//                   a workgroup walks many 16-sample tiles and ACCUMULATES its weight gradients into its own slab
//                   (8 waves: policy and value chains, 2 waves each; backward: dgrad + wgrad chains side by side).  [fp32 MFMA]
//   k_ppo_reduce    grads = fixed-order sum of the slabs; loss metrics.                                    [HBM]
//   k_ppo_apply     optax.adamw(lr, wd) (ppo.py:128).                                                     [HBM]
//   k_ppo_clip_apply  max_grad_norm > 0 (ppo_brax_env.py:137-141): every workgroup re-adds the per-64-element sum-of-squares
//                   partials (k_ppo_reduce<true> / k_ppo_sumsq) in fixed order -> the global norm, clip_by_global_norm, AdamW.  [HBM]
// non_equidistant_time (losses_new.py:105-120): every values/GAE launch takes a NEQ template flag; with it the per-sample discount
// n1_discount(last action component) replaces `discounting` in compute_gae (an LDS array in the fused launches, a workspace array
// for mbpo_gae_scan_discounts otherwise).  Without it the kernels are the constant-discount code, unchanged.
// Algorithmic work per sample: 3*(2P + 2V) FLOP fwd+bwd (+2V for the value pre-pass), 4*(2x+2u+4) B of row data.
#include "common.hpp"
#include "chain_run.hpp"
#include "ppo_layered.hpp"
#include "ppo_lean.hpp"

#define LOG_SQRT_2PI 0.91893853320467274178f
#define LOG_2 0.69314718055994530942f
#define PPO_MOM_WGS 64

struct PpoArgs {
  MlpDev pi, v;
  NetShape sh_pi, sh_v;
  int X, U, B, T, D;
  const float *data, *norm_mean, *norm_std, *ent_noise;
  unsigned long long seed, offset;
  const unsigned long long *rng_dev;
  float entropy_cost, discounting, reward_scaling, gae_lambda, clip_eps;
  int normalize_advantage;
  // workspace pieces
  float *baseline, *boot, *trunc, *term, *rew, *vs, *adv, *mom, *slabs, *extras;
  int n_slabs;
  int ld_x, ld_h, ld_y, LH;
  int mom_inline;            // (unused)
  float *mom_part;
  int mom_parts;
  int vg_G;                  // k_ppo_values_gae: trajectories per workgroup; its workgroups leave {n, mean, M2} partials in mom_part
  float *step_count_rw;      // optax's count: bumped by block 0 of the FIRST launch of a minibatch_step (k_ppo_values), so that every
                             // later launch of the step — the reduce launch that also applies AdamW, or k_ppo_apply — reads the final value
  // N1 (the NEQ instantiations only): per-sample discount n1_discount(row[X + U - 1], cd, tl, tu, dt); k_ppo_values writes it to disc [M]
  float *disc;
  float neq_cd, neq_tl, neq_tu, neq_dt;
};

// ------------------------------------------------------------------------------------------------ values pre-pass
template <int H, bool NEQ>
__global__ void __launch_bounds__(256) k_ppo_values(PpoArgs A) {
  extern __shared__ __align__(16) float smem[];
  constexpr int HT = H / 16;
  const int tid_ = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid_ >> 6);
  const int X = A.X, U = A.U, D = A.D, T = A.T;
  const long long M = (long long)A.B * T, rows = M + A.B;     // samples, then one bootstrap row per trajectory
  float *s_x = smem;                         // [16][ld_x]
  float *s_pp = s_x + 16 * A.ld_x;           // 2 hidden tiles
  float *s_y = s_pp + 2 * 16 * A.ld_h;       // [16][ld_y]
  const long long n_tiles = (rows + 15) >> 4;
  if (blockIdx.x == 0 && tid_ == 0) A.step_count_rw[0] = A.step_count_rw[0] + 1.0f;     // (nothing in this launch reads it)
#pragma nounroll
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int tid = opaque(tid_), lane = tid & 63;
    const long long r0 = tile * 16;
    WSet<HT, 4> R;
    chain_fwd_prefetch<HT, 4>(R, A.sh_v, A.v.params, wave, lane);
    for (int idx = tid; idx < 16 * X; idx += 256) {
      const int r = idx & 15, c = idx >> 4;
      const long long i = r0 + r;
      float o = 0.f;
      if (i < M) o = A.data[i * D + c];                                                   // observation
      else if (i < rows) o = A.data[((i - M) * T + (T - 1)) * D + X + U + 2 + c];         // next_observation[-1]  (losses.py:84-85)
      if (A.norm_mean) o = (o - A.norm_mean[c]) / A.norm_std[c];
      s_x[r * A.ld_x + c] = o;
    }
    if (tid < 16) {
      const long long i = r0 + tid;
      if (i < M) {
        const float *row = A.data + i * D;
        const float tr = row[D - 1], disc = row[X + U + 1];
        A.trunc[i] = tr;
        A.term[i] = (1.f - disc) * (1.f - tr);                 // termination = (1 - discount) * (1 - truncation)   (:89)
        A.rew[i] = row[X + U] * A.reward_scaling;              // rewards = data.reward * reward_scaling             (:87)
        if (NEQ) A.disc[i] = n1_discount(row[X + U - 1], A.neq_cd, A.neq_tl, A.neq_tu, A.neq_dt);   // losses_new.py:105-112
      }
    }
    __syncthreads();
    chain_fwd_run<HT, 4>(A.sh_v, A.v.params, s_x, A.ld_x, s_pp, s_pp + 16 * A.ld_h, nullptr, nullptr, s_y, A.ld_y, A.ld_h, A.sh_v.L,
                         wave, lane, R);
    if (tid < 16) {
      const long long i = r0 + tid;
      if (i < M) A.baseline[i] = s_y[tid * A.ld_y];
      else if (i < rows) A.boot[i - M] = s_y[tid * A.ld_y];
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ wave sum (moments, norms)
__device__ __forceinline__ float ppo_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// ------------------------------------------------------------------------------------------------ values + GAE + moment partials
// One launch for k_ppo_values + mbpo_gae_scan + the advantage moments' first stage: a workgroup owns G whole trajectories (T samples +
// the bootstrap row each), runs the value net on their rows tile by tile (values stay in LDS), then one thread per trajectory walks
// compute_gae's recurrences backwards in the reference's own order (losses.py:150-184, as k_scan_time_major) and the first wave
// leaves {n, mean, M2} of the workgroup's advantages (two passes over LDS: exact).  k_ppo_fwd_bwd combines the partials (Chan et
// al.: M2 = sum M2_i + sum n_i (mean_i - mean)^2, fixed order).  Three launches and two kernel boundaries less per minibatch_step.
// NEQ: one more [G][T] LDS array, the per-sample discount (losses_new.py:105-120), read by the recurrence in place of `discounting`.
template <int H, int NC, bool NEQ>     // NC tiles at a time, each on its own chain of 4 waves (a trajectory of T = 40 is 3 tiles: one chain latency, not three)
__global__ void __launch_bounds__(256 * NC) k_ppo_values_gae(PpoArgs A) {
  extern __shared__ __align__(16) float smem[];
  constexpr int HT = H / 16;
  const int tid_ = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid_ >> 6);
  const int chain = wave >> 2, sub = wave & 3;
  const int X = A.X, U = A.U, D = A.D, T = A.T, R = T + 1, G = A.vg_G;
  const int per_chain = 16 * A.ld_x + 2 * 16 * A.ld_h + 16 * A.ld_y;
  float *s_x = smem + chain * per_chain;     // [16][ld_x]
  float *s_pp = s_x + 16 * A.ld_x;           // 2 hidden tiles
  float *s_y = s_pp + 2 * 16 * A.ld_h;       // [16][ld_y]
  float *s_val = smem + NC * per_chain;      // [G][R] values (the last of each row: the bootstrap)
  float *s_tr = s_val + ((G * R + 3) & ~3);  // [G][T] truncation | termination | scaled reward | advantages
  float *s_te = s_tr + ((G * T + 3) & ~3), *s_rw = s_te + ((G * T + 3) & ~3), *s_adv = s_rw + ((G * T + 3) & ~3);
  float *s_dc = s_adv + ((G * T + 3) & ~3);  // [G][T] per-sample discount (NEQ only)
  const long long b0 = (long long)blockIdx.x * G;
  const int g_here = (int)((A.B - b0 < G) ? A.B - b0 : G);
  const int rows = g_here * R;
  if (blockIdx.x == 0 && tid_ == 0) A.step_count_rw[0] = A.step_count_rw[0] + 1.0f;     // (nothing in this launch reads it)
#pragma nounroll
  for (int rr = 0; rr < rows; rr += 16 * NC) {
    const int tid = opaque(tid_), lane = tid & 63, ctid = tid & 255;
    const int r0 = rr + 16 * chain;
    const bool live = r0 < rows;             // (wave-uniform: a chain without a tile only keeps the barriers)
    WSet<HT, 4> Rw;
    if (live) {
      chain_fwd_prefetch<HT, 4>(Rw, A.sh_v, A.v.params, sub, lane);
      for (int idx = ctid; idx < 16 * X; idx += 256) {
        const int r = idx & 15, c = idx >> 4;
        const int lrow = r0 + r;
        float o = 0.f;
        if (lrow < rows) {
          const int g = lrow / R, t = lrow - g * R;
          const long long base = ((b0 + g) * T + (t < T ? t : T - 1)) * D;
          o = A.data[base + (t < T ? c : X + U + 2 + c)];                  // observation | next_observation[-1]  (losses.py:84-85)
          if (A.norm_mean) o = (o - A.norm_mean[c]) / A.norm_std[c];
        }
        s_x[r * A.ld_x + c] = o;
      }
      if (ctid < 16) {
        const int lrow = r0 + ctid;
        if (lrow < rows) {
          const int g = lrow / R, t = lrow - g * R;
          if (t < T) {
            const float *row = A.data + ((b0 + g) * T + t) * D;
            const float tr = row[D - 1], disc = row[X + U + 1];
            s_tr[g * T + t] = tr;
            s_te[g * T + t] = (1.f - disc) * (1.f - tr);             // termination = (1 - discount) * (1 - truncation)   (:89)
            s_rw[g * T + t] = row[X + U] * A.reward_scaling;          // rewards = data.reward * reward_scaling             (:87)
            if (NEQ) s_dc[g * T + t] = n1_discount(row[X + U - 1], A.neq_cd, A.neq_tl, A.neq_tu, A.neq_dt);   // losses_new.py:105-112
          }
        }
      }
    }
    __syncthreads();
    if (live)
      chain_fwd_run<HT, 4>(A.sh_v, A.v.params, s_x, A.ld_x, s_pp, s_pp + 16 * A.ld_h, nullptr, nullptr, s_y, A.ld_y, A.ld_h, A.sh_v.L,
                           sub, lane, Rw);
    else
      chain_idle_run(A.sh_v.L);
    if (live && ctid < 16 && r0 + ctid < rows) s_val[r0 + ctid] = s_y[ctid * A.ld_y];
    __syncthreads();
  }
  // compute_gae, one thread per trajectory, backwards (losses.py:150-184)
  if (tid_ < g_here) {
    const int g = tid_;
    const float boot = s_val[g * R + T];
    float acc = 0.f, v_next = boot, vs_next = boot;
    for (int t = T - 1; t >= 0; --t) {
      const float tr = s_tr[g * T + t], te = s_te[g * T + t], r = s_rw[g * T + t], v = s_val[g * R + t];
      const float m = 1.f - tr;
      const float g1 = (NEQ ? s_dc[g * T + t] : A.discounting) * (1.f - te);     // losses_new.py:182,193,221
      const float delta = (r + g1 * v_next - v) * m;        // :157-158
      acc = delta + g1 * m * A.gae_lambda * acc;            // :166
      const float vs = acc + v;                             // :176
      const float adv = (r + g1 * vs_next - v) * m;         // :181-182
      const long long i = (b0 + g) * T + t;
      A.vs[i] = vs;
      A.adv[i] = adv;
      s_adv[g * T + t] = adv;
      v_next = v;
      vs_next = vs;
    }
  }
  __syncthreads();
  if (wave == 0) {
    const int n = g_here * T, lane = tid_ & 63;
    float a = 0.f;
    for (int i = lane; i < n; i += 64) a += s_adv[i];
    a = ppo_wave_sum(a);
    const float mean = __shfl(a, 0, 64) / (float)n;
    float q = 0.f;
    for (int i = lane; i < n; i += 64) {
      const float dd = s_adv[i] - mean;
      q += dd * dd;
    }
    q = ppo_wave_sum(q);
    if (lane == 0) {
      A.mom_part[4 * blockIdx.x + 0] = (float)n;
      A.mom_part[4 * blockIdx.x + 1] = mean;
      A.mom_part[4 * blockIdx.x + 2] = q;
    }
  }
}

// PASS 0: partial[g] = sum x ; PASS 1: partial[g] = sum (x - mean)^2
template <int PASS>
__global__ void __launch_bounds__(256) k_moments_partial(const float *x, long long n, const float *mom, float *partial) {
  __shared__ float s_w[4];
  const float mean = PASS ? mom[0] : 0.f;
  float acc = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float d = x[i] - mean;
    acc += PASS ? d * d : d;
  }
  acc = ppo_wave_sum(acc);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

template <int PASS>
__global__ void k_moments_final(const float *partial, int n_parts, long long n, float *mom) {
  if (threadIdx.x == 0) {
    float acc = 0.f;
    for (int g = 0; g < n_parts; ++g) acc += partial[g];
    if (PASS == 0) mom[0] = acc / (float)n;                // mean
    else mom[1] = sqrtf(acc / (float)n);                   // population std (jnp.std)
  }
}

// minibatches up to PPO_MOM_FUSED_MAX elements: both passes in ONE workgroup of 1024 threads (3 kernel boundaries of ~4.5 us less
// per minibatch_step; the data is a few KB).  Fixed strides and a fixed shuffle/LDS tree: deterministic.
#define PPO_MOM_FUSED_MAX 65536
__global__ void __launch_bounds__(1024) k_moments_fused(const float *x, long long n, float *mom) {
  __shared__ float s_w[16];
  __shared__ float s_mean;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  float acc = 0.f;
#pragma unroll 4
  for (long long i = tid; i < n; i += 1024) acc += x[i];
  acc = ppo_wave_sum(acc);
  if (lane == 0) s_w[w] = acc;
  __syncthreads();
  if (tid == 0) {
    float a = 0.f;
    for (int k = 0; k < 16; ++k) a += s_w[k];
    s_mean = a / (float)n;
  }
  __syncthreads();
  const float mean = s_mean;
  acc = 0.f;
#pragma unroll 4
  for (long long i = tid; i < n; i += 1024) {
    const float d = x[i] - mean;
    acc += d * d;
  }
  acc = ppo_wave_sum(acc);
  __syncthreads();
  if (lane == 0) s_w[w] = acc;
  __syncthreads();
  if (tid == 0) {
    float a = 0.f;
    for (int k = 0; k < 16; ++k) a += s_w[k];
    mom[0] = mean;
    mom[1] = sqrtf(a / (float)n);                          // population std (jnp.std)
  }
}

// ------------------------------------------------------------------------------------------------ loss fwd/bwd
// The loss section runs on a few lanes while the other waves of the workgroup wait at its barrier, so its instruction count is tile
// latency: it takes its transcendentals from fast_math.hpp (libm's expf / log1pf / logf / tanhf are 30-60 instructions each).

// The advantage moments from the per-workgroup partials {n_i, mean_i, M2_i} of k_ppo_values_gae (Chan et al.: mean = sum n_i mean_i / M,
// M2 = sum M2_i + sum n_i (mean_i - mean)^2), one workgroup, fixed order.  A launch of its own: k_ppo_fwd_bwd<64,2> sits at 128 VGPRs
// with ~50 spilled, and ANY code added to it — this combine inlined, behind a barrier-free LDS hand-off, or behind a noinline call —
// moved the allocator's choices in its tile loop: 6-9 us per launch at every size (rocprofv3, round 3), more than this launch costs.
// (Finishing in the last workgroup of k_ppo_values_gae behind an arrival counter cost that kernel 7 us.)
__global__ void __launch_bounds__(256) k_ppo_moments_combine(const float *part, int n_parts, float M, float *mom) {
  __shared__ float s_cw[4];
  __shared__ float s_cm;
  const int tid = threadIdx.x;
  constexpr int NPT = 4;                      // <= 4 * CUs partials
  float pn[NPT], pm[NPT], pq[NPT];
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    const int p = tid + k * 256;
    const bool ok = p < n_parts;
    pn[k] = ok ? part[4 * p] : 0.f;
    pm[k] = ok ? part[4 * p + 1] : 0.f;
    pq[k] = ok ? part[4 * p + 2] : 0.f;
  }
  float a = 0.f;
#pragma unroll
  for (int k = 0; k < NPT; ++k) a += pn[k] * pm[k];
  a = ppo_wave_sum(a);
  if ((tid & 63) == 0) s_cw[tid >> 6] = a;
  __syncthreads();
  if (tid == 0) s_cm = (((s_cw[0] + s_cw[1]) + s_cw[2]) + s_cw[3]) / M;
  __syncthreads();
  const float mean = s_cm;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    const float dm = pm[k] - mean;
    q += pq[k] + pn[k] * dm * dm;
  }
  q = ppo_wave_sum(q);
  if ((tid & 63) == 0) s_cw[tid >> 6] = q;
  __syncthreads();
  if (tid == 0) {
    mom[0] = mean;
    mom[1] = sqrtf((((s_cw[0] + s_cw[1]) + s_cw[2]) + s_cw[3]) / M);     // population std (jnp.std)
  }
}

// SP = 2 at H = 64 (512 threads, held to 128 VGPRs by the waves-per-SIMD request): TWO workgroups share a CU, so a tile's chain of
// dependent layer steps overlaps with another tile's — the launch is a latency chain per tile (MFMA pipes ~17 % busy with one
// 1024-thread workgroup per CU), not a throughput problem.  The host picks it when there are more tiles than CUs.
template <int H, int SP, bool WIDE>   // 4 chains x SP waves; WIDE: chain_run.hpp fast_shape
__global__ void __launch_bounds__(256 * SP, (H == 64 && SP == 2) ? 4 : 1) k_ppo_fwd_bwd(PpoArgs A) {
  extern __shared__ __align__(16) float smem[];
  constexpr int HT = H / 16;
  const int tid_ = threadIdx.x, nthreads = 256 * SP;
  const int wave = __builtin_amdgcn_readfirstlane(tid_ >> 6);
  const int chain = wave / SP, sub = wave % SP;
  const int X = A.X, U = A.U, D = A.D;
  const long long M = (long long)A.B * A.T;
  const int ld_x = A.ld_x, ld_h = A.ld_h, ld_y = A.ld_y, LH = A.LH;
  const int TT = 16 * ld_h;
  const int D4 = (D + 3) & ~3;
  float *s_row = smem;                       // [16][D] flat copy of the tile's rows (16*D4 floats reserved)
  float *s_x = s_row + 16 * D4;              // [16][ld_x]   normalised obs
  float *s_store = s_x + 16 * ld_x;          // 4*LH tiles: policy z,h | value z,h
  float *s_pp = s_store + 4 * LH * TT;       // 4 tiles: delta ping-pong (policy, value)
  float *s_y = s_pp + 4 * TT;                // [2][16][ld_y]  logits | value
  float *s_dy = s_y + 2 * 16 * ld_y;         // [2][16][ld_y]
  float *s_scal = s_dy + 2 * 16 * ld_y;      // [4][16]
  float *s_eps = s_scal + 64;                // [16][U]  entropy-sample noise, drawn in the tile-load section
  float *s_lpt = s_eps + ((16 * U + 3) & ~3);   // [16][U] per-dimension log-prob terms  | then [16][U] entropy terms
  float *s_ent = s_lpt + ((16 * U + 3) & ~3);
  float *zp = s_store, *hp = s_store + LH * TT, *zv = s_store + 2 * LH * TT, *hv = s_store + 3 * LH * TT;
  float *y_pi = s_y, *y_v = s_y + 16 * ld_y;
  const int PL = A.pi.n_layers, VL = A.v.n_layers;
  const int Lmax = PL > VL ? PL : VL;
  const float invM = 1.0f / (float)M;
  const float adv_mean = A.normalize_advantage ? A.mom[0] : 0.f;
  const float adv_istd = A.normalize_advantage ? 1.0f / (A.mom[1] + 1e-8f) : 1.f;          // losses.py:101-102
  const RngKey rk_ = rng_resolve(A.seed, A.offset, A.rng_dev);
  const unsigned long long rng_off = rk_.offset, rng_seed = rk_.seed;
  float *slab = A.slabs + (long long)blockIdx.x * (A.pi.n_params + A.v.n_params);
  float *slab_pi = slab, *slab_v = slab + A.pi.n_params;
  float loss_pol = 0.f, loss_v = 0.f, loss_ent = 0.f;     // thread 0..15 partials, reduced at the end
  const long long n_tiles = (M + 15) >> 4;
  bool first = true;
  const int net = chain & 1;   // 0 = policy, 1 = value
  const NetShape sh = net ? A.sh_v : A.sh_pi;
  const float *nparams = net ? A.v.params : A.pi.params;
  const int H1 = 16 * HT;
#pragma nounroll
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x, first = false) {
    const int tid = opaque(tid_), lane = tid & 63;
    const long long r0 = tile * 16;
    WSet<HT, SP> R;
    if (chain < 2) chain_fwd_prefetch<HT, SP, WIDE>(R, sh, nparams, sub, lane);
    {
      const long long nvalid = (M - r0 < 16 ? M - r0 : 16) * D;
      for (int idx = tid; idx < 16 * D; idx += nthreads) {   // flat copy, row stride D (no padding, no division)
        s_row[idx] = idx < nvalid ? A.data[r0 * D + idx] : 0.f;
      }
      for (int idx = tid; idx < 16 * X; idx += nthreads) {
        const int r = idx & 15, c = idx >> 4;
        float o = (r0 + r < M) ? A.data[(r0 + r) * D + c] : 0.f;
        if (A.norm_mean) o = (o - A.norm_mean[c]) / A.norm_std[c];
        s_x[r * ld_x + c] = o;
      }
      // the entropy sample's noise depends on (seed, offset, element) only: drawn HERE, once, by the last threads of the workgroup
      // while the tile is in flight (Philox + Box-Muller is ~250 instructions; it used to be drawn twice per element inside the
      // loss section, on the 16 lanes every other wave waits for)
      for (int idx = nthreads - 1 - tid; idx < 16 * U; idx += nthreads) {
        const int r = idx / U, d = idx - r * U;
        const long long i = r0 + r;
        float e = 0.f;
        if (i < M) {
          const long long nidx = i * U + d;
          e = A.ent_noise ? A.ent_noise[nidx] : philox_normal(rng_seed, rng_off, MBPO_STREAM_ENTROPY, (unsigned long long)nidx);
        }
        s_eps[idx] = e;
      }
    }
    __syncthreads();
    // ---- forward: policy logits (:80) and value baseline (:82), both stored for the backward
    if (chain < 2)
      chain_fwd_run<HT, SP, WIDE>(sh, nparams, s_x, ld_x, nullptr, nullptr, net ? zv : zp, net ? hv : hp, net ? y_v : y_pi, ld_y, ld_h, Lmax,
                            sub, lane, R);
    else
      chain_idle_run(Lmax);
    if (chain < 2) chain_dgrad_prefetch<HT, SP, WIDE>(R, sh, nparams, sub, lane);
    // ---- per-sample loss terms and output gradients.  Stage 1: one lane per (row, action dim) forms that dimension's log-prob
    //      and entropy terms; stage 2 (after a barrier of its own: the stage-1 lanes may sit in other waves): one lane per row sums them
    //      in dimension order, forms rho and the clipped surrogate's weight and writes the value gradient; stage 3: one lane per
    //      (row, dim) again writes the logits' gradients.  Same arithmetic as the one-lane-per-row loop it replaces.
    for (int idx = tid; idx < 16 * U; idx += nthreads) {
      const int r = idx / U, d = idx - r * U;
      const float *row = s_row + r * D;
      const float loc = y_pi[r * ld_y + d], raw = y_pi[r * ld_y + U + d];
      const float sg = fm_softplus(raw) + 0.001f;
      const float z = row[2 * X + U + 3 + d];                      // raw_action
      const float q = (z - loc) / sg;
      const float lsg = fm_log(sg);
      s_lpt[idx] = -0.5f * q * q - lsg - LOG_SQRT_2PI - 2.0f * (LOG_2 - z - fm_softplus(-2.0f * z));   // log_prob (:91-92)
      const float zf = loc + sg * s_eps[idx];
      s_ent[idx] = 0.5f + LOG_SQRT_2PI + lsg + 2.0f * (LOG_2 - zf - fm_softplus(-2.0f * zf));          // entropy (:117)
    }
    __syncthreads();
    if (tid < 16) {
      const int r = tid;
      const long long i = r0 + r;
      const bool ok = i < M;
      const float *row = s_row + r * D;
      const float lp_b = row[2 * X + U + 2];                       // behaviour log-prob (policy_extras.log_prob)
      const float adv = ok ? (A.adv[i] - adv_mean) * adv_istd : 0.f;
      const float vs = ok ? A.vs[i] : 0.f;
      float lp_t = 0.f, ent = 0.f;
      for (int d = 0; d < U; ++d) {
        lp_t += s_lpt[r * U + d];
        ent += s_ent[r * U + d];
      }
      const float rho = fm_exp(lp_t - lp_b);                                                             // :103
      const float lo = 1.f - A.clip_eps, hi = 1.f + A.clip_eps;
      const float s1 = rho * adv, s2 = fminf(fmaxf(rho, lo), hi) * adv;
      // d min(s1,s2)/d rho: inside the clip range s1 == s2 (tie, both branches carry adv); outside only s1 can carry it
      const bool inside = (rho >= lo) && (rho <= hi);
      const float w = inside ? 1.f : (s1 < s2 ? 1.f : 0.f);
      s_scal[48 + r] = ok ? -invM * rho * adv * w : 0.f;            // g_lp = d policy_loss / d lp_t
      const float v = y_v[r * ld_y];
      if (ok) {
        loss_pol += -fminf(s1, s2);
        loss_v += 0.5f * (vs - v) * (vs - v);
        loss_ent += ent;
      }
      s_dy[(16 + r) * ld_y] = ok ? -(vs - v) * invM : 0.f;          // d (0.5*mean((vs-V)^2)) / dV   (:112-114)
    }
    __syncthreads();
    for (int idx = tid; idx < 16 * U; idx += nthreads) {
      const int r = idx / U, d = idx - r * U;
      const bool ok = r0 + r < M;
      const float *row = s_row + r * D;
      const float g_lp = s_scal[48 + r];
      const float g_ent = ok ? -A.entropy_cost * invM : 0.f;        // d entropy_loss / d entropy_i
      const float loc = y_pi[r * ld_y + d], raw = y_pi[r * ld_y + U + d];
      const float sg = fm_softplus(raw) + 0.001f;
      const float z = row[2 * X + U + 3 + d];
      const float q = (z - loc) / sg;
      const float eps = s_eps[idx];
      const float th = fm_tanh(loc + sg * eps);
      // lp_t: d/dloc = q/sg, d/dsigma = (q*q - 1)/sg ; entropy: d/dloc = -2 tanh(zf), d/dsigma = 1/sg - 2 tanh(zf) eps
      const float g_loc = g_lp * (q / sg) + g_ent * (-2.f * th);
      const float g_sig = g_lp * ((q * q - 1.f) / sg) + g_ent * (1.f / sg - 2.f * th * eps);
      s_dy[r * ld_y + d] = g_loc;
      s_dy[r * ld_y + U + d] = g_sig * fast_sigmoid(raw);
    }
    __syncthreads();
    // ---- backward: chains 0/1 push delta down (policy / value), chains 2/3 accumulate dW/db into this WG's slab
    {
      float *d0 = s_pp + (2 * net) * TT, *d1 = d0 + TT;
      if (chain < 2)
        chain_dgrad_run<HT, SP, WIDE>(sh, nparams, s_dy + net * 16 * ld_y, ld_y, net ? zv : zp, d0, d1, nullptr, ld_x, ld_h, Lmax, sub, lane, R);
      else
        chain_wgrad_run<HT, SP, WIDE>(sh, s_x, ld_x, net ? hv : hp, s_dy + net * 16 * ld_y, ld_y, d0, d1, net ? slab_v : slab_pi, !first, ld_h,
                                Lmax, sub, lane);
    }
  }
  (void)H1;
  const int tid = tid_;
  // ---- loss partials of this workgroup (fixed order)
  if (tid < 16) {
    s_scal[tid] = loss_pol;
    s_scal[16 + tid] = loss_v;
    s_scal[32 + tid] = loss_ent;
  }
  __syncthreads();
  if (tid == 0) {
    float a = 0.f, b = 0.f, c = 0.f;
    for (int i = 0; i < 16; ++i) {
      a += s_scal[i];
      b += s_scal[16 + i];
      c += s_scal[32 + i];
    }
    A.extras[blockIdx.x * 4 + 0] = a;
    A.extras[blockIdx.x * 4 + 1] = b;
    A.extras[blockIdx.x * 4 + 2] = c;
  }
}

struct PpoReduceArgs {
  const float *slabs, *extras;
  int n_slabs, NPV, slab_step;
  int n_extras;              // loss partials to add (= n_slabs on the fused path: one set per workgroup of k_ppo_fwd_bwd)
  long long M;
  float entropy_cost;
  float *grads, *metrics, *metrics_accum;
  const float *step_count;   // already this step's count (k_ppo_values bumped it)
  // fused optimizer step (mbpo_ppo_step: no all-reduce sits between the gradient and AdamW): params != nullptr
  float *params, *adam_m, *adam_v;
  float lr, wd, grad_scale;
  float *ss_part;            // SSQ: [gridDim.x] sum of (grad_scale * grads)^2 over this workgroup's 64 elements (clip_by_global_norm)
};

// optax.adamw on one element (constants as optax forms them: f32(0.1), f32(0.001) — see sac.hip); `count` is this step's count
__device__ __forceinline__ void ppo_adamw(float *params, float *adam_m, float *adam_v, int i, float g, float count, float lr, float wd) {
  const float b1 = 0.9f, b2 = 0.999f, eps = 1e-8f;
  const float mu = b1 * adam_m[i] + 0.1f * g;
  const float nu = b2 * adam_v[i] + 0.001f * (g * g);
  adam_m[i] = mu;
  adam_v[i] = nu;
  const float mu_hat = mu / (1.f - powf(b1, count));
  const float nu_hat = nu / (1.f - powf(b2, count));
  const float p = params[i];
  const float upd = mu_hat / (sqrtf(nu_hat) + eps) + wd * p;
  params[i] = p + (-lr) * upd;
}

// one wave: the sum of squares of the scaled gradient over 64 consecutive elements, a fixed shuffle tree (k_ppo_reduce<true> on the
// sums it has just formed, k_ppo_sumsq on `grads` after an all-reduce: the same values give the same bits)
__device__ __forceinline__ float ppo_sumsq64(float g) {
  const float q = g * g;
  return ppo_wave_sum(q);
}

// stage 1 of the two-stage slab sum (many slabs): groups of 16 slabs, 4-KB contiguous runs (common.hpp slab_group16_sum)
__global__ void __launch_bounds__(256) k_ppo_reduce_groups(float *slabs, int NPV, int n_slabs) { slab_group16_sum(slabs, NPV, n_slabs, NPV); }

// SSQ (mbpo_ppo_step with max_grad_norm > 0): no AdamW here — the norm needs every workgroup's part first — but wave 0 leaves the
// sum of squares of its 64 scaled sums in ss_part[blockIdx.x] for k_ppo_clip_apply.
template <bool SSQ>
__global__ void __launch_bounds__(256) k_ppo_reduce(PpoReduceArgs A) {
  // (A.slab_step = 16 after k_ppo_reduce_groups: the group sums sit in slabs 0, 16, 32, ...)
  const int i = blockIdx.x * 64 + (threadIdx.x & 63);
  const float gsum = slab_sum_wg64(A.slabs, (long long)A.NPV * A.slab_step, (A.n_slabs + A.slab_step - 1) / A.slab_step, i, i < A.NPV);
  if (threadIdx.x < 64 && i < A.NPV) {
    A.grads[i] = gsum;
    // k_ppo_apply's arithmetic on the element this thread has just summed: one launch less per minibatch_step, the same bits
    if (!SSQ && A.params) ppo_adamw(A.params, A.adam_m, A.adam_v, i, gsum * A.grad_scale, A.step_count[0], A.lr, A.wd);
  }
  if (SSQ && threadIdx.x < 64) {
    const float q = ppo_sumsq64(i < A.NPV ? gsum * A.grad_scale : 0.f);
    if (threadIdx.x == 0) A.ss_part[blockIdx.x] = q;
  }
  if (blockIdx.x == 0) {
    // The loss partials (three per slab) are summed by the whole workgroup: thread t takes slabs t, t + 256, ..., then a fixed tree
    // over the 256 partial sums in LDS.  ONE thread walking 3 x n_slabs values (its loads in dependent batches of 16) was the
    // launch: 21.6 us at 512 slabs with the gradient sum itself done in 3 (rocprofv3, round 3).
    __shared__ float s_e[3][256];
    const int t = threadIdx.x;
    float e[3] = {0.f, 0.f, 0.f};
    for (int sl = t; sl < A.n_extras; sl += 256) {
#pragma unroll
      for (int k = 0; k < 3; ++k) e[k] += A.extras[(long long)sl * 4 + k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) s_e[k][t] = e[k];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (t < w) {
#pragma unroll
        for (int k = 0; k < 3; ++k) s_e[k][t] += s_e[k][t + w];
      }
      __syncthreads();
    }
    if (t == 0) {
      // (what this thread read-modify-writes is requested together)
      float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
      if (A.metrics_accum) {
#pragma unroll
        for (int k = 0; k < 5; ++k) acc[k] = A.metrics_accum[k];
      }
      const float a = s_e[0][0], b = s_e[1][0], c = s_e[2][0];
      const float invM = 1.0f / (float)A.M;
      const float pl = a * invM, vl = b * invM, el = A.entropy_cost * -(c * invM);
      const float m[4] = {pl + vl + el, pl, vl, el};   // m[0]: total_loss
#pragma unroll
      for (int k = 0; k < 4; ++k) A.metrics[k] = m[k];
      if (A.metrics_accum) {
#pragma unroll
        for (int k = 0; k < 4; ++k) A.metrics_accum[k] = acc[k] + m[k];
        A.metrics_accum[4] = acc[4] + 1.0f;
      }
    }
  }
}

struct PpoApplyArgs {
  float *params, *adam_m, *adam_v;
  const float *grads, *step_count;
  int NPV;
  float lr, wd, grad_scale;
};

__global__ void __launch_bounds__(256) k_ppo_apply(PpoApplyArgs A) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= A.NPV) return;
  // [3P optax.adamw]
  ppo_adamw(A.params, A.adam_m, A.adam_v, i, A.grads[i] * A.grad_scale, A.step_count[0], A.lr, A.wd);
}

// mbpo_ppo_apply with max_grad_norm > 0, after an all-reduce changed `grads`: the partials k_ppo_reduce<true> would have formed
__global__ void __launch_bounds__(64) k_ppo_sumsq(const float *grads, int NPV, float grad_scale, float *ss_part) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  const float q = ppo_sumsq64(i < NPV ? grads[i] * grad_scale : 0.f);
  if (threadIdx.x == 0) ss_part[blockIdx.x] = q;
}

struct PpoClipArgs {
  float *params, *adam_m, *adam_v;
  const float *grads, *step_count, *ss_part;
  int NPV, n_parts;
  float lr, wd, grad_scale, max_norm;
};

// [3P optax.chain(clip_by_global_norm(max_norm), adamw)] (ppo_brax_env.py:137-141).  Every workgroup forms the global norm from the
// n_parts partials itself — thread t adds parts t, t + 256, ... in order, a fixed shuffle tree per wave, the four waves in order —
// so it is the same float in every workgroup and on every run; then g <- g if norm < max_norm else (g / norm) * max_norm (optax's
// form, as sac.hip) and AdamW on the workgroup's elements (grid-stride).
__global__ void __launch_bounds__(256) k_ppo_clip_apply(PpoClipArgs A) {
  __shared__ float s_w[4];
  const int tid = threadIdx.x;
  float a = 0.f;
  for (int p = tid; p < A.n_parts; p += 256) a += A.ss_part[p];
  a = ppo_wave_sum(a);
  if ((tid & 63) == 0) s_w[tid >> 6] = a;
  __syncthreads();
  const float norm = sqrtf(((s_w[0] + s_w[1]) + s_w[2]) + s_w[3]);
  const bool clip = !(norm < A.max_norm);
  const float count = A.step_count[0];
  for (int i = blockIdx.x * 256 + tid; i < A.NPV; i += gridDim.x * 256) {
    float g = A.grads[i] * A.grad_scale;
    if (clip) g = (g / norm) * A.max_norm;
    ppo_adamw(A.params, A.adam_m, A.adam_v, i, g, count, A.lr, A.wd);
  }
}

// ------------------------------------------------------------------------------------------------ host
// validate + geometry (ppo_plan) -> kernels for the shape (ppo_variant) -> one fill function per argument block -> one launch function
// per stage -> ppo_update.

// The dynamic LDS of the tile kernels: float offsets of their regions in carve order, `end` = the layout's size in floats.  The host's
// one statement of the layouts (ppo_plan's byte counts, the LDS sizes of both values + GAE launches); the carves at the top of
// k_ppo_values, k_ppo_values_gae (ppo_lean.hip: k_ppo_vg_lean) and k_ppo_fwd_bwd keep their own expressions and must agree with this.
struct PpoLds {
  struct { long long x, pp, y, end; } values;                                    // k_ppo_values
  // k_ppo_values_gae: NC per-chain blocks of `chain` floats (the values layout), then the [G][.] arrays: val .. end count from there
  struct { long long chain, val, tr, te, rw, adv, dc, end; } vg;
  struct { long long row, x, store, pp, y, dy, scal, eps, lpt, ent, end; } fb;   // k_ppo_fwd_bwd
};
static inline PpoLds ppo_lds(int row_len, int U, int ld_x, int ld_h, int ld_y, int LH, long long G, int T, bool neq) {
  const long long TT = 16LL * ld_h, U4 = (16LL * U + 3) & ~3LL;      // one hidden tile; one [16][U] array
  const long long GR4 = (G * (T + 1) + 3) & ~3LL, GT4 = (G * T + 3) & ~3LL;
  PpoLds L;
  auto &v = L.values;      // [16][ld_x] normalised obs | 2 hidden tiles | [16][ld_y]
  v.x = 0; v.pp = v.x + 16LL * ld_x; v.y = v.pp + 2 * TT; v.end = v.y + 16LL * ld_y;
  auto &g = L.vg;          // [G][T + 1] values (the last of each row: the bootstrap) | [G][T] truncation | termination | scaled reward |
                           // advantages | per-sample discount (neq only)
  g.chain = v.end; g.val = 0; g.tr = g.val + GR4; g.te = g.tr + GT4; g.rw = g.te + GT4; g.adv = g.rw + GT4; g.dc = g.adv + GT4;
  g.end = g.dc + (neq ? GT4 : 0);
  auto &f = L.fb;          // [16][D] flat copy of the tile's rows | [16][ld_x] normalised obs | 4*LH tiles: policy z,h, value z,h | 4 tiles:
                           // delta ping-pong | [2][16][ld_y] logits, value | [2][16][ld_y] their gradients | [4][16] | three [16][U] arrays
  f.row = 0; f.x = f.row + 16LL * up4(row_len); f.store = f.x + 16LL * ld_x; f.pp = f.store + 4LL * LH * TT; f.y = f.pp + 4 * TT;
  f.dy = f.y + 2 * 16LL * ld_y; f.scal = f.dy + 2 * 16LL * ld_y; f.eps = f.scal + 64; f.lpt = f.eps + U4; f.ent = f.lpt + U4; f.end = f.ent + U4;
  return L;
}

// Which kernels one update launches (ppo_variant): everything that is a choice rather than geometry.
enum PpoLayeredBy { PPO_FUSED = 0, PPO_LAYERED_KNOB, PPO_LAYERED_WIDTHS, PPO_LAYERED_LDS };
enum class PpoValues { LAYERED, VG_LEAN, VG, SEPARATE };
enum class PpoMoments { NONE, COMBINE, FUSED, TWO_PASS };
struct PpoVariant {
  // hidden layers outside the fused kernels' range (one width in {64,128} for both networks), MBPO_PPO_LAYERED=1, or more stored
  // activations than a tile's LDS holds: values pre-pass and loss forward/backward run layer by layer (ppo_layered.hip) and leave ONE
  // slab; GAE scan, moments, reduction, metrics and AdamW are shared
  PpoLayeredBy layered;
  bool lean;                 // the benchmark networks (64 x 3 or 64 x 2, swish, u = 1): k_ppo_lean (ppo_lean.hip), one workgroup and ONE slab per CU
  bool vg_lean;              // k_ppo_vg_lean instead of k_ppo_values_gae: the value network alone decides (64 x 2 or 64 x 3)
  bool sp2;                  // H == 64, one-tile network ends, more tiles than CUs: the two-workgroups-per-CU launch (k_ppo_fwd_bwd<64, 2>)
  bool wide;                 // k_ppo_fwd_bwd<64, 4, true>: a network end wider than one tile (chain_run.hpp fast_shape)
  int H;                     // the tile kernels' hidden width (64 or 128 unless layered)
  PpoValues values;          // stages 1-3: layered | values + GAE + moment partials in one launch (lean or generic) | three separate stages
  PpoMoments moments;        // COMBINE after a values + GAE launch; else one workgroup up to PPO_MOM_FUSED_MAX elements, two passes above
  bool reduce_two_stage;     // 64 slabs or more: k_ppo_reduce_groups first
  int n_slabs;               // one gradient slab per resident workgroup of the forward/backward launch
  int vg_G, n_vg, NC;        // values + GAE: trajectories per workgroup, workgroups (0 = not that launch), value chains (<= 4 tiles at a time)
  int vgrid;                 // k_ppo_values' grid
};

struct PpoPlan {
  MlpDev pi, v;
  NetShape sh_pi, sh_v;
  int P, V, NPV, LH;
  int Hp, Hv;                // the common hidden width of each network (-1: none)
  long long M, tiles;
  int ld_x, ld_h, ld_y;
  // ppo_brax_env.py's options: neq -> per-sample discount (off_disc: [M], the separate-scan and layered paths); clip -> n_ss sum-of-
  // squares partials at off_sspart (one per 64 gradient elements, k_ppo_reduce<true>'s grid).  Neither takes workspace when off.
  bool neq, clip;
  int n_ss;
  int vg_fit;                // trajectories per workgroup of a values + GAE launch; 0 = too long for a workgroup's LDS arrays
  PpoLds lds;
  size_t lds_values, lds_fb;
  PpoVariant var;            // (the workspace holds n_slabs slabs and n_vg moment partials: the carve follows the choice)
  long long off_baseline, off_boot, off_trunc, off_term, off_rew, off_vs, off_adv, off_mom, off_part, off_slabs, off_extras, off_mompart,
      off_disc, off_sspart, off_layered, total;
};

// measurement hook: device buffer of >= 64 uint64 that k_ppo_lean fills with s_memtime stamps (workgroup 0, 12 per tile); NULL = off
static unsigned long long *g_ppo_stamps = nullptr;
extern "C" int mbpo_debug_set_ppo_stamps(void *buf) {
  g_ppo_stamps = (unsigned long long *)buf;
  return MBPO_OK;
}
// Measurement / test hook (not part of include/mbpo_hip.h): 0 = always the generic k_ppo_fwd_bwd, 1 = k_ppo_lean where it applies,
// -1 = the MBPO_PPO_LEAN environment default (on).
extern "C" int mbpo_debug_set_ppo_lean(int mode) { return mbpo_knob_set_override(KNOB_PPO_LEAN, mode); }

// The one place where a shape is mapped to kernels.  The knobs in this order: layered, sp2, lean, values + GAE.
//   values    LAYERED   ppo_layered_values                       fwd/bwd  layered      ppo_layered_fwd_bwd
//             VG_LEAN   k_ppo_vg_lean                                     lean         k_ppo_lean
//             VG        k_ppo_values_gae<H, NC, neq>                      H = 64       k_ppo_fwd_bwd<64, 4, wide> | <64, 2, false> (sp2)
//             SEPARATE  k_ppo_values<H, neq>, then the GAE scan           H = 128      k_ppo_fwd_bwd<128, 2, false>
//   moments   COMBINE   k_ppo_moments_combine                    reduce   [k_ppo_reduce_groups,] k_ppo_reduce<false>, or with a
//             FUSED     k_moments_fused                                   clipped fused step k_ppo_reduce<true> + k_ppo_clip_apply
//             TWO_PASS  k_moments_partial / k_moments_final x 2
static PpoVariant ppo_variant(const mbpo_ppo_desc *d, const PpoPlan &pl) {
  const int cus = mbpo_num_cus();
  PpoVariant v;
  v.H = pl.Hp;
  // decided once, before anything depends on it
  v.layered = mbpo_knob(KNOB_PPO_LAYERED) != 0 ? PPO_LAYERED_KNOB
              : !(pl.Hp == pl.Hv && (pl.Hp == 64 || pl.Hp == 128)) ? PPO_LAYERED_WIDTHS
              : (pl.lds_fb > 160 * 1024 || pl.lds_values > 160 * 1024) ? PPO_LAYERED_LDS : PPO_FUSED;
  const bool fused = !v.layered;
  const bool wide_ends = net_is_wide(pl.sh_pi) || net_is_wide(pl.sh_v);
  const bool want_sp2 = fused && pl.Hp == 64 && !wide_ends && pl.tiles > cus && mbpo_knob(KNOB_PPO_SP2) != 0;
  const bool want_lean = mbpo_knob(KNOB_PPO_LEAN) != 0;
  v.lean = want_lean && fused &&
           ppo_lean_supports(d->x_dim, d->u_dim, d->policy_dims, d->policy_layers, d->policy_activation, d->value_dims, d->value_layers,
                             d->value_activation);
  v.vg_lean = want_lean && fused && d->u_dim == 1 &&      // (the kernel's row offsets assume u = 1)
              ppo_vg_lean_supports(d->x_dim, d->value_dims, d->value_layers, d->value_activation);
  v.sp2 = want_sp2 && !v.lean;
  v.wide = fused && !v.lean && pl.Hp == 64 && wide_ends;
  // one gradient slab per RESIDENT workgroup: a 1024-thread (or 512 x 256-VGPR) workgroup fills a CU's registers, so more of them
  // per CU only waited their turn while k_ppo_reduce summed twice the slabs (512 x 17 k floats = 35 MB per minibatch at C3's
  // T = 40: 22 us of a 158 us minibatch_step, rocprofv3 round 3).  The 512-thread / 128-VGPR launch (sp2) holds two per CU.
  const long long cap = (v.sp2 ? 2LL : 1LL) * cus;
  v.n_slabs = fused ? (int)(pl.tiles < cap ? pl.tiles : cap) : 1;
  v.reduce_two_stage = v.n_slabs >= 64;
  v.vg_G = (fused && mbpo_knob(KNOB_PPO_VALUES_GAE) != 0) ? pl.vg_fit : 0;
  v.n_vg = v.vg_G ? (d->batch_size + v.vg_G - 1) / v.vg_G : 0;
  const long long tiles_wg = ((long long)v.vg_G * (d->unroll_length + 1) + 15) / 16;
  v.NC = (int)(tiles_wg >= 4 ? 4 : tiles_wg);
  v.values = v.layered ? PpoValues::LAYERED : !v.vg_G ? PpoValues::SEPARATE : v.vg_lean ? PpoValues::VG_LEAN : PpoValues::VG;
  const long long vt = (pl.M + d->batch_size + 15) / 16;
  v.vgrid = (int)(vt < 4LL * cus ? vt : 4LL * cus);
  v.moments = !d->normalize_advantage ? PpoMoments::NONE : v.vg_G ? PpoMoments::COMBINE
              : pl.M <= PPO_MOM_FUSED_MAX ? PpoMoments::FUSED : PpoMoments::TWO_PASS;
  return v;
}

static int ppo_plan(const mbpo_ppo_desc *d, PpoPlan *pl, bool need_ptrs) {
  MBPO_REQUIRE(d, MBPO_ERR_ARG, "ppo: null descriptor");
  MBPO_REQUIRE(d->x_dim > 0 && d->u_dim > 0 && d->batch_size > 0 && d->unroll_length > 0, MBPO_ERR_ARG, "ppo: bad sizes");
  MBPO_REQUIRE(d->row_len == 2 * d->x_dim + 2 * d->u_dim + 4, MBPO_ERR_ARG, "ppo: row_len %d != 2x+2u+4", d->row_len);
  MBPO_REQUIRE(d->policy_layers >= 2 && d->policy_layers <= MBPO_MAX_LAYERS && d->value_layers >= 2 && d->value_layers <= MBPO_MAX_LAYERS,
               MBPO_ERR_ARG, "ppo: networks need at least one hidden layer");
  MBPO_REQUIRE(d->policy_dims[0] == d->x_dim && d->policy_dims[d->policy_layers] == 2 * d->u_dim, MBPO_ERR_ARG,
               "ppo: policy must map [x_dim] -> [2*u_dim]");
  MBPO_REQUIRE(d->value_dims[0] == d->x_dim && d->value_dims[d->value_layers] == 1, MBPO_ERR_ARG, "ppo: value net must map [x_dim] -> [1]");
  MBPO_REQUIRE(!d->non_equidistant_time || d->env_dt > 0.f, MBPO_ERR_ARG, "ppo: non_equidistant_time needs env_dt > 0");
  pl->neq = d->non_equidistant_time != 0;
  pl->clip = d->max_grad_norm > 0.f;
  int rc = mbpo_make_mlp_dev_from(d->policy_dims, d->policy_layers, d->policy_activation, d->params, 1, "ppo.policy", &pl->pi);
  if (rc != MBPO_OK) return rc;
  pl->P = pl->pi.n_params;
  rc = mbpo_make_mlp_dev_from(d->value_dims, d->value_layers, d->value_activation, d->params, 1, "ppo.value", &pl->v);
  if (rc != MBPO_OK) return rc;
  pl->V = pl->v.n_params;
  pl->v.params = d->params ? d->params + pl->P : nullptr;
  pl->NPV = pl->P + pl->V;
  pl->sh_pi = net_shape(pl->pi);
  pl->sh_v = net_shape(pl->v);
  pl->Hp = same_hidden(d->policy_dims, d->policy_layers);
  pl->Hv = same_hidden(d->value_dims, d->value_layers);
  const int lhp = d->policy_layers - 1, lhv = d->value_layers - 1;
  pl->LH = lhp > lhv ? lhp : lhv;
  pl->M = (long long)d->batch_size * d->unroll_length;
  pl->tiles = (pl->M + 15) / 16;
  pl->ld_x = up4(d->x_dim) + 4;
  pl->ld_h = pl->Hp + 4;
  pl->ld_y = up4(2 * d->u_dim) + 4;
  {
    // G = 1 while that does not oversubscribe the chip (a tile with a few rows of one trajectory wastes MFMA lanes nobody else wants:
    // the launch is a latency chain per workgroup); beyond 4 workgroups per CU, more trajectories per workgroup
    // at most 1024 workgroups: k_ppo_moments_combine reads NPT * 256 = 1024 {n, mean, M2} partials (4 x 256 CUs sits exactly at
    // that limit; a device with more CUs must not drop partials silently: ADVICE r3)
    const long long cap_wg = 4LL * mbpo_num_cus() < 1024 ? 4LL * mbpo_num_cus() : 1024;
    long long G = (d->batch_size + cap_wg - 1) / cap_wg;
    if (G < 1) G = 1;
    // the [G][T + 1] / [G][T] LDS arrays: values, truncation, termination, reward, advantages (+ the per-sample discount with neq), each
    // at most 1024 floats' worth of the constant-discount launch's five
    pl->vg_fit = (pl->neq ? 6 : 5) * G * (d->unroll_length + 1LL) <= 5 * 1024 ? (int)G : 0;
  }
  pl->lds = ppo_lds(d->row_len, d->u_dim, pl->ld_x, pl->ld_h, pl->ld_y, pl->LH, pl->vg_fit, d->unroll_length, pl->neq);
  pl->lds_values = sizeof(float) * (size_t)pl->lds.values.end;
  pl->lds_fb = sizeof(float) * (size_t)pl->lds.fb.end;
  pl->var = ppo_variant(d, *pl);
  const PpoVariant &v = pl->var;
  Carve c;
  pl->off_baseline = c.take(pl->M); pl->off_boot = c.take(d->batch_size); pl->off_trunc = c.take(pl->M); pl->off_term = c.take(pl->M);
  pl->off_rew = c.take(pl->M); pl->off_vs = c.take(pl->M); pl->off_adv = c.take(pl->M); pl->off_mom = c.take(4); pl->off_part = c.take(PPO_MOM_WGS);
  pl->off_slabs = c.take((long long)v.n_slabs * pl->NPV); pl->off_extras = c.take((long long)v.n_slabs * 4);
  pl->off_mompart = c.take(4LL * (v.n_vg > 0 ? v.n_vg : 1));
  pl->off_disc = c.take(pl->neq ? pl->M : 0);
  pl->n_ss = (pl->NPV + 63) / 64;
  pl->off_sspart = c.take(pl->clip ? pl->n_ss : 0);
  pl->off_layered = c.off;
  if (v.layered) c.off += ppo_layered_floats(d, pl->pi, pl->v);
  pl->total = c.off;
  if (need_ptrs)
    MBPO_REQUIRE(d->params && d->adam_m && d->adam_v && d->step_count && d->grads && d->workspace && d->metrics, MBPO_ERR_ARG,
                 "ppo: null state pointer");
  return MBPO_OK;
}

extern "C" int64_t mbpo_ppo_workspace_floats(const mbpo_ppo_desc *d) {
  PpoPlan pl;
  int rc = ppo_plan(d, &pl, false);
  if (rc != MBPO_OK) return rc;
  return pl.total;
}

// ---- one fill function per argument block
static void ppo_fill_args(const mbpo_ppo_desc *d, const PpoPlan &pl, PpoArgs *A) {
  float *ws = d->workspace;
  A->pi = pl.pi; A->v = pl.v;
  A->sh_pi = pl.sh_pi; A->sh_v = pl.sh_v;
  A->X = d->x_dim; A->U = d->u_dim; A->B = d->batch_size; A->T = d->unroll_length; A->D = d->row_len;
  A->data = d->data; A->norm_mean = d->norm_mean; A->norm_std = d->norm_std; A->ent_noise = d->entropy_noise;
  A->step_count_rw = d->step_count;
  A->mom_inline = 0;
  A->mom_part = ws + pl.off_mompart; A->mom_parts = pl.var.n_vg; A->vg_G = pl.var.vg_G;
  A->seed = d->seed; A->offset = d->offset; A->rng_dev = (const unsigned long long *)d->rng_dev;
  A->entropy_cost = d->entropy_cost; A->discounting = d->discounting; A->reward_scaling = d->reward_scaling;
  A->gae_lambda = d->gae_lambda; A->clip_eps = d->clipping_epsilon; A->normalize_advantage = d->normalize_advantage;
  A->baseline = ws + pl.off_baseline; A->boot = ws + pl.off_boot; A->trunc = ws + pl.off_trunc; A->term = ws + pl.off_term;
  A->rew = ws + pl.off_rew; A->vs = ws + pl.off_vs; A->adv = ws + pl.off_adv; A->mom = ws + pl.off_mom;
  A->slabs = ws + pl.off_slabs; A->extras = ws + pl.off_extras; A->n_slabs = pl.var.n_slabs;
  A->ld_x = pl.ld_x; A->ld_h = pl.ld_h; A->ld_y = pl.ld_y; A->LH = pl.LH;
  A->disc = pl.neq ? ws + pl.off_disc : nullptr;
  A->neq_cd = d->continuous_discounting; A->neq_tl = d->min_time_between_switches; A->neq_tu = d->max_time_between_switches;
  A->neq_dt = d->env_dt;
}

// k_ppo_vg_lean on the value network's resident images (ppo_lean.hip): the same bits as k_ppo_values_gae
static void ppo_fill_vg_lean(const mbpo_ppo_desc *d, const PpoPlan &pl, const PpoArgs &A, PpoVgLeanArgs *V) {
  V->v_params = d->params + pl.pi.n_params; V->data = d->data; V->norm_mean = d->norm_mean; V->norm_std = d->norm_std;
  V->B = d->batch_size; V->T = d->unroll_length; V->D = A.D; V->G = pl.var.vg_G; V->n_hid = d->value_layers - 2;
  V->reward_scaling = d->reward_scaling; V->discounting = d->discounting; V->gae_lambda = d->gae_lambda;
  V->vs = A.vs; V->adv = A.adv; V->mom_part = A.mom_part; V->step_count_rw = A.step_count_rw;
  V->neq = pl.neq ? 1 : 0; V->neq_cd = A.neq_cd; V->neq_tl = A.neq_tl; V->neq_tu = A.neq_tu; V->neq_dt = A.neq_dt;
}

static void ppo_fill_lean(const mbpo_ppo_desc *d, const PpoPlan &pl, const PpoArgs &A, PpoLeanArgs *L) {
  L->params = d->params; L->data = d->data; L->norm_mean = d->norm_mean; L->norm_std = d->norm_std;
  L->adv = A.adv; L->vs = A.vs; L->mom = A.mom; L->ent_noise = d->entropy_noise;
  L->rng_dev = A.rng_dev; L->seed = A.seed; L->offset = A.offset;
  L->slabs = A.slabs; L->extras = A.extras; L->M = pl.M;
  L->entropy_cost = d->entropy_cost; L->clip_eps = d->clipping_epsilon; L->normalize_advantage = d->normalize_advantage;
  L->stamps = g_ppo_stamps;
}

// the optimizer's operands, the same fields in PpoReduceArgs, PpoApplyArgs and PpoClipArgs
template <class OptArgs>
static void ppo_fill_opt(const mbpo_ppo_desc *d, OptArgs *O) {
  O->params = d->params; O->adam_m = d->adam_m; O->adam_v = d->adam_v; O->grads = d->grads; O->step_count = d->step_count;
  O->lr = d->lr; O->wd = d->wd; O->grad_scale = d->grad_scale;
}

// fuse_apply: the reduce launch also applies AdamW (params != nullptr); the loss partials are one set per slab (the layered path
// names its own in ppo_fwd_bwd_launch)
static void ppo_fill_reduce(const mbpo_ppo_desc *d, const PpoPlan &pl, const PpoArgs &A, bool fuse_apply, PpoReduceArgs *R) {
  ppo_fill_opt(d, R);
  if (!fuse_apply) R->params = nullptr;
  R->slabs = A.slabs; R->extras = A.extras; R->n_slabs = pl.var.n_slabs; R->n_extras = pl.var.n_slabs;
  R->slab_step = pl.var.reduce_two_stage ? 16 : 1;
  R->NPV = pl.NPV; R->M = pl.M; R->entropy_cost = d->entropy_cost;
  R->metrics = d->metrics; R->metrics_accum = d->metrics_accum;
  R->ss_part = d->workspace + pl.off_sspart;
}

// ---- one launch function per stage, each a switch over the variant
// A runtime int selects a template int among V, Vs... (the last one where none matches): f is called with std::integral_constant<int, .>{}.
template <int V, int... Vs, class F>
static int ppo_with_int(int v, F &&f) {
  if constexpr (sizeof...(Vs) == 0) return f(std::integral_constant<int, V>{});
  else return v == V ? f(std::integral_constant<int, V>{}) : ppo_with_int<Vs...>(v, f);
}

// 1. values pre-pass; with a values + GAE launch also 2 and the first half of 3
static int ppo_values_launch(const mbpo_ppo_desc *d, const PpoPlan &pl, PpoArgs *A, hipStream_t st) {
  const PpoVariant &v = pl.var;
  switch (v.values) {
    case PpoValues::LAYERED: {
      float *values = nullptr;
      const int rc = ppo_layered_values(d, pl.pi, pl.v, d->workspace + pl.off_layered, A->trunc, A->term, A->rew, A->disc, &values, st);
      if (rc != MBPO_OK) return rc;
      A->baseline = values;
      A->boot = values + pl.M;
      return MBPO_OK;
    }
    case PpoValues::VG_LEAN: {
      PpoVgLeanArgs V;
      ppo_fill_vg_lean(d, pl, *A, &V);
      return ppo_vg_lean_launch(V, d->x_dim, v.n_vg, (size_t)pl.lds.vg.end, st);
    }
    case PpoValues::VG: {
      // NC = the workgroup's value chains (1..4), each with its own block of LDS
      const size_t lds = sizeof(float) * (size_t)(v.NC * pl.lds.vg.chain + pl.lds.vg.end);
      return ppo_with_int<64, 128>(v.H, [&](auto H) {
        return ppo_with_int<1, 2, 3, 4>(v.NC, [&](auto NC) {
          return mbpo_with_bool(pl.neq, [&](auto Q) {
            constexpr int h = decltype(H)::value, nc = decltype(NC)::value;
            return mbpo_launch<k_ppo_values_gae<h, nc, Q.value>>(v.n_vg, 256 * nc, lds, st, "ppo_grads", *A);
          }); }); });
    }
    case PpoValues::SEPARATE:
      return ppo_with_int<64, 128>(v.H, [&](auto H) {
        return mbpo_with_bool(pl.neq, [&](auto Q) {
          return mbpo_launch<k_ppo_values<decltype(H)::value, Q.value>>(v.vgrid, 256, pl.lds_values, st, "ppo_grads", *A);
        }); });
  }
  return MBPO_OK;
}

// 2. GAE on [B,T] (batch-major: the data's native layout, no transpose)   losses.py:94-99,128-184 (losses_new.py:181-226 with neq)
static int ppo_gae_launch(const mbpo_ppo_desc *d, const PpoPlan &pl, const PpoArgs &A, hipStream_t st) {
  if (pl.var.vg_G) return MBPO_OK;      // (done by the values + GAE launch)
  if (pl.neq)
    return mbpo_gae_scan_discounts(A.trunc, A.term, A.rew, A.baseline, A.boot, A.disc, A.vs, A.adv, d->batch_size, d->unroll_length,
                                   d->gae_lambda, 0, st);
  return mbpo_gae_scan(A.trunc, A.term, A.rew, A.baseline, A.boot, A.vs, A.adv, d->batch_size, d->unroll_length, d->discounting,
                       d->gae_lambda, 0, st);
}

// 3. advantage moments over the whole minibatch
static void ppo_moments_launch(const mbpo_ppo_desc *d, const PpoPlan &pl, const PpoArgs &A, hipStream_t st) {
  const float *adv = A.adv, *mom = A.mom;
  switch (pl.var.moments) {
    case PpoMoments::NONE: return;
    case PpoMoments::COMBINE:
      hipLaunchKernelGGL(k_ppo_moments_combine, dim3(1), dim3(256), 0, st, (const float *)A.mom_part, pl.var.n_vg, (float)pl.M, A.mom);
      return;
    case PpoMoments::FUSED: hipLaunchKernelGGL(k_moments_fused, dim3(1), dim3(1024), 0, st, adv, pl.M, A.mom); return;
    case PpoMoments::TWO_PASS: {
      float *part = d->workspace + pl.off_part;
      const long long blocks = (pl.M + 255) / 256;
      const int g = (int)(blocks < PPO_MOM_WGS ? blocks : PPO_MOM_WGS);
      hipLaunchKernelGGL(k_moments_partial<0>, dim3(g), dim3(256), 0, st, adv, pl.M, mom, part);
      hipLaunchKernelGGL(k_moments_final<0>, dim3(1), dim3(64), 0, st, (const float *)part, g, pl.M, A.mom);
      hipLaunchKernelGGL(k_moments_partial<1>, dim3(g), dim3(256), 0, st, adv, pl.M, mom, part);
      hipLaunchKernelGGL(k_moments_final<1>, dim3(1), dim3(64), 0, st, (const float *)part, g, pl.M, A.mom);
      return;
    }
  }
}

// 4. loss forward/backward into the slabs (the layered path: ONE slab, and loss partials of its own for the reduce launch)
static int ppo_fwd_bwd_launch(const mbpo_ppo_desc *d, const PpoPlan &pl, const PpoArgs &A, PpoReduceArgs *R, hipStream_t st) {
  const PpoVariant &v = pl.var;
  if (v.layered) {
    float *extras = nullptr;
    const int rc = ppo_layered_fwd_bwd(d, pl.pi, pl.v, d->workspace + pl.off_layered, A.vs, A.adv, A.mom, A.slabs, &extras, &R->n_extras, st);
    R->extras = extras;
    return rc;
  }
  if (v.lean) {
    PpoLeanArgs L;
    ppo_fill_lean(d, pl, A, &L);
    return ppo_lean_launch(L, d->x_dim, d->policy_layers - 2, v.n_slabs, st);
  }
  // (the instantiations are named in this order: it is their order in the device code object)
  if (v.wide) return mbpo_launch<k_ppo_fwd_bwd<64, 4, true>>(v.n_slabs, 1024, pl.lds_fb, st, "ppo_grads", A);
  if (v.H == 64 && !v.sp2) return mbpo_launch<k_ppo_fwd_bwd<64, 4, false>>(v.n_slabs, 1024, pl.lds_fb, st, "ppo_grads", A);
  if (v.sp2) return mbpo_launch<k_ppo_fwd_bwd<64, 2, false>>(v.n_slabs, 512, pl.lds_fb, st, "ppo_grads", A);      // (never wide)
  return mbpo_launch<k_ppo_fwd_bwd<128, 2, false>>(v.n_slabs, 512, pl.lds_fb, st, "ppo_grads", A);
}

// [3P optax.chain(clip_by_global_norm, adamw)] on the n_ss partials at off_sspart
static void ppo_clip_apply_launch(const mbpo_ppo_desc *d, const PpoPlan &pl, hipStream_t st) {
  PpoClipArgs C;
  ppo_fill_opt(d, &C);
  C.ss_part = d->workspace + pl.off_sspart; C.NPV = pl.NPV; C.n_parts = pl.n_ss; C.max_norm = d->max_grad_norm;
  // a few elements per thread: every workgroup re-adds all n_ss partials, so the grid is kept to at most 4 per CU
  const int want = (pl.NPV + 255) / 256, cap = 4 * mbpo_num_cus();
  hipLaunchKernelGGL(k_ppo_clip_apply, dim3(want < cap ? want : cap), dim3(256), 0, st, C);
}

// 5. grads = the sum of the slabs, loss metrics; fuse_apply: and the optimizer step
static void ppo_reduce_launch(const mbpo_ppo_desc *d, const PpoPlan &pl, const PpoReduceArgs &R, bool fuse_apply, hipStream_t st) {
  // The one-stage sum reads 256-byte pieces 68 KB apart: 22.7 us for the 35 MB of 512 slabs (C3, T = 40), unchanged by 4x the loads
  // in flight or by 1-KB pieces.  With many slabs: first groups of 16 over 4-KB contiguous runs, in place, then the 32 group sums.
  if (pl.var.reduce_two_stage)
    hipLaunchKernelGGL(k_ppo_reduce_groups, dim3((pl.NPV + 1023) / 1024, (R.n_slabs + 15) / 16), dim3(256), 0, st,
                       d->workspace + pl.off_slabs, pl.NPV, R.n_slabs);
  if (fuse_apply && pl.clip) {
    // clip_by_global_norm needs every workgroup's part of the norm before any element may move: the reduce launch leaves the
    // partials, one more launch clips and applies (the same partials and arithmetic as mbpo_ppo_apply: the same bits)
    hipLaunchKernelGGL(k_ppo_reduce<true>, dim3(pl.n_ss), dim3(256), 0, st, R);
    ppo_clip_apply_launch(d, pl, st);
  } else {
    hipLaunchKernelGGL(k_ppo_reduce<false>, dim3((pl.NPV + 63) / 64), dim3(256), 0, st, R);
  }
}

// One minibatch update: the five stages in order.  fuse_apply: mbpo_ppo_step, no seam for a collective.
static int ppo_update(const mbpo_ppo_desc *d, void *stream, bool fuse_apply) {
  PpoPlan pl;
  int rc = ppo_plan(d, &pl, true);
  if (rc != MBPO_OK) return rc;
  MBPO_REQUIRE(d->data, MBPO_ERR_ARG, "ppo_grads: null data");
  MBPO_REQUIRE((d->norm_mean == nullptr) == (d->norm_std == nullptr), MBPO_ERR_ARG, "ppo_grads: norm_mean/norm_std mismatch");
  hipStream_t st = (hipStream_t)stream;
  PpoArgs A;
  ppo_fill_args(d, pl, &A);
  rc = ppo_values_launch(d, pl, &A, st);
  if (rc != MBPO_OK) return rc;
  rc = ppo_gae_launch(d, pl, A, st);
  if (rc != MBPO_OK) return rc;
  ppo_moments_launch(d, pl, A, st);
  PpoReduceArgs R;
  ppo_fill_reduce(d, pl, A, fuse_apply, &R);
  rc = ppo_fwd_bwd_launch(d, pl, A, &R, st);
  if (rc != MBPO_OK) return rc;
  ppo_reduce_launch(d, pl, R, fuse_apply, st);
  MBPO_CHECK_LAUNCH("ppo_grads");
  return MBPO_OK;
}

extern "C" int mbpo_ppo_grads(const mbpo_ppo_desc *d, void *stream) { return ppo_update(d, stream, false); }

// One minibatch_step without a seam for a collective: the reduce launch applies AdamW to the elements it has just summed
// (k_ppo_apply's arithmetic, bit for bit) — one launch less per minibatch_step.
extern "C" int mbpo_ppo_step(const mbpo_ppo_desc *d, void *stream) { return ppo_update(d, stream, true); }

extern "C" int mbpo_ppo_apply(const mbpo_ppo_desc *d, void *stream) {
  PpoPlan pl;
  int rc = ppo_plan(d, &pl, true);
  if (rc != MBPO_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (pl.clip) {
    // the norm of the (all-reduced) scaled gradient as it stands in `grads` now, then the clipped step
    hipLaunchKernelGGL(k_ppo_sumsq, dim3(pl.n_ss), dim3(64), 0, st, (const float *)d->grads, pl.NPV, d->grad_scale,
                       d->workspace + pl.off_sspart);
    ppo_clip_apply_launch(d, pl, st);
  } else {
    PpoApplyArgs A;
    ppo_fill_opt(d, &A);
    A.NPV = pl.NPV;
    hipLaunchKernelGGL(k_ppo_apply, dim3((pl.NPV + 255) / 256), dim3(256), 0, st, A);
  }
  MBPO_CHECK_LAUNCH("ppo_apply");
  return MBPO_OK;
}
