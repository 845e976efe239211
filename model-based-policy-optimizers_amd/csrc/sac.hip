// sac.hip — S3-S8: SAC sgd_step as three kernels (see include/mbpo_hip.h for the flat state layout), and its host half.
//
//   k_sac_fwd_bwd   2 workgroups per 16-sample tile: a CRITIC role (pi(s') fwd, target-Q fwd, Q fwd+bwd) and an
//                   ACTOR role (pi(s) fwd+bwd, alpha loss, Q fwd + input-gradient bwd).  All three losses are taken
//                   at the OLD parameters (sac/sac.py:234-258), so the roles are independent.  fp32 MFMA; activations,
//                   pre-activations and deltas live in LDS; each workgroup writes its weight gradients to a private
//                   SLAB laid out like the flat params (no atomics: the cross-tile sum is a fixed-order reduce ->
//                   bitwise reproducible).
//   k_sac_reduce    grads[i] = sum over tiles of slab[t][i]; loss metrics; per-group sum-of-squares partials.
//   k_sac_apply     clip_by_global_norm + AdamW per optimizer group + Polyak on the critics.
//   k_sac_reduce_apply  (the default path, 2 launches per sgd_step instead of 3) both of the above in ONE launch: the optimizer step
//                   is applied UNCLIPPED, the previous state goes to an undo log, and the clip decision — which needs the global
//                   norm, i.e. every block's partial — is resolved by the NEXT consumer of the parameters: the prologue of the
//                   next k_sac_fwd_bwd, or k_sac_finalize.  clip_by_global_norm(max_grad_norm = 1e5, the reference default,
//                   sac/sac.py:96) practically never triggers; when it does, the consumer recomputes the clipped step from the
//                   undo log (same formulas, same order: bit-identical to the three-launch path).  A device-wide meeting point
//                   inside one launch was measured SLOWER than the kernel boundary it removes (round 1: 48 vs 40 us).
//
// Host half (behind the kernels): every update takes ONE path:  sac_plan (validate, sizes, workspace offsets)  ->  sac_variant (which
// forward/backward kernel)  ->  sac_fill_* (the kernels' argument blocks)  ->  sac_update (the launches).  The entry points differ in
// whether the forward/backward half runs and in the SacReduceKind that follows it.
// The kernels stay in this one unit, in this order: the device code object is then byte for byte the one it was before the host half
// was rewritten, so what a captured graph replays is unchanged by construction (DESIGN.md "Where dispatch lives").
//
// Algorithmic work per sample per sgd_step: 2*(5P + 12Q) FLOP — latency-bound at B=256, hence the
// few fat launches and the slab scheme instead of a tree of small kernels.
#include "common.hpp"
#include "chain_run.hpp"
#include "p2p.hpp"
#include "sac_layered.hpp"
#include <string.h>
#include <stdlib.h>
int mbpo_p2p_make_dev(const mbpo_p2p_desc *d, P2pDev *P);

#include "sac_shared.hpp"
#include "sac_lean.hpp"

// What one wave group walks in one phase, filled in by the host (sac_chain_table): the kernel fetches its entry with one
// scalar load instead of ~200 scalar instructions of role/phase/chain case analysis per phase.
struct SacChainDesc {
  int mode;        // CH_*
  int netid;       // 0 = policy shape, 1 = critic shape
  int base_sel;    // parameters relative to: 0 = params, 1 = target_q
  int param_off;   // floats
  int x, ldx;      // LDS offsets (floats from the dynamic-LDS base), -1 = none
  int pp0, pp1, zb, hb, y, dx;
  int slab_sel;    // 0 none, 1 = policy slab, 2 = critic slab
  int slab_off;    // floats inside the tile's slab
  int tp0, tp1;    // CH_FWD with a tangent (jvp): the tangent's ping-pong hidden tiles (its output goes to `dx`), -1 = none
};


struct SacArgs {
  MlpDev pi, q, qt;
  NetShape sh_pi, sh_q;
  SacChainDesc tab[3][5][4];   // [table role][phase (index nph = idle)][chain]; table role 2 exists only with `split`
  int X, U, B, D;
  const float *batch, *norm_mean, *norm_std, *log_alpha;
  const float *noise_alpha, *noise_critic, *noise_actor;
  unsigned long long seed, offset;
  const unsigned long long *rng_dev;
  float discounting, reward_scaling, target_entropy;
  int neq;                      // non_equidistant_time (losses.py:90-98)
  float neq_cd, neq_tl, neq_tu, neq_dt;
  float *slab_pi, *slab_q, *slab_ex;
  int ld_x, ld_xu, ld_h, ld_y, LH;
  unsigned int *p2p_epoch;      // multi-GPU peer exchange: [0] += 1, [1] += p2p_blocks at the start of every step (or NULL)
  unsigned int p2p_blocks;
  unsigned long long *stamps;   // measurement hook (mbpo_debug_set_stamps): [2 roles][16] s_memtime values of tile 0, or NULL
  SacOptArgs opt;               // clip check of the previous speculative step
  float *step_count_rw;         // optimizer count: bumped by block 0 of every fwd/bwd launch
  int split;                    // 1: THREE workgroups per tile — critic 0, actor(+alpha), critic 1 (see k_sac_fwd_bwd)
  int thin;                     // 1: layers with <= 8 inputs / <= 4 outputs by VALU around the runners (chain_run.hpp 'thin layers')
  int jvp;                      // 1 (u_dim == 1): the actor role gets dQ/da in FORWARD mode — the tangent rides along the critics' forward
                                // pass (chain_run.hpp JVP) and the critics' input-gradient phase does not exist: 12 dependent layer
                                // steps instead of 16 on the role that bounds the kernel
};

// The dynamic LDS of k_sac_fwd_bwd: float offsets of its regions in carve order, `end` = the launch's LDS size in floats.  The host's
// one statement of the layout (sac_plan's byte count, sac_chain_table's operands); the carve at the top of the kernel keeps its own
// expressions and must agree with this.
struct SacLds {
  long long row, sn, sn2, qin, qin2, pp, store, y, dy, dx, eps, a, sig, raw, lp, lpa, scal, gn, end;
};
static inline SacLds sac_lds(int row_len, int ld_x, int ld_xu, int ld_h, int ld_y, int LH, int U) {
  const long long T = 16LL * ld_h, U4 = (16LL * U + 3) & ~3LL;      // one hidden tile; one [16][U] sample array
  SacLds L;
  L.row = 0;                                      // [16][D] (flat copy of the tile's transitions)
  L.sn = L.row + 16LL * ((row_len + 3) & ~3);     // [16][ld_x]   normalised obs
  L.sn2 = L.sn + 16LL * ld_x;                     // [16][ld_x]   normalised next obs
  L.qin = L.sn2 + 16LL * ld_x;                    // [16][ld_xu]  [sn, a]
  L.qin2 = L.qin + 16LL * ld_xu;                  // [16][ld_xu]  [s'n, a']
  L.pp = L.qin2 + 16LL * ld_xu;                   // 4 tiles: ping-pong hidden / delta tiles
  L.store = L.pp + 4 * T;                         // 4*LH tiles: stored z / h
  L.y = L.store + 4LL * LH * T;                   // [3][16][ld_y]  network outputs
  L.dy = L.y + 3 * 16LL * ld_y;                   // [2][16][ld_y]  output gradients
  L.dx = L.dy + 2 * 16LL * ld_y;                  // [2][16][ld_xu] critic input gradients (actor role)
  L.eps = L.dx + 2 * 16LL * ld_xu;                // six [16][U] sample arrays
  L.a = L.eps + U4;
  L.sig = L.a + U4;
  L.raw = L.sig + U4;
  L.lp = L.raw + U4;
  L.lpa = L.lp + U4;
  L.scal = L.lpa + U4;                            // [4][16]
  L.gn = L.scal + 64;                             // [4]: group norms of the previous speculative optimizer step
  L.end = L.gn + 4;
  return L;
}

// Which forward/backward kernel one update launches and how (sac.hip, sac_variant): the layered path (sac_layered.hip), the
// specialised k_sac_lean (sac_lean.hip), or the instantiation of k_sac_fwd_bwd that sac_fwd_bwd_launch picks.
struct SacVariant {
  bool layered, lean, split, jvp, thin, wide_any;
  int H, wg_per_tile;
};

// Timeline stamps for DESIGN.md's phase breakdown: one s_memtime per phase boundary, written by thread 0 of tile 0.
#define SAC_STAMP(i)                                                                   \
  if (A.stamps && tile == 0 && tid == 0) {                                             \
    unsigned long long t_;                                                             \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");         \
    A.stamps[role * 16 + (i)] = t_;                                                    \
  }

// Workgroup = 8 waves = one 16-sample tile in one ROLE.  Wave w = (chain c = w/2, sub = w%2): each network chain is
// shared by 2 waves (column slices of H/2), chains advance side by side in lockstep, one workgroup barrier per layer
// (wave_mlp.hpp "Lockstep groups").  The per-sgd_step critical path is ~16 layer-steps of ~32 MFMAs per wave.
// (16 waves x 4 per chain halves the MFMAs per step again but caps a wave at 128 VGPRs: hipcc spilled ~850 registers.)
//   CRITIC role                                     ACTOR(+alpha) role
//   P1  c0: pi(s') fwd  c1: Q1(s,a) fwd+store       P1  c0: pi(s) fwd+store
//                       c2: Q2(s,a) fwd+store
//   -- sample a', log pi'                           -- sample alpha/actor actions
//   P2  c0: Qtgt1(s',a')  c1: Qtgt2(s',a')          P2  c0: Q1(s,a~) fwd (z kept)  c1: Q2(s,a~)
//   -- target y, errors, dL/dq                      -- min_q, dL/dq
//   P3  per layer: c0/c1: Q1/Q2 dgrad               P3  per layer: c0/c1: Q1/Q2 input-gradient
//                  c2/c3: Q1/Q2 wgrad               -- dL/dlogits
//                                                   P4  per layer: c0: pi dgrad   c1: pi wgrad
// SP = waves per chain, NCH = chain slots: NCH x SP waves; WIDE: chain_run.hpp fast_shape.  NCH = 2 is for the `split` launch, where
// no role carries more than two chains at a time: at hidden width 128 that makes room for 4 waves per chain (8 waves, 2 per SIMD,
// 256 VGPRs each) and with them for the register-image weight prefetch (a lane's share of a 128-wide layer is 64 weights + 2
// biases per image, two images) that 16 waves x 128 VGPRs cannot hold.
template <int H, int SP, bool WIDE, int NCH = 4, bool THIN = false>
__global__ void __launch_bounds__(64 * SP * NCH) k_sac_fwd_bwd(SacArgs A) {
  extern __shared__ __align__(16) float smem[];
  constexpr int HT = H / 16;
  const int tid_ = threadIdx.x, nthreads = 64 * SP * NCH;
  const int wave = __builtin_amdgcn_readfirstlane(tid_ >> 6);
  const int chain = wave / SP, sub = wave % SP;
  // Two workgroups per tile (critic role, actor role), or — `split`, used at hidden width 128 where a phase is bound by the
  // fp32-MFMA rate of its CU — three: the critic role once per critic.  Each critic workgroup runs pi(s') and BOTH target critics
  // (the target needs their minimum) but the forward, dgrad and wgrad of ITS critic only: no phase carries more than two chains, the
  // critic backward 2 x 256 MFMAs per layer on a CU instead of 4 x 256.  kq = the critic this workgroup owns (-1: both).
  int role, tile, trole, kq = -1;
  if (A.split) {
    trole = blockIdx.x % 3;
    tile = blockIdx.x / 3;
    role = trole == 1 ? 1 : 0;
    kq = trole == 1 ? -1 : (trole >> 1);
  } else {
    role = blockIdx.x & 1;   // 0 = critic, 1 = actor(+alpha)
    tile = blockIdx.x >> 1;
    trole = role;
  }
  const int X = A.X, U = A.U, D = A.D, B = A.B;
  const int row0 = tile * 16;
  const int ld_x = A.ld_x, ld_xu = A.ld_xu, ld_h = A.ld_h, ld_y = A.ld_y, LH = A.LH;
  const int T = 16 * ld_h;  // one hidden tile

  // ---- LDS carve (every region a multiple of 4 floats: rows stay 16-byte aligned) ----
  // The layout is SacLds (above), which the host sizes the launch and fills the chain table from: the two must agree.  The
  // carve keeps its own expressions (a folded local has moved scalar-register spills in this kernel before).
  float *s_row = smem;                      // [16][D] (flat copy of the tile's transitions)
  const int D4 = D;
  float *s_sn = s_row + 16 * ((D + 3) & ~3);  // [16][ld_x]   normalised obs
  float *s_sn2 = s_sn + 16 * ld_x;          // [16][ld_x]   normalised next obs
  float *s_qin = s_sn2 + 16 * ld_x;         // [16][ld_xu]  [sn, a]
  float *s_qin2 = s_qin + 16 * ld_xu;       // [16][ld_xu]  [s'n, a']
  float *s_pp = s_qin2 + 16 * ld_xu;        // 4 tiles: ping-pong hidden / delta tiles
  float *s_store = s_pp + 4 * T;            // 4*LH tiles: stored z / h
  float *s_y = s_store + 4 * LH * T;        // [3][16][ld_y]  network outputs
  float *s_dy = s_y + 3 * 16 * ld_y;        // [2][16][ld_y]  output gradients
  float *s_dx = s_dy + 2 * 16 * ld_y;       // [2][16][ld_xu] critic input gradients (actor role)
  const int U4 = (16 * U + 3) & ~3;
  float *s_eps = s_dx + 2 * 16 * ld_xu;     // [16][U] ...
  float *s_a = s_eps + U4;
  float *s_sig = s_a + U4;
  float *s_raw = s_sig + U4;
  float *s_lp = s_raw + U4;
  float *s_lpa = s_lp + U4;
  float *s_scal = s_lpa + U4;               // [4][16]
  float *s_gn = s_scal + 64;                // [4]: group norms of the previous speculative optimizer step

  {
    const int tid = tid_;
    SAC_STAMP(0);
  }
  // Clip check of the previous speculative optimizer step (k_sac_reduce_apply).  Nothing here may WAIT for a load (a branch on these
  // words at this point put a whole cold-miss latency in front of the tile loads: +2 us per launch), nothing may add work to a wave
  // the other waves wait for, and nothing may live in registers across the phase loop (this kernel is short of scalar registers;
  // every such value costs the lone waves spill code in every phase — measured 0.2-0.4 us each).  So: ONE scalar load of eight
  // words here (sequence numbers + the two slots of the quick verdict); after the first barrier they are folded into one flag —
  // "some workgroup of the reduce launch found its sum of squares at or above limit / n_workgroups, or not finite, and raised the
  // slot's word to +inf with a plain store" (group_sumsq): practically never at the reference's max_grad_norm = 1e5.  Only then,
  // behind the phases, are the canonical norms formed (fixed order: the clip decision and the clipped step are bit-identical to
  // mbpo_sac_apply's).
  // Warm the scalar cache with the whole kernel-argument block.  The phase loop fetches its operands lazily — the 64-byte chain
  // descriptor of each phase, network shapes, slab pointers — and every first touch of a kernarg line was a miss to memory
  // (the block is fresh for every launch): ~2 k cycles of "chain set-up" per phase, on every wave.  The LAST wave, which has no
  // tile element to load, reads one dword of every 64-byte line here (scalar loads: they fill the scalar cache the whole CU
  // shares) and pays the one cold-miss latency while the other waves wait for the tile anyway.
  if (wave == NCH * SP - 1) {
    const int *ka = reinterpret_cast<const int *>(&A.pi);
    int acc = 0;
#pragma unroll
    for (int i = 0; i < (int)(sizeof(SacArgs) / 64); ++i) acc += ka[i * 16];
    asm volatile("" ::"s"(acc));
  }
  const uint4 qw0 = *reinterpret_cast<const uint4 *>(A.opt.seq), qw1 = *reinterpret_cast<const uint4 *>(A.opt.seq + 4);
  const float count_in = A.step_count_rw[0];
  const unsigned int ep0_in = A.p2p_epoch ? A.p2p_epoch[0] : 0u, ep1_in = A.p2p_epoch ? A.p2p_epoch[1] : 0u;
  bool maybe_clip = false;
  // requested now, consumed after the first layer phase: the two scalar loads overlap the tile load instead of preceding it
  const float log_alpha_top = A.log_alpha[0];   // requested now, consumed after the first layer phase
  const float invB = 1.0f / (float)B;
  const float *pi_p = A.pi.params, *q1_p = A.q.params, *q2_p = A.q.params + A.q.net_stride;
  const float *t1_p = A.qt.params, *t2_p = A.qt.params + A.qt.net_stride;
  const int QL = A.q.n_layers, PL = A.pi.n_layers;
  const int Lmax = QL > PL ? QL : PL;
  float *y_pi = s_y, *y_q1 = s_y + 16 * ld_y, *y_q2 = s_y + 2 * 16 * ld_y;
  // stored activations.  critic role: Q1 (z,h), Q2 (z,h);  actor role: policy (z,h), Q1 z, Q2 z
  const int o_sn = (int)(s_sn - smem), o_sn2 = (int)(s_sn2 - smem), o_qin = (int)(s_qin - smem), o_qin2 = (int)(s_qin2 - smem);
  const int o_pp = (int)(s_pp - smem), o_y = (int)(s_y - smem), o_dy = (int)(s_dy - smem), o_dx = (int)(s_dx - smem);
  const int o_st0 = (int)(s_store - smem), o_st1 = o_st0 + LH * T, o_st2 = o_st0 + 2 * LH * T, o_st3 = o_st0 + 3 * LH * T;

  // Phases (one barrier per layer step inside a phase, one after each elementwise section E):
  //   critic role:  E load | F0: c0 pi(s') fwd, c1/c2 Q1/Q2(s,a) fwd | E sample a' | F1: c0/c1 Qtgt1/2(s',a') fwd | E targets
  //                 | B2: c0/c1 Q1/Q2 dgrad, c2/c3 Q1/Q2 wgrad | E loss partials
  //   actor role:   E load | F0: c0 pi(s) fwd | E sample a | F1: c0/c1 Q1/Q2(s,a) fwd | E dL/dq | B2: c0/c1 Q input-grad
  //                 | E dL/dlogits | B3: c0 pi dgrad, c1 pi wgrad | E loss partials
  // What this wave walks in the current phase (wave-uniform scalars; LDS operands as offsets from smem, -1 = none).
  WSet<HT, SP> R;
  constexpr int H_ = H;
  constexpr bool THIN_OK = THIN;     // thin layers by VALU (chain_run.hpp): a kernel variant of its own, chosen by the host
  static_assert(!THIN || (H_ == 64 && SP == 4 && !WIDE && NCH == 2), "thin layers: H = 64, four waves per chain, two chain slots");
  float tw[THIN_KMAX + 1];                 // this lane's share of the next phase's thin layer (a column of W0 + bias, or a row of Wout)
#pragma unroll
  for (int k = 0; k <= THIN_KMAX; ++k) tw[k] = 0.f;
  int mode = CH_IDLE, netid = 0;
  const float *cparams = pi_p;
  float *cslab = nullptr;
  int cx = -1, cldx = ld_x, cpp0 = -1, cpp1 = -1, czb = -1, chb = -1, cy = -1, cdx = -1, ctp0 = -1, ctp1 = -1;
#define P(off) ((off) < 0 ? (float *)nullptr : smem + (off))
  const int nph = (role == 0 || A.jvp) ? 3 : 4;
  // At most two passes over the phases: the second one only after a clip fix-up of the previous optimizer step (rare), whose code
  // sits behind the phase loop so that it costs the loop neither registers nor instruction-cache lines.
  // The clip decision must not touch the phase loop's control flow: a `break` on it, or a loop bound that depends on it, made hipcc
  // duplicate the runners' code (+2.8 us per launch).  So the phases always run to the end; the norms (formed on the side by an
  // idle wave during phase 0) are looked at AFTER the loop, and in the rare case of a clip the optimizer step is fixed up and ALL
  // phases run a second time — whatever the first pass wrote (slabs, loss partials) is overwritten.
  // (A loop around the phase loop for the second pass cost the first pass 2 us — hipcc compiles a phase loop nested in another
  // loop worse than one that stands alone — so the phases are a lambda expanded twice: the second copy is cold code behind the first.)
  auto run_phases = [&](const float log_alpha_v) __attribute__((always_inline)) {
#pragma nounroll
  for (int ph = -1; ph < nph; ++ph) {
    const int tid = opaque(tid_), lane = tid & 63;   // keeps per-lane addresses of all phases from being hoisted and spilled
    if (ph >= 0) {
      int len = (role == 0) ? (ph == 0 ? Lmax : QL) : ((ph == 0 || ph == nph - 1) ? PL : QL);
      const NetShape sh = netid == 0 ? A.sh_pi : A.sh_q;
      constexpr bool thin = THIN_OK;
      if constexpr (THIN_OK) {
        {
          // thin layers by VALU (chain_run.hpp): the chain's four waves form layer 0 of a forward chain, or delta_{L-2} and the
          // output layer's weight gradient of a backward pair, from what the preceding section left in LDS; then the runners
          // walk the H x H layers only (forward: L - 1 barriers instead of L, backward: L - 2)
          if (mode == CH_FWD)
            thin_fwd_first(tw, sh.K_in, sh.act, P(cx), cldx, chb >= 0 ? P(chb) : P(cpp0), P(czb), P(ctp0), X, ld_h, sub, lane);
          else if (mode == CH_DGRAD)
            thin_dgrad_out(tw, sh.N_out, sh.act, P(cy), ld_y, P(czb) + (sh.L - 2) * T, ((sh.L - 1) & 1) ? P(cpp1) : P(cpp0), ld_h, sub, lane);
          else if (mode == CH_WGRAD)
            thin_wgrad_out<H>(sh.N_out, P(chb) + (sh.L - 2) * T, ld_h, P(cy), ld_y,
                              cslab + (sh.K_in * H + H) + (sh.L - 2) * (H * H + H), sub, lane);
          __syncthreads();
          len -= (ph == nph - 1) ? 2 : 1;
        }
      }
      if (mode == CH_FWD)
        chain_fwd_run<HT, SP, WIDE, !WIDE, THIN_OK>(sh, cparams, P(cx), cldx, P(cpp0), P(cpp1), P(czb), P(chb), P(cy), ld_y, ld_h, len, sub, lane, R,
                                           (A.stamps && tile == 0 && role == 1 && ph == 0 && wave == 0) ? A.stamps + 40 : nullptr,
                                           P(ctp0), P(ctp1), ctp0 >= 0 ? P(cdx) : nullptr, ld_xu, X);
      else if (mode == CH_DGRAD)
        chain_dgrad_run<HT, SP, WIDE, THIN_OK>(sh, cparams, P(cy), ld_y, P(czb), P(cpp0), P(cpp1), P(cdx), ld_xu, ld_h, len, sub, lane, R);
      else if (mode == CH_WGRAD) {
        chain_wgrad_run<HT, SP, WIDE, THIN_OK>(sh, P(cx), cldx, P(chb), P(cy), ld_y, P(cpp0), P(cpp1), cslab, false, ld_h, len, sub, lane,
                                (A.stamps && tile == 0 && role == 0 && sub == 0 && chain == (A.split ? 1 : 2)) ? A.stamps + 48 : nullptr);
      } else
        chain_idle_run(len);
      if constexpr (THIN_OK) {
        // layer 0's weight gradient: delta_0 is complete (the runners' last barrier); the dgrad and the wgrad chain of the pair
        // share input tile, delta tiles and slab, so all eight waves take one input row k (or the bias) each
        if (ph == nph - 1 && (mode == CH_WGRAD || mode == CH_DGRAD))
          thin_wgrad_first<H>(sh.K_in, P(cx), cldx, P(cpp1), ld_h, cslab, chain * SP + sub, lane);
      }
    }
    SAC_STAMP(2 * ph + 3);
    // ---- the chain this wave walks in the NEXT phase; its first layer's weights are requested now ----
    {
      const int nx = ph + 1;
      const SacChainDesc &cd = A.tab[trole][nx][chain];
      mode = cd.mode;
      netid = cd.netid;
      cparams = (cd.base_sel ? A.qt.params : A.pi.params) + cd.param_off;
      cx = cd.x; cldx = cd.ldx; cpp0 = cd.pp0; cpp1 = cd.pp1; czb = cd.zb; chb = cd.hb; cy = cd.y; cdx = cd.dx;
      ctp0 = cd.tp0; ctp1 = cd.tp1;
      cslab = cd.slab_sel == 1 ? A.slab_pi + (long long)tile * A.pi.n_params + cd.slab_off
                               : (cd.slab_sel == 2 ? A.slab_q + (long long)tile * (2 * A.q.n_params) + cd.slab_off : nullptr);
      const NetShape shn = netid == 0 ? A.sh_pi : A.sh_q;
      if constexpr (THIN_OK) {
        if (mode == CH_FWD) chain_fwd_prefetch_thin<HT, SP, WIDE>(R, shn, cparams, sub, lane, tw);
        else if (mode == CH_DGRAD) chain_dgrad_prefetch_thin<HT, SP>(R, shn, cparams, sub, lane, tw);
      } else {
        if (mode == CH_FWD) chain_fwd_prefetch<HT, SP, WIDE>(R, shn, cparams, sub, lane);
        else if (mode == CH_DGRAD) chain_dgrad_prefetch<HT, SP, WIDE>(R, shn, cparams, sub, lane);
      }
    }
    if (A.stamps && tile == 0 && tid == 0 && ph == 1) {
      unsigned long long t_;
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");
      A.stamps[role * 16 + 14] = t_;
    }
    // ---- elementwise section after phase ph ----
    if (ph == -1) {
      // load the tile's transitions; normalise observations (q and policy both preprocess obs: sac/networks.py:76-78,96-98).
      // Every global load of this section is independent: one latency, one barrier.
      const long long nvalid = (long long)(B - row0 < 16 ? B - row0 : 16) * D;
      for (int idx = tid; idx < 16 * D; idx += nthreads) s_row[idx] = idx < nvalid ? A.batch[(long long)row0 * D + idx] : 0.f;
      for (int idx = tid; idx < 16 * X; idx += nthreads) {
        const int r = idx & 15, cc = idx >> 4;
        float o = 0.f, o2 = 0.f;
        if (row0 + r < B) {
          o = A.batch[(long long)(row0 + r) * D + cc];
          o2 = A.batch[(long long)(row0 + r) * D + X + U + 2 + cc];
        }
        if (A.norm_mean) {
          const float mu = A.norm_mean[cc], sd = A.norm_std[cc];
          o = (o - mu) / sd;
          o2 = (o2 - mu) / sd;
        }
        s_sn[r * ld_x + cc] = o;
        s_sn2[r * ld_x + cc] = o2;
        s_qin[r * ld_xu + cc] = o;
        s_qin2[r * ld_xu + cc] = o2;
      }
      if (role == 0) {
        for (int idx = tid; idx < 16 * U; idx += nthreads) {
          const int r = idx & 15, d = idx >> 4;
          s_qin[r * ld_xu + X + d] = (row0 + r < B) ? A.batch[(long long)(row0 + r) * D + X + d] : 0.f;  // transitions.action
        }
      }
      // The noise of the sampling sections depends on (seed, offset, element) only: it is drawn HERE, by waves that have no tile
      // element to load, while the tile is in flight — Philox + Box-Muller (logf, sqrtf, cosf: ~250 instructions) used to sit in
      // the sampling sections, on the lone wave every other wave waits for.  critic role: next-action noise -> s_eps;
      // actor role: actor-loss noise -> s_eps, alpha-loss noise -> s_lpa (replaced by the log-prob when it is used).
      {
        const int half = nthreads / 2;
        const RngKey rkq = rng_resolve(A.seed, A.offset, A.rng_dev);
        if (tid >= half) {
          const bool second = tid >= half + half / 2;
          if (!second || role == 1) {
            for (int i2 = tid - half - (second ? half / 2 : 0); i2 < 16 * U; i2 += half / 2) {
              const int r = i2 & 15, d = i2 >> 4, idx = r * U + d;
              const long long nidx = (long long)(row0 + r) * U + d;
              float e = 0.f;
              if (row0 + r < B) {
                const float *given = second ? A.noise_alpha : (role == 0 ? A.noise_critic : A.noise_actor);
                const unsigned int stream = second ? MBPO_STREAM_SAC_ALPHA : (role == 0 ? MBPO_STREAM_SAC_CRITIC : MBPO_STREAM_SAC_ACTOR);
                e = given ? given[nidx] : philox_normal(rkq.seed, rkq.offset, stream, (unsigned long long)nidx);
              }
              (second ? s_lpa : s_eps)[idx] = e;
            }
          }
        }
      }
    }
    const float alpha = expf(log_alpha_v);
    if (ph == -1) {
    } else if (role == 0) {
      // ============================== CRITIC (sac/losses.py:74-110) ==============================
      if (ph == 0) {
        // next_action ~ policy(next_observation); next_log_prob (:80-87)
        for (int i2 = tid; i2 < 16 * U; i2 += nthreads) {
          const int r = i2 & 15, d = i2 >> 4, idx = r * U + d;
          const float eps = s_eps[idx];      // drawn in the tile section
          ActSample sm = normal_tanh_sample(y_pi[r * ld_y + d], y_pi[r * ld_y + U + d], eps);
          s_qin2[r * ld_xu + X + d] = sm.a;  // postprocess(next_action)
          s_lp[idx] = sm.lp;
        }
        if (tid < 32) {  // keep q_old_action (:78-79) out of the way of the target critics' outputs
          const int k = tid >> 4, r = tid & 15;
          if (kq < 0 || k == kq) s_scal[32 + tid] = (k == 0 ? y_q1 : y_q2)[r * ld_y];
        }
      } else if (ph == 1) {
        float e2 = 0.f;
        if (tid < 32) {
          const int k = tid >> 4, r = tid & 15;
          const bool ok = row0 + r < B;
          float nlp = 0.f;
          for (int d = 0; d < U; ++d) nlp += s_lp[r * U + d];
          const float nq = fminf(y_q1[r * ld_y], y_q2[r * ld_y]);
          const float next_v = nq - alpha * nlp;                                                   // :89
          const float rew = s_row[r * D4 + X + U], disc = s_row[r * D4 + X + U + 1];
          float gamma = A.discounting;
          if (A.neq) {                                                                             // :90-96
            const float pseudo = s_row[r * D4 + X + U - 1];                                        // transitions.action[..., -1]
            float tfa = (A.neq_tu - A.neq_tl) / 2.0f * pseudo + (A.neq_tu + A.neq_tl) / 2.0f;
            tfa = floor_divide_f(tfa, A.neq_dt) * A.neq_dt;
            gamma = expf(-A.neq_cd * tfa);
          }
          const float target = rew * A.reward_scaling + disc * gamma * next_v;                     // :101-103
          const float trunc = s_row[r * D4 + D - 1];
          const float err = (ok && (kq < 0 || k == kq)) ? (s_scal[32 + tid] - target) * (1.f - trunc) : 0.f;   // q_error :104-108 (own critic)
          e2 = err * err;
          // loss = 0.5*mean(err^2) over [B,2]  ->  dL/dq = err*(1-trunc)/(2B)
          s_dy[(k * 16 + r) * ld_y] = err * (1.f - trunc) * (0.5f * invB);
        }
        // the tile's loss partial, formed here from the producers' registers (a shuffle tree over the first wave: fixed order)
        // instead of by one thread re-reading 32 LDS words at the very end of the launch
        if (wave == 0) {
          const float acc = wave_sum64(e2);
          if (tid == 0) A.slab_ex[tile * 4 + (kq == 1 ? 3 : 0)] = acc;     // (split: the two critics' partials in slots 0 and 3, added by the reduce)
        }
      }
    } else {
      // ============================== ACTOR + ALPHA (sac/losses.py:61-72, 112-125) ==============================
      if (ph == 0) {
        // two independent samples per element: the first half of the workgroup draws the actor-loss sample, the second half
        // the alpha-loss sample (different waves: the two instruction streams run side by side)
        const int half = nthreads / 2;
        const bool second = tid >= half;
        for (int i2 = second ? tid - half : tid; i2 < 16 * U; i2 += half) {
          const int r = i2 & 15, d = i2 >> 4, idx = r * U + d;
          const float loc = y_pi[r * ld_y + d], raw = y_pi[r * ld_y + U + d];
          if (second) {
            const float e_al = s_lpa[idx];     // drawn in the tile section
            ActSample sal = normal_tanh_sample(loc, raw, e_al);   // alpha loss sample (:66-68)
            s_lpa[idx] = sal.lp;
          } else {
            const float e_ac = s_eps[idx];     // drawn in the tile section
            ActSample sac = normal_tanh_sample(loc, raw, e_ac);   // actor loss sample (:117-119)
            s_lp[idx] = sac.lp;
            s_eps[idx] = e_ac;
            s_a[idx] = sac.a;
            s_sig[idx] = sac.sigma;
            s_raw[idx] = raw;
            s_qin[r * ld_xu + X + d] = sac.a;  // postprocess(action) (:120)
          }
        }
      } else if (ph == 1) {
        float l_al = 0.f, l_ac = 0.f;
        if (tid < 16) {
          const int r = tid;
          const bool ok = row0 + r < B;
          float lp_al = 0.f, lp_ac = 0.f;
          for (int d = 0; d < U; ++d) {
            lp_al += s_lpa[r * U + d];
            lp_ac += s_lp[r * U + d];
          }
          // alpha_loss = alpha * stop_gradient(-log_prob - target_entropy); d/dlog_alpha = the same value   (:70-72)
          l_al = ok ? alpha * (-lp_al - A.target_entropy) : 0.f;
          const float q0 = y_q1[r * ld_y], q1 = y_q2[r * ld_y];
          const float mq = fminf(q0, q1);
          l_ac = ok ? (alpha * lp_ac - mq) : 0.f;   // actor_loss = alpha*log_prob - min_q   (:123-124)
          // d(mean(-min_q))/dq_k: -1/B on the arg-min critic (ties split evenly, as jnp.min's gradient does)
          float g0 = 0.f, g1 = 0.f;
          if (ok) {
            if (q0 < q1) g0 = -invB;
            else if (q1 < q0) g1 = -invB;
            else g0 = g1 = -0.5f * invB;
          }
          if (A.jvp) {
            // forward mode (u_dim == 1): the critics' forward pass carried d q_k / d a along (s_dx[k][r][0]); the actor loss's
            // gradient with respect to the action and, from it, the logits' gradients follow here — no critic backward phase
            const float dLda = g0 * s_dx[r * ld_xu] + g1 * s_dx[(16 + r) * ld_xu];
            const float a = s_a[r], sg = s_sig[r], eps = s_eps[r], raw = s_raw[r];
            const float gz = dLda * (1.f - a * a) + alpha * invB * 2.f * a;
            const float gsig = gz * eps - alpha * invB / sg;
            s_dy[r * ld_y] = ok ? gz : 0.f;                              // d/dloc
            s_dy[r * ld_y + 1] = ok ? gsig * fast_sigmoid(raw) : 0.f;    // d/draw = d/dsigma * softplus'(raw)
          } else {
            s_dy[r * ld_y] = g0;
            s_dy[(16 + r) * ld_y] = g1;
          }
        }
        if (wave == 0) {     // the tile's loss partials from the producers' registers (shuffle tree: fixed order)
          const float al = wave_sum64(l_al), ac = wave_sum64(l_ac);
          if (tid == 0) {
            A.slab_ex[tile * 4 + 1] = ac;
            A.slab_ex[tile * 4 + 2] = al;
          }
        }
      } else if (ph == 2 && !A.jvp) {
        for (int i2 = tid; i2 < 16 * U; i2 += nthreads) {
          const int r = i2 & 15, d = i2 >> 4, idx = r * U + d;
          const bool ok = row0 + r < B;
          const float a = s_a[idx], sg = s_sig[idx], eps = s_eps[idx], raw = s_raw[idx];
          const float dLda = s_dx[r * ld_xu + X + d] + s_dx[(16 + r) * ld_xu + X + d];
          // z = loc + sigma*eps;  log_prob = const - log(sigma) - log(1 - tanh(z)^2)  =>  dlp/dz = 2a, dlp/dsigma = -1/sigma
          const float gz = dLda * (1.f - a * a) + alpha * invB * 2.f * a;
          const float gsig = gz * eps - alpha * invB / sg;
          s_dy[r * ld_y + d] = ok ? gz : 0.f;                              // d/dloc
          s_dy[r * ld_y + U + d] = ok ? gsig * fast_sigmoid(raw) : 0.f;    // d/draw = d/dsigma * softplus'(raw)
        }
      }
    }
    __syncthreads();
    if (ph == -1) {
      // the words requested at the top have arrived with the tile: use them up (idempotent: a second pass repeats the same stores)
      {
        const unsigned int seq_issued = qw0.x, seq_resolved = qw0.y;
        const bool odd = (seq_issued & 1u) == 0u;        // the step being checked is number seq_issued - 1: its slot is the OTHER one
        const float q0 = __uint_as_float(odd ? qw1.y : qw0.z), q1 = __uint_as_float(odd ? qw1.z : qw0.w), q2 = __uint_as_float(odd ? qw1.w : qw1.x);
        const float lim = (A.opt.max_norm / A.opt.grad_scale) * (A.opt.max_norm / A.opt.grad_scale) * 0.9998f;
        maybe_clip = seq_issued != seq_resolved && !(q0 < lim && q1 < lim && q2 < lim);
      }
      if (blockIdx.x == 0 && tid == 0) {
        // this step's slot: published for the reduce launch, emptied for its atomics
        const unsigned int slot = qw0.x & 1u;
        A.opt.slot_word[0] = slot;
        float *q = reinterpret_cast<float *>(A.opt.seq) + 2 + 3 * slot;
        q[0] = 0.f; q[1] = 0.f; q[2] = 0.f;
        // optax's count: one per sgd_step.  Nothing in this kernel uses it; the reduce / apply launches of this step read the final
        // value (kernel boundary), the clip fix-up of the NEXT launch reads the copy k_sac_reduce_apply keeps.  (A load -> add ->
        // store chain at the very top made block 0 wait a cold-miss latency before its first tile load.)
        A.step_count_rw[0] = count_in + 1.0f;
        if (A.p2p_epoch) {   // multi-GPU peer exchange: the epoch is stable while the reduce / gather launches of this step read it
          A.p2p_epoch[0] = ep0_in + 1u;
          A.p2p_epoch[1] = ep1_in + A.p2p_blocks;
        }
      }
    }

    SAC_STAMP(2 * ph + 4);
  }
  };
  run_phases(log_alpha_top);
  if (!maybe_clip) return;        // the common case: this launch is done
  // RARE from here on.  Canonical norms (fixed order), the exact decision, and if a group really clips: fix its step up from the undo
  // log and run ALL phases again — what the first pass wrote (slabs, loss partials) is overwritten.
  sac_group_norms(A.opt, s_gn, tid_);
  __syncthreads();
  if (s_gn[0] < A.opt.max_norm && s_gn[1] < A.opt.max_norm && s_gn[2] < A.opt.max_norm) return;
  if (blockIdx.x == 0 && tid_ == 0) A.opt.seq[SAC_CTL_CLIP_EVENTS] += 1u;     // (one writer per launch; read by the host between epochs)
  sac_clip_fixup(A.opt, s_gn, opaque(tid_), nthreads);
  __threadfence();
  __syncthreads();
  run_phases(A.log_alpha[0]);
}

// ------------------------------------------------------------------------------------------------
struct SacReduceArgs {
  const float *slab_pi, *slab_q, *slab_ex;
  int n_tiles, P, Q2, B;
  float *grads, *metrics, *metrics_accum, *ss_part, *step_count;
  // sequence words {issued, resolved} of the speculative two-launch steps (SacOptArgs::seq).  The reduce launch of EVERY step
  // flavour records that whatever was pending before this step's fwd/bwd launch has been resolved by it (its prologue ran the
  // check and the fix-up) — this launch overwrites ss_part, the operands of that check, so a later reader must not repeat it on
  // the new step's partials (mbpo_sac_step -> mbpo_sac_grads + mbpo_sac_apply -> mbpo_sac_finalize).  Written by the
  // launch AFTER the fwd/bwd launch, never from inside it: late-starting workgroups read these words at their top.
  unsigned int *seq;
};

// What follows the forward/backward launch of one update:
//   PLAIN           k_sac_reduce: grads[i] = sum over tiles of slab[t][i]; loss metrics; per-group sum-of-squares partials
//   PUSH            k_sac_reduce_push: the local sums go to every rank's exchange region (k_sac_gather completes them)
//   EXCHANGE        k_sac_reduce_exchange: push, wait for the peers and sum the world slots in one launch
//   APPLY           k_sac_reduce_apply<false>: the reduction and the unclipped optimizer step in one launch (the default path)
//   APPLY_EXCHANGE  k_sac_reduce_apply<true>: the same with the peer exchange in between
enum class SacReduceKind { NONE, PLAIN, PUSH, EXCHANGE, APPLY, APPLY_EXCHANGE };
// the kinds whose workgroups wait inside the kernel for the peers' same kernel: the whole grid must be co-resident
static inline bool sac_reduce_waits(SacReduceKind k) { return k == SacReduceKind::EXCHANGE || k == SacReduceKind::APPLY_EXCHANGE; }
// the kinds that use the peer exchange regions at all
static inline bool sac_reduce_p2p(SacReduceKind k) { return k == SacReduceKind::PUSH || sac_reduce_waits(k); }

// sum-of-squares partials per workgroup and optimizer group (0 policy, 1 critics, 2 alpha), fixed order
__device__ __forceinline__ void group_sumsq(float g, int i, int P, int Q2, int NP, float *ss_part, float *quick = nullptr,
                                            float blk_lim = 0.f) {
  __shared__ float s_ss[3][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float gg = (i < NP) ? g * g : 0.f;
  const int grp = (i < P) ? 0 : (i < P + Q2 ? 1 : 2);
  float v0 = wave_sum64(grp == 0 ? gg : 0.f), v1 = wave_sum64(grp == 1 ? gg : 0.f), v2 = wave_sum64(grp == 2 ? gg : 0.f);
  if (lane == 0) {
    s_ss[0][wave] = v0;
    s_ss[1][wave] = v1;
    s_ss[2][wave] = v2;
  }
  __syncthreads();
  if (tid < 3) {
    const float part = s_ss[tid][0] + s_ss[tid][1] + s_ss[tid][2] + s_ss[tid][3];
    ss_part[blockIdx.x * 3 + tid] = part;       // the canonical partials: summed in a FIXED order by whoever needs the norm
  }
  // The quick clip test, without atomics: the groups share max_grad_norm, so if EVERY workgroup's sum over the three groups stays
  // below limit / n_workgroups, every group's total is below the limit.  A workgroup that is not (or holds a NaN) raises the
  // slot's word with a plain store (several may: same value); the reader's "word < limit" then fails and the canonical norms
  // decide.  (Round 2 first added the per-group sums up with float atomics: 309 same-line atomics per launch, and a launch does
  // not end before its last atomic has been performed — 0.5-0.9 us per update.)
  if (quick && tid == 0) {
    float tot = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) tot += s_ss[k][0] + s_ss[k][1] + s_ss[k][2] + s_ss[k][3];
    // +inf, not a large finite number: with max_grad_norm so large that the limits overflow to +inf (clipping "disabled") a
    // non-finite gradient must still fail the reader's `word < limit` (inf < inf is false), as the three-launch path's
    // canonical check does
    if (!(tot < blk_lim)) quick[0] = __builtin_inff();
  }
}

// One element of the multi-launch reductions (k_sac_reduce, k_sac_reduce_push, k_sac_reduce_exchange): element i's slab sum over the
// tiles, returned; the thread that owns log_alpha (i == NP - 1) also forms the loss metrics, adds them to metrics_accum and records in
// seq[1] that nothing is pending any more.
__device__ __forceinline__ float sac_reduce_element(const SacReduceArgs &A, int i, int NP) {
  const unsigned int seq_issued = (i == NP - 1) ? A.seq[0] : 0u;      // requested beside the slab sums
  float g = 0.f;
  if (i < A.P) {
    g = slab_sum<16>(A.slab_pi, A.P, A.n_tiles, i);
  } else if (i < A.P + A.Q2) {
    const int j = i - A.P;
    g = slab_sum<16>(A.slab_q, A.Q2, A.n_tiles, j);
  } else if (i == NP - 1) {
    // (all loads of the three sums in flight together: this one thread is the kernel's critical path)
    const float ce = slab_sum<16>(A.slab_ex, 4, A.n_tiles, 0) + slab_sum<16>(A.slab_ex, 4, A.n_tiles, 3), ac = slab_sum<16>(A.slab_ex, 4, A.n_tiles, 1),
                al = slab_sum<16>(A.slab_ex, 4, A.n_tiles, 2);
    const float invB = 1.0f / (float)A.B;
    g = al * invB;                          // d alpha_loss / d log_alpha
    const float m0 = 0.5f * ce * (0.5f * invB), m1 = ac * invB, m2 = al * invB;   // critic_loss = 0.5 * mean over [B,2]
    A.metrics[0] = m0;
    A.metrics[1] = m1;
    A.seq[1] = seq_issued;       // nothing is pending any more: this step is not speculative
    A.metrics[2] = m2;
    if (A.metrics_accum) {       // (no load of what was just stored: each such round trip is part of the launch's tail)
      const float a0 = A.metrics_accum[0], a1 = A.metrics_accum[1], a2 = A.metrics_accum[2], a4 = A.metrics_accum[4];
      A.metrics_accum[0] = a0 + m0;
      A.metrics_accum[1] = a1 + m1;
      A.metrics_accum[2] = a2 + m2;
      A.metrics_accum[4] = a4 + 1.0f;
    }
  }
  return g;
}

__global__ void __launch_bounds__(256) k_sac_reduce(SacReduceArgs A) {
  const int NP = A.P + A.Q2 + 1;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const float g = sac_reduce_element(A, i, NP);
  if (i < NP) A.grads[i] = g;
  group_sumsq(g, i, A.P, A.Q2, NP, A.ss_part);
}

// multi-GPU: the reduced local gradient goes straight into every rank's exchange region (p2p.hpp) instead of a collective
__global__ void __launch_bounds__(256) k_sac_reduce_push(SacReduceArgs A, P2pDev X) {
  const int NP = A.P + A.Q2 + 1;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const unsigned epoch = X.epoch[0];
  const float g = sac_reduce_element(A, i, NP);
  p2p_push(X, epoch, i, NP, g);
}

// multi-GPU: wait for every rank's gradient, add the world slots in rank order, form the clip-norm partials
__global__ void __launch_bounds__(256) k_sac_gather(P2pDev X, float *grads, int P, int Q2, float *ss_part) {
  const int NP = P + Q2 + 1;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const unsigned epoch = X.epoch[0];
  const bool ok = p2p_wait(X, X.epoch[1]);
  float g = 0.f;
  if (i < NP) {
    g = ok ? p2p_sum(X, epoch, i) : NAN;
    grads[i] = g;
  }
  group_sumsq(g, i, P, Q2, NP, ss_part);
}

// multi-GPU, one launch: local slab reduction -> stores into every rank's region -> wait for every rank's arrivals -> sum of the
// world slots in rank order -> clip-norm partials.  All workgroups of the grid (NP/256 ~ 100) are co-resident, so waiting inside
// the producing kernel for the peers' same kernel cannot deadlock; compared with k_sac_reduce_push + k_sac_gather this removes a
// kernel boundary from every sgd_step and leaves the xGMI store latency as the only cost of the exchange.
__global__ void __launch_bounds__(256) k_sac_reduce_exchange(SacReduceArgs A, P2pDev X) {
  const int NP = A.P + A.Q2 + 1;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const unsigned epoch = X.epoch[0], want = X.epoch[1];
  const float g = sac_reduce_element(A, i, NP);
  p2p_push(X, epoch, i, NP, g);
  const bool ok = p2p_wait(X, want);
  float gs = 0.f;
  if (i < NP) {
    gs = ok ? p2p_sum(X, epoch, i) : NAN;
    A.grads[i] = gs;
  }
  group_sumsq(gs, i, A.P, A.Q2, NP, A.ss_part);
}

__global__ void __launch_bounds__(256) k_sac_sumsq(const float *grads, int P, int Q2, float *ss_part) {
  const int NP = P + Q2 + 1;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const float g = i < NP ? grads[i] : 0.f;
  group_sumsq(g, i, P, Q2, NP, ss_part);
}

__global__ void __launch_bounds__(256) k_sac_apply(SacOptArgs A) {
  __shared__ float s_scale[3];
  __shared__ float s_corr[2];
  const int tid = threadIdx.x;
  // the element's own operands are requested first: their latency overlaps the norm reduction below
  const int NP = A.P + A.Q2 + 1;
  const int i = blockIdx.x * 256 + tid;
  const bool in = i < NP;
  const float g_in = in ? A.grads[i] : 0.f, m_in = in ? A.adam_m[i] : 0.f, v_in = in ? A.adam_v[i] : 0.f, p_in = in ? A.params[i] : 0.f;
  const float count_in = A.step_count[0];
  const bool crit = in && i >= A.P && i < A.P + A.Q2;
  const float tq_in = crit ? A.target_q[i - A.P] : 0.f;
  sac_group_norms(A, s_scale, tid);          // waves 0..2: fixed shuffle tree -> deterministic
  if (tid == 192) {
    // the Adam bias corrections are the same for every element: the fourth wave forms them (two powf, ~300 instructions)
    // beside the three norm reductions instead of every wave after the barrier
    s_corr[0] = 1.f - powf(0.9f, count_in);
    s_corr[1] = 1.f - powf(0.999f, count_in);
  }
  __syncthreads();
  if (!in) return;
  const int grp = (i < A.P) ? 0 : (i < A.P + A.Q2 ? 1 : 2);
  const float gnorm = s_scale[grp];
  float g = g_in * A.grad_scale;
  // [3P optax.clip_by_global_norm] g_norm = sqrt(sum g^2); g <- g if g_norm < max_norm else (g / g_norm) * max_norm
  if (!(gnorm < A.max_norm)) g = (g / gnorm) * A.max_norm;
  const AdamOut o = sac_adam(p_in, m_in, v_in, g, s_corr[0], s_corr[1], A.lr[grp], A.wd[grp]);   // count_in is already this step's count
  A.adam_m[i] = o.m;
  A.adam_v[i] = o.v;
  A.params[i] = o.p;
  if (grp == 1) {
    A.target_q[i - A.P] = tq_in * A.one_minus_tau + o.p * A.tau;           // sac.py:260-261 ((1 - tau) formed in double on the host)
  } else if (grp == 2) {
    A.metrics[3] = expf(o.p);                                      // 'alpha': exp(alpha_params) (sac.py:267)
    if (A.metrics_accum) A.metrics_accum[3] += A.metrics[3];
    // (this is the one thread of the launch that owns log_alpha) a step in which any group was clipped counts as a clip event
    if (!(s_scale[0] < A.max_norm) || !(s_scale[1] < A.max_norm) || !(s_scale[2] < A.max_norm)) A.seq[SAC_CTL_CLIP_EVENTS] += 1u;
  }
}

// ------------------------------------------------------------------------------------------------
// One batch of up to NB slab terms of one column, t0 <= t < min(t0 + NB, n_tiles).  Every load of the batch is issued without a
// branch: a term past the end re-reads the last tile (in bounds) and is never added.  The additions are those of slab_sum
// (g += v[t], t ascending): bit-identical.
template <int NB>
__device__ __forceinline__ void slab_batch_load(float (&v)[NB], const float *col, long long stride, int t0, int n_tiles) {
  if (t0 + NB <= n_tiles) {
#pragma unroll
    for (int k = 0; k < NB; ++k) v[k] = col[(long long)(t0 + k) * stride];
  } else {
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      const int t = (t0 + k < n_tiles) ? t0 + k : n_tiles - 1;
      v[k] = col[(long long)t * stride];
    }
  }
}
template <int NB>
__device__ __forceinline__ float slab_batch_add(float g, const float (&v)[NB], int t0, int n_tiles) {
  if (t0 + NB <= n_tiles) {
#pragma unroll
    for (int k = 0; k < NB; ++k) g += v[k];
  } else {
#pragma unroll
    for (int k = 0; k < NB; ++k)
      if (t0 + k < n_tiles) g += v[k];
  }
  return g;
}
// The four extras sums (slab_ex[t * 4 + c]) of the wave that owns log_alpha: NB tiles are 4 NB contiguous words, ONE load
// instruction of the wave (lane l holds word l of the batch); the sums then read the lanes in t order — per sum the additions of
// slab_sum.  (As four slab_sum<16> calls these were eight dependent batches of scalar loads in the launch's last wave.)
__device__ __forceinline__ float slab_ex_load(const float *slab_ex, int t0, int n_tiles, int lane) {
  const int w = t0 * 4 + lane, w_end = n_tiles * 4 - 1;
  return slab_ex[w < w_end ? w : w_end];
}
__device__ __forceinline__ void slab_ex_add(float (&s)[4], float exv, int t0, int n_tiles) {
  const int xi = __float_as_int(exv);
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    if (t0 + k < n_tiles) {        // (uniform)
#pragma unroll
      for (int c = 0; c < 4; ++c) s[c] += __int_as_float(__builtin_amdgcn_readlane(xi, 4 * k + c));
    }
  }
}

// k_sac_reduce_apply: k_sac_reduce (+ the peer exchange when EXCHANGE) and the optimizer step in ONE launch, without a device-wide
// meeting point: the step is applied UNCLIPPED and the previous (params, m, v, target) go to the undo log; whoever reads the
// parameters next (k_sac_fwd_bwd's prologue, k_sac_finalize) sums the clip-norm partials this kernel leaves and, if a group's
// norm reached max_norm, recomputes that group's step from the undo log (sac_clip_fixup).  step_count was bumped by this step's
// fwd/bwd launch: every block reads the same final count.
template <bool EXCHANGE>
__global__ void __launch_bounds__(256) k_sac_reduce_apply(SacReduceArgs A, SacOptArgs O, P2pDev X) {
  __shared__ float s_corr[2];
  constexpr int NB = 16;
  typedef __attribute__((address_space(1))) float GF;
  typedef __attribute__((address_space(1))) unsigned int GU;
  // The argument block: every field this kernel uses, fetched in ONE burst of scalar loads and pinned in SGPRs here (sac_lean.hip
  // does the same).  Left to itself hipcc fetched each field next to its use, inside the branch that uses it, every piece behind
  // a full wait: seven dependent round trips before the first data load, and lr / wd as per-lane loads from the argument segment
  // behind the barrier.  (A and O carry the same grads, metrics, metrics_accum, ss_part, P, Q2: one copy is read.)
  // (pinned as global-address-space pointers: a generic pointer out of an asm statement would make every access a flat one)
  GF *g_slab_pi = (GF *)A.slab_pi, *g_slab_q = (GF *)A.slab_q, *g_slab_ex = (GF *)A.slab_ex, *g_grads = (GF *)A.grads,
     *g_metrics = (GF *)A.metrics, *g_metrics_accum = (GF *)A.metrics_accum, *g_ss_part = (GF *)A.ss_part, *g_params = (GF *)O.params,
     *g_target_q = (GF *)O.target_q, *g_adam_m = (GF *)O.adam_m, *g_adam_v = (GF *)O.adam_v, *g_undo = (GF *)O.undo,
     *g_undo_count = (GF *)O.undo_count, *g_step_count = (GF *)O.step_count;
  GU *g_seq = (GU *)O.seq, *g_slot_word = (GU *)O.slot_word, *g_epoch = EXCHANGE ? (GU *)X.epoch : nullptr;
  int n_tiles = A.n_tiles, P = A.P, Q2 = A.Q2, B = A.B, n_parts = O.n_parts;
  float lr0 = O.lr[0], lr1 = O.lr[1], lr2 = O.lr[2], wd0 = O.wd[0], wd1 = O.wd[1], wd2 = O.wd[2];
  float max_norm = O.max_norm, grad_scale = O.grad_scale, tau = O.tau, one_minus_tau = O.one_minus_tau;
  asm("" : "+s"(g_slab_pi), "+s"(g_slab_q), "+s"(g_slab_ex), "+s"(n_tiles), "+s"(P), "+s"(Q2), "+s"(B), "+s"(g_grads),
               "+s"(g_metrics), "+s"(g_metrics_accum), "+s"(g_ss_part), "+s"(g_params), "+s"(g_target_q), "+s"(g_adam_m), "+s"(g_adam_v));
  asm("" : "+s"(g_undo), "+s"(g_undo_count), "+s"(g_step_count), "+s"(g_seq), "+s"(g_slot_word), "+s"(g_epoch), "+s"(n_parts),
               "+s"(lr0), "+s"(lr1), "+s"(lr2), "+s"(wd0), "+s"(wd1), "+s"(wd2), "+s"(max_norm), "+s"(grad_scale));
  asm("" : "+s"(tau), "+s"(one_minus_tau));
  const float *slab_pi = (const float *)g_slab_pi, *slab_q = (const float *)g_slab_q, *slab_ex = (const float *)g_slab_ex,
              *step_count = (const float *)g_step_count;
  float *grads = (float *)g_grads, *metrics = (float *)g_metrics, *metrics_accum = (float *)g_metrics_accum, *ss_part = (float *)g_ss_part,
        *params = (float *)g_params, *target_q = (float *)g_target_q, *adam_m = (float *)g_adam_m, *adam_v = (float *)g_adam_v,
        *undo = (float *)g_undo, *undo_count = (float *)g_undo_count;
  unsigned int *seq = (unsigned int *)g_seq, *slot_word = (unsigned int *)g_slot_word, *x_epoch = (unsigned int *)g_epoch;
  const int NP = P + Q2 + 1;
  const int tid = threadIdx.x, lane = tid & 63;
  const int i = blockIdx.x * 256 + tid;
  const bool in = i < NP, last = (i == NP - 1);
  const int grp = (i < P) ? 0 : (i < P + Q2 ? 1 : 2);
  const bool crit = in && grp == 1;
  // the wave that holds the launch's last element (log_alpha): uniform, so what only that element needs costs the others nothing
  const bool last_wave = __builtin_amdgcn_readfirstlane(i >> 6) == ((NP - 1) >> 6);

  // ---- ONE burst: every load this thread will ever need, no wait in between.
  // The uniform words first (scalar loads, a queue of their own): step_count heads the launch's longest chain, count -> powf.
  // (step_count was bumped and slot_word published by this step's fwd/bwd launch: stable during this launch)
  const float count = step_count[0];
  const unsigned int slot = slot_word[0];
  // the last element also keeps the running metric sums and the sequence word: everything it will read-modify-write.  Uniform
  // addresses: scalar loads, issued by every wave rather than behind a branch (without running sums the five words come from
  // params, in bounds, and are dropped)
  const unsigned int seq0 = seq[0];
  const float *ma = metrics_accum ? metrics_accum : params;
  const float ma0 = ma[0], ma1 = ma[1], ma2 = ma[2], ma3 = ma[3], ma4 = ma[4];
  unsigned epoch = 0, want = 0;
  if (EXCHANGE) {
    epoch = x_epoch[0];
    want = x_epoch[1];
  }
  asm volatile("" ::: "memory");          // (keeps the scalar loads here, as the one at the end of the burst does)
  // Lanes without a weight gradient (past the end, log_alpha) read column 0 of the policy slab and element NP - 1 of the state:
  // in bounds, unused, and no branch in the burst.
  const bool wl = in && !last;
  const float *col = !wl ? slab_pi : (grp == 0 ? slab_pi + i : slab_q + (i - P));
  const long long stride = (wl && grp == 1) ? Q2 : P;
  float exv = 0.f;
  if (last_wave) exv = slab_ex_load(slab_ex, 0, n_tiles, lane);        // ahead of the wave's vector path
  float v[NB];
  slab_batch_load<NB>(v, col, stride, 0, n_tiles);
  // the element's own optimizer operands
  const int ic = in ? i : NP - 1, jc = crit ? i - P : 0;
  const float p_in = params[ic], m_in = adam_m[ic], v_in = adam_v[ic], tq_in = target_q[jc];
  // (a compiler-level store barrier: without one behind them in their block, scalar loads are sunk past the powf branches to
  // their first uses)
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  // The Adam bias corrections run in the shadow of that burst, and they wait for step_count alone (scalar loads count apart from
  // the vector ones).  count -> powf stays the longest chain of the launch, every wave meets its end at group_sumsq's barrier:
  // hence step_count at the head of the burst, and the two powf calls (~160 instructions each on a lone lane) on the first
  // lanes of two waves, side by side on two SIMDs, instead of one after the other on thread 0.
  if (tid == 0) s_corr[0] = 1.f - powf(0.9f, count);
  if (tid == 64) s_corr[1] = 1.f - powf(0.999f, count);
  __builtin_amdgcn_sched_barrier(0);

  const float acc0 = ma0, acc1 = ma1, acc2 = ma2, acc3 = metrics_accum ? ma3 : 0.f, acc4 = ma4;
  float g = slab_batch_add<NB>(0.f, v, 0, n_tiles);
  float ex[4] = {0.f, 0.f, 0.f, 0.f};
  if (last_wave) slab_ex_add(ex, exv, 0, n_tiles);
  for (int t0 = NB; t0 < n_tiles; t0 += NB) {          // more than NB tiles (batch_size > 256): further bursts
    if (last_wave) exv = slab_ex_load(slab_ex, t0, n_tiles, lane);
    slab_batch_load<NB>(v, col, stride, t0, n_tiles);
    g = slab_batch_add<NB>(g, v, t0, n_tiles);
    if (last_wave) slab_ex_add(ex, exv, t0, n_tiles);
  }
  if (!wl) g = 0.f;
  if (last) {
    const float ce = ex[0] + ex[3], ac = ex[1], al = ex[2];
    const float invB = 1.0f / (float)B;
    g = al * invB;
    const float m0 = 0.5f * ce * (0.5f * invB), m1 = ac * invB, m2 = al * invB;
    metrics[0] = m0;
    metrics[1] = m1;
    metrics[2] = m2;
    if (metrics_accum) {
      metrics_accum[0] = acc0 + m0;
      metrics_accum[1] = acc1 + m1;
      metrics_accum[2] = acc2 + m2;
      metrics_accum[4] = acc4 + 1.0f;
    }
    undo_count[0] = count;
    undo_count[1] = acc3;          // metrics_accum[3] before this step adds its 'alpha' (0 without running sums)
    seq[1] = seq0;                 // everything before this step was resolved by this step's fwd/bwd launch ...
    seq[0] = seq0 + 1u;            // ... and this one speculative step is pending now
  }
  if (EXCHANGE) {
    p2p_push(X, epoch, i, NP, g);
    const bool ok = p2p_wait(X, want);
    g = in ? (ok ? p2p_sum(X, epoch, i) : NAN) : 0.f;
  }
  if (in) grads[i] = g;
  group_sumsq(g, i, P, Q2, NP, ss_part, reinterpret_cast<float *>(seq) + 2 + 3 * (slot & 1u),
              (max_norm / grad_scale) * (max_norm / grad_scale) * 0.9998f / (float)n_parts);   // ends in a __syncthreads
  if (!in) return;
  float *u_p = undo, *u_m = undo + NP, *u_v = undo + 2 * NP, *u_tq = undo + 3 * NP;
  u_p[i] = p_in;
  u_m[i] = m_in;
  u_v[i] = v_in;
  // lr / wd arrive as scalars and are selected by group
  const float lr = grp == 0 ? lr0 : (grp == 1 ? lr1 : lr2), wd = grp == 0 ? wd0 : (grp == 1 ? wd1 : wd2);
  const AdamOut o = sac_adam(p_in, m_in, v_in, g * grad_scale, s_corr[0], s_corr[1], lr, wd);
  params[i] = o.p;
  adam_m[i] = o.m;
  adam_v[i] = o.v;
  if (grp == 1) {
    u_tq[i - P] = tq_in;
    target_q[i - P] = tq_in * one_minus_tau + o.p * tau;       // sac.py:260-261
  } else if (grp == 2) {
    undo_count[2] = s_corr[0];
    undo_count[3] = s_corr[1];
    const float al = expf(o.p);                                        // 'alpha' (sac.py:267); repaired by the fix-up if the group clips
    metrics[3] = al;
    if (metrics_accum) metrics_accum[3] = acc3 + al;
  }
}

// Resolves the clip check of the last speculative step when no further fwd/bwd launch will (end of training_step's sgd scan,
// a single sgd_step of the eager API): one workgroup.  Idempotent.
__global__ void __launch_bounds__(1024) k_sac_finalize(SacOptArgs O, unsigned long long *rng_dev, unsigned long long rng_inc) {
  __shared__ float s_gn[4];
  const int tid = threadIdx.x;
  // (mbpo_sac_finalize_advance) the end of a training step: the device RNG's step counter moves on in this launch as well
  if (rng_dev && tid == 0) rng_dev[1] += rng_inc;
  if (O.seq[0] == O.seq[1]) return;
  sac_group_norms(O, s_gn, tid);
  __syncthreads();
  const bool clip = !(s_gn[0] < O.max_norm) || !(s_gn[1] < O.max_norm) || !(s_gn[2] < O.max_norm);
  if (clip) {
    sac_clip_fixup(O, s_gn, tid, 1024);
    if (tid == 0) O.seq[SAC_CTL_CLIP_EVENTS] += 1u;
    __threadfence();
  }
  __syncthreads();
  if (tid == 0) O.seq[1] = O.seq[0];
}

// ------------------------------------------------------------------------------------------------ launches
constexpr int SP64 = 4;   // waves per chain at hidden width 64

static int sac_fwd_bwd_launch(const SacVariant &v, int grid_, size_t lds, hipStream_t st, const SacArgs &A) {
  const dim3 grid(grid_);
  const bool wide_any = v.wide_any, split = v.split;
  if (v.H == 64) {
    if (wide_any) return mbpo_launch<k_sac_fwd_bwd<64, SP64, true>>(grid, 256 * SP64, lds, st, "sac_grads", A);
    else if (split && v.thin) return mbpo_launch<k_sac_fwd_bwd<64, SP64, false, 2, true>>(grid, 128 * SP64, lds, st, "sac_grads", A);
    else if (split) return mbpo_launch<k_sac_fwd_bwd<64, SP64, false, 2>>(grid, 128 * SP64, lds, st, "sac_grads", A);
    else return mbpo_launch<k_sac_fwd_bwd<64, SP64, false>>(grid, 256 * SP64, lds, st, "sac_grads", A);
  } else if (split && !wide_any) {
    return mbpo_launch<k_sac_fwd_bwd<128, 4, false, 2>>(grid, 512, lds, st, "sac_grads", A);
  } else {
    return mbpo_launch<k_sac_fwd_bwd<128, 2, false>>(grid, 512, lds, st, "sac_grads", A);
  }
}

static void sac_reduce_launch(SacReduceKind kind, int n_red, hipStream_t st, const SacReduceArgs &R, const SacOptArgs &O, const P2pDev &X) {
  const dim3 grid(n_red), block(256);
  switch (kind) {
    case SacReduceKind::NONE: break;
    case SacReduceKind::PLAIN: hipLaunchKernelGGL(k_sac_reduce, grid, block, 0, st, R); break;
    case SacReduceKind::PUSH: hipLaunchKernelGGL(k_sac_reduce_push, grid, block, 0, st, R, X); break;
    case SacReduceKind::EXCHANGE: hipLaunchKernelGGL(k_sac_reduce_exchange, grid, block, 0, st, R, X); break;
    // (<true> is named before <false>, and the ladder above before both: templates are emitted in the order the host first names
    // them, and the unit's device code object is kept byte for byte)
    case SacReduceKind::APPLY_EXCHANGE: hipLaunchKernelGGL(k_sac_reduce_apply<true>, grid, block, 0, st, R, O, X); break;
    case SacReduceKind::APPLY: hipLaunchKernelGGL(k_sac_reduce_apply<false>, grid, block, 0, st, R, O, X); break;
  }
}

static void sac_sumsq_launch(int n_red, hipStream_t st, const float *grads, int P, int Q2, float *ss_part) {
  hipLaunchKernelGGL(k_sac_sumsq, dim3(n_red), dim3(256), 0, st, grads, P, Q2, ss_part);
}

static void sac_gather_launch(int n_red, hipStream_t st, const P2pDev &X, float *grads, int P, int Q2, float *ss_part) {
  hipLaunchKernelGGL(k_sac_gather, dim3(n_red), dim3(256), 0, st, X, grads, P, Q2, ss_part);
}

static void sac_apply_launch(int n_red, hipStream_t st, const SacOptArgs &O) {
  hipLaunchKernelGGL(k_sac_apply, dim3(n_red), dim3(256), 0, st, O);
}

static void sac_finalize_launch(hipStream_t st, const SacOptArgs &O, unsigned long long *rng_dev, unsigned long long rng_inc) {
  hipLaunchKernelGGL(k_sac_finalize, dim3(1), dim3(1024), 0, st, O, rng_dev, rng_inc);
}

// ------------------------------------------------------------------------------------------------ host side
static unsigned long long *g_sac_stamps = nullptr;
// Measurement / test hook (not part of include/mbpo_hip.h): 0 = always the generic k_sac_fwd_bwd, 1 = the specialised k_sac_lean
// where it applies, -1 = the MBPO_SAC_LEAN environment default (on).  tests/test_gpu_sac_lean.py flips it inside one process.
extern "C" int mbpo_debug_set_sac_lean(int mode) { return mbpo_knob_set_override(KNOB_SAC_LEAN, mode); }
// Measurement hook (not part of include/mbpo_hip.h): device buffer of >= 32 uint64 that k_sac_fwd_bwd fills with
// s_memtime stamps at its phase boundaries (tile 0, both roles); NULL switches the stamps off.
extern "C" int mbpo_debug_set_stamps(void *buf) {
  g_sac_stamps = (unsigned long long *)buf;
  return MBPO_OK;
}

struct SacPlan {
  MlpDev pi, q, qt;
  NetShape sh_pi, sh_q;
  int P, Q, NP, n_tiles, H, LH, n_red;
  size_t lds;
  int ld_x, ld_xu, ld_h, ld_y;
  // workspace offsets (floats)
  long long off_slab_pi, off_slab_q, off_slab_ex, off_ss, off_seq, off_undo, off_layered, total;
  // hidden layers outside the fused kernel's range (one width in {64,128} that fits a tile's LDS): the forward/backward half runs
  // layer by layer (sac_layered.hip) and leaves ONE tile of slabs; everything behind it is shared
  bool layered;
};

static int sac_plan(const mbpo_sac_desc *d, SacPlan *pl, bool need_ptrs) {
  MBPO_REQUIRE(d, MBPO_ERR_ARG, "sac: null descriptor");
  MBPO_REQUIRE(d->x_dim > 0 && d->u_dim > 0 && d->batch_size > 0, MBPO_ERR_ARG, "sac: x_dim/u_dim/batch_size must be positive");
  MBPO_REQUIRE(d->row_len == 2 * d->x_dim + d->u_dim + 3, MBPO_ERR_ARG, "sac: row_len %d != 2x+u+3", d->row_len);
  MBPO_REQUIRE(d->policy_layers >= 2 && d->policy_layers <= MBPO_MAX_LAYERS && d->q_layers >= 2 && d->q_layers <= MBPO_MAX_LAYERS,
               MBPO_ERR_ARG, "sac: networks need at least one hidden layer and at most %d Dense layers", MBPO_MAX_LAYERS);
  MBPO_REQUIRE(d->policy_dims[0] == d->x_dim && d->policy_dims[d->policy_layers] == 2 * d->u_dim, MBPO_ERR_ARG,
               "sac: policy must map [x_dim] -> [2*u_dim]");
  MBPO_REQUIRE(d->q_dims[0] == d->x_dim + d->u_dim && d->q_dims[d->q_layers] == 1, MBPO_ERR_ARG,
               "sac: critic must map [x_dim+u_dim] -> [1]");
  const int Hp = same_hidden(d->policy_dims, d->policy_layers), Hq = same_hidden(d->q_dims, d->q_layers);
  pl->layered = mbpo_knob(KNOB_SAC_LAYERED) != 0 || !(Hp == Hq && (Hp == 64 || Hp == 128));
  int rc = mbpo_make_mlp_dev_from(d->policy_dims, d->policy_layers, d->policy_activation, d->params, 1, "sac.policy", &pl->pi);
  if (rc != MBPO_OK) return rc;
  pl->P = pl->pi.n_params;
  rc = mbpo_make_mlp_dev_from(d->q_dims, d->q_layers, d->q_activation, d->params, 1, "sac.q", &pl->q);
  if (rc != MBPO_OK) return rc;
  pl->Q = pl->q.n_params;
  pl->q.n_nets = 2;
  pl->q.net_stride = pl->Q;
  pl->q.params = d->params ? d->params + pl->P : nullptr;
  pl->qt = pl->q;
  pl->qt.params = d->target_q;
  pl->NP = pl->P + 2 * pl->Q + 1;
  pl->sh_pi = net_shape(pl->pi);
  pl->sh_q = net_shape(pl->q);
  pl->H = Hp;
  const int lhp = d->policy_layers - 1, lhq = d->q_layers - 1;
  pl->LH = lhp > lhq ? lhp : lhq;
  pl->n_tiles = (d->batch_size + 15) / 16;
  pl->n_red = (pl->NP + 255) / 256;
  pl->off_layered = 0;
  pl->ld_x = up4(d->x_dim) + 4;
  pl->ld_xu = up4(d->x_dim + d->u_dim) + 4;
  pl->ld_h = Hp + 4;
  pl->ld_y = up4(2 * d->u_dim) + 4;
  pl->lds = (size_t)sac_lds(d->row_len, pl->ld_x, pl->ld_xu, pl->ld_h, pl->ld_y, pl->LH, d->u_dim).end * sizeof(float);
  if (!pl->layered && pl->lds > 160 * 1024) pl->layered = true;      // more stored activations than a tile's LDS holds
  if (pl->layered) pl->n_tiles = 1;
  pl->off_slab_pi = 0;
  pl->off_slab_q = pl->off_slab_pi + (long long)pl->n_tiles * pl->P;
  pl->off_slab_ex = pl->off_slab_q + (long long)pl->n_tiles * 2 * pl->Q;
  pl->off_ss = pl->off_slab_ex + (long long)pl->n_tiles * 4;
  pl->off_seq = (pl->off_ss + (long long)pl->n_red * 3 + 3) & ~3LL;   // 8 words {seq issued, seq resolved, 2 x 3 quick sums} (16-byte aligned),
                                                                       // then slot word + undo count, accum, 2 bias corrections (zero at start)
  pl->off_undo = pl->off_seq + 16;                                     // undo log of the speculative optimizer step
  pl->total = pl->off_undo + 3LL * pl->NP + 2LL * pl->Q;
  if (pl->layered) {
    pl->off_layered = (pl->total + 3) & ~3LL;
    pl->total = pl->off_layered + sac_layered_floats(d, pl->pi, pl->q);
  }
  if (need_ptrs) {
    MBPO_REQUIRE(d->params && d->target_q && d->adam_m && d->adam_v && d->step_count && d->grads && d->workspace && d->metrics,
                 MBPO_ERR_ARG, "sac: null state pointer");
  }
  return MBPO_OK;
}

extern "C" int64_t mbpo_sac_workspace_floats(const mbpo_sac_desc *d) {
  SacPlan pl;
  int rc = sac_plan(d, &pl, false);
  if (rc != MBPO_OK) return rc;
  return pl.total;
}

extern "C" int64_t mbpo_sac_control_offset(const mbpo_sac_desc *d) {
  SacPlan pl;
  int rc = sac_plan(d, &pl, false);
  if (rc != MBPO_OK) return rc;
  return pl.off_seq;
}

// the chain descriptors of every (table role, phase, chain); LDS operands as SacLds offsets
static void sac_chain_table(const SacPlan &pl, int D, int U, SacArgs *A, bool split, bool jvp) {
  const int ld_x = pl.ld_x, ld_xu = pl.ld_xu, ld_y = pl.ld_y, LH = pl.LH;
  const int T = 16 * pl.ld_h;
  const SacLds L = sac_lds(D, ld_x, ld_xu, pl.ld_h, ld_y, LH, U);
  const int o_sn = (int)L.sn, o_sn2 = (int)L.sn2, o_qin = (int)L.qin, o_qin2 = (int)L.qin2;
  const int o_pp = (int)L.pp, o_st0 = (int)L.store, o_y = (int)L.y, o_dy = (int)L.dy, o_dx = (int)L.dx;
  const int o_st1 = o_st0 + LH * T, o_st2 = o_st0 + 2 * LH * T, o_st3 = o_st0 + 3 * LH * T;
  const int P = pl.P, Q = pl.Q;   // params = [policy | critic0 | critic1 | log_alpha]; target_q = [critic0 | critic1]
  for (int role = 0; role < 3; ++role)
    for (int ph = 0; ph < 5; ++ph)
      for (int c = 0; c < 4; ++c) {
        SacChainDesc d;
        memset(&d, 0, sizeof(d));
        d.mode = CH_IDLE;
        d.x = d.pp0 = d.pp1 = d.zb = d.hb = d.y = d.dx = d.tp0 = d.tp1 = -1;
        d.ldx = ld_x;
        const int net = c & 1;
        if (split && role != 1) {              // critic role of ONE critic kq: never more than two chains
          const int kq = role >> 1;
          if (ph == 0 && c < 2) {              // pi(s') || Qk(s,a)
            d.mode = CH_FWD;
            if (c == 0) {
              d.netid = 0; d.param_off = 0; d.x = o_sn2; d.ldx = ld_x; d.pp0 = o_pp; d.pp1 = o_pp + T; d.y = o_y;
            } else {
              d.netid = 1; d.param_off = P + kq * Q; d.x = o_qin; d.ldx = ld_xu;
              d.zb = kq == 0 ? o_st0 : o_st2; d.hb = kq == 0 ? o_st1 : o_st3; d.y = o_y + (kq + 1) * 16 * ld_y;
            }
          } else if (ph == 1 && c < 2) {       // BOTH target critics on (s', a')
            d.mode = CH_FWD;
            d.netid = 1; d.base_sel = 1; d.param_off = c * Q; d.x = o_qin2; d.ldx = ld_xu;
            d.pp0 = o_pp + 2 * c * T; d.pp1 = d.pp0 + T; d.y = o_y + (c + 1) * 16 * ld_y;
          } else if (ph == 2 && c < 2) {       // critic kq backward: dgrad beside wgrad
            d.mode = c == 0 ? CH_DGRAD : CH_WGRAD;
            d.netid = 1; d.param_off = P + kq * Q; d.x = o_qin; d.ldx = ld_xu;
            d.pp0 = o_pp + 2 * kq * T; d.pp1 = d.pp0 + T; d.zb = kq ? o_st2 : o_st0; d.hb = kq ? o_st3 : o_st1;
            d.y = o_dy + kq * 16 * ld_y;
            d.slab_sel = 2; d.slab_off = kq * Q;
          }
        } else if (role == 2) {
          // (table role 2 is not used without `split`)
        } else if (role == 0) {                // critic role
          if (ph == 0 && c < 3) {              // pi(s') || Q1(s,a) || Q2(s,a)
            d.mode = CH_FWD;
            if (c == 0) {
              d.netid = 0; d.param_off = 0; d.x = o_sn2; d.ldx = ld_x; d.pp0 = o_pp; d.pp1 = o_pp + T; d.y = o_y;
            } else {
              d.netid = 1; d.param_off = P + (c - 1) * Q; d.x = o_qin; d.ldx = ld_xu;
              d.zb = c == 1 ? o_st0 : o_st2; d.hb = c == 1 ? o_st1 : o_st3; d.y = o_y + c * 16 * ld_y;
            }
          } else if (ph == 1 && c < 2) {       // target critics on (s', a')
            d.mode = CH_FWD;
            d.netid = 1; d.base_sel = 1; d.param_off = c * Q; d.x = o_qin2; d.ldx = ld_xu;
            d.pp0 = o_pp + 2 * c * T; d.pp1 = d.pp0 + T; d.y = o_y + (c + 1) * 16 * ld_y;
          } else if (ph == 2) {                // critics backward: dgrad (c < 2) beside wgrad
            d.mode = c < 2 ? CH_DGRAD : CH_WGRAD;
            d.netid = 1; d.param_off = P + net * Q; d.x = o_qin; d.ldx = ld_xu;
            d.pp0 = o_pp + 2 * net * T; d.pp1 = d.pp0 + T; d.zb = net ? o_st2 : o_st0; d.hb = net ? o_st3 : o_st1;
            d.y = o_dy + net * 16 * ld_y;
            d.slab_sel = 2; d.slab_off = net * Q;
          }
        } else {                               // actor + alpha role
          if (ph == 0 && c == 0) {
            d.mode = CH_FWD;
            d.netid = 0; d.param_off = 0; d.x = o_sn; d.ldx = ld_x; d.zb = o_st0; d.hb = o_st1; d.y = o_y;
          } else if (ph == 1 && c < 2) {
            d.mode = CH_FWD;
            d.netid = 1; d.param_off = P + c * Q; d.x = o_qin; d.ldx = ld_xu;
            d.pp0 = o_pp + 2 * c * T; d.pp1 = d.pp0 + T; d.zb = c == 0 ? o_st2 : o_st3; d.y = o_y + (c + 1) * 16 * ld_y;
            if (jvp) {     // no z store (no backward through the critics): its tiles carry the tangent, whose output goes to s_dx[c]
              d.zb = -1;
              d.tp0 = c == 0 ? o_st2 : o_st3; d.tp1 = d.tp0 + T; d.dx = o_dx + c * 16 * ld_xu;
            }
          } else if (jvp && ph == 2 && c < 2) {      // the policy's backward pass follows at once
            d.mode = c == 0 ? CH_DGRAD : CH_WGRAD;
            d.netid = 0; d.param_off = 0; d.x = o_sn; d.ldx = ld_x; d.pp0 = o_pp; d.pp1 = o_pp + T; d.zb = o_st0; d.hb = o_st1;
            d.y = o_dy; d.slab_sel = 1; d.slab_off = 0;
          } else if (jvp) {
            // (idle)
          } else if (ph == 2 && c < 2) {
            d.mode = CH_DGRAD;
            d.netid = 1; d.param_off = P + net * Q; d.pp0 = o_pp + 2 * net * T; d.pp1 = d.pp0 + T; d.zb = net ? o_st3 : o_st2;
            d.y = o_dy + net * 16 * ld_y; d.dx = o_dx + net * 16 * ld_xu;
          } else if (ph == 3 && c < 2) {
            d.mode = c == 0 ? CH_DGRAD : CH_WGRAD;
            d.netid = 0; d.param_off = 0; d.x = o_sn; d.ldx = ld_x; d.pp0 = o_pp; d.pp1 = o_pp + T; d.zb = o_st0; d.hb = o_st1;
            d.y = o_dy; d.slab_sel = 1; d.slab_off = 0;
          }
        }
        A->tab[role][ph][c] = d;
      }
}

static void sac_fill_opt(const mbpo_sac_desc *d, const SacPlan &pl, SacOptArgs *A) {
  A->params = d->params; A->target_q = d->target_q; A->adam_m = d->adam_m; A->adam_v = d->adam_v; A->grads = d->grads;
  A->metrics = d->metrics; A->metrics_accum = d->metrics_accum; A->step_count = d->step_count; A->ss_part = d->workspace + pl.off_ss;
  A->undo = d->workspace + pl.off_undo;
  A->seq = reinterpret_cast<unsigned int *>(d->workspace + pl.off_seq);
  A->slot_word = reinterpret_cast<unsigned int *>(d->workspace + pl.off_seq + 8);
  A->undo_count = d->workspace + pl.off_seq + 9;
  A->n_parts = pl.n_red; A->P = pl.P; A->Q2 = 2 * pl.Q;
  A->lr[0] = d->lr_policy; A->lr[1] = d->lr_q; A->lr[2] = d->lr_alpha;
  A->wd[0] = d->wd_policy; A->wd[1] = d->wd_q; A->wd[2] = d->wd_alpha;
  A->max_norm = d->max_grad_norm; A->tau = d->tau; A->one_minus_tau = (float)(1.0 - (double)d->tau); A->grad_scale = d->grad_scale;
}
static SacOptArgs sac_opt(const mbpo_sac_desc *d, const SacPlan &pl) {
  SacOptArgs O;
  sac_fill_opt(d, pl, &O);
  return O;
}

// Which forward/backward kernel one update launches.  The knobs in this order: split, jvp (asked only where it can apply), thin, lean.
static SacVariant sac_variant(const mbpo_sac_desc *d, const SacPlan &pl) {
  const NetShape &sh_pi = pl.sh_pi, &sh_q = pl.sh_q;
  SacVariant v;
  v.layered = pl.layered;
  v.H = pl.H;
  // three workgroups per tile (one critic each): at hidden width 128 a phase is MFMA-bound on its CU, at 64 the two critic
  // workgroups finish before the actor role does and 8-wave workgroups have cheaper barriers (26.9 -> 24.0 us with the forward-mode
  // actor role).  The WIDE kernels keep two workgroups per tile.  MBPO_SAC_SPLIT=0/1 overrides (measurement).
  const long long split_env = mbpo_knob(KNOB_SAC_SPLIT);
  v.wide_any = net_is_wide(sh_pi) || net_is_wide(sh_q);
  v.split = split_env >= 0 ? split_env != 0 : !v.wide_any;
  v.wg_per_tile = v.split ? 3 : 2;
  // forward-mode dQ/da in the actor role: one action dimension (one tangent), register-image kernels with one-tile network ends
  const bool reg_path = (pl.H == 64 || v.split) && !v.wide_any && pl.LH >= 2;
  v.jvp = d->u_dim == 1 && reg_path && mbpo_knob(KNOB_SAC_JVP) != 0;
  // thin layers: the three-workgroup launch at H = 64 with forward-mode actor (no input-gradient chains), small input / output
  // layers and at least one H x H layer in each network
  v.thin = mbpo_knob(KNOB_SAC_THIN) != 0 && v.split && v.jvp && pl.H == 64 && sh_pi.K_in <= THIN_KMAX && sh_q.K_in <= THIN_KMAX &&
           sh_pi.N_out <= THIN_NMAX && sh_q.N_out <= THIN_NMAX && sh_pi.L >= 3 && sh_q.L >= 3;
  // MBPO_SAC_LEAN=0 keeps the generic kernel on the benchmark networks too (A/B runs, the bit-identity test)
  v.lean = mbpo_knob(KNOB_SAC_LEAN) != 0 && !pl.layered && v.thin &&
           sac_lean_supports(d->x_dim, d->u_dim, d->policy_dims, d->policy_layers, d->policy_activation, d->q_dims, d->q_layers,
                             d->q_activation);
  return v;
}

// p2p_epoch: the peer exchange's epoch words where this update's reduction uses the exchange regions, else null
static void sac_fill_args(const mbpo_sac_desc *d, const SacPlan &pl, const SacVariant &v, const SacOptArgs &O, unsigned int *p2p_epoch,
                          SacArgs *A) {
  A->pi = pl.pi; A->q = pl.q; A->qt = pl.qt;
  A->sh_pi = pl.sh_pi; A->sh_q = pl.sh_q;
  A->split = v.split ? 1 : 0; A->jvp = v.jvp ? 1 : 0; A->thin = v.thin ? 1 : 0;
  sac_chain_table(pl, d->row_len, d->u_dim, A, v.split, v.jvp);
  A->X = d->x_dim; A->U = d->u_dim; A->B = d->batch_size; A->D = d->row_len;
  A->batch = d->batch; A->norm_mean = d->norm_mean; A->norm_std = d->norm_std;
  A->log_alpha = d->params + pl.NP - 1;
  A->noise_alpha = d->noise_alpha; A->noise_critic = d->noise_critic; A->noise_actor = d->noise_actor;
  A->seed = d->seed; A->offset = d->offset; A->rng_dev = (const unsigned long long *)d->rng_dev;
  A->opt = O;
  A->step_count_rw = d->step_count;
  A->stamps = g_sac_stamps;
  A->p2p_epoch = p2p_epoch;
  A->p2p_blocks = (unsigned)pl.n_red;
  A->discounting = d->discounting; A->reward_scaling = d->reward_scaling; A->target_entropy = d->target_entropy;
  A->neq = d->non_equidistant_time; A->neq_cd = d->continuous_discounting; A->neq_tl = d->min_time_between_switches;
  A->neq_tu = d->max_time_between_switches; A->neq_dt = d->env_dt;
  A->slab_pi = d->workspace + pl.off_slab_pi; A->slab_q = d->workspace + pl.off_slab_q; A->slab_ex = d->workspace + pl.off_slab_ex;
  A->ld_x = pl.ld_x; A->ld_xu = pl.ld_xu; A->ld_h = pl.ld_h; A->ld_y = pl.ld_y; A->LH = pl.LH;
}

// the benchmark networks: every shape a compile-time constant (sac_lean.hip), same slabs bit for bit
static void sac_fill_lean(const mbpo_sac_desc *d, const SacPlan &pl, const SacOptArgs &O, unsigned int *p2p_epoch, SacLeanArgs *L) {
  L->params = d->params; L->target_q = d->target_q; L->batch = d->batch; L->norm_mean = d->norm_mean; L->norm_std = d->norm_std;
  L->noise_alpha = d->noise_alpha; L->noise_critic = d->noise_critic; L->noise_actor = d->noise_actor;
  L->rng_dev = (const unsigned long long *)d->rng_dev; L->seed = d->seed; L->offset = d->offset;
  L->slab_pi = d->workspace + pl.off_slab_pi; L->slab_q = d->workspace + pl.off_slab_q; L->slab_ex = d->workspace + pl.off_slab_ex;
  L->step_count_rw = d->step_count; L->p2p_epoch = p2p_epoch; L->p2p_blocks = (unsigned)pl.n_red; L->B = d->batch_size;
  L->discounting = d->discounting; L->reward_scaling = d->reward_scaling; L->target_entropy = d->target_entropy;
  L->neq = d->non_equidistant_time; L->neq_cd = d->continuous_discounting; L->neq_tl = d->min_time_between_switches;
  L->neq_tu = d->max_time_between_switches; L->neq_dt = d->env_dt;
  L->stamps = g_sac_stamps;
  L->pad0 = 0;
  L->opt = O;
}

static void sac_fill_reduce(const mbpo_sac_desc *d, const SacPlan &pl, const SacOptArgs &O, SacReduceArgs *R) {
  R->slab_pi = d->workspace + pl.off_slab_pi; R->slab_q = d->workspace + pl.off_slab_q; R->slab_ex = d->workspace + pl.off_slab_ex;
  R->n_tiles = pl.n_tiles; R->P = pl.P; R->Q2 = 2 * pl.Q; R->B = d->batch_size;
  R->grads = d->grads; R->metrics = d->metrics; R->metrics_accum = d->metrics_accum; R->ss_part = d->workspace + pl.off_ss; R->step_count = d->step_count;
  R->seq = O.seq;
}

// One update: the forward/backward half (fwd) in the variant's kernel, then the reduction `kind` (NONE: nothing).  xd: the peer exchange
// of the p2p kinds.
static int sac_update(const mbpo_sac_desc *d, bool fwd, SacReduceKind kind, void *stream, const mbpo_p2p_desc *xd = nullptr) {
  SacPlan pl;
  int rc = sac_plan(d, &pl, true);
  if (rc != MBPO_OK) return rc;
  if (sac_reduce_waits(kind)) {
    // every workgroup of the reduction waits inside the kernel for the peers' same kernel: they must all be resident at once
    const bool step = kind == SacReduceKind::APPLY_EXCHANGE;
    MBPO_REQUIRE(pl.n_red <= 1024, MBPO_ERR_UNSUPPORTED, "%s: %d workgroups cannot be assumed co-resident; use "
                 "mbpo_sac_grads_p2p + mbpo_sac_gather_p2p%s", step ? "sac_step_p2p" : "sac_grads_exchange_p2p", pl.n_red,
                 step ? " + mbpo_sac_apply" : "");
  }
  MBPO_REQUIRE(d->batch, MBPO_ERR_ARG, "sac_grads: null batch");
  MBPO_REQUIRE((d->norm_mean == nullptr) == (d->norm_std == nullptr), MBPO_ERR_ARG, "sac_grads: norm_mean/norm_std mismatch");
  P2pDev X;
  memset(&X, 0, sizeof(X));
  if (sac_reduce_p2p(kind)) {
    rc = mbpo_p2p_make_dev(xd, &X);
    if (rc != MBPO_OK) return rc;
    MBPO_REQUIRE(xd->n_max >= pl.NP, MBPO_ERR_ARG, "sac_grads_p2p: exchange regions hold %lld floats, the gradient has %d",
                 (long long)xd->n_max, pl.NP);
  }
  MBPO_REQUIRE(!d->non_equidistant_time || d->env_dt > 0.f, MBPO_ERR_ARG, "sac: non_equidistant_time needs env_dt > 0");
  const SacVariant v = sac_variant(d, pl);
  const SacOptArgs O = sac_opt(d, pl);
  unsigned int *p2p_epoch = sac_reduce_p2p(kind) ? X.epoch : nullptr;
  hipStream_t st = (hipStream_t)stream;
  if (fwd) {
    if (v.layered) {
      const SacLayeredBegin bg = {d->step_count, O.seq, O.slot_word, p2p_epoch, (unsigned)pl.n_red};
      rc = sac_layered_fwd_bwd(d, pl.pi, pl.q, pl.qt, d->workspace + pl.off_layered, d->workspace + pl.off_slab_pi,
                               d->workspace + pl.off_slab_q, d->workspace + pl.off_slab_ex, bg, st);
    } else if (v.lean) {
      SacLeanArgs L;
      sac_fill_lean(d, pl, O, p2p_epoch, &L);
      rc = sac_lean_launch(L, d->x_dim, pl.n_tiles, stream);
    } else {
      SacArgs A;
      sac_fill_args(d, pl, v, O, p2p_epoch, &A);
      rc = sac_fwd_bwd_launch(v, v.wg_per_tile * pl.n_tiles, pl.lds, st, A);
    }
    if (rc != MBPO_OK) return rc;
  }
  if (kind == SacReduceKind::NONE) {
    MBPO_CHECK_LAUNCH("sac_grads");
    return MBPO_OK;
  }
  SacReduceArgs R;
  sac_fill_reduce(d, pl, O, &R);
  if (v.layered && (kind == SacReduceKind::APPLY || kind == SacReduceKind::APPLY_EXCHANGE)) {
    // no speculative step on the layered path (two launches out of ~50 is nothing to win): the reduction, then the clipped
    // optimizer step — what mbpo_sac_step is defined to equal bit for bit
    sac_reduce_launch(kind == SacReduceKind::APPLY ? SacReduceKind::PLAIN : SacReduceKind::EXCHANGE, pl.n_red, st, R, O, X);
    sac_apply_launch(pl.n_red, st, O);
  } else {
    sac_reduce_launch(kind, pl.n_red, st, R, O, X);
  }
  MBPO_CHECK_LAUNCH("sac_grads");
  return MBPO_OK;
}

// The entry points that only plan and launch one optimizer-side kernel (on sac_opt(d, pl) where the kernel takes SacOptArgs).
template <class Launch>
static int sac_opt_entry(const mbpo_sac_desc *d, const char *what, Launch &&launch) {
  SacPlan pl;
  int rc = sac_plan(d, &pl, true);
  if (rc != MBPO_OK) return rc;
  rc = launch(pl);
  if (rc != MBPO_OK) return rc;
  MBPO_CHECK_LAUNCH(what);
  return MBPO_OK;
}

extern "C" int mbpo_sac_grads(const mbpo_sac_desc *d, void *stream) { return sac_update(d, true, SacReduceKind::PLAIN, stream); }

extern "C" int mbpo_sac_grads_phase(const mbpo_sac_desc *d, int32_t phase_mask, void *stream) {
  MBPO_REQUIRE(phase_mask >= 1 && phase_mask <= 3, MBPO_ERR_ARG, "sac_grads_phase: phase_mask must be 1, 2 or 3");
  // bit0 = the forward/backward launch, bit1 = the slab reduction
  return sac_update(d, (phase_mask & 1) != 0, (phase_mask & 2) ? SacReduceKind::PLAIN : SacReduceKind::NONE, stream);
}

extern "C" int mbpo_sac_grads_p2p(const mbpo_sac_desc *d, const mbpo_p2p_desc *x, void *stream) {
  MBPO_REQUIRE(x, MBPO_ERR_ARG, "sac_grads_p2p: null exchange descriptor");
  return sac_update(d, true, SacReduceKind::PUSH, stream, x);
}

extern "C" int mbpo_sac_grads_exchange_p2p(const mbpo_sac_desc *d, const mbpo_p2p_desc *x, void *stream) {
  MBPO_REQUIRE(x, MBPO_ERR_ARG, "sac_grads_exchange_p2p: null exchange descriptor");
  return sac_update(d, true, SacReduceKind::EXCHANGE, stream, x);
}

// One sgd_step in TWO launches: k_sac_fwd_bwd, then k_sac_reduce_apply (slab reduction + [peer exchange +] unclipped optimizer
// step + undo log).  The clip check is resolved by the next mbpo_sac_step / mbpo_sac_grads launch or by mbpo_sac_finalize.
extern "C" int mbpo_sac_step(const mbpo_sac_desc *d, void *stream) { return sac_update(d, true, SacReduceKind::APPLY, stream); }

extern "C" int mbpo_sac_step_p2p(const mbpo_sac_desc *d, const mbpo_p2p_desc *x, void *stream) {
  MBPO_REQUIRE(x, MBPO_ERR_ARG, "sac_step_p2p: null exchange descriptor");
  return sac_update(d, true, SacReduceKind::APPLY_EXCHANGE, stream, x);
}

extern "C" int mbpo_sac_gather_p2p(const mbpo_sac_desc *d, const mbpo_p2p_desc *x, void *stream) {
  return sac_opt_entry(d, "sac_gather_p2p", [&](const SacPlan &pl) -> int {
    P2pDev X;
    const int rc = mbpo_p2p_make_dev(x, &X);
    if (rc != MBPO_OK) return rc;
    MBPO_REQUIRE(x->n_max >= pl.NP, MBPO_ERR_ARG, "sac_gather_p2p: exchange regions too small");
    sac_gather_launch(pl.n_red, (hipStream_t)stream, X, d->grads, pl.P, 2 * pl.Q, d->workspace + pl.off_ss);
    return MBPO_OK;
  });
}

extern "C" int mbpo_sac_grad_norms(const mbpo_sac_desc *d, void *stream) {
  return sac_opt_entry(d, "sac_grad_norms", [&](const SacPlan &pl) -> int {
    sac_sumsq_launch(pl.n_red, (hipStream_t)stream, d->grads, pl.P, 2 * pl.Q, d->workspace + pl.off_ss);
    return MBPO_OK;
  });
}

extern "C" int mbpo_sac_apply(const mbpo_sac_desc *d, void *stream) {
  return sac_opt_entry(d, "sac_apply", [&](const SacPlan &pl) -> int {
    sac_apply_launch(pl.n_red, (hipStream_t)stream, sac_opt(d, pl));
    return MBPO_OK;
  });
}

extern "C" int mbpo_sac_finalize(const mbpo_sac_desc *d, void *stream) {
  return sac_opt_entry(d, "sac_finalize", [&](const SacPlan &pl) -> int {
    sac_finalize_launch((hipStream_t)stream, sac_opt(d, pl), nullptr, 0ull);
    return MBPO_OK;
  });
}

extern "C" int mbpo_sac_finalize_advance(const mbpo_sac_desc *d, uint64_t *rng_dev, uint64_t inc, void *stream) {
  MBPO_REQUIRE(rng_dev, MBPO_ERR_ARG, "sac_finalize_advance: null rng_dev");
  return sac_opt_entry(d, "sac_finalize_advance", [&](const SacPlan &pl) -> int {
    sac_finalize_launch((hipStream_t)stream, sac_opt(d, pl), (unsigned long long *)rng_dev, (unsigned long long)inc);
    return MBPO_OK;
  });
}
