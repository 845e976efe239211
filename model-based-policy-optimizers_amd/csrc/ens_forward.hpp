// ens_forward.hpp — R2 ensemble MLP forward (see include/mbpo_hip.h): the generic kernel for hidden widths 64 / 128 / 256 and the host entry,
// which hands the benchmark shapes to the throughput kernel (ens_lean.hip).  The body of a translation unit, not an interface: included
// once, by rollout64.hip, which says why the kernel is compiled beside k_model_rollout64.
//
// Decomposition (MI355X): one workgroup owns a tile of 16 rows for ALL ensemble members; each wave walks a whole (tile, member) chain
// (wave_mlp.hpp).  Activations live in LDS, weights stream from L2 (flat params are ~0.2 MB, shared by every workgroup).
#pragma once
#include "common.hpp"
#include "chain_run.hpp"
#include "ens_lean.hpp"
#include "rollout_shared.hpp"

// ------------------------------------------------------------------------------------------------
// R2: y[e][row][:] = MLP_e(x[row])  — replaces vmap(Dynamics.next_state) (base_dynamics.py:15-20).
// ------------------------------------------------------------------------------------------------
struct EnsFwdArgs {
  MlpDev mlp;
  const float *x;
  float *y;
  long long n_rows;
  int shared_input;
  int ld_x, ld_h, ld_y, n_chains;
};

// workgroup = n_chains waves; wave w walks member (round*n_chains + w)'s chain on the tile
template <int H>
__global__ void __launch_bounds__(512) k_ensemble_forward(EnsFwdArgs A) {
  extern __shared__ __align__(16) float smem[];
  constexpr int HT = H / 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x;
  const MlpDev &m = A.mlp;
  const int E = m.n_nets, din = m.dims[0], dout = m.dims[m.n_layers];
  const int n_in_nets = A.shared_input ? 1 : E;
  const int T = 16 * A.ld_h;
  float *s_x = smem;                                // [n_in_nets][16][ld_x]
  float *s_pp = s_x + n_in_nets * 16 * A.ld_x;      // [n_chains][2] hidden tiles
  float *s_y = s_pp + A.n_chains * 2 * T;           // [E][16][ld_y]
  const long long n_tiles = (A.n_rows + 15) >> 4;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long row0 = tile * 16;
    for (int idx = tid; idx < n_in_nets * 16 * din; idx += nthreads) {
      int e = idx / (16 * din), rem = idx - e * 16 * din;
      int r = rem / din, c = rem - r * din;
      long long row = row0 + r;
      float v = 0.f;
      if (row < A.n_rows) v = A.x[((long long)e * A.n_rows + row) * din + c];
      s_x[(e * 16 + r) * A.ld_x + c] = v;
    }
    __syncthreads();
    for (int e0 = 0; e0 < E; e0 += A.n_chains) {
      const int e = e0 + wave;
      if (e < E)
        wave_mlp_fwd<HT>(m, m.params + (long long)e * m.net_stride, s_x + (A.shared_input ? 0 : e * 16 * A.ld_x), A.ld_x,
                         s_pp + wave * 2 * T, s_pp + wave * 2 * T + T, nullptr, nullptr, A.ld_h, s_y + e * 16 * A.ld_y, A.ld_y, lane);
    }
    __syncthreads();
    for (int idx = tid; idx < E * 16 * dout; idx += nthreads) {
      int e = idx / (16 * dout), rem = idx - e * 16 * dout;
      int r = rem / dout, c = rem - r * dout;
      long long row = row0 + r;
      if (row < A.n_rows) A.y[((long long)e * A.n_rows + row) * dout + c] = s_y[(e * 16 + r) * A.ld_y + c];
    }
    __syncthreads();
  }
}

// Measurement / test hook (not part of include/mbpo_hip.h): 0 = always the generic k_ensemble_forward, 1 = k_ens_fwd_lean where it applies,
// -1 = the MBPO_ENS_LEAN environment default (on).
extern "C" int mbpo_debug_set_ens_lean(int mode) { return mbpo_knob_set_override(KNOB_ENS_LEAN, mode); }

extern "C" int mbpo_ensemble_mlp_forward(const mbpo_mlp_desc *mlp, const float *x, int32_t shared_input, float *y,
                                         int64_t n_rows, void *stream) {
  MBPO_REQUIRE(mlp && x && y, MBPO_ERR_ARG, "ensemble_mlp_forward: null pointer");
  MBPO_REQUIRE(n_rows >= 0, MBPO_ERR_ARG, "ensemble_mlp_forward: n_rows < 0");
  EnsFwdArgs A;
  int rc = mbpo_make_mlp_dev(mlp, &A.mlp, "ensemble_mlp_forward");
  if (rc != MBPO_OK) return rc;
  if (n_rows == 0) return MBPO_OK;
  {
    // 64-wide member networks with 4 or 5 inputs: the throughput kernel (ens_lean.hip) — weights resident per workgroup, two tiles in
    // flight per workgroup, two workgroups per CU.  MBPO_ENS_LEAN=0 / mbpo_debug_set_ens_lean(0) keeps the generic kernel.
    if (mbpo_knob(KNOB_ENS_LEAN) != 0 && ens_lean_supports(A.mlp.dims, A.mlp.n_layers, A.mlp.act)) {
      EnsLeanArgs L;
      L.params = mlp->params; L.net_stride = mlp->n_nets > 1 ? mlp->net_stride : A.mlp.n_params;
      L.x = x; L.y = y; L.n_rows = n_rows; L.E = mlp->n_nets; L.N = A.mlp.dims[A.mlp.n_layers]; L.shared_input = shared_input ? 1 : 0;
      const long long pairs = (((n_rows + 15) >> 4) + 1) >> 1;
      long long wpm = (2LL * mbpo_num_cus()) / L.E;
      if (wpm < 1) wpm = 1;
      if (wpm > pairs) wpm = pairs;
      L.wgs_per_member = (int)wpm;
      L.n_hid = A.mlp.n_layers - 2;
      rc = ens_lean_launch(L, A.mlp.dims[0], mbpo_num_cus(), stream);
      if (rc != MBPO_OK) return rc;
      MBPO_CHECK_LAUNCH("ensemble_mlp_forward");
      return MBPO_OK;
    }
  }
  const int H = hidden_width(A.mlp);
  MBPO_REQUIRE(H == 64 || H == 128 || H == 256, MBPO_ERR_UNSUPPORTED,
               "ensemble_mlp_forward: hidden layers must share one width in {64,128,256}");
  A.x = x;
  A.y = y;
  A.n_rows = n_rows;
  A.shared_input = shared_input ? 1 : 0;
  A.ld_x = up4(A.mlp.dims[0]) + 4;
  A.ld_h = H + 4;
  A.ld_y = up4(A.mlp.dims[A.mlp.n_layers]) + 4;
  const int E = A.mlp.n_nets;
  const size_t fixed_f = (size_t)(shared_input ? 1 : E) * 16 * A.ld_x + (size_t)E * 16 * A.ld_y;
  A.n_chains = pick_chains(E, fixed_f, A.ld_h);
  MBPO_REQUIRE(A.n_chains >= 1, MBPO_ERR_UNSUPPORTED, "ensemble_mlp_forward: shapes do not fit 160 KiB of LDS");
  size_t lds = sizeof(float) * (fixed_f + 2ull * A.n_chains * 16 * A.ld_h);
  long long n_tiles = (n_rows + 15) >> 4;
  int grid = (int)(n_tiles < 8LL * mbpo_num_cus() ? n_tiles : 8LL * mbpo_num_cus());
  hipStream_t st = (hipStream_t)stream;
  const dim3 block(A.n_chains * 64);
  if (H == 64) rc = mbpo_launch<k_ensemble_forward<64>>(grid, block, lds, st, "ensemble_mlp_forward", A);
  else if (H == 128) rc = mbpo_launch<k_ensemble_forward<128>>(grid, block, lds, st, "ensemble_mlp_forward", A);
  else rc = mbpo_launch<k_ensemble_forward<256>>(grid, block, lds, st, "ensemble_mlp_forward", A);
  if (rc != MBPO_OK) return rc;
  MBPO_CHECK_LAUNCH("ensemble_mlp_forward");
  return MBPO_OK;
}
