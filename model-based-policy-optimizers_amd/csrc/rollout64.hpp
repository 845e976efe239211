// rollout64.hpp — host interface of the tile rollout kernel for hidden width 64 (k_model_rollout64, rollout64_kernel.hpp).
// One translation unit (rollout64.hip) holds the 60 instantiations: see there why they are not cut further.
#pragma once
#include "chain_run.hpp"
#include "rollout_tile.hpp"

// ------------------------------------------------------------------------------------------------
// H == 64: the rollout on phase runners (chain_run.hpp).  12 waves per 16-env tile:
//   policy phase   waves 0..3 walk the policy chain in lockstep (SP = 4), one barrier per layer;
//   model phase    waves 2e, 2e+1 walk member e's chain (SP = 2), up to 6 members side by side, one barrier per layer —
//                  5 members x 64 MFMAs per layer is 2560 MFMA cycles per SIMD and layer: this phase is fp32-MFMA-throughput
//                  bound on the CU, everything else is arranged to stay out of its way;
//   next-layer weights are requested one step ahead (first layers before the preceding bookkeeping section);
//   bookkeeping sections index with r = idx & 15 (no integer division), use the hardware transcendentals for the NormalTanh
//   sample, and the transition rows are double-buffered so a step's write-out overlaps the next step's first section.
// Barriers per env step (action_repeat 1): policy layers + model layers + 4.
// ------------------------------------------------------------------------------------------------
struct RolloutArgs64 {
  RolloutArgs a;
  NetShape sh_pi, sh_dyn;
  unsigned long long *stamps;   // measurement hook (mbpo_debug_set_rollout_stamps): s_memtime at the section boundaries of tile 0, step 1
};

// 12 waves (3 per SIMD -> 170 VGPRs each): with 16 waves the 128-register cap spilled 60 VGPRs into the step loop and the PMC
// counters showed 63 MB of scratch writes per launch against 1 MB of transition rows (profiles/r01_pmc_traffic.json).
// (Dealing the members 2,2,2,2,4 waves to level the MFMA load per SIMD was tried: the second runner instantiation brought
// 26 spills back and the kernel got slower, 82 -> 92 us.)
#define RO64_WAVES 12

// lr: RO_LR_*.  Every flag is a template argument of the kernel.  halluc_beta with hal, hold with ta.  Returns the status of the launch's
// LDS grant, or the refusal of ta with hal or with wide.
int rollout64_launch(int lr, const RolloutFlags &f, const RolloutArgs64 &AA, const float *halluc_beta, const HoldArgs *hold, int grid, int block,
                     size_t lds, hipStream_t st);
