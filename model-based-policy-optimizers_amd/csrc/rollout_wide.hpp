// rollout_wide.hpp — host interface of the tile rollout kernel for hidden widths 128 and 256 (k_model_rollout, rollout_wide_kernel.hpp).
// One translation unit per reward selector (rollout_wide_formula.hip, rollout_wide_learned.hip, rollout_wide_terms.hip): the three values never
// share an instantiation, and the 36 instantiations compile side by side.
#pragma once
#include "rollout_tile.hpp"

// H: 128 or 256.  Of the flags the kernel reads start, hal and ta (the termination box is a run-time test here, and there is no WIDE).
// halluc_beta with hal, hold with ta.  Returns the status of the launch's LDS grant, or the refusal of ta with hal.
int rollout_wide_launch_formula(int H, const RolloutFlags &f, const RolloutArgs &A, const float *halluc_beta, const HoldArgs *hold, int grid,
                                int block, size_t lds, hipStream_t st);
int rollout_wide_launch_learned(int H, const RolloutFlags &f, const RolloutArgs &A, const float *halluc_beta, const HoldArgs *hold, int grid,
                                int block, size_t lds, hipStream_t st);
int rollout_wide_launch_terms(int H, const RolloutFlags &f, const RolloutArgs &A, const float *halluc_beta, const HoldArgs *hold, int grid,
                              int block, size_t lds, hipStream_t st);
