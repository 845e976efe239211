// rollout_wide_terms.hip — k_model_rollout<128 | 256, RO_LR_TERMS, ...>: the term-table reward (rollout_wide_kernel.hpp).
#include "rollout_wide_kernel.hpp"

int rollout_wide_launch_terms(int H, const RolloutFlags &f, const RolloutArgs &A, const float *halluc_beta, const HoldArgs *hold, int grid,
                              int block, size_t lds, hipStream_t st) {
  return rollout_wide_launch_lr<RO_LR_TERMS>(H, f, A, halluc_beta, hold, grid, block, lds, st);
}
