// rollout64.hip — every instantiation of k_model_rollout64 (rollout64_kernel.hpp) behind one launch function, and the ensemble forward.
//
// The 60 instantiations stay in one unit, and k_ensemble_forward with them: the HT = 4 routines of wave_mlp.hpp / chain_run.hpp that
// k_ensemble_forward<64> and k_model_rollout64 both inline are optimised once per module, in front of the inlining, against all their
// callers.  Apart, k_ensemble_forward<64> comes out with 222 VGPRs instead of 225 and every k_model_rollout64 one to three hundred bytes
// shorter; cut by reward selector, the same.  Together they are what they have been (profiles/r15_rollout_split_registers.txt).
#include "rollout64_kernel.hpp"

// WIDE, LR, TERM, START, HAL and TA become template arguments here.  TA with HAL or with WIDE has no instantiation (the host refuses the
// first itself; the guard keeps the nest from creating either).
int rollout64_launch(int lr, const RolloutFlags &f, const RolloutArgs64 &AA, const float *halluc_beta, const HoldArgs *hold, int grid, int block,
                     size_t lds, hipStream_t st) {
  return mbpo_with_lr(lr, [&](auto LR) {
    return mbpo_with_bool(f.wide, [&](auto W) {
      return mbpo_with_bool(f.term, [&](auto TM) {
        return mbpo_with_bool(f.start, [&](auto SB) {
          return mbpo_with_bool(f.hal, [&](auto HL) {
            return mbpo_with_bool(f.ta, [&](auto TA) {
              if constexpr (TA.value && (HL.value || W.value)) {
                return rollout_refuse_ta(HL.value);
              } else {
                RolloutArgs64For<HL.value, TA.value> AH;
                static_cast<RolloutArgs64 &>(AH) = AA;
                if constexpr (HL.value) AH.halluc_beta = halluc_beta;
                if constexpr (TA.value) AH.hold = *hold;
                rollout_note_kernel({RO_FAMILY_64, 64, 0, 0, 0, LR.value, W.value, TM.value, SB.value, HL.value, TA.value});
                return mbpo_launch<k_model_rollout64<W.value, LR.value, TM.value, SB.value, HL.value, TA.value>>(grid, block, lds, st, "model_rollout", AH);
              }
            });
          });
        });
      });
    });
  });
}

#include "ens_forward.hpp"
