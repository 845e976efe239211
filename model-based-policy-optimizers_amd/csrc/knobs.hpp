// knobs.hpp — every switch the host dispatch reads, in one table: the MBPO_* environment variables and the int-valued
// debug overrides (mbpo_debug_set_*).  The storage, and the one place that reads the environment, are in api.hip; INTEGRATION.md
// lists the same names (tests/test_cpu_abi.py checks both).
#pragma once

// X(id, environment name or nullptr, default, re-read per query, meaning)
//   environment value: unset -> default, else atoll(string); read on the first query of that knob and kept for the life of the
//   process, unless the entry is marked re-read.  Entries without an environment name are set through their debug override only.
#define MBPO_KNOB_TABLE(X)                                                                                                          \
  X(SAC_LEAN, "MBPO_SAC_LEAN", 1, false, "0: the generic k_sac_fwd_bwd also where k_sac_lean applies")                             \
  X(SAC_LAYERED, "MBPO_SAC_LAYERED", 0, false, "1: force SAC's layer-by-layer path (tests)")                                        \
  X(SAC_SPLIT, "MBPO_SAC_SPLIT", -1, false, "0/1: two / three workgroups per SAC tile; -1: by network shape")                       \
  X(SAC_JVP, "MBPO_SAC_JVP", -1, false, "0: no forward-mode dQ/da in SAC's actor role; -1: where the shapes allow it")              \
  /* re-read on every call: tests/test_gpu_sac.py and tests/test_gpu_regimes.py flip it in-process with monkeypatch.setenv */      \
  X(SAC_THIN, "MBPO_SAC_THIN", 1, true, "0: SAC's thin first / last layers go through the MFMA runners too")                        \
  X(PPO_LEAN, "MBPO_PPO_LEAN", 1, false, "0: the generic PPO kernels also where k_ppo_lean / k_ppo_vg_lean apply")                  \
  X(PPO_LAYERED, "MBPO_PPO_LAYERED", 0, false, "1: force PPO's layer-by-layer path (tests)")                                        \
  X(PPO_SP2, "MBPO_PPO_SP2", -1, false, "0: never the 512-thread two-per-CU k_ppo_fwd_bwd; -1: by shape and tile count")            \
  X(PPO_VALUES_GAE, "MBPO_PPO_VALUES_GAE", -1, false, "0: separate values / GAE / moments launches; -1: fused where it fits")       \
  X(ENS_LEAN, "MBPO_ENS_LEAN", 1, false, "0: the generic k_ensemble_forward also where k_ens_fwd_lean applies")                     \
  X(ROLLOUT_LEAN, "MBPO_ROLLOUT_LEAN", 1, false, "0 generic 64-wide rollout kernel, 1 k_rollout_lean, 2 / 3 lean with two tiles in flight forced on / off") \
  X(ROLLOUT_PIPE, "MBPO_ROLLOUT_PIPE", -1, false, "0/1: two tiles in flight per k_rollout_lean workgroup off / on; -1: by tile count") \
  X(LAYERED_T2_MIN, "MBPO_LAYERED_T2_MIN", 4096, false, "64x64-tile count from which the layered GEMM keeps 64x64 tiles (below: 32x32)") \
  X(LAYERED_GROUP, "MBPO_LAYERED_GROUP", 1, false, "0: every layered GEMM its own launch instead of one per dependency level")      \
  X(PERM_BUCKETS, "MBPO_PERM_BUCKETS", 1, false, "0: philox_permutation without the bucket pre-sort")                               \
  X(BPTT_ZSTORE_MAX_MB, "MBPO_BPTT_ZSTORE_MAX_MB", 16384, false, "largest BPTT member pre-activation store; above it the backward sweep recomputes") \
  X(ICEM_UPDATE, nullptr, -1, false, "override only: 0 the global-memory k_icem_update, 1 k_icem_update_lds where it fits")         \
  X(BPTT_ZSTORE, nullptr, -1, false, "override only: 0 no BPTT pre-activation store (recompute)")                                   \
  X(TRAJ_COST_SLOTS, nullptr, -1, false, "override only: step slots per k_traj_cost workgroup (1, 2, .., 32); unset: by horizon and trajectory count") \
  X(PLAN_REWARD_FLAT, nullptr, -1, false, "override only: 1 k_plan_reward_flat also where k_plan_reward_grouped applies")

enum KnobId {
#define MBPO_KNOB_ID_(id, env, dflt, reread, meaning) KNOB_##id,
  MBPO_KNOB_TABLE(MBPO_KNOB_ID_)
#undef MBPO_KNOB_ID_
  KNOB_COUNT
};

// The debug override of `id` when one is set (>= 0), else its environment value, else its default.
long long mbpo_knob(KnobId id);
// The raw override slot: -1 (or any negative value) = not set.  mbpo_knob_set_override returns MBPO_OK.
int mbpo_knob_override(KnobId id);
int mbpo_knob_set_override(KnobId id, int mode);
