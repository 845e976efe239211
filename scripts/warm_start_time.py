#!/usr/bin/env python
"""Wall time of the SECOND SACOptimizer.train() call of 8 training steps at the benchmark's SAC shape (bench.py: N = 4096 envs, B = 256,
G = 64, horizon 5, 5 members, 64x3 nets, a 2^20-row model replay buffer), three ways in one session:

  1. cold                 warm_start=False: a new trainer and a fresh learner per call (the reference's behaviour)
  2. warm_fresh_trainer   warm_start=True, the trainer released before every call (BraxOptimizer.close()): the learner is carried, the
                          trainer construction, the eager warm-up step and the graph capture are paid per call
  3. warm_kept_trainer    warm_start=True: the learner is carried and the trainer kept; the model replay buffer is new per call (its
                          address differs, so the kept trainer captures its step again)
  +  warm_kept_retained   as 3 with retain_replay_buffer=True: no prefill, every address as captured, the step replays

Each call is synchronised around; a configuration's first call is not timed, the next `--reps` (5) are, and the median is reported.

    python scripts/warm_start_time.py [--reps 5] [--out profiles/r12_warm_start.json]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "model-based-policy-optimizers_amd"))

import torch  # noqa: E402

X_DIM, U_DIM, N_MEMBERS, HIDDEN = 4, 1, 5, (64, 64, 64)
N_ENVS, EPISODE_LEN, S_STEPS, BATCH, GRAD_UPDATES, MAX_REPLAY = 4096, 5, 5, 256, 64, 2 ** 20
TRAIN_STEPS = 8


def make_optimizer(device, **switches):
    from mbpo.optimizers import SACOptimizer
    from mbpo.replay import UniformSamplingQueue
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, QuadraticReward
    from mbpo.types import Transition
    dyn = EnsembleDynamics(X_DIM, U_DIM, n_members=N_MEMBERS, hidden_layer_sizes=HIDDEN, device=device)
    system = EnsembleSystem(dyn, QuadraticReward(X_DIM, U_DIM), mode="mean", predict_delta=True)
    sys_params = system.init_params(1)
    sys_params.dynamics_params.params.mul_(0.5)          # as bench.py: 5-step rollouts of a random ensemble stay O(1)
    g = torch.Generator().manual_seed(0)
    n_true = 2 ** 16
    th = (torch.rand(n_true, generator=g) * 2 - 1) * 3.14159265
    obs = torch.stack([torch.cos(th), torch.sin(th), (torch.rand(n_true, generator=g) * 2 - 1) * 8,
                       (torch.rand(n_true, generator=g) * 2 - 1) * 8], dim=1)
    act = torch.rand(n_true, U_DIM, generator=g) * 2 - 1
    dummy = Transition(observation=torch.zeros(X_DIM), action=torch.zeros(U_DIM), reward=torch.zeros(1), discount=torch.zeros(1),
                       next_observation=torch.zeros(X_DIM))
    true_buffer = UniformSamplingQueue(n_true, dummy, 1, device=device)
    rows = torch.cat([obs, act, torch.zeros(n_true, 1), torch.ones(n_true, 1), obs], dim=1).to(device)
    tbs = true_buffer.insert_rows(true_buffer.init(0), rows)
    per_step = N_ENVS * S_STEPS
    opt = SACOptimizer(system=system, true_buffer=true_buffer, num_timesteps=per_step + TRAIN_STEPS * per_step,
                       episode_length=EPISODE_LEN, num_env_steps_between_updates=S_STEPS, num_envs=N_ENVS, batch_size=BATCH,
                       grad_updates_per_step=GRAD_UPDATES, normalize_observations=True, discounting=0.99, lr_policy=3e-4, lr_q=3e-4,
                       lr_alpha=3e-4, min_replay_size=per_step, max_replay_size=MAX_REPLAY, policy_hidden_layer_sizes=HIDDEN,
                       critic_hidden_layer_sizes=HIDDEN, use_graph=True, **switches)
    assert opt.dummy_trainer.num_training_steps_per_epoch == TRAIN_STEPS
    state = opt.init(key=3, true_buffer_state=tbs).replace(system_params=sys_params)
    return opt, state


def measure(device, reps, release_trainer=False, **switches):
    opt, state = make_optimizer(device, **switches)
    state = opt.train(state).optimizer_state              # the FIRST call: not timed
    times, captures, seen = [], 0, [None if opt._trainer is None else opt._trainer._graph]      # (kept alive: `is` stays meaningful)
    for _ in range(reps):
        if release_trainer:
            opt.close()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        state = opt.train(state).optimizer_state
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        graph = None if opt._trainer is None else opt._trainer._graph
        captures += graph is not seen[-1]
        seen.append(graph)
    ls = state.learner_state
    out = dict(ms=[round(t, 3) for t in times], median_ms=round(statistics.median(times), 3),
               optimizer_steps_at_end=None if ls is None else int(ls.step_count),
               graph_captures_in_timed_calls=captures if switches.get("warm_start") else reps)
    opt.close()
    del opt, state
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r12_warm_start.json"))
    a = ap.parse_args()
    device = torch.device("cuda", torch.cuda.current_device())
    res = dict(
        what="wall ms of one SACOptimizer.train() call after the first (prefill + 8 training steps + 1 evaluation), median of reps",
        shape=dict(num_envs=N_ENVS, batch_size=BATCH, grad_updates_per_step=GRAD_UPDATES, episode_length=EPISODE_LEN,
                   num_env_steps_between_updates=S_STEPS, members=N_MEMBERS, hidden=list(HIDDEN), max_replay_size=MAX_REPLAY,
                   training_steps_per_call=TRAIN_STEPS),
        reps=a.reps, device=torch.cuda.get_device_name(device))
    res["cold"] = measure(device, a.reps)
    res["warm_fresh_trainer"] = measure(device, a.reps, release_trainer=True, warm_start=True)
    res["warm_kept_trainer"] = measure(device, a.reps, warm_start=True)
    res["warm_kept_retained"] = measure(device, a.reps, warm_start=True, retain_replay_buffer=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: (v["median_ms"] if isinstance(v, dict) and "median_ms" in v else None) for k, v in res.items()
                      if k in ("cold", "warm_fresh_trainer", "warm_kept_trainer", "warm_kept_retained")}))


if __name__ == "__main__":
    main()
