#!/usr/bin/env python
"""MPC on the true Pendulum with iCEM, every planning iteration a launch chain on the MI355X path:

    mbpo_icem_sample -> [mbpo_icem_seed_candidates] -> mbpo_model_rollout (open loop) -> [mbpo_plan_reward_eval] -> [mbpo_terminal_value_eval] -> [mbpo_traj_cost_eval]
                     -> mbpo_icem_update

    python examples/icem_pendulum.py [--steps 100] [--horizon 20] [--speed-limit V] [--lambda-constraint L] [--seed 0]
                                     [--targets A0,A1,...] [--track AMPL,PERIOD] [--terminal-value] [--policy-prior [K]] [--tv-horizon 5] [--sac-steps 30000]

--speed-limit V: the plan is constrained to |thetadot| <= V at every step of the horizon — a TermCost, max_t(|thetadot_{t+1}| - V), written as
data and evaluated on the rollout's rows by one launch (iCemTO(cost_fn=TermCost(...), use_pessimism=True)); the objective of a candidate
is its reward minus lambda_constraint * max(cost, 0).  The run prints the return and the largest speed the true system reached.  Without
the option the same planner runs unconstrained.

--targets A0,A1,...: batched MPC, one environment per target angle (rad), all planned in one launch chain: the Pendulum's own reward with
a target angle per problem, PlanRewardParams.stack(system.reward, [[PendulumRewardParams(target_angle=a)] for a in targets]) in the
state's reward_params.  Prints each environment's final angle error and its return under its own target.

--track AMPL,PERIOD: one environment follows the target angle AMPL * sin(2 pi t / PERIOD) (t and PERIOD in seconds, dt = 0.05).  The
planner previews the reference over its horizon — a [1, H, 3] table whose target column is refilled IN PLACE before every `act`
(no new object, no reallocation; the launch reads what the table holds).  Prints the tracking error.

--terminal-value: a short SAC run on the Pendulum (SACOptimizer(warm_start=True), whose learner state carries the policy, the target
critics and the observation normaliser), then MPC on the true Pendulum at the short horizon --tv-horizon twice: with
TerminalValue.from_sac(learner_state, weight=gamma^H / reward_scaling) — min(Q1, Q2) under the policy's mode action at the state the
horizon ends in, added to every candidate's objective by one launch per iteration — and without it.  Both returns are printed, one seed.

--policy-prior [K]: the same short SAC run, then MPC at --tv-horizon with PolicyPrior.from_sac(learner_state, n_candidates=K) (K = 24
when omitted): once per `act` the policy is rolled closed-loop through the model from the current state, K proposals — its mode sequence
and K - 1 noisy ones — and one launch per iteration puts them into the first K of the sampled candidates.  Alone: with the prior and
without.  Together with --terminal-value the short-horizon MPC runs four ways from the one SAC run: plain, critic only, prior only, both.

A torque-limited pendulum cannot hold every angle: the prints are a record of what happened, not a claim.
"""
from __future__ import annotations

import argparse
import math
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "model-based-policy-optimizers_amd"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--speed-limit", type=float, default=None, metavar="V", help="constrain the plan to |thetadot| <= V (a TermCost)")
    ap.add_argument("--lambda-constraint", type=float, default=1e4, metavar="L")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--targets", type=str, default=None, metavar="A0,A1,...", help="batched MPC: one environment per target angle (rad)")
    ap.add_argument("--track", type=str, default=None, metavar="AMPL,PERIOD", help="follow AMPL * sin(2 pi t / PERIOD), previewed over the horizon")
    ap.add_argument("--terminal-value", action="store_true", help="train SAC briefly, then plan at --tv-horizon with and without its critic")
    ap.add_argument("--policy-prior", type=int, nargs="?", const=24, default=None, metavar="K",
                    help="train SAC briefly, then plan at --tv-horizon with K of its policy's rollouts among the candidates and without")
    ap.add_argument("--tv-horizon", type=int, default=5, metavar="H")
    ap.add_argument("--sac-steps", type=int, default=30000, help="--terminal-value / --policy-prior: environment steps of the SAC run")
    args = ap.parse_args()
    if args.targets is not None and args.track is not None:
        raise SystemExit("--targets and --track are two runs")
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: the HIP path has no CPU fallback")
    from mbpo.optimizers import iCemParams, iCemTO
    from mbpo.systems import Group, PendulumSystem, Term, TermCost
    dev = torch.device("cuda:0")
    system = PendulumSystem()
    if args.terminal_value or args.policy_prior is not None:
        if args.targets is not None or args.track is not None or args.speed_limit is not None:
            raise SystemExit("--terminal-value / --policy-prior is a run of its own")
        return run_terminal_value(args, system, dev)
    cost = None
    if args.speed_limit is not None:
        cost = TermCost(system.x_dim, system.u_dim, bias=-args.speed_limit, groups=[Group([Term("x_next", 2, "abs")])], reduce="max")
    opt = iCemTO(horizon=args.horizon, action_dim=system.action_dim, opt_params=iCemParams(lambda_constraint=args.lambda_constraint),
                 system=system, cost_fn=cost, use_pessimism=cost is not None)
    if args.targets is not None:
        return run_targets(args, opt, system, dev)
    if args.track is not None:
        return run_track(args, opt, system, dev)
    state = opt.init(args.seed)
    sp = state.system_params
    x = torch.tensor([math.cos(math.pi), math.sin(math.pi), 0.0], device=dev)      # hanging down, at rest
    ret, top = 0.0, 0.0
    for _ in range(args.steps):
        u, state = opt.act(x, state)
        st = system.step(x, u, sp)
        x, ret, top = st.x_next, ret + float(st.reward), max(top, abs(float(st.x_next[2])))
    limit = "none" if args.speed_limit is None else f"{args.speed_limit:g}"
    print(f"steps {args.steps}  speed limit {limit}  return {ret:.2f}  max |thetadot| {top:.3f}  final angle "
          f"{math.atan2(float(x[1]), float(x[0])):+.3f} rad")


def _angle_error(x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """theta - target wrapped to [-pi, pi), the reward's own difference."""
    d = torch.atan2(x[..., 1], x[..., 0]) - target
    return torch.remainder(d + math.pi, 2 * math.pi) - math.pi


def run_targets(args, opt, system, dev):
    from mbpo.systems import PlanRewardParams
    from mbpo.systems.rewards.pendulum_reward import PendulumRewardParams
    angles = [float(a) for a in args.targets.split(",")]
    B = len(angles)
    prp = PlanRewardParams.stack(system.reward, [[PendulumRewardParams(target_angle=a)] for a in angles], dev)      # [B, 1, 3]
    state = opt.init(args.seed, batch_size=B)
    sp = state.system_params                                                    # the true system steps under its ordinary parameters
    state = state.replace(system_params=sp.replace(reward_params=prp))
    tgt = torch.tensor(angles, device=dev)
    x = torch.tensor([math.cos(math.pi), math.sin(math.pi), 0.0], device=dev).repeat(B, 1)
    ret = torch.zeros(B, device=dev)
    for _ in range(args.steps):
        u, state = opt.act(x, state)
        ret += -(_angle_error(x, tgt) ** 2 + 0.1 * x[:, 2] ** 2) - 0.02 * u[:, 0] ** 2      # PendulumReward under each env's own target
        x = system.step(x, u, sp).x_next
    err = _angle_error(x, tgt)
    for b in range(B):
        print(f"env {b}  target {angles[b]:+.3f} rad  final angle error {float(err[b]):+.4f} rad  final |thetadot| {abs(float(x[b, 2])):.3f}  "
              f"return {float(ret[b]):.2f}")


def run_track(args, opt, system, dev):
    from mbpo.systems import PlanRewardParams
    from mbpo.systems.rewards.pendulum_reward import PendulumRewardParams
    ampl, period = [float(v) for v in args.track.split(",")]
    H, dt = args.horizon, 0.05
    ref = ampl * torch.sin(2 * math.pi * dt * torch.arange(args.steps + H, dtype=torch.float32) / period).to(dev)
    prp = PlanRewardParams.stack(system.reward, [[PendulumRewardParams(target_angle=0.0)] * H], dev)               # [1, H, 3]
    state = opt.init(args.seed)
    sp = state.system_params
    state = state.replace(system_params=sp.replace(reward_params=prp))
    ptr = prp.table.data_ptr()
    x = torch.tensor([1.0, 0.0, 0.0], device=dev)                              # upright, at rest: where the reference starts
    errs = []
    for t in range(args.steps):
        prp.table[0, :, 2].copy_(ref[t:t + H])                                  # the preview window, in place
        u, state = opt.act(x, state)
        x = system.step(x, u, sp).x_next
        errs.append(float(_angle_error(x, ref[t + 1])))
    assert prp.table.data_ptr() == ptr
    e = torch.tensor(errs)
    half = e[len(errs) // 2:]
    print(f"steps {args.steps}  track {ampl:g} * sin(2 pi t / {period:g})  RMS angle error {float(e.pow(2).mean().sqrt()):.4f} rad "
          f"(second half {float(half.pow(2).mean().sqrt()):.4f})  max |error| {float(e.abs().max()):.4f}  final {errs[-1]:+.4f}")


def run_terminal_value(args, system, dev):
    from mbpo.optimizers import PolicyPrior, SACOptimizer, TerminalValue, iCemParams, iCemTO
    from mbpo.replay import UniformSamplingQueue
    from mbpo.types import Transition
    gamma, reward_scaling, H, n_true = 0.99, 1.0, args.tv_horizon, 2048
    # a true buffer of start states all over the state space (SAC's environment resets draw from it)
    gen = torch.Generator().manual_seed(args.seed)
    th = (torch.rand(n_true, generator=gen) * 2 - 1) * math.pi
    x = torch.stack([torch.cos(th), torch.sin(th), (torch.rand(n_true, generator=gen) * 2 - 1) * 8], dim=1).to(dev)
    u = (torch.rand(n_true, 1, generator=gen) * 2 - 1).to(dev)
    sp = system.init_params(args.seed)
    st = system.step(x, u, sp)
    s0 = system.reset()
    dummy = Transition(observation=s0.x_next, action=torch.zeros(1, device=dev), reward=s0.reward, discount=torch.tensor(gamma, device=dev),
                       next_observation=s0.x_next)
    true_buffer = UniformSamplingQueue(max_replay_size=n_true, dummy_data_sample=dummy, sample_batch_size=1, device=dev)
    tbs = true_buffer.insert(true_buffer.init(args.seed), Transition(observation=x, action=u, reward=st.reward.reshape(-1),
                                                                     discount=torch.ones(n_true, device=dev), next_observation=st.x_next))
    sac = SACOptimizer(system=system, true_buffer=true_buffer, warm_start=True, num_timesteps=args.sac_steps, num_evals=1,
                       reward_scaling=reward_scaling, episode_length=200, normalize_observations=True, discounting=gamma, lr_policy=3e-4,
                       lr_alpha=3e-4, lr_q=3e-4, num_envs=64, batch_size=128, grad_updates_per_step=32, max_replay_size=2 ** 15,
                       min_replay_size=2 ** 9, num_eval_envs=1, tau=0.005, num_env_steps_between_updates=5)
    out = sac.train(opt_state=sac.init(key=args.seed + 3, true_buffer_state=tbs))
    learner_state = out.optimizer_state.learner_state                     # (warm_start=True: the learner as a value)
    tv = TerminalValue.from_sac(learner_state, weight=gamma ** H / reward_scaling) if args.terminal_value else None
    prior = PolicyPrior.from_sac(learner_state, n_candidates=args.policy_prior) if args.policy_prior is not None else None
    sac.close()
    print(f"SAC: {args.sac_steps} environment steps, {int(learner_state.step_count)} gradient steps;  " +
          ";  ".join(str(v) for v in (tv, prior) if v is not None))
    if prior is None:
        runs = (("with the critic", tv, None), ("without", None, None))
    elif tv is None:
        runs = (("with the prior", None, prior), ("without", None, None))
    else:
        runs = (("plain", None, None), ("critic only", tv, None), ("prior only", None, prior), ("critic and prior", tv, prior))
    for name, value, pp in runs:
        opt = iCemTO(horizon=H, action_dim=system.action_dim, opt_params=iCemParams(), system=system, terminal_value=value, policy_prior=pp)
        state = opt.init(args.seed)
        x = torch.tensor([math.cos(math.pi), math.sin(math.pi), 0.0], device=dev)      # hanging down, at rest
        ret = 0.0
        for _ in range(args.steps):
            a, state = opt.act(x, state)
            step = system.step(x, a, state.system_params)
            x, ret = step.x_next, ret + float(step.reward)
        print(f"horizon {H}  {name:16s} steps {args.steps}  return {ret:.2f}  final angle {math.atan2(float(x[1]), float(x[0])):+.3f} rad  "
              f"final |thetadot| {abs(float(x[2])):.3f}")


if __name__ == "__main__":
    main()
