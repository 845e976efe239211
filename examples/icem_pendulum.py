#!/usr/bin/env python
"""MPC on the true Pendulum with iCEM, every planning iteration a launch chain on the MI355X path:

    mbpo_icem_sample -> mbpo_model_rollout (open loop) -> [mbpo_traj_cost_eval] -> mbpo_icem_update

    python examples/icem_pendulum.py [--steps 100] [--horizon 20] [--speed-limit V] [--lambda-constraint L] [--seed 0]

--speed-limit V: the plan is constrained to |thetadot| <= V at every step of the horizon — a TermCost, max_t(|thetadot_{t+1}| - V), written as
data and evaluated on the rollout's rows by one launch (iCemTO(cost_fn=TermCost(...), use_pessimism=True)); the objective of a candidate
is its reward minus lambda_constraint * max(cost, 0).  The run prints the return and the largest speed the true system reached.  Without
the option the same planner runs unconstrained.
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
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: the HIP path has no CPU fallback")
    from mbpo.optimizers import iCemParams, iCemTO
    from mbpo.systems import Group, PendulumSystem, Term, TermCost
    dev = torch.device("cuda:0")
    system = PendulumSystem()
    cost = None
    if args.speed_limit is not None:
        cost = TermCost(system.x_dim, system.u_dim, bias=-args.speed_limit, groups=[Group([Term("x_next", 2, "abs")])], reduce="max")
    opt = iCemTO(horizon=args.horizon, action_dim=system.action_dim, opt_params=iCemParams(lambda_constraint=args.lambda_constraint),
                 system=system, cost_fn=cost, use_pessimism=cost is not None)
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


if __name__ == "__main__":
    main()
