"""PlanRewardParams — reward parameters that differ per planned problem and per planned step (include/mbpo_hip.h "plan rewards").  Not in
the reference: there a batch of plans is `jax.vmap(iCemTO.optimize)` and a vmapped `reward_params` comes with it; here batched MPC is one
launch chain whose rollout kernels stage ONE reward vector per workgroup.

    r(t, b, j) = R(table[b or 0][t or 0]; x, u, x_next of row (t, b, j))

iCEM alone consumes it (`iCemTO.optimize` / `act`, single and batched): after the rollout one launch of mbpo_plan_reward_eval rewrites
the rows' reward column under the table, and the unchanged update launch reads it.  A goal per robot is a `[B, 1, P]` table, a reference
that moves inside the preview window is `[1, H, P]`, both are `[B, H, P]`.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from mbpo import _hip
from mbpo.systems.rewards.pendulum_reward import PendulumReward, QuadraticReward
from mbpo.systems.rewards.term_reward import TermReward


def reward_param_len(reward) -> int:
    """Floats of `reward`'s kernel vector; a ValueError for a reward no plan reward can hold."""
    if isinstance(reward, TermReward):
        return _hip.REWARD_TERMS_FLOATS
    if isinstance(reward, QuadraticReward):
        return 2 * reward.x_dim + reward.u_dim
    if isinstance(reward, PendulumReward):
        return 3
    if type(reward).__name__ == "LearnedReward":
        raise ValueError("a LearnedReward cannot be a plan reward: the learned head is not a function of the row (x, u, x_next), and a "
                         "learned reward per problem is not built")
    raise ValueError(f"a plan reward is a QuadraticReward, TermReward or PendulumReward, got {type(reward).__name__}")


def _vector(reward, params) -> torch.Tensor:
    """One parameter object of `reward` as its fp32 kernel vector, on the host."""
    if isinstance(reward, TermReward):
        return reward._check(params).vector()
    return reward.kernel_spec(params, "cpu")[1]


class PlanRewardParams:
    """PlanRewardParams(reward, table): `reward` a QuadraticReward, TermReward or PendulumReward, `table` a float32 device tensor
    [PB, PH, param_len] with PB in {1, B} (B the planner's batch_size; 1 on a single state) and PH in {1, horizon}; an axis of size 1 is
    broadcast.  Goes where the reward's own parameters go: `opt_state.system_params.reward_params`.

    `table[b, t]` is the reward's kernel vector, the layout the rollout kernels read:
        PendulumReward   [angle_cost, control_cost, target_angle]                                      param_len 3
        QuadraticReward  [target (x_dim) | q (x_dim) | r (u_dim)]                                      param_len 2 x_dim + u_dim
        TermReward       TermRewardParams.vector(): [n_groups, n_terms, bias, 0 | 16 x (weight, link, first_term, n_terms) |
                         128 x (z_index, fn, coef, offset)]                                            param_len 580
    so `prp.table[..., :x_dim] = targets` sets quadratic targets and `prp.table[..., 2] = angles` Pendulum target angles.

    The table is kept BY REFERENCE and read by the launch, not before: a tracking loop refills it in place between `act` calls
    (`prp.table.copy_(ref[t:t + H])`) with no reallocation.  `reward` need not be the system's own reward; its x_dim / u_dim must be the
    system's (u_dim: the control width the dynamics see).  `base`: one ordinary parameter object of `reward` (stack: nested[0][0]), what the
    in-rollout reward runs under when `reward` is the system's own — that column is computed and then replaced."""

    def __init__(self, reward, table: torch.Tensor, base=None):
        P = reward_param_len(reward)
        if not isinstance(table, torch.Tensor) or table.dtype != torch.float32:
            raise ValueError("table must be a float32 tensor [PB, PH, param_len]")
        if table.dim() != 3 or table.shape[0] < 1 or table.shape[1] < 1:
            raise ValueError(f"table must be [PB, PH, param_len] with PB, PH >= 1, got {tuple(table.shape)}")
        if table.shape[2] != P:
            raise ValueError(f"table has param_len {table.shape[2]}, a {type(reward).__name__} vector at x_dim {reward.x_dim}, u_dim "
                             f"{reward.u_dim} holds {P} floats")
        if not table.is_contiguous():
            raise ValueError("table must be contiguous (the launch reads it through one pointer)")
        self.reward, self.table = reward, table
        self.base = base if base is not None else reward.init_params(0)

    @classmethod
    def stack(cls, reward, nested: Sequence[Sequence], device) -> "PlanRewardParams":
        """The table from a nested list [PB][PH] of `reward`'s ordinary parameter objects (PendulumRewardParams, QuadraticRewardParams,
        TermRewardParams): assembled on the host, uploaded once."""
        P = reward_param_len(reward)
        PB = len(nested)
        PH = len(nested[0]) if PB else 0
        if PB < 1 or PH < 1 or any(len(row) != PH for row in nested):
            raise ValueError("nested must be a rectangular list [PB][PH] with PB, PH >= 1")
        host = torch.empty(PB, PH, P, dtype=torch.float32)
        for b, row in enumerate(nested):
            for t, p in enumerate(row):
                v = _vector(reward, p).reshape(-1)
                if v.numel() != P:
                    raise ValueError(f"nested[{b}][{t}] gives {v.numel()} floats, a {type(reward).__name__} vector holds {P}")
                host[b, t] = v
        return cls(reward, host.to(device).contiguous(), base=nested[0][0])

    @property
    def problems(self) -> int:
        return int(self.table.shape[0])

    @property
    def steps(self) -> int:
        return int(self.table.shape[1])

    @property
    def param_len(self) -> int:
        return int(self.table.shape[2])

    @property
    def kind(self) -> int:
        return (_hip.REWARD_TERMS if isinstance(self.reward, TermReward) else
                _hip.REWARD_QUADRATIC if isinstance(self.reward, QuadraticReward) else _hip.REWARD_PENDULUM)

    def check_plan(self, system, horizon: int, batch: Optional[int]) -> None:
        """The table against the planner's shapes: ValueError where PB / PH / the widths do not fit.  batch None: a single state."""
        r = self.reward
        if r.x_dim != system.x_dim or r.u_dim != system.u_dim:
            raise ValueError(f"the plan reward is a {type(r).__name__} at x_dim {r.x_dim}, u_dim {r.u_dim}; the system has x_dim "
                             f"{system.x_dim}, u_dim {system.u_dim} (the control width the dynamics see; its action_dim is "
                             f"{system.action_dim})")
        if batch is None and self.problems != 1:
            raise ValueError(f"the plan reward's table holds {self.problems} problems: a single state needs PB = 1 (a batched state: "
                             f"iCemTO.init(key, batch_size=B))")
        if batch is not None and self.problems not in (1, batch):
            raise ValueError(f"the plan reward's table holds {self.problems} problems, the state has batch_size {batch}: PB must be 1 or "
                             f"{batch}")
        if self.steps not in (1, int(horizon)):
            raise ValueError(f"the plan reward's table holds {self.steps} steps, the horizon is {horizon}: PH must be 1 or {horizon}")

    def rollout_reward_params(self, system, system_params):
        """What the rollout itself runs under (its reward column is replaced afterwards): `base` when `reward` is the system's own reward,
        else the system's own default parameters (a learned reward's are the dynamics')."""
        if self.reward is system.reward:
            return self.base
        if type(system.reward).__name__ == "LearnedReward":
            return system_params.dynamics_params
        return system.reward.init_params(0)

    def __repr__(self):
        return f"PlanRewardParams({type(self.reward).__name__}, table {tuple(self.table.shape)})"


def refuse_plan_reward(system_params, who: str) -> None:
    """Every consumer of a system's parameters but iCEM passes its `rollout_spec`; iCEM takes the plan reward out before it calls it."""
    if isinstance(getattr(system_params, "reward_params", None), PlanRewardParams):
        raise ValueError(f"{who}: reward_params is a PlanRewardParams, which only iCEM consumes (iCemTO / iCEMOptimizer optimize and act, "
                         f"single and batched).  System.step, rollout_actions / rollout_policy, BraxWrapper (SAC, PPO) and BPTT evaluate "
                         f"one reward vector per launch; a goal-conditioned policy needs the goal in its observation")
