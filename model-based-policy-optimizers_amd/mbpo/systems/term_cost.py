"""TermCost — a trajectory constraint written as data (include/mbpo_hip.h "term costs").  Not in the reference: there `cost_fn` is a
callable over one trajectory (icem_optimizer.py:99,161-166), which cannot run inside a kernel.

    c_t  = the term table (mbpo.systems.TermReward's Term / Group records, same format and capacity) on (x_t, u_t, x_{t+1})
    cost = sum_t c_t   (reduce="sum", the reference's reading of a stage cost)   or   max_t c_t   (reduce="max")

Positive means violated.  The max form is how a state constraint that must hold at every step is written: max_t(|x_t[2]| - 5) <= 0.
iCemTO(cost_fn=TermCost(...)) evaluates it on the rollout's rows in one launch (mbpo_traj_cost_eval) between the rollout and the update;
called like a function it is the same cost in torch, vmappable, and runs as any other `cost_fn`.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from mbpo import _hip
from mbpo.systems.rewards.term_reward import Group, TermRewardParams, term_reward_torch


class TermCost:
    """TermCost(x_dim, u_dim, bias=0.0, groups=[Group([Term("x_next", 2, "abs")]), ...], reduce="max").  u_dim is the control width the
    dynamics see: of the action columns [u | eta] of an optimistic system the table reads the first u_dim only."""

    def __init__(self, x_dim: int, u_dim: int, bias: float = 0.0, groups: Sequence[Group] = (), reduce: str = "sum"):
        if reduce not in _hip.COST_REDUCE_IDS:
            raise ValueError(f"unknown reduce {reduce!r} (one of {sorted(_hip.COST_REDUCE_IDS)})")
        self.params = TermRewardParams(int(x_dim), int(u_dim), float(bias), tuple(groups))      # TermReward's checks and packing
        self.x_dim, self.u_dim, self.reduce = self.params.x_dim, self.params.u_dim, reduce
        self._vec = {}                # device -> device vector: a captured launch replays the pointer it recorded

    @property
    def has_next_state_terms(self) -> bool:
        return self.params.has_next_state_terms

    def table(self, device) -> torch.Tensor:
        """The packed table on `device` (built once per device)."""
        k = str(device)
        if k not in self._vec:
            self._vec[k] = self.params.vector().to(device).contiguous()
        return self._vec[k]

    def stage_costs(self, observation: torch.Tensor, action: torch.Tensor, next_observation: Optional[torch.Tensor] = None) -> torch.Tensor:
        """c_t in torch, [..., H]: term_reward_torch on (observation [..., H, x], action [..., H, >= u_dim], next_observation)."""
        if next_observation is None and self.has_next_state_terms:
            raise ValueError("this table has next-state terms: pass next_observation")
        return term_reward_torch(self.params, observation, action, next_observation)

    def __call__(self, observation: torch.Tensor, action: torch.Tensor, next_observation: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The cost of one trajectory in torch, in the inputs' dtype: observation [H, x], action [H, >= u_dim], next_observation [H, x]
        (needed when the table has x_next terms) -> scalar.  Vmappable; a plain `cost_fn`."""
        c = self.stage_costs(observation, action, next_observation)
        return c.sum(dim=-1) if self.reduce == "sum" else c.max(dim=-1).values

    def trajectory_cost(self, rows: torch.Tensor, n_steps: int, n_traj: int, next_off: Optional[int] = None,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[n_traj]: the device path (mbpo_traj_cost_eval) on the step-major rows mbpo_model_rollout writes with open-loop actions,
        rows [n_steps * n_traj, row_len] with row t * n_traj + i = step t of trajectory i.  next_off: the next state's column, by default
        the rollout's own layout [obs | action | reward | discount | next_obs | truncation]: row_len - x_dim - 1."""
        from mbpo import ops
        if next_off is None:
            next_off = rows.shape[1] - self.x_dim - 1
        return ops.traj_cost_eval(self.table(rows.device), rows, n_steps, n_traj, self.x_dim, self.u_dim, next_off,
                                  _hip.COST_REDUCE_IDS[self.reduce], out=out)
