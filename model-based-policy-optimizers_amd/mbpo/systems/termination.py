"""BoxTermination — the termination function of a model environment: a per-dimension interval on the next state plus a
finiteness check (MBPO's termination functions, Janner et al. 2019, are all of this form).

NOT IN THE REFERENCE: its Systems never set SystemState.done (base_systems.py:25 defaults it to 0.0), so its model episodes end by
truncation only.  Semantics (include/mbpo_hip.h "termination"; restated by oracle/rollout.py:env_step given a system that returns
done), for a step's pre-auto-reset next state x':
    violated_d = !(low_d <= x'_d && x'_d <= high_d) || isinf(x'_d)          (NaN fails the compares: violated)
    sys_done   = any_d violated_d ? 1 : 0
    over = steps >= episode_length;  done = over ? 1 : sys_done;  truncation = over ? 1 - sys_done : 0
    obs <- first_obs where done;  discount = 1 - done;  next_observation = the post-reset obs
Unbounded dimensions carry -inf / +inf.  The bounds are CLOSED: a state exactly on a bound is not terminal.

The fused rollout kernels evaluate it (mbpo_rollout_desc.term_low / term_high) for PendulumSystem(termination=) and
EnsembleSystem(termination=); `__call__` is the same formula on the host.
"""
from __future__ import annotations

import math
from typing import Dict, Sequence, Tuple, Union

import torch

_INF = math.inf
TERMINATION_KEYS = ("term_low", "term_high")


class BoxTermination:
    def __init__(self, low: Union[Sequence[float], torch.Tensor], high: Union[Sequence[float], torch.Tensor]):
        self.low = torch.as_tensor(low, dtype=torch.float32).reshape(-1).cpu().clone()
        self.high = torch.as_tensor(high, dtype=torch.float32).reshape(-1).cpu().clone()
        if self.low.shape != self.high.shape or self.low.numel() == 0:
            raise ValueError(f"low and high must have the same length x_dim > 0 (got {self.low.numel()}, {self.high.numel()})")
        if bool(torch.isnan(self.low).any()) or bool(torch.isnan(self.high).any()):
            raise ValueError("NaN bound (an unbounded dimension carries -inf / +inf)")
        self.x_dim = int(self.low.numel())
        # what rollout_spec's cache key holds: the bounds' values (host tuples: no device read-back)
        self.key: Tuple[Tuple[float, ...], Tuple[float, ...]] = (tuple(self.low.tolist()), tuple(self.high.tolist()))
        self._dev: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}

    def __call__(self, x_next: torch.Tensor) -> torch.Tensor:
        """done (float, 1 = terminal) of next states [..., x_dim] — the formula above, on x_next's device."""
        if x_next.shape[-1] != self.x_dim:
            raise ValueError(f"x_next must be [..., {self.x_dim}]")
        lo, hi = self.low.to(x_next.device, x_next.dtype), self.high.to(x_next.device, x_next.dtype)
        violated = ~((lo <= x_next) & (x_next <= hi)) | torch.isinf(x_next)
        return violated.any(dim=-1).to(x_next.dtype)

    def kernel_spec(self, device) -> Tuple[torch.Tensor, torch.Tensor]:
        """(term_low, term_high) on `device`, cached per device: no host-to-device copy inside a captured graph."""
        k = str(device)
        if k not in self._dev:
            self._dev[k] = (self.low.to(device).contiguous(), self.high.to(device).contiguous())
        return self._dev[k]

    def __repr__(self) -> str:
        return f"BoxTermination(low={list(self.key[0])}, high={list(self.key[1])})"

    # ---- the common conditions -----------------------------------------------------------------------------------------------
    # The interval values below are MBPO's published termination functions (mbpo/static/*.py of the authors' code) AS REMEMBERED:
    # they are UNVERIFIED against upstream.  Upstream writes strict inequalities (e.g. height > 0.7); the bounds here are closed
    # (height >= 0.7), which differs only for a state exactly on a bound.
    @classmethod
    def from_intervals(cls, x_dim: int, intervals: Dict[int, Tuple[float, float]]) -> "BoxTermination":
        """Unbounded except for {dimension: (low, high)}."""
        low, high = [-_INF] * x_dim, [_INF] * x_dim
        for d, (lo, hi) in intervals.items():
            low[d], high[d] = float(lo), float(hi)
        return cls(low, high)

    @classmethod
    def inverted_pendulum(cls, x_dim: int = 4) -> "BoxTermination":
        """|x[1]| <= 0.2 (the pole angle).  Unverified against upstream; closed bounds (see above)."""
        return cls.from_intervals(x_dim, {1: (-0.2, 0.2)})

    @classmethod
    def hopper(cls, x_dim: int = 11) -> "BoxTermination":
        """x[0] >= 0.7 (height), |x[1]| <= 0.2 (angle), |x[d]| <= 100 for d >= 1.  Unverified against upstream; closed bounds."""
        iv = {d: (-100.0, 100.0) for d in range(1, x_dim)}
        iv[0] = (0.7, _INF)
        iv[1] = (-0.2, 0.2)
        return cls.from_intervals(x_dim, iv)

    @classmethod
    def walker2d(cls, x_dim: int = 17) -> "BoxTermination":
        """0.8 <= x[0] <= 2.0 (height), |x[1]| <= 1.0 (angle).  Unverified against upstream; closed bounds."""
        return cls.from_intervals(x_dim, {0: (0.8, 2.0), 1: (-1.0, 1.0)})

    @classmethod
    def ant(cls, x_dim: int = 27) -> "BoxTermination":
        """0.2 <= x[0] <= 1.0 (torso height).  Unverified against upstream; closed bounds."""
        return cls.from_intervals(x_dim, {0: (0.2, 1.0)})

    @classmethod
    def humanoid(cls, x_dim: int = 45) -> "BoxTermination":
        """1.0 <= x[0] <= 2.0 (torso height).  Unverified against upstream; closed bounds."""
        return cls.from_intervals(x_dim, {0: (1.0, 2.0)})


def termination_spec(termination, x_dim: int, device) -> dict:
    """The rollout-spec entries of a system's termination: {} without one."""
    if termination is None:
        return {}
    if termination.x_dim != x_dim:
        raise ValueError(f"the termination has {termination.x_dim} dimensions, the system {x_dim}")
    lo, hi = termination.kernel_spec(device)
    return dict(term_low=lo, term_high=hi)


def without_termination(spec: dict) -> dict:
    """The rollout spec with the termination dropped: for the consumers whose scans ignore SystemState.done, as the reference's
    rollout_actions / rollout_policy do (utils/optimizer_utils.py:31-47, 85-93) — iCEM, BPTT, rollout_actions, rollout_policy."""
    if TERMINATION_KEYS[0] not in spec:
        return spec
    return {k: v for k, v in spec.items() if k not in TERMINATION_KEYS}
