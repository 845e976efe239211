"""Reference for terminating model rollouts: an oracle.systems system wrapped so that its `step` reports done.

    violated_d = !(low_d <= x'_d && x'_d <= high_d) || isinf(x'_d)      (NaN fails the compares: violated)
    done       = any_d violated_d ? 1 : 0

oracle/rollout.py:env_step consumes a third result of `step` as SystemState.done (done = over ? 1 : sys_done, truncation =
over ? 1 - sys_done : 0, obs <- first_obs where done), so oracle.rollout and the oracle trainer loops run a wrapped system unchanged.

`done` is a discontinuous decision and device rows match the oracle only to a tolerance, so the wrapper records, per step call, every
env's smallest distance of x' to any finite bound; `near_mask` names the envs that ever came closer than a margin.  The tests
exclude those envs from the comparison as a whole (an env whose decision flipped diverges from there on) and cap their share.
"""
from __future__ import annotations

import torch

ATOL = 2e-4                 # the rollout rows' stated tolerance (tests/test_gpu_rollout.py)
MARGIN = 10 * ATOL          # an env ever closer than this to a bound is excluded
MAX_EXCLUDED = 0.10         # ... and at most this share of the envs may be
MIN_TERMINATING = 0.10      # at least this share of the envs must terminate by sys_done


def box_done(x_next: torch.Tensor, low: torch.Tensor, high: torch.Tensor) -> torch.Tensor:
    violated = ~((low <= x_next) & (x_next <= high)) | torch.isinf(x_next)
    return violated.any(dim=-1).to(x_next.dtype)


class TerminatingSystem:
    """system.step(x, u, **kw) -> (x', r, done) with the box's done; everything else is the wrapped system's."""

    def __init__(self, system, low, high):
        self.system = system
        self.low = torch.as_tensor(low, dtype=torch.float32)
        self.high = torch.as_tensor(high, dtype=torch.float32)
        self.x_dim, self.u_dim = system.x_dim, system.u_dim
        self.distances = []          # per step call: [N] smallest |x'_d - bound_d| over the finite bounds
        self.dones = []              # per step call: [N]

    def reward(self, x, u):
        return self.system.reward(x, u)

    def step(self, x, u, **kw):
        res = self.system.step(x, u, **kw)
        xn, r = res[0], res[1]
        lo, hi = self.low.to(xn.dtype), self.high.to(xn.dtype)
        done = box_done(xn, lo, hi)
        d = torch.full(xn.shape[:1], float("inf"), dtype=xn.dtype)
        for b in (lo, hi):
            fin = torch.isfinite(b)
            if bool(fin.any()):
                d = torch.minimum(d, (xn[:, fin] - b[fin]).abs().min(dim=1).values)
        self.distances.append(d)
        self.dones.append(done)
        return xn, r, done

    def near_mask(self, margin: float = MARGIN) -> torch.Tensor:
        """[N] bool: envs that were ever within `margin` of a finite bound (NaN distances count as near)."""
        d = torch.stack(self.distances)
        return ~(d >= margin).all(dim=0)

    def terminated_mask(self, last_of: int = 1) -> torch.Tensor:
        """[N] bool: envs for which some env step reported done (with action_repeat = last_of inner step calls per env step, the
        env step's done is its last inner call's)."""
        return torch.stack(self.dones[last_of - 1::last_of]).bool().any(dim=0)


def check_oracle_run(wrapped: TerminatingSystem, truncation: torch.Tensor, last_of: int = 1) -> torch.Tensor:
    """The three conditions on the oracle run itself (asserted before any device result is looked at): at most MAX_EXCLUDED of the
    envs near a bound, at least MIN_TERMINATING terminating by sys_done, and a truncation somewhere.  Returns the kept-env mask."""
    near = wrapped.near_mask()
    n = near.numel()
    assert int(near.sum()) <= MAX_EXCLUDED * n, f"{int(near.sum())} of {n} envs within {MARGIN} of a bound"
    term = wrapped.terminated_mask(last_of)
    assert int(term.sum()) >= MIN_TERMINATING * n, f"only {int(term.sum())} of {n} envs terminate"
    assert float(truncation.sum()) >= 1, "no truncation in the oracle run"
    return ~near
