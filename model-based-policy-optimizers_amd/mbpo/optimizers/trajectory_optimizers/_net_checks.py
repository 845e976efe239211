"""Checks shared by the objects that hand a trainer's networks to iCEM (TerminalValue, PolicyPrior): kernel dims, flat float32 parameter
tensors, and the LearnerState behind whatever a caller holds."""
from __future__ import annotations

from typing import Sequence

import torch

from mbpo import _hip

KERNEL_WIDTHS = (64, 128, 256)      # what the wave chains take (mbpo_terminal_value_eval: MBPO_ERR_UNSUPPORTED otherwise)


def _n_params(dims: Sequence[int]) -> int:
    return sum(dims[i] * dims[i + 1] + dims[i + 1] for i in range(len(dims) - 1))


def _check_dims(name: str, dims, d_in: int, d_out: int, what: str) -> list:
    dims = [int(v) for v in dims]
    if not (2 <= len(dims) <= _hip.MBPO_MAX_LAYERS + 1) or min(dims) < 1:
        raise ValueError(f"{name} must hold 2 .. {_hip.MBPO_MAX_LAYERS + 1} positive sizes [in, hidden..., out], got {dims}")
    if dims[0] != d_in or dims[-1] != d_out:
        raise ValueError(f"{name} must run [{d_in}] -> [{d_out}] ({what}), got {dims}")
    hid = dims[1:-1]
    if hid and (any(h != hid[0] for h in hid) or hid[0] not in KERNEL_WIDTHS):
        raise ValueError(f"{name}: hidden layers {hid} must share one width in {KERNEL_WIDTHS} (the kernel's wave chains take no other; "
                         f"a trainer's KERNEL dims are already padded to one of them)")
    return dims


def _check_flat(name: str, t, n: int, exact: bool = True) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise ValueError(f"{name} must be a float32 tensor")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous (the launch reads it through one pointer)")
    if (t.numel() != n) if exact else (t.numel() < n):
        raise ValueError(f"{name} holds {t.numel()} floats, expected {n}")
    return t


def _learner_state_of(obj, who: str = "from_sac", trainer: str = "SAC"):
    """A LearnerState, the one a BraxState carries, or the last one of a SAC trainer / of the trainer a SACOptimizer keeps (PPO alike)."""
    if hasattr(obj, "params") and hasattr(obj, "normalizer"):
        return obj
    for holder in (obj, getattr(obj, "_trainer", None)):
        for attr in ("learner_state", "last_learner_state"):
            ls = getattr(holder, attr, None)
            if ls is not None and hasattr(ls, "params"):
                return ls
    raise ValueError(f"{who} needs {trainer}'s LearnerState (train with warm_start=True), got {type(obj).__name__}")
