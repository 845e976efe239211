"""Torch restatement of include/mbpo_hip.h "terminal values", in the dtype of its input, built on oracle.nets alone (mlp_forward,
q_forward, mode, normalize).  Test infrastructure: the definition is the header text.

    kind V   v = min_k V_k(n(x))                               k < n_critics
    kind Q   a = tanh(loc(pi(n(x))));  v = min(Q1, Q2)([n(x) | a])
    out      = weight * v, -inf where a component of x is not finite
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from oracle import nets


def v_hat(x: torch.Tensor, critic: torch.Tensor, critic_dims: Sequence[int], n_critics: int, act: str = "swish",
          policy: Optional[torch.Tensor] = None, policy_dims: Optional[Sequence[int]] = None, policy_act: Optional[str] = None,
          mean: Optional[torch.Tensor] = None, std: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[n]: the value of every state of x [n, x_dim], parameters cast to x's dtype."""
    dt = x.dtype
    c = lambda t: None if t is None else t.to(dt)
    xn = nets.normalize(x, c(mean), c(std))
    p = nets.n_params(critic_dims)
    if policy is None:
        vs = torch.cat([nets.mlp_forward(c(critic)[k * p:(k + 1) * p], critic_dims, xn, act) for k in range(n_critics)], dim=-1)
    else:
        a = nets.mode(nets.mlp_forward(c(policy), policy_dims, xn, policy_act or act))
        vs = nets.q_forward(c(critic), critic_dims, xn, a, act, n_critics)
    return vs.min(dim=-1).values


def bonus(x: torch.Tensor, weight: float, *args, **kwargs) -> torch.Tensor:
    """weight * v_hat, -inf on rows with a non-finite component (those rows are evaluated on zeros, so that nothing else sees them)."""
    bad = ~torch.isfinite(x).all(dim=-1)
    v = v_hat(torch.where(bad[:, None], torch.zeros_like(x), x), *args, **kwargs)
    w = torch.tensor(weight, dtype=torch.float32).to(x.dtype)
    return torch.where(bad, torch.full_like(v, float("-inf")), w * v)
