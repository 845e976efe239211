"""Test-tree restatement of the learned reward (MBPO_REWARD_LEARNED, include/mbpo_hip.h), built on the oracle.

A reward-predicting ensemble's member output is [mu_x (X) | raw_x (X) | mu_r | raw_r] (dout = 2X + 2).  The reward of a step is the
reward head at the pre-step (x, u):
    'mean'           r = mean_e mu_r,e
    'ts1' / 'tsinf'  r = mu_r,m, m the member the state takes at that (env, step)
The state follows oracle.systems.EnsembleSystem unchanged; the reward carries no noise.  The fit adds
    0.5 ((r - mu_r) / sigma_r)^2 + log sigma_r,   sigma_r = softplus(raw_r) + min_std,   r = row[reward_off]
to every member's Gaussian NLL (oracle.ensemble.member_nll).
"""
from __future__ import annotations

from typing import Sequence

import torch
import torch.nn.functional as F

from oracle import ensemble as oens
from oracle import nets
from oracle import systems as osys


class LearnedRewardEnsembleSystem(osys.EnsembleSystem):
    """oracle.systems.EnsembleSystem whose reward is its own reward head (for oracle.rollout.rollout)."""

    def __init__(self, params, dims, n_members, x_dim, u_dim, **kw):
        assert dims[-1] == 2 * x_dim + 2
        # (the base step's reward is replaced below)
        super().__init__(params, dims, n_members, x_dim, u_dim, reward_fn=lambda x, u: torch.zeros(x.shape[0], dtype=x.dtype), **kw)

    def step(self, x, u, member_idx=None, model_noise=None, env_index=None):
        xn, _ = super().step(x, u, member_idx=member_idx, model_noise=model_noise, env_index=env_index)
        return xn, self.learned_reward(x, u, member_idx, env_index)

    def learned_reward(self, x, u, member_idx=None, env_index=None):
        X = self.x_dim
        y = nets.ensemble_forward(self.params, self.dims, self.E, torch.cat([x, u], dim=1), self.act)
        if self.mode == "mean":
            acc = torch.zeros(x.shape[0], dtype=x.dtype)
            for e in range(self.E):
                acc = acc + y[e, :, 2 * X]
            return acc / self.E
        if self.mode == "tsinf":
            member_idx = env_index % self.E
        return y[member_idx.long(), torch.arange(x.shape[0]), 2 * X]


class TorchLearnedRewardSystem:
    """Differentiable twin for oracle.bptt.actor_grads: 'mean' (members None), or trajectory sampling with the members [n, H] and
    optional state noise [n, H, X] of each horizon step (the pathwise gradient through the selected member)."""

    def __init__(self, params, dims, E, X, U, predict_delta=True, min_std=1e-3, members=None, eps=None):
        self.params, self.dims, self.E, self.X, self.U = params, list(dims), E, X, U
        self.predict_delta, self.min_std, self.members, self.eps = predict_delta, min_std, members, eps
        self.t = 0

    def set_draws(self, members, eps):
        """The draws of the next horizon walk (members None: 'mean'); rewinds the step counter."""
        self.members, self.eps, self.t = members, eps, 0
        return self

    def step(self, x, u):
        X, n = self.X, x.shape[0]
        y = nets.ensemble_forward(self.params, self.dims, self.E, torch.cat([x, u], dim=1))
        base = x if self.predict_delta else torch.zeros_like(x)
        if self.members is None:
            acc, racc = torch.zeros_like(x), torch.zeros(n, dtype=x.dtype)
            for e in range(self.E):
                acc = acc + y[e, :, :X]
                racc = racc + y[e, :, 2 * X]
            xn, r = base + acc / self.E, racc / self.E
        else:
            ym = y[self.members[:, self.t].long(), torch.arange(n)]
            xn, r = base + ym[:, :X], ym[:, 2 * X]
            if self.eps is not None:
                xn = xn + (F.softplus(ym[:, X:2 * X]) + self.min_std) * self.eps[:, self.t].to(x.dtype)
        self.t += 1
        return xn, r


def member_nll(params_e, dims, xu, x, x_next, r, predict_delta=True, min_std=1e-3, act="swish"):
    """oracle.ensemble.member_nll plus the reward term (r: [B] targets, or None for the state terms alone)."""
    X = x.shape[1]
    out = nets.mlp_forward(params_e, dims, xu, act)
    mean = out[:, :X] + (x if predict_delta else 0.0)
    sigma = F.softplus(out[:, X:2 * X]) + min_std
    q = (x_next - mean) / sigma
    per_row = (0.5 * q * q + torch.log(sigma)).sum(dim=1)
    if r is not None:
        sr = F.softplus(out[:, 2 * X + 1]) + min_std
        qr = (r - out[:, 2 * X]) / sr
        per_row = per_row + 0.5 * qr * qr + torch.log(sr)
    return per_row.mean()


def nll_grads(params: torch.Tensor, dims: Sequence[int], n_members: int, rows: torch.Tensor, idx: torch.Tensor, x_dim: int, u_dim: int,
              predict_delta: bool = True, min_std: float = 1e-3, reward_off: int | None = None, next_obs_off: int | None = None):
    """Like oracle.ensemble.nll_grads, with the reward head fitted to rows[:, reward_off] (None: no reward term)."""
    P = nets.n_params(dims)
    noff = x_dim + u_dim + 2 if next_obs_off is None else next_obs_off
    grads, losses = [], []
    for e in range(n_members):
        p = params[e * P:(e + 1) * P].clone().requires_grad_(True)
        b = rows[idx[e]]
        r = b[:, reward_off] if reward_off is not None else None
        loss = member_nll(p, dims, b[:, :x_dim + u_dim], b[:, :x_dim], b[:, noff:noff + x_dim], r, predict_delta, min_std)
        loss.backward()
        grads.append(p.grad.detach())
        losses.append(loss.detach())
    return torch.cat(grads), torch.stack(losses)


def reward_head_params(params: torch.Tensor, dims: Sequence[int], n_members: int) -> torch.Tensor:
    """The same members with the reward columns cut: [x+u] -> ... -> [2x] (flat layout of oracle.nets: W [in, out] then b)."""
    P = nets.n_params(dims)
    out = []
    for e in range(n_members):
        layers = nets.unflatten(params[e * P:(e + 1) * P], dims)
        for i, (w, b) in enumerate(layers):
            if i == len(layers) - 1:
                w, b = w[:, :dims[-1] - 2], b[:dims[-1] - 2]
            out += [w.reshape(-1), b]
    return torch.cat(out)


__all__ = ["LearnedRewardEnsembleSystem", "TorchLearnedRewardSystem", "member_nll", "nll_grads", "reward_head_params", "oens"]
