"""Test-tree restatement of the term reward (MBPO_REWARD_TERMS, include/mbpo_hip.h "term rewards"), built on the oracle.

    z   = [x | u | x_next],   x_next = x where any component of the step's next state is not finite
    s_g = sum_k c_k f_k(z[i_k] - t_k),   r = bias + sum_g w_g L_g(s_g)

`reward` evaluates a table given as plain data (tests/term_reward_cases.py) in the dtype of its inputs: in fp64 it is the reference, in
fp32 it is the kernel's order — terms and groups in table order, one accumulator each, every product and sum rounded on its own (torch
on the host fuses nothing).  The systems below put that reward behind oracle.systems.EnsembleSystem and its test-tree variants, so that
oracle/rollout.py, tests/time_adaptive_ref.py and oracle/bptt.py drive them unchanged.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import nets
from oracle import systems as osys

import halluc_ref as href

FN = {"identity": lambda v: v, "square": lambda v: v * v, "abs": torch.abs, "relu": torch.relu, "cos": torch.cos, "sin": torch.sin}
LINK = {"identity": lambda s: s, "sqrt": lambda s: torch.sqrt(torch.clamp(s, min=0.0)), "exp": torch.exp, "tanh": torch.tanh}


def next_state_columns(x: torch.Tensor, x_next: torch.Tensor) -> torch.Tensor:
    """The non-finite rule: rows of x_next with a non-finite component read x."""
    return torch.where(torch.isfinite(x_next).all(dim=1, keepdim=True), x_next, x)


def reward(table, x: torch.Tensor, u: torch.Tensor, x_next: torch.Tensor | None, record: dict | None = None) -> torch.Tensor:
    """[n] in x's dtype.  u: the control columns the dynamics see.  record: filled with the largest |term| and |s_g| met."""
    X, U, bias, groups = table
    assert x.shape[1] == X and u.shape[1] == U
    part = {"x": x, "u": u, "x_next": x if x_next is None else next_state_columns(x, x_next)}
    c = lambda v: torch.tensor(v, dtype=torch.float32).to(x.dtype)      # the table's numbers are fp32 values in every dtype
    r = torch.full((x.shape[0],), 0.0, dtype=x.dtype) + c(bias)
    for w, link, terms in groups:
        s = torch.zeros(x.shape[0], dtype=x.dtype)
        for on, idx, fn, coef, off in terms:
            term = c(coef) * FN[fn](part[on][:, idx] - c(off))
            s = s + term
            if record is not None:
                record["term"] = max(record.get("term", 0.0), float(term.abs().max()))
        if record is not None:
            record["s"] = max(record.get("s", 0.0), float(s.abs().max()))
        r = r + c(w) * LINK[link](s)
    return r


def reward_sqrt_masked(table, x, u):
    """`reward` for autograd (tables of x / u terms): the sqrt link masked so that its gradient is 0 at s <= 0, as the kernels define it."""
    X, U, bias, groups = table
    part = {"x": x, "u": u}
    r = torch.zeros(x.shape[0], dtype=x.dtype) + bias
    for w, link, terms in groups:
        s = torch.zeros(x.shape[0], dtype=x.dtype)
        for on, idx, fn, coef, off in terms:
            s = s + coef * FN[fn](part[on][:, idx] - off)
        if link == "sqrt":
            pos = s > 0
            ls = torch.where(pos, torch.sqrt(torch.where(pos, s, torch.ones_like(s))), torch.zeros_like(s))
        else:
            ls = LINK[link](s)
        r = r + w * ls
    return r


def quadratic(x, u, target, q, r):
    """oracle.systems.quadratic_reward from python lists, in x's dtype."""
    c = lambda v: torch.tensor(v, dtype=torch.float32).to(x.dtype)
    return osys.quadratic_reward(x, u, c(target), c(q), c(r))


class TermEnsembleSystem(osys.EnsembleSystem):
    """oracle.systems.EnsembleSystem whose reward is the table on (x, u, x'), x' the step's own next state."""

    def __init__(self, table, params, dims, n_members, **kw):
        super().__init__(params, dims, n_members, table[0], table[1], reward_fn=lambda x, u: torch.zeros(x.shape[0], dtype=x.dtype), **kw)
        self.table = table

    def double(self):
        return TermEnsembleSystem(self.table, self.params.double(), self.dims, self.E, act=self.act, mode=self.mode,
                                  predict_delta=self.predict_delta, sample_noise=self.sample_noise, min_std=self.min_std)

    def step(self, x, u, member_idx=None, model_noise=None, env_index=None):
        xn, _ = super().step(x, u, member_idx=member_idx, model_noise=model_noise, env_index=env_index)
        return xn, reward(self.table, x, u, xn)


class TermHallucinatedSystem(href.HallucinatedEnsembleSystem):
    """tests/halluc_ref.py's system (its reward is a function of (x, u) only) with the table on (x, u, x'); eta never enters z."""

    def __init__(self, table, params, dims, n_members, beta, **kw):
        super().__init__(params, dims, n_members, table[0], table[1], beta, reward_fn=None, **kw)
        self.table = table

    def double(self):
        return TermHallucinatedSystem(self.table, self.params.double(), self.dims, self.E, self.beta.double(), act=self.act,
                                      predict_delta=self.predict_delta, min_std=self.min_std)

    def step(self, x, a, env_index=None, **_):
        X, UE = self.x_dim, self.u_env
        u, eta = a[:, :UE], a[:, UE:UE + X]
        m, sd, _y = self.spread(x, u)
        xn = (x if self.predict_delta else torch.zeros_like(x)) + m + self.beta.to(x.dtype) * sd * eta
        return xn, reward(self.table, x, u, xn)


class TorchTermSystem:
    """Differentiable 'mean' twin for oracle.bptt.actor_grads (tables of x / u terms)."""

    def __init__(self, table, params, dims, E, predict_delta=True):
        self.table, self.params, self.dims, self.E, self.predict_delta = table, params, list(dims), E, predict_delta

    def step(self, x, u):
        X = self.table[0]
        y = nets.ensemble_forward(self.params, self.dims, self.E, torch.cat([x, u], dim=1))
        acc = torch.zeros_like(x)
        for e in range(self.E):
            acc = acc + y[e, :, :X]
        return (x if self.predict_delta else torch.zeros_like(x)) + acc / self.E, reward_sqrt_masked(self.table, x, u)
