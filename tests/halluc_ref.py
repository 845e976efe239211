"""Test-tree restatement of hallucinated control (include/mbpo_hip.h, "hallucinated control"), built on the oracle.

The policy's action is [u (u_env) | eta (x)].  The dynamics read [x, u] only; with mu_e,c member e's mean head at (x, u):
    m_c  = (sum_e mu_e,c) / E             e ascending (oracle.systems.EnsembleSystem's 'mean' sum)
    q_c  = sum_e (mu_e,c - m_c)^2         e ascending
    sd_c = sqrt(q_c / E)                  population std
    x'_c = base_c + m_c + beta_c * sd_c * eta_c
The reward is evaluated at the pre-step (x, u) and never sees eta: the system's reward_fn, or with learned_reward the mean over
members of the reward head (column 2x of a 2x + 2 member output).

oracle.rollout.rollout / env_step are duck-typed on `system.step` and drive this class unchanged: the policy they run has
2 * (u_env + x) outputs and `step` receives the whole action.
"""
from __future__ import annotations

import torch

from oracle import nets
from oracle import systems as osys


class HallucinatedEnsembleSystem(osys.EnsembleSystem):
    """u_dim is the action width u_env + x_dim (what oracle.rollout's rows carry); u_env is what the dynamics read."""

    def __init__(self, params, dims, n_members, x_dim, u_env, beta, learned_reward=False, **kw):
        assert dims[0] == x_dim + u_env and kw.get("mode", "mean") == "mean"
        assert not learned_reward or dims[-1] == 2 * x_dim + 2
        super().__init__(params, dims, n_members, x_dim, u_env + x_dim, **kw)
        self.u_env, self.learned_reward = u_env, learned_reward
        b = torch.as_tensor(beta, dtype=params.dtype).reshape(-1)
        self.beta = b.expand(x_dim).clone() if b.numel() == 1 else b.clone()
        assert self.beta.numel() == x_dim

    def double(self) -> "HallucinatedEnsembleSystem":
        """The same system in fp64 (parameters and beta converted; reward_fn is dtype-agnostic)."""
        return HallucinatedEnsembleSystem(self.params.double(), self.dims, self.E, self.x_dim, self.u_env, self.beta.double(),
                                          learned_reward=self.learned_reward, act=self.act, predict_delta=self.predict_delta,
                                          min_std=self.min_std, reward_fn=self.reward_fn)

    def spread(self, x, u):
        """(m, sd, y): the members' mean, their population std, and the raw member outputs at (x, u), in x's dtype."""
        X = self.x_dim
        y = nets.ensemble_forward(self.params.to(x.dtype), self.dims, self.E, torch.cat([x, u], dim=1), self.act)
        acc = torch.zeros_like(x)
        for e in range(self.E):
            acc = acc + y[e, :, :X]
        m = acc / self.E
        q = torch.zeros_like(x)
        for e in range(self.E):
            d = y[e, :, :X] - m
            q = q + d * d
        return m, torch.sqrt(q / self.E), y

    def step(self, x, a, env_index=None, **_):
        X, UE = self.x_dim, self.u_env
        u, eta = a[:, :UE], a[:, UE:UE + X]
        m, sd, y = self.spread(x, u)
        base = x if self.predict_delta else torch.zeros_like(x)
        xn = base + m + self.beta.to(x.dtype) * sd * eta
        if self.learned_reward:
            racc = torch.zeros(x.shape[0], dtype=x.dtype)
            for e in range(self.E):
                racc = racc + y[e, :, 2 * X]
            return xn, racc / self.E
        return xn, self.reward_fn(x, u)
