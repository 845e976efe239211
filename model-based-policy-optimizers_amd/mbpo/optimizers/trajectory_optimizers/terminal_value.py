"""TerminalValue — a learned critic at the end of iCEM's horizon (include/mbpo_hip.h "terminal values").  Not in the reference, whose iCEM
objective is the sum of the horizon's rewards; build-defined, the standard remedy for a short horizon (POLO, LOOP, TD-MPC):

    J_i = sum_{t<H} r_t(i) + weight * V(x_H(i))

V is either a state value (kind V: the minimum over one or two networks [x] -> [1] — BPTT's twin target critic, PPO's value network with
n_critics=1) or SAC's pair (kind Q: min(Q1, Q2)([n(x) | tanh(loc(pi(n(x))))]), the policy's mode action).  n(x) = (x - mean) / std with
the trainer's normaliser, the identity without one.  `iCemTO(..., terminal_value=tv)` issues one launch of mbpo_terminal_value_eval per
iteration, which adds the bonus into the last step's rewards the update launch reads; nothing else changes.

There is no entropy term, no discounting and no reward un-scaling inside: `weight` carries them.  Typical values: gamma^H /
reward_scaling for SAC's critics (they estimate the discounted sum of SCALED rewards), r_std * gamma^H for BPTT's critic (it estimates
normalised rewards).  A constant shift of V changes no ranking and is not offered.  Out of scope: an entropy term, per-step
discounting of iCEM's sum, BPTT or SAC consuming a TerminalValue, networks wider than 256.  (The actor half of the same methods —
the policy's rollouts among the candidates — is PolicyPrior, policy_prior.py.)
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from mbpo import _hip, ops

from mbpo.optimizers.trajectory_optimizers._net_checks import (KERNEL_WIDTHS, _check_dims, _check_flat, _learner_state_of,  # noqa: F401
                                                               _n_params)


class TerminalValue:
    """TerminalValue(x_dim, critic_params, critic_dims, n_critics=2, activation="swish", policy_params=None, policy_dims=None,
    policy_activation="swish", norm_mean=None, norm_std=None, weight=1.0).

    critic_params: flat float32 [n_critics * params(critic_dims)], the networks one after the other (W[in][out] row-major, then b, per
    layer).  Without a policy: kind V, critic_dims [x_dim, hidden..., 1], n_critics 1 or 2.  With policy_params / policy_dims
    [x_dim, hidden..., 2 A]: kind Q, critic_dims [x_dim + A, hidden..., 1], n_critics 2; A is the policy's action width (on an
    optimistic system u_dim + x_dim).  Hidden layers of a network share one width in 64 / 128 / 256.

    All tensors are kept BY REFERENCE and read by the launch, not before: after more training refresh them in place
    (`tv.critic_params.copy_(...)`), no new object is needed.  `weight` is a plain attribute."""

    def __init__(self, x_dim: int, critic_params: torch.Tensor, critic_dims: Sequence[int], n_critics: int = 2, activation: str = "swish",
                 policy_params: Optional[torch.Tensor] = None, policy_dims: Optional[Sequence[int]] = None,
                 policy_activation: str = "swish", norm_mean: Optional[torch.Tensor] = None, norm_std: Optional[torch.Tensor] = None,
                 weight: float = 1.0):
        self.x_dim = int(x_dim)
        if self.x_dim < 1:
            raise ValueError(f"x_dim must be >= 1, got {x_dim}")
        self.n_critics = int(n_critics)
        if self.n_critics not in (1, 2):
            raise ValueError(f"n_critics must be 1 or 2, got {n_critics}")
        for name, act in (("activation", activation), ("policy_activation", policy_activation)):
            if act not in _hip.ACT_IDS:
                raise ValueError(f"{name} must be one of {sorted(_hip.ACT_IDS)}, got {act!r}")
        if (policy_params is None) != (policy_dims is None):
            raise ValueError("policy_params and policy_dims must both be given (kind Q) or both be None (kind V)")
        if policy_dims is not None:
            pd = [int(v) for v in policy_dims]
            if len(pd) < 2 or pd[-1] < 2 or pd[-1] % 2:
                raise ValueError(f"policy_dims must end in 2 * action_dim outputs, got {pd}")
            self.action_dim = pd[-1] // 2
            if self.action_dim > 64:
                raise ValueError(f"policy_dims: action_dim {self.action_dim} > 64 is not built")
            self.policy_dims = _check_dims("policy_dims", pd, self.x_dim, 2 * self.action_dim, "x_dim -> 2 * action_dim")
            self.policy_params = _check_flat("policy_params", policy_params, _n_params(self.policy_dims))
            if self.n_critics != 2:
                raise ValueError(f"n_critics must be 2 with a policy (kind Q: SAC's twin critics), got {n_critics}")
        else:
            self.action_dim, self.policy_dims, self.policy_params = 0, None, None
        what = "x_dim + action_dim -> 1" if self.action_dim else "x_dim -> 1"
        self.critic_dims = _check_dims("critic_dims", critic_dims, self.x_dim + self.action_dim, 1, what)
        self.critic_params = _check_flat("critic_params", critic_params, self.n_critics * _n_params(self.critic_dims))
        if (norm_mean is None) != (norm_std is None):
            raise ValueError("norm_mean and norm_std must both be given or both be None")
        self.norm_mean = None if norm_mean is None else _check_flat("norm_mean", norm_mean, self.x_dim)
        self.norm_std = None if norm_std is None else _check_flat("norm_std", norm_std, self.x_dim)
        dev = self.critic_params.device
        for name, t in (("policy_params", self.policy_params), ("norm_mean", self.norm_mean), ("norm_std", self.norm_std)):
            if t is not None and t.device != dev:
                raise ValueError(f"{name} lies on {t.device}, critic_params on {dev}")
        self.activation, self.policy_activation = activation, policy_activation
        self.weight = float(weight)

    # -- from a trainer's state ----------------------------------------------------------------------------------------
    @classmethod
    def from_sac(cls, learner_state, policy_dims: Optional[Sequence[int]] = None, q_dims: Optional[Sequence[int]] = None,
                 activation: str = "swish", policy_activation: Optional[str] = None, weight: float = 1.0,
                 target: bool = True) -> "TerminalValue":
        """From SAC's LearnerState (`SACOptimizer(..., warm_start=True)`, `SAC.export_learner_state()`): the policy from `params`, the
        twin critics from `target_q` (target=True) or from `params`, mean / std from the normaliser vector [count | mean | summed
        variance | std] when the learner normalises observations.  `learner_state` may also be the BraxState that carries one, or the
        SACOptimizer / SAC trainer itself (the trainer's last learner state is read).  policy_dims / q_dims: the KERNEL dims (hidden layers padded to the kernel width), read off the
        state's signature when None.  The tensors are views of the state's: a state refreshed in place is honoured."""
        ls = _learner_state_of(learner_state)
        sig = getattr(ls, "signature", None) or {}
        if sig.get("trainer", "SAC") != "SAC":
            raise ValueError(f"from_sac needs SAC's learner state, this one is {sig.get('trainer')!r}'s")
        policy_dims = [int(v) for v in (policy_dims if policy_dims is not None else sig.get("policy_dims") or ())]
        q_dims = [int(v) for v in (q_dims if q_dims is not None else sig.get("q_dims") or ())]
        if len(policy_dims) < 2 or len(q_dims) < 2:
            raise ValueError("policy_dims and q_dims are needed (the learner state carries no signature to read them from)")
        X, P, Q = policy_dims[0], _n_params(policy_dims), _n_params(q_dims)
        params = _check_flat("learner_state.params", ls.params, P + 2 * Q + 1)
        pol = params[:P]
        if target:
            if ls.target_q is None:
                raise ValueError("learner_state.target_q is None (target=False reads the online critics from params)")
            q = _check_flat("learner_state.target_q", ls.target_q, 2 * Q)
        else:
            q = params[P:P + 2 * Q]
        mean = std = None
        if sig.get("normalize_observations", True):
            vec = _check_flat("learner_state.normalizer", ls.normalizer, 1 + 3 * X)
            mean, std = vec[1:1 + X], vec[1 + 2 * X:1 + 3 * X]
        return cls(X, q, q_dims, n_critics=2, activation=activation, policy_params=pol, policy_dims=policy_dims,
                   policy_activation=activation if policy_activation is None else policy_activation, norm_mean=mean, norm_std=std,
                   weight=weight)

    @classmethod
    def from_bptt(cls, opt_state, critic_dims: Sequence[int], activation: str = "swish", weight: float = 1.0) -> "TerminalValue":
        """From a BPTTState: the twin target critic [critic_1 | critic_2] and the state normaliser (BPTT always normalises: a fresh
        normaliser is mean 0, std 1).  critic_dims: the KERNEL dims, `BPTTOptimizer.critic_dims`."""
        critic_dims = [int(v) for v in critic_dims]
        ns = opt_state.state_normalizer_state
        return cls(critic_dims[0], opt_state.target_critic_params, critic_dims, n_critics=2, activation=activation,
                   norm_mean=ns.mean, norm_std=ns.std, weight=weight)

    # -- use -----------------------------------------------------------------------------------------------------------
    @property
    def kind(self) -> str:
        return "Q" if self.action_dim else "V"

    def check_system(self, system) -> None:
        """The widths against a system's: x_dim, and kind Q's action width against system.action_dim (on an optimistic system u + x:
        the critics were trained on [u | eta])."""
        if system is None:
            return
        if self.x_dim != system.x_dim:
            raise ValueError(f"terminal_value is built at x_dim {self.x_dim}, the system has x_dim {system.x_dim}")
        if self.action_dim and self.action_dim != system.action_dim:
            raise ValueError(f"terminal_value is a kind-Q value at action_dim {self.action_dim}, the system has action_dim "
                             f"{system.action_dim} (u_dim {system.u_dim}; an optimistic system acts in u_dim + x_dim)")

    def eval_into(self, x: torch.Tensor, x_offset: int, x_stride: int, out: torch.Tensor, out_offset: int, out_stride: int, n: int,
                  accumulate: bool) -> torch.Tensor:
        """One launch of mbpo_terminal_value_eval on states and outputs addressed by (tensor, float offset, float stride)."""
        return ops.terminal_value_eval(
            x_dim=self.x_dim, action_dim=self.action_dim, critic_params=self.critic_params, critic_dims=self.critic_dims,
            n_critics=self.n_critics, activation=self.activation, policy_params=self.policy_params, policy_dims=self.policy_dims,
            policy_activation=self.policy_activation, norm_mean=self.norm_mean, norm_std=self.norm_std, x=x, x_offset=x_offset,
            x_stride=x_stride, out=out, out_offset=out_offset, out_stride=out_stride, n=n, weight=self.weight, accumulate=accumulate)

    def __call__(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[n] = weight * V(x), x [n, x_dim] (or [x_dim]); -inf where a state is not finite."""
        if x.dim() == 1:
            x = x.reshape(1, -1)
        if x.dim() != 2 or x.shape[1] != self.x_dim:
            raise ValueError(f"x must be [n, {self.x_dim}], got {tuple(x.shape)}")
        x = x.to(torch.float32).contiguous()
        n = x.shape[0]
        if out is None:
            out = torch.empty(n, device=x.device, dtype=torch.float32)
        elif out.shape != (n,):
            raise ValueError(f"out must be [{n}]")
        return self.eval_into(x, 0, self.x_dim, out, 0, 1, n, accumulate=False)

    def __repr__(self):
        return (f"TerminalValue(kind {self.kind}, x_dim {self.x_dim}, action_dim {self.action_dim}, critic {self.critic_dims} x "
                f"{self.n_critics}, weight {self.weight})")
