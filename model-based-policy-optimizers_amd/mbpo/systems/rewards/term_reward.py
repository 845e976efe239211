"""TermReward — a known closed-form reward written as data (MBPO_REWARD_TERMS; include/mbpo_hip.h "term rewards").  Not in the reference.

    z   = [x (x_dim) | u (u_dim) | x_next (x_dim)]
    s_g = sum_{k in group g} coef_k * fn_k(z[i_k] - offset_k)        fn: identity, square, abs, relu, cos, sin
    r   = bias + sum_g weight_g * link_g(s_g)                        link: identity, sqrt (of max(s, 0)), exp, tanh

Linear, quadratic and L1 costs, Euclidean distances (square terms under a sqrt link), exp(-sum q d^2) tolerances, barrier-style
penalties.  There is no product of two different columns.  The fused tile rollouts evaluate the table inside the kernel, on every inner
step's (x, u, x_next); where the next state is not finite the x_next columns read x, so a diverged row keeps a finite reward.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import torch

from mbpo import _hip
from mbpo.systems.dynamics.base_dynamics import Normal
from mbpo.systems.rewards.base_rewards import Reward

_PARTS = ("x", "u", "x_next")


@dataclass(frozen=True)
class Term:
    """coef * fn(part[index] - offset); on: 'x' | 'u' | 'x_next'."""
    on: str
    index: int
    fn: str = "identity"
    coef: float = 1.0
    offset: float = 0.0


@dataclass(frozen=True)
class Group:
    """weight * link(sum of the terms)."""
    terms: Tuple[Term, ...]
    weight: float = 1.0
    link: str = "identity"

    def __post_init__(self):
        object.__setattr__(self, "terms", tuple(self.terms))


@dataclass(frozen=True)
class TermRewardParams:
    """The table: validated when it is built, so `replace` cannot produce one the kernels would read differently from what it says."""
    x_dim: int
    u_dim: int
    bias: float = 0.0
    groups: Tuple[Group, ...] = ()

    def __post_init__(self):
        object.__setattr__(self, "groups", tuple(self.groups))
        if len(self.groups) > _hip.REWARD_TERMS_MAX_GROUPS:
            raise ValueError(f"{len(self.groups)} groups: a term table holds at most {_hip.REWARD_TERMS_MAX_GROUPS} groups")
        width = {"x": self.x_dim, "u": self.u_dim, "x_next": self.x_dim}
        n_terms = 0
        for gi, g in enumerate(self.groups):
            if not isinstance(g, Group):
                raise ValueError(f"group {gi}: expected a Group, got {type(g).__name__}")
            if g.link not in _hip.TERM_LINK_IDS:
                raise ValueError(f"group {gi}: unknown link {g.link!r} (one of {sorted(_hip.TERM_LINK_IDS)})")
            if len(g.terms) == 0:
                raise ValueError(f"group {gi} is empty")
            for ti, t in enumerate(g.terms):
                if not isinstance(t, Term):
                    raise ValueError(f"group {gi} term {ti}: expected a Term, got {type(t).__name__}")
                if t.on not in _PARTS:
                    raise ValueError(f"group {gi} term {ti}: unknown part {t.on!r} (one of {list(_PARTS)})")
                if t.fn not in _hip.TERM_FN_IDS:
                    raise ValueError(f"group {gi} term {ti}: unknown fn {t.fn!r} (one of {sorted(_hip.TERM_FN_IDS)})")
                if not 0 <= int(t.index) < width[t.on]:
                    raise ValueError(f"group {gi} term {ti}: index {t.index} out of range for {t.on!r} (width {width[t.on]})")
            n_terms += len(g.terms)
        if n_terms > _hip.REWARD_TERMS_MAX_TERMS:
            raise ValueError(f"{n_terms} terms: a term table holds at most {_hip.REWARD_TERMS_MAX_TERMS} terms")

    def replace(self, **kw):
        return dataclasses.replace(self, **kw)

    @property
    def has_next_state_terms(self) -> bool:
        return any(t.on == "x_next" for g in self.groups for t in g.terms)

    def z_index(self, t: Term) -> int:
        return int(t.index) + {"x": 0, "u": self.x_dim, "x_next": self.x_dim + self.u_dim}[t.on]

    def vector(self) -> torch.Tensor:
        """The packed fp32 table, always REWARD_TERMS_FLOATS long: header [n_groups, n_terms, bias, 0], 16 group records
        [weight, link, first_term, n_terms], 128 term records [z_index, fn, coef, offset]."""
        v = torch.zeros(_hip.REWARD_TERMS_FLOATS, dtype=torch.float32)
        g_off, t_off = 4, 4 + 4 * _hip.REWARD_TERMS_MAX_GROUPS
        k = 0
        for gi, g in enumerate(self.groups):
            v[g_off + 4 * gi:g_off + 4 * gi + 4] = torch.tensor([g.weight, _hip.TERM_LINK_IDS[g.link], k, len(g.terms)], dtype=torch.float32)
            for t in g.terms:
                v[t_off + 4 * k:t_off + 4 * k + 4] = torch.tensor([self.z_index(t), _hip.TERM_FN_IDS[t.fn], t.coef, t.offset],
                                                                  dtype=torch.float32)
                k += 1
        v[0], v[1], v[2] = len(self.groups), k, self.bias
        return v


_FN = {"identity": lambda v: v, "square": lambda v: v * v, "abs": torch.abs, "relu": torch.relu, "cos": torch.cos, "sin": torch.sin}
_LINK = {"identity": lambda s: s, "sqrt": lambda s: torch.sqrt(torch.clamp(s, min=0.0)), "exp": torch.exp, "tanh": torch.tanh}


def term_reward_torch(params: TermRewardParams, x: torch.Tensor, u: torch.Tensor, x_next: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The function in torch, in the table's order and the inputs' dtype, differentiable (abs and relu take torch's gradient at 0, the
    sqrt link is masked so that its gradient is 0 at s <= 0): the wide BPTT path's reward.
    x [..., x_dim], u [..., >= u_dim] (further action columns are ignored), x_next [..., x_dim] or None without next-state terms."""
    if x_next is None and params.has_next_state_terms:
        raise ValueError("this table has next-state terms: x_next is needed")
    if x_next is not None:
        ok = torch.isfinite(x_next).all(dim=-1, keepdim=True)
        x_next = torch.where(ok, x_next, x)            # the non-finite rule
    part = {"x": x, "u": u, "x_next": x_next}
    r = torch.full(x.shape[:-1], float(params.bias), dtype=x.dtype, device=x.device)
    for g in params.groups:
        s = torch.zeros_like(r)
        for t in g.terms:
            s = s + t.coef * _FN[t.fn](part[t.on][..., int(t.index)] - t.offset)
        if g.link == "sqrt":
            pos = s > 0
            ls = torch.where(pos, torch.sqrt(torch.where(pos, s, torch.ones_like(s))), torch.zeros_like(s))      # gradient 0 at s <= 0
        else:
            ls = _LINK[g.link](s)
        r = r + g.weight * ls
    return r


class TermReward(Reward[TermRewardParams]):
    """TermReward(x_dim, u_dim, bias=0.0, groups=[Group([Term("x", 0, "square", coef=-1.0)]), ...]).  u_dim is the control width the
    dynamics see: a hallucinated eta or a time-adaptive tau never enters the reward."""

    def __init__(self, x_dim: int, u_dim: int, bias: float = 0.0, groups: Sequence[Group] = ()):
        super().__init__(x_dim, u_dim)
        self._default = TermRewardParams(int(x_dim), int(u_dim), float(bias), tuple(groups))
        self._vec = {}                # (table, device) -> device vector: a captured step replays the pointer it recorded

    @classmethod
    def from_quadratic(cls, target, q, r) -> "TermReward":
        """The table equal to QuadraticReward(target, q, r): -(sum_d q_d (x_d - target_d)^2) - sum_d r_d u_d^2, as two groups of square
        terms of weight -1 (the sums in the quadratic kernel's order, each product rounded on its own)."""
        target, q, r = [float(v) for v in target], [float(v) for v in q], [float(v) for v in r]
        if len(target) != len(q):
            raise ValueError("target and q must both hold x_dim values")
        gx = Group([Term("x", c, "square", q[c], target[c]) for c in range(len(q))], weight=-1.0)
        gu = Group([Term("u", d, "square", r[d], 0.0) for d in range(len(r))], weight=-1.0)
        return cls(len(q), len(r), 0.0, [gx, gu])

    @property
    def has_next_state_terms(self) -> bool:
        return self._default.has_next_state_terms

    def init_params(self, key: int) -> TermRewardParams:
        return self._default

    def _check(self, p: TermRewardParams) -> TermRewardParams:
        if not isinstance(p, TermRewardParams) or (p.x_dim, p.u_dim) != (self.x_dim, self.u_dim):
            raise ValueError(f"these reward parameters are not a term table at x_dim {self.x_dim}, u_dim {self.u_dim}")
        return p

    def kernel_spec(self, reward_params, device):
        p = self._check(reward_params)
        k = (p, str(device))
        if k not in self._vec:
            self._vec[k] = p.vector().to(device).contiguous()
        return _hip.REWARD_TERMS, self._vec[k]

    def torch_reward(self, x, u, reward_params, x_next=None) -> torch.Tensor:
        return term_reward_torch(self._check(reward_params), x, u, x_next)

    def __call__(self, x, u, reward_params, x_next=None):
        """Host evaluation through mbpo_reward_eval (the rollout kernels' own device function): Normal(reward, 0)."""
        from mbpo import ops
        from mbpo.systems.base_systems import _device_of
        p = self._check(reward_params)
        if x_next is None and p.has_next_state_terms:
            raise ValueError("this table has next-state terms: pass x_next")
        dev = _device_of(x)
        single = x.dim() == 1
        xb = x.reshape(-1, self.x_dim).to(dev, torch.float32).contiguous()
        ub = u.reshape(xb.shape[0], -1)[:, :self.u_dim].to(dev, torch.float32).contiguous()
        nb = None if x_next is None else x_next.reshape(-1, self.x_dim).to(dev, torch.float32).contiguous()
        r = ops.reward_eval(_hip.REWARD_TERMS, self.kernel_spec(p, dev)[1], xb, ub, nb)
        r = r[0] if single else r.reshape(x.shape[:-1])
        return Normal(r, torch.zeros_like(r)), reward_params
