"""The fixed shapes, parameters and states of tests/test_cpu_terminal_value.py and tests/test_gpu_terminal_value.py (include/mbpo_hip.h
"terminal values"), as plain data built on the host.

Parameters are init_mlp_flat (lecun-uniform kernels) plus N(0, 0.1^2) on EVERY entry, so that biases are non-zero; states are mean + 2 std
randn under the normaliser's own vectors.  Tolerances are the project's forward tolerances (test_ensemble_forward_parity's figures), not
figures of the code under test: 2e-5 against the fp32 restatement, 5e-5 against the fp64 one.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from oracle import nets

TOL32, TOL64 = 2e-5, 5e-5

# (x_dim, action width A, hidden sizes, activation)
SHAPES = [
    (3, 1, (64, 64, 64), "swish"),
    (3, 4, (64, 64, 64), "swish"),        # the optimistic layout: A = u + x
    (17, 6, (64, 64, 64), "swish"),
    (17, 23, (128, 128, 128), "swish"),   # the critics' input (40) is wider than the input layer's unrolled path
    (4, 1, (64, 64), "relu"),
    (5, 2, (256, 256), "tanh"),
]
KINDS = ["V1", "V2", "Q"]                 # state value with one net, with two, SAC's pair under its policy


def shape_id(s) -> str:
    return f"x{s[0]}a{s[1]}h{s[2][0]}x{len(s[2])}{s[3]}"


class Case(NamedTuple):
    x_dim: int
    action_dim: int                       # 0: kind V
    n_critics: int
    act: str
    critic_dims: list
    critic: torch.Tensor                  # [n_critics * params]
    policy_dims: Optional[list]
    policy: Optional[torch.Tensor]
    mean: torch.Tensor                    # [x_dim]
    std: torch.Tensor

    def ref_args(self, norm: bool = True):
        """positional and keyword arguments of terminal_value_ref.v_hat after x"""
        return ((self.critic, self.critic_dims, self.n_critics, self.act),
                dict(policy=self.policy, policy_dims=self.policy_dims, mean=self.mean if norm else None, std=self.std if norm else None))


def _net(dims, g: torch.Generator) -> torch.Tensor:
    p = nets.init_mlp_flat(dims, g)
    return p + 0.1 * torch.randn(p.shape, generator=g)


def make_case(shape, kind: str, seed: int = 0) -> Case:
    X, A, hidden, act = shape
    g = torch.Generator().manual_seed(7100 + 97 * seed + 13 * SHAPES.index(shape) + KINDS.index(kind))
    q = kind == "Q"
    n_critics = 1 if kind == "V1" else 2
    critic_dims = [X + (A if q else 0), *hidden, 1]
    critic = torch.cat([_net(critic_dims, g) for _ in range(n_critics)])
    policy_dims = [X, *hidden, 2 * A] if q else None
    policy = _net(policy_dims, g) if q else None
    mean = torch.randn(X, generator=g)
    std = torch.rand(X, generator=g) * 1.5 + 0.5
    return Case(X, A if q else 0, n_critics, act, critic_dims, critic, policy_dims, policy, mean, std)


def make_states(case: Case, n: int, seed: int = 0, norm: bool = True) -> torch.Tensor:
    """[n, x_dim] fp32: mean + 2 std randn (without a normaliser the networks see the states themselves: 2 randn)."""
    g = torch.Generator().manual_seed(300 + seed + 31 * case.x_dim + n)
    z = 2.0 * torch.randn(n, case.x_dim, generator=g)
    return (case.mean + case.std * z) if norm else z


def icem_layout(x_dim: int, action_width: int):
    """(row_len, reward_col, next_off) of the rollout's rows [obs | action | reward | discount | next_obs | truncation]"""
    return 2 * x_dim + action_width + 3, x_dim + action_width, x_dim + action_width + 2
