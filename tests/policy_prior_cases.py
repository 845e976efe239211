"""Inputs for the policy-prior tests (include/mbpo_hip.h "policy priors"): seed-launch cases laid out as iCEM passes them — the action
columns of step-major rollout rows, every other column NaN, outputs pre-filled with random bits — a hand-written two-problem case, and
the policies the iCemTO tests plan with.  Host tensors only; the GPU tests move them."""
import itertools
import math
from types import SimpleNamespace

import torch

X_DIM = 3
# B, K, H, A, P: one and several problems / proposals / steps / action dims / particles (H * A from 1 to 21: below one wave's 64 lanes;
# LONG adds a trajectory of more than 64 elements, where a lane walks more than one)
SHAPES = list(itertools.product((1, 3), (1, 5), (1, 7), (1, 3), (1, 4)))
LONG = (2, 3, 45, 3, 2)
N_PREV = 2


def row_len(A: int, x_dim: int = X_DIM) -> int:
    return 2 * x_dim + A + 3


def bounds(A: int):
    """per-dimension bounds; at A = 3 the last dimension has u_min == u_max"""
    if A == 1:
        return torch.tensor([-0.9]), torch.tensor([0.8])
    lo = torch.tensor([-1.0, -0.5, 0.25] + [-1.0] * (A - 3))[:A]
    hi = torch.tensor([1.0, 0.7, 0.25] + [1.0] * (A - 3))[:A]
    return lo.contiguous(), hi.contiguous()


def poison(gen: torch.Generator, *shape) -> torch.Tensor:
    """random bits as floats (NaN payloads, infinities and denormals among them)"""
    return torch.randint(-2 ** 31, 2 ** 31 - 1, shape, generator=gen, dtype=torch.int64).to(torch.int32).view(torch.float32)


def make_seed_case(shape, k_equals_samples: bool, seed: int = 0) -> SimpleNamespace:
    """rows [H * B * K, row_len] as mbpo_model_rollout writes them (step-major), action columns N(0, 1.2^2) — about 40 % outside the
    bounds — with one -0.0, every other column NaN; outputs poisoned."""
    B, K, H, A, P = shape
    g = torch.Generator().manual_seed(1000 * seed + sum(v * 7 ** i for i, v in enumerate(shape)) + int(k_equals_samples))
    n_samples = K if k_equals_samples else K + 3
    NC = n_samples + N_PREV
    D = row_len(A)
    rows = torch.full((H * B * K, D), float("nan"))
    rows[:, X_DIM:X_DIM + A] = torch.randn(H * B * K, A, generator=g) * 1.2
    rows[(H * B * K) // 2, X_DIM] = -0.0
    u_min, u_max = bounds(A)
    return SimpleNamespace(B=B, K=K, H=H, A=A, P=P, NC=NC, n_samples=n_samples, rows=rows, offset=X_DIM, step_stride=B * K * D, traj_stride=D,
                           u_min=u_min, u_max=u_max, actions=poison(g, H, B * NC * P, A), candidates=poison(g, B, NC, H, A),
                           mean=poison(g, B, H, A))


def hand_case() -> SimpleNamespace:
    """Two problems, two proposals, two steps, one action dim, two particles, NC = 3; written out by hand.  Proposal (1, 0) holds a NaN
    and is dropped — with it problem 1's mean —, proposal (0, 1) lies outside the bounds in both steps."""
    B, K, H, A, P, NC = 2, 2, 2, 1, 2, 3
    nan = float("nan")
    # dense [H][B * K][A]: offset 0, traj_stride 1, step_stride 4
    src = torch.tensor([0.5, -3.0, nan, 0.25,
                        -0.0, 2.0, 0.1, -0.75])
    u_min, u_max = torch.tensor([-1.0]), torch.tensor([1.5])
    cand = torch.full((B, NC, H, A), 7.0)
    act = torch.full((H, B * NC * P, A), 8.0)
    mean = torch.full((B, H, A), 9.0)
    want_cand = torch.tensor([[[0.5, -0.0], [-1.0, 1.5], [7.0, 7.0]],
                              [[7.0, 7.0], [0.25, -0.75], [7.0, 7.0]]]).reshape(B, NC, H, A)
    #                          b0c0 b0c0 b0c1  b0c1 b0c2 b0c2 b1c0 b1c0 b1c1  b1c1  b1c2 b1c2
    want_act = torch.tensor([[0.5, 0.5, -1.0, -1.0, 8.0, 8.0, 8.0, 8.0, 0.25, 0.25, 8.0, 8.0],
                             [-0.0, -0.0, 1.5, 1.5, 8.0, 8.0, 8.0, 8.0, -0.75, -0.75, 8.0, 8.0]]).reshape(H, B * NC * P, A)
    want_mean = torch.tensor([[0.5, -0.0], [9.0, 9.0]]).reshape(B, H, A)
    return SimpleNamespace(B=B, K=K, H=H, A=A, P=P, NC=NC, src=src, offset=0, step_stride=4, traj_stride=1, u_min=u_min, u_max=u_max,
                           actions=act, candidates=cand, mean=mean, want_actions=want_act, want_candidates=want_cand, want_mean=want_mean)


def n_params(dims) -> int:
    return sum(dims[i] * dims[i + 1] + dims[i + 1] for i in range(len(dims) - 1))


def random_policy(dims, seed: int = 0, scale: float = 1.0) -> torch.Tensor:
    """flat [W | b per layer], weights N(0, scale^2 / fan_in), biases N(0, 0.1^2)"""
    g = torch.Generator().manual_seed(seed)
    parts = []
    for i in range(len(dims) - 1):
        parts.append((torch.randn(dims[i], dims[i + 1], generator=g) * scale / math.sqrt(dims[i])).reshape(-1))
        parts.append(torch.randn(dims[i + 1], generator=g) * 0.1)
    return torch.cat(parts).contiguous()


def constant_policy(dims, mode_action: float, raw_scale: float = -10.0) -> torch.Tensor:
    """All weights zero; the last bias is [atanh(mode_action)] * A | [raw_scale] * A: swish(0) = relu(0) = tanh(0) = 0, so the policy's
    loc is atanh(mode_action) at every state and its mode is tanh(loc)."""
    A = dims[-1] // 2
    flat = torch.zeros(n_params(dims))
    flat[-2 * A:-A] = math.atanh(mode_action)
    flat[-A:] = raw_scale
    return flat
