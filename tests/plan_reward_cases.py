"""The fixed shapes, rows and parameter tables of tests/test_cpu_plan_reward.py and tests/test_gpu_plan_reward.py (include/mbpo_hip.h
"plan rewards"), as plain data built on the host.

Rows have the rollout's layout [obs (X) | action (A) | reward | discount | next_obs (X) | truncation]: row_len = 2 X + A + 3, reward at
X + A, next state at X + A + 2.  Of the A action columns the first u_dim are the controls; the others (an optimistic system's eta) must
never be read.
"""
from __future__ import annotations

import math

import torch

import plan_reward_ref as pref

# (n_steps, n_problems, group, x_dim, u_dim, action width)
SHAPES = [
    (1, 1, 1, 3, 1, 1),
    (5, 3, 7, 3, 1, 1),        # many problems inside one workgroup
    (4, 2, 300, 4, 2, 2),      # 256 consecutive rows straddle two problems; the kernel that stages term tables in LDS, a partly idle tile
    (3, 4, 64, 5, 2, 7),       # eta columns after the controls: an action width above u_dim
    (2, 1, 515, 3, 1, 1),
]
FORMS = ["11", "B1", "1H", "BH"]                      # the table's [PB, PH]: 1 = broadcast
PENDULUM_TARGETS = [-math.pi, -2.0, 0.0, 0.7, 3.0, math.pi]


def layout(x_dim: int, action_width: int):
    """(row_len, reward_col, next_off)"""
    return 2 * x_dim + action_width + 3, x_dim + action_width, x_dim + action_width + 2


def form_shape(form: str, n_steps: int, n_problems: int):
    return (n_problems if form[0] == "B" else 1, n_steps if form[1] == "H" else 1)


def term_data(x_dim: int, u_dim: int, g: torch.Generator, extra: bool):
    """A term table as plain data (tests/term_reward_cases.py's format) with cos, exp, sqrt and two x_next terms, its numbers drawn from
    g; `extra` appends a group, so that tables of one launch differ in their term counts too."""
    c = lambda lo=0.2, hi=1.2: float(torch.rand((), generator=g) * (hi - lo) + lo)
    o = lambda: float(torch.rand((), generator=g) * 0.6 - 0.3)
    L = x_dim - 1
    groups = [
        (0.5, "identity", [("x_next", L, "identity", c(), o())]),
        (-0.1, "identity", [("u", d, "square", c(), 0.0) for d in range(u_dim)]),
        (-0.4, "sqrt", [("x", 0, "square", c(), o()), ("x", L, "square", c(), o())]),
        (1.0, "exp", [("x_next", 0, "square", -c(), o()), ("x", 1, "square", -c(), o())]),
        (0.25, "identity", [("x", min(2, L), "cos", c(), o()), ("x", 0, "abs", -c(), o()), ("x_next", 1, "sin", c(), o())]),
    ]
    if extra:
        groups.append((c(), "tanh", [("u", 0, "identity", c(), 0.0), ("x", 1, "relu", -c(), o())]))
    return (x_dim, u_dim, c(-0.5, 0.5), groups)


def term_params(data):
    """The product's TermRewardParams of plain term data."""
    from mbpo.systems import Group, Term, TermRewardParams
    X, U, bias, groups = data
    return TermRewardParams(X, U, bias, tuple(Group(tuple(Term(*t) for t in terms), weight=w, link=link) for w, link, terms in groups))


def make_table(kind: int, form: str, shape, seed: int = 0) -> torch.Tensor:
    """[PB, PH, param_len] fp32 on the host: distinct random parameters per (b, t)."""
    H, B, _, X, U, _ = shape
    PB, PH = form_shape(form, H, B)
    g = torch.Generator().manual_seed(9000 + 131 * seed + 7 * kind + FORMS.index(form))
    tab = torch.zeros(PB, PH, pref.param_len(kind, X, U))
    for b in range(PB):
        for t in range(PH):
            if kind == pref.PENDULUM:
                ac, cc = float(torch.rand((), generator=g) + 0.5), float(torch.rand((), generator=g) * 0.04 + 0.01)
                tab[b, t] = torch.tensor([ac, cc, PENDULUM_TARGETS[(b * PH + t + seed) % len(PENDULUM_TARGETS)]])
            elif kind == pref.QUADRATIC:
                tab[b, t] = torch.cat([torch.rand(X, generator=g) - 0.5, torch.rand(X, generator=g) + 0.1, torch.rand(U, generator=g) * 0.3])
            else:
                tab[b, t] = term_params(term_data(X, U, g, extra=(b + t) % 2 == 1)).vector()
    return tab


def make_rows(shape, seed: int = 0, pendulum: bool = False) -> torch.Tensor:
    """[n_steps * n_problems * group, row_len] fp32 on the host.  pendulum: obs = [cos, sin, thetadot] with theta uniform in [-pi, pi],
    |thetadot| <= 8, |u| <= 1; else everything uniform in [-1, 1].  The reward, discount and truncation columns hold other numbers."""
    H, B, G, X, U, A = shape
    row_len, reward_col, next_off = layout(X, A)
    g = torch.Generator().manual_seed(500 + seed + 17 * G + X)
    rows = torch.rand(H * B * G, row_len, generator=g) * 2 - 1
    if pendulum:
        assert (X, U) == (3, 1)
        th = (torch.rand(H * B * G, generator=g) * 2 - 1) * math.pi
        rows[:, 0], rows[:, 1], rows[:, 2] = torch.cos(th), torch.sin(th), rows[:, 2] * 8.0
    return rows
