"""The fixed term tables of tests/test_cpu_term_reward.py and tests/test_gpu_term_reward.py (MBPO_REWARD_TERMS, include/mbpo_hip.h "term
rewards"), as plain data: (x_dim, u_dim, bias, [(weight, link, [(on, index, fn, coef, offset), ...]), ...]).  tests/term_reward_ref.py
evaluates the data itself; `make_reward` builds the product's TermReward from the same data.

On inputs in [-1, 1] every |term| <= 2 and every |s_g| <= 4 (asserted by the CPU tests), so that no case leans on the range reduction of
cos / sin or on exp's growth.
"""
from __future__ import annotations

import functools

import torch

MIXED = (5, 2, 0.3, [
    (0.5, "identity", [("x_next", 3, "identity", 0.8, 0.1)]),                                             # linear on x_next[3]
    (-0.1, "identity", [("u", 0, "square", 1.0, 0.0), ("u", 1, "square", 0.5, 0.0)]),                     # control cost
    (-0.4, "sqrt", [("x", 0, "square", 1.0, 0.2), ("x", 1, "square", 1.0, -0.3)]),                        # distance of x[0:2] to a goal
    (1.0, "exp", [("x_next", 0, "square", -1.5, 0.1), ("x_next", 1, "square", -1.2, 0.0)]),             # tolerance around a set point
    (0.25, "identity", [("x", 2, "cos", 1.0, 0.0), ("x_next", 4, "sin", 0.7, 0.5), ("x", 4, "abs", -0.5, 0.2),
                        ("x_next", 2, "relu", -0.6, 0.1)]),
    (0.2, "tanh", [("u", 1, "identity", 1.5, 0.0), ("x", 3, "identity", -1.0, 0.0)]),
])

WIDE = (17, 6, -0.2, [
    (-1.0, "identity", [("x", c, "square", 0.05 * (1 + c % 3), 0.1 * ((c % 5) - 2)) for c in range(17)]),
    (-0.1, "identity", [("u", d, "square", 0.4 + 0.05 * d, 0.0) for d in range(6)]),
    (-0.3, "sqrt", [("x", 3, "square", 1.0, 0.2), ("x", 9, "square", 0.5, -0.1), ("x", 16, "square", 1.0, 0.0)]),
    (0.5, "exp", [("x", 1, "square", -0.8, 0.3), ("x", 12, "square", -1.2, -0.2)]),
    (0.2, "identity", [("x", 5, "cos", 1.0, 0.1), ("x", 14, "sin", 0.8, -0.4), ("x", 7, "abs", -0.5, 0.15), ("x", 10, "relu", 0.6, -0.1),
                       ("u", 5, "identity", 0.3, 0.0)]),
    (0.3, "tanh", [("x", 2, "identity", 1.2, 0.0), ("x", 8, "identity", -0.9, 0.1)]),
])

QUAD_TARGET = [0.3, -0.2, 0.1, 0.0, 0.5]
QUAD_Q = [1.0, 0.5, 0.25, 0.8, 0.1]
QUAD_R = [0.1, 0.05]
QUADRATIC = (5, 2, 0.0, [
    (-1.0, "identity", [("x", c, "square", QUAD_Q[c], QUAD_TARGET[c]) for c in range(5)]),
    (-1.0, "identity", [("u", d, "square", QUAD_R[d], 0.0) for d in range(2)]),
])

CASES = {"mixed": MIXED, "wide": WIDE, "quadratic": QUADRATIC}
N_EVAL = 1000            # rows of the evaluation inputs: not a multiple of the 256-thread block


@functools.lru_cache(maxsize=None)
def eval_inputs(name: str):
    """(x, u, x_next) fp32, uniform in [-1, 1], fixed per case."""
    X, U = CASES[name][0], CASES[name][1]
    g = torch.Generator().manual_seed(700 + sorted(CASES).index(name))
    f = lambda w: torch.rand(N_EVAL, w, generator=g) * 2 - 1
    return f(X), f(U), f(X)


def has_next_state_terms(name: str) -> bool:
    return any(t[0] == "x_next" for g in CASES[name][3] for t in g[2])


def make_reward(name: str):
    """The product's TermReward of case `name`."""
    from mbpo.systems import Group, Term, TermReward
    X, U, bias, groups = CASES[name]
    return TermReward(X, U, bias=bias, groups=[Group([Term(*t) for t in terms], weight=w, link=link) for w, link, terms in groups])
