"""Test-tree restatement of plan rewards (include/mbpo_hip.h "plan rewards"), built on the oracle.

    r(t, b, j) = R_kind(params[b or 0][t or 0]; x, u, x_next of row ((t * n_problems + b) * group + j))

`rows_reward` evaluates the three kinds on step-major rollout rows in the rows' dtype (fp64: the reference), slice by slice, through
oracle.systems.pendulum_reward / quadratic_reward and tests/term_reward_ref.py.  `icem_loop` is the numpy iCEM loop of
tests/test_gpu_icem.py built on oracle.icem.sample_candidates / update, with an objective whose step is told the planned step t.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import icem as oicem
from oracle import systems as osys

import term_reward_ref as tref

PENDULUM, QUADRATIC, TERMS = 0, 1, 3            # MBPO_REWARD_* (include/mbpo_hip.h)
MAX_GROUPS, MAX_TERMS = 16, 128
TERMS_FLOATS = 4 + 4 * MAX_GROUPS + 4 * MAX_TERMS
_FN = ["identity", "square", "abs", "relu", "cos", "sin"]
_LINK = ["identity", "sqrt", "exp", "tanh"]


def param_len(kind: int, x_dim: int, u_dim: int) -> int:
    return {PENDULUM: 3, QUADRATIC: 2 * x_dim + u_dim, TERMS: TERMS_FLOATS}[kind]


def unpack_term_vector(vec, x_dim: int, u_dim: int):
    """A packed term table (TermRewardParams.vector()) as tests/term_reward_cases.py's plain data; a table the packer wrote (ids and
    indices in range)."""
    v = [float(f) for f in torch.as_tensor(vec).reshape(-1)[:TERMS_FLOATS]]
    n_groups, bias = int(v[0]), v[2]
    groups = []
    for g in range(n_groups):
        w, link, first, cnt = v[4 + 4 * g:8 + 4 * g]
        terms = []
        for k in range(int(first), int(first) + int(cnt)):
            zi, fn, coef, off = v[4 + 4 * MAX_GROUPS + 4 * k:8 + 4 * MAX_GROUPS + 4 * k]
            zi = int(zi)
            on, idx = ("x", zi) if zi < x_dim else (("u", zi - x_dim) if zi < x_dim + u_dim else ("x_next", zi - x_dim - u_dim))
            terms.append((on, idx, _FN[int(fn)], coef, off))
        groups.append((w, _LINK[int(link)], terms))
    return (x_dim, u_dim, bias, groups)


def reward(kind: int, vec, x: torch.Tensor, u: torch.Tensor, x_next: torch.Tensor) -> torch.Tensor:
    """[n] in x's dtype: one parameter vector `vec` (fp32 values) on the rows (x [n, X], u [n, U] the controls, x_next [n, X])."""
    X, U = x.shape[1], u.shape[1]
    v = torch.as_tensor(vec, dtype=torch.float32).reshape(-1)
    if kind == PENDULUM:
        p = osys.PendulumParams(angle_cost=float(v[0]), control_cost=float(v[1]), target_angle=float(v[2]))
        return osys.pendulum_reward(x, u, p)
    if kind == QUADRATIC:
        c = v.to(x.dtype)
        return osys.quadratic_reward(x, u, c[:X], c[X:2 * X], c[2 * X:2 * X + U])
    assert kind == TERMS
    return tref.reward(unpack_term_vector(v, X, U), x, u, x_next)


def rows_reward(kind: int, table: torch.Tensor, rows: torch.Tensor, n_steps: int, n_problems: int, group: int, x_dim: int, u_dim: int,
                next_off: int) -> torch.Tensor:
    """[n_steps * n_problems * group] in rows' dtype.  table [PB, PH, param_len] (fp32 values), an axis of size 1 broadcast."""
    PB, PH, _ = table.shape
    assert PB in (1, n_problems) and PH in (1, n_steps) and rows.shape[0] == n_steps * n_problems * group
    r3 = rows.reshape(n_steps, n_problems, group, rows.shape[1])
    out = torch.empty(n_steps, n_problems, group, dtype=rows.dtype)
    for t in range(n_steps):
        for b in range(n_problems):
            s = r3[t, b]
            out[t, b] = reward(kind, table[b if PB > 1 else 0, t if PH > 1 else 0], s[:, :x_dim], s[:, x_dim:x_dim + u_dim],
                               s[:, next_off:next_off + x_dim])
    return out.reshape(-1)


def objective_t(step_t, x0: np.ndarray, candidates: np.ndarray) -> np.ndarray:
    """oracle.icem.objective for a deterministic system whose step is told the planned step: values[c] = mean_t r_t."""
    NC, H, _ = candidates.shape
    x = np.repeat(x0[None], NC, axis=0)
    tot = np.zeros(NC, candidates.dtype)
    for t in range(H):
        x, r = step_t(t, x, candidates[:, t])
        tot += r
    return tot / H


def icem_loop(step_t, x0: np.ndarray, warm: np.ndarray, params, H: int, U: int, state_key: int):
    """(best_value, best_sequence) of iCemTO.optimize's loop in fp64 numpy under the keys the product derives from `state_key` (the
    state's key) — tests/test_gpu_icem.py's loop with `objective_t`."""
    from mbpo.utils import keys as K
    mean = np.zeros((H, U)); mean[:-1] = warm[1:]; mean[-1] = warm[-1]
    std = np.full((H, U), params.init_std)
    best_v, best_s = -np.inf, mean.copy()
    nprev = max(int(params.elite_set_fraction * params.num_elites), 1)
    prev = np.zeros((nprev, H, U))
    carry, _ = K.split(state_key, 2)
    for it in range(params.num_steps):
        sampling_key, _pk = K.split(carry, 2)
        carry = K.split(sampling_key, 2)[0]
        cand = oicem.sample_candidates(mean, std, prev, -1.0, 1.0, params.num_samples, H, U, params.exponent, sampling_key, it)
        vals = objective_t(step_t, x0, cand)
        mean, std, best_v, best_s, prev = oicem.update(vals, cand, mean, std, best_v, best_s, params.num_elites, nprev, params.alpha)
    return best_v, best_s


def pendulum_step_t(targets):
    """step_t for the analytic Pendulum under a target-angle schedule `targets` [H] (angle_cost / control_cost at their defaults)."""
    def step(t, x, u):
        p = osys.PendulumParams(target_angle=float(targets[t]))
        xt, ut = torch.from_numpy(x), torch.from_numpy(u)
        return osys.pendulum_next_state(xt, ut, p).numpy(), osys.pendulum_reward(xt, ut, p).numpy()
    return step
