"""Calibration of the ensemble's spread — torch-CPU restatement (test infrastructure) of what mbpo_ens_calibrate defines
(include/mbpo_hip.h, "N3d").  The procedure is the reference's declared-but-unimported `bsm` package's as remembered, unverified
against its code: parity unpinned by construction, the definition is the header's.

    statistic   t = next_obs - (obs if predict_delta);  m = (sum_e mu_e) / E in member order;  v = (sum_e (mu_e - m)^2) / E;
                d2 = (t - m)^2 — every operation one rounded operation of `dtype`
    counts      counts[c][a][j] = #{k : d2 <= (((alphas[a] * scale[c])^2) * level_q[j]) * v}      (IEEE: NaN covers nothing)
    levels      p_j = j / (P + 1), level_q[j - 1] = 2 erfinv(p_j)^2 in float64, cast to fp32
    pick        S[c][a] = sum_j (counts[c][a][j - 1] (P + 1) - j n)^2 in int64, argmin over a, ties to the lower index

Fixtures (build): random data has near ties — elements whose d2 / v lies within fp32 rounding of a threshold — and a count that
hinges on one is not a property of the kernel.  The builder draws every element's rho^2 = d2 / v at the log-midpoint of a gap between
two neighbouring thresholds that is wider than 1e-2 (or well below the smallest / above the largest threshold) and sets
t = m + s sqrt(rho^2 v) in float64; tests/test_cpu_ens_calibrate.py then checks, for every fixture the GPU file uses, that the fp32 and
the fp64 counts agree in every cell and do not move when every threshold is scaled by 1 +- 1e-3.
"""
from __future__ import annotations

import functools
from typing import Optional

import numpy as np
import torch

N_ALPHAS, ALPHA_ONE = 61, 20
MIN_LOG_GAP = 1e-2


def levels(P: int) -> torch.Tensor:
    p = torch.arange(1, P + 1, dtype=torch.float64) / (P + 1)
    return (2.0 * torch.erfinv(p) ** 2).to(torch.float32)


def default_alphas() -> torch.Tensor:
    a = torch.arange(N_ALPHAS, dtype=torch.float64)
    return torch.pow(torch.tensor(10.0, dtype=torch.float64), (a - ALPHA_ONE) / 20.0).to(torch.float32)


def grid(A: int) -> torch.Tensor:
    """A small grid around 1 for the test shapes: A = 61 the default, else A log-spaced values from 0.1 to 10 (A = 1: [1])."""
    if A == N_ALPHAS:
        return default_alphas()
    if A == 1:
        return torch.ones(1)
    return torch.pow(torch.tensor(10.0, dtype=torch.float64), torch.linspace(-1, 1, A, dtype=torch.float64)).to(torch.float32)


def targets(rows: torch.Tensor, idx: Optional[torch.Tensor], n: int, x_dim: int, next_obs_off: int, predict_delta: bool) -> torch.Tensor:
    """[n, x] in the dtype of `rows`."""
    b = rows[:n] if idx is None else rows[idx.long()]
    nxt = b[:, next_obs_off:next_obs_off + x_dim]
    return nxt - b[:, :x_dim] if predict_delta else nxt.clone()


def stats(mu: torch.Tensor, t: torch.Tensor):
    """mu [E, n, x], t [n, x] (one dtype) -> (d2, v), each [n, x]; the members are added in order."""
    E = mu.shape[0]
    s = torch.zeros_like(mu[0])
    for e in range(E):
        s = s + mu[e]
    m = s / E
    q = torch.zeros_like(mu[0])
    for e in range(E):
        d = mu[e] - m
        q = q + d * d
    dt = t - m
    return dt * dt, q / E


def counts(mu: torch.Tensor, t: torch.Tensor, alphas: torch.Tensor, level_q: torch.Tensor, scale: Optional[torch.Tensor] = None,
           dtype=torch.float32, thr_factor: float = 1.0) -> torch.Tensor:
    """int32 [x, A, P].  mu [E, n, >= x] (the first x columns are read), t [n, x].  thr_factor scales every threshold (robustness
    checks only)."""
    x = t.shape[1]
    d2, v = stats(mu[..., :x].to(dtype), t.to(dtype))
    al, lq = alphas.to(dtype), level_q.to(dtype)
    out = torch.zeros(x, al.numel(), lq.numel(), dtype=torch.int32)
    for c in range(x):
        a_s = al * (scale[c].to(dtype) if scale is not None else torch.ones((), dtype=dtype))
        tq = (a_s * a_s)[:, None] * lq[None, :]
        if thr_factor != 1.0:
            tq = tq * thr_factor
        thr = tq[:, :, None] * v[None, None, :, c]
        out[c] = (d2[None, None, :, c] <= thr).sum(dim=2).to(torch.int32)
    return out


def pick(cnt: torch.Tensor, n: int):
    """(best_idx int32 [x], S int64 [x, A]) from counts [x, A, P]."""
    P = cnt.shape[2]
    j = torch.arange(1, P + 1, dtype=torch.int64)
    d = cnt.to(torch.int64) * (P + 1) - j[None, None, :] * int(n)
    S = (d * d).sum(dim=2)
    best = torch.from_numpy(np.argmin(S.numpy(), axis=1).astype(np.int32))      # numpy: the first minimum
    return best, S


def calibration(alphas: torch.Tensor, best: torch.Tensor, scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    a = alphas.float()[best.long()]
    return a * scale.float() if scale is not None else a


# ------------------------------------------------------------------------------------------------ fixtures
def _kept_gaps(thr: torch.Tensor) -> torch.Tensor:
    """Log-midpoints of the gaps wider than MIN_LOG_GAP between the sorted thresholds, plus one point below and one above all."""
    lt = torch.log(thr.double().reshape(-1)).sort().values
    gap = lt[1:] - lt[:-1]
    keep = gap > MIN_LOG_GAP
    mids = 0.5 * (lt[1:] + lt[:-1])[keep]
    return torch.cat([lt[:1] - 1.0, mids, lt[-1:] + 1.0])


def build(n: int, x: int, E: int, A: int, P: int, seed: int, *, y_extra: int = 0, with_idx: bool = False, predict_delta: bool = True,
          next_obs_off: Optional[int] = None, with_scale: bool = False, alphas: Optional[torch.Tensor] = None, u: int = 1) -> dict:
    """A near-tie-free case in the entry point's own layout: y [E, n, 2x + y_extra] (the columns past x are noise), rows [R, D] with
    row k of the case at rows[idx[k]] (with_idx: R = n + 7 and idx a partial permutation; else idx None), alphas, level_q, scale."""
    g = torch.Generator().manual_seed(seed)
    alphas = grid(A) if alphas is None else alphas.float()
    level_q = levels(P)
    scale = torch.exp(0.7 * torch.randn(x, generator=g)).float() if with_scale else None
    noff = x + u + 2 if next_obs_off is None else next_obs_off
    D = noff + x + 1
    ys = 2 * x + y_extra
    y = 0.5 * torch.randn(E, n, ys, generator=g)
    mu = y[..., :x].double()
    s = torch.zeros_like(mu[0])
    for e in range(E):
        s = s + mu[e].float()
    m32 = (s.float() / E).double()                  # the fp32 mean the kernel forms; the spread around it in float64
    v = ((mu - m32) ** 2).sum(dim=0) / E
    t = torch.empty(n, x, dtype=torch.float64)
    n_gaps = []
    for c in range(x):
        a_s = alphas.double() * (scale[c].double() if scale is not None else 1.0)
        mids = _kept_gaps((a_s * a_s)[:, None] * level_q.double()[None, :])
        n_gaps.append(int(mids.numel()))
        rho2 = torch.exp(mids[torch.randint(0, mids.numel(), (n,), generator=g)])
        sign = torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
        t[:, c] = m32[:, c] + sign * torch.sqrt(rho2 * v[:, c])
    R = n + 7 if with_idx else n
    rows = torch.randn(R, D, generator=g)
    idx = torch.randperm(R, generator=g)[:n].to(torch.int32) if with_idx else None
    sel = idx.long() if with_idx else torch.arange(n)
    obs = 0.25 * torch.randn(n, x, generator=g)
    rows[sel, :x] = obs
    rows[sel, noff:noff + x] = (t + obs.double()).float() if predict_delta else t.float()
    return dict(n=n, x=x, u=u, E=E, y=y.contiguous(), rows=rows.contiguous(), idx=idx, alphas=alphas, level_q=level_q, scale=scale,
                next_obs_off=noff, predict_delta=predict_delta, n_gaps=n_gaps)


# (n, x, E, A, P) and layout of the launch-level GPU cases: one row, under a wave, ragged, many workgroups; y_stride 2x and 2x + 2;
# idx given and NULL; predict_delta on and off; a non-default next_obs_off; scale given and NULL
CASES = {
    "one_row":      dict(n=1, x=1, E=2, A=1, P=1, seed=1),
    "under_a_wave": dict(n=63, x=1, E=2, A=1, P=1, seed=2, y_extra=2, with_idx=True),
    "ragged":       dict(n=300, x=3, E=5, A=7, P=4, seed=3, y_extra=2, with_idx=True, predict_delta=False, next_obs_off=9,
                         with_scale=True),
    "many_wg":      dict(n=5000, x=17, E=7, A=61, P=19, seed=4, with_idx=True),
    "wide_ragged":  dict(n=300, x=17, E=5, A=61, P=19, seed=5, y_extra=2, with_scale=True),
    "many_wg_nodelta": dict(n=5000, x=3, E=7, A=7, P=4, seed=6, predict_delta=False),
}
ONE_CELL = ("one_row", "under_a_wave")


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    return build(**CASES[name])


@functools.lru_cache(maxsize=None)
def tie_case() -> dict:
    """Two alphas of one value (indices 2 and 3) that are also the best: identical counts, the lower index must win."""
    al = torch.tensor([0.25, 0.5, 1.0, 1.0, 2.0, 4.0])
    return build(n=300, x=3, E=5, A=6, P=4, seed=7, alphas=al)


@functools.lru_cache(maxsize=None)
def degenerate(kind: str) -> dict:
    """The ragged fixture with non-finite or collapsed rows; the fp32 restatement is the expectation (the same IEEE comparison)."""
    one = kind == "one_member"                      # (without the delta the stored target IS the member's output, bit for bit)
    b = build(n=300, x=3, E=1 if one else 5, A=7, P=4, seed=8, predict_delta=not one)
    b = dict(b, y=b["y"].clone(), rows=b["rows"].clone())
    x, noff = b["x"], b["next_obs_off"]
    if kind == "one_member":                        # v = 0 everywhere: only d2 = 0 is covered — every third row is made to miss
        b["rows"][::3, noff:noff + x] += 0.5
    elif kind == "nan_member":
        b["y"][2, 5:40, 1] = float("nan")
    elif kind == "inf_target":
        b["rows"][17, noff + 2] = float("inf")
    elif kind == "all_equal":                       # one row whose members all equal the target: v = 0 and d2 = 0, covered everywhere
        b["rows"][11, :x] = 0.25
        b["rows"][11, noff:noff + x] = 0.75
        b["y"][:, 11, :x] = 0.5
    else:
        raise KeyError(kind)
    return b


DEGENERATE = ("one_member", "nan_member", "inf_target", "all_equal")


def case_targets(b: dict, dtype=torch.float32) -> torch.Tensor:
    """The targets as the kernel forms them: ONE fp32 subtraction on the stored rows (then cast for the fp64 restatement)."""
    return targets(b["rows"], b["idx"], b["n"], b["x"], b["next_obs_off"], b["predict_delta"]).to(dtype)


@functools.lru_cache(maxsize=None)
def _expected(key: str):
    b = {"tie": tie_case}.get(key, None)
    b = b() if b else (degenerate(key[4:]) if key.startswith("deg:") else case(key))
    cnt = counts(b["y"], case_targets(b), b["alphas"], b["level_q"], b["scale"])
    best, S = pick(cnt, b["n"])
    return cnt, best, calibration(b["alphas"], best, b["scale"]), S


def expected(key: str):
    """(counts, best_idx, calibration, S) of case `key` ('tie', 'deg:<kind>' or a CASES name) in fp32, computed once."""
    return _expected(key)


def recovery_case(k: float, seed: int = 0):
    """Overconfidence factor k: n = 4000, x = 3 with member spreads {0.01, 0.1, 1}, E = 7, targets m + k sd N(0, 1).
    Returns (mu [E, n, x] fp32, targets [n, x] fp32)."""
    g = torch.Generator().manual_seed(1000 + seed)
    n, x, E = 4000, 3, 7
    spread = torch.tensor([0.01, 0.1, 1.0], dtype=torch.float64)
    mu = (torch.randn(n, x, generator=g, dtype=torch.float64)[None] + spread * torch.randn(E, n, x, generator=g, dtype=torch.float64)).float()
    d2v = stats(mu.double(), torch.zeros(n, x, dtype=torch.float64))
    m = mu.double().mean(dim=0)
    sd = torch.sqrt(d2v[1])
    t = m + k * sd * torch.randn(n, x, generator=g, dtype=torch.float64)
    return mu.contiguous(), t.float()


RECOVERY_K = (0.3, 1.0, 3.0, 12.0)
RECOVERY_TOL = 0.075            # |log10(calibration / k)|: 1.5 steps of the default grid (ratio 10^(1/20))
