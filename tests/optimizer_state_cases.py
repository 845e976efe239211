"""Host side of tests/test_gpu_optimizer_trained_state.py: an optimizer state that looks like a trained learner's, the constants
of optax.adamw as float32 arithmetic sees them, the error units of that module, and the generic optimizer's oracle chain.
tests/test_cpu_optimizer_state_cases.py checks all of it without a GPU.

Why a built state and not a trained one: what a late step can get wrong (a bias correction off by one step, (1 - b2) formed in
float32, a moment recurrence that only holds from zero, decay or Polyak on the wrong parameter) shows only when the moments are
non-zero, of mixed sign and scale, when m / sqrt(v) lies on both sides of 1, and when the count is late.  A built state has all of
that at any count, deterministically, in microseconds.

  m        sign * 10^U(-6, 1)
  v        (k m)^2 with k log-uniform in [0.3, 30]  ->  |m| / sqrt(v) = 1 / k in [1/30, 3.3];
           N_SPECIAL elements exactly 0 and N_SPECIAL elements ~1e-30 (n >= 32; the last element is one of the zeros).  There the new
           v is (1 - b2) g^2 alone, so these are the elements at which the weight of g^2 itself shows in the PARAMETER (in v it is
           far below one ulp of max |v|).  v = (k m)^2 holds there too, as it would in a learner that has seen no gradient on an
           element: m = 0 where v = 0 and |m| = sqrt(v) / k ~ 1e-15 where v ~ 1e-30.  (A moment of 1e-3 over v = 0 and a gradient
           the device happens to give as 1e-9 is an update of m / eps = 1e5: one such element sets the largest error of the
           reference and of the kernel alike, and the measured tolerance would then say nothing about all the others.)
  params   generic kernel: uniform in [-1e-2, 1e-2].  Networks: the usual initialisation (lecun-uniform + the case builders' noise)
           times NET_SCALE = 2^-4, an exact scaling that keeps its shape and brings every |p| below 0.125, where one ulp is at most
           7.5e-9 = 7.5e-7 lr.  Unscaled, a weight of a fan-in-1 layer reaches 1.8 and its ulp, 1.2e-5 lr, would hide (1 - b2)
           formed in float32 (1.29e-5 too small: 6.5e-6 of an update) behind the reference's own rounding.
  target   params + uniform noise of a fifth of their range (generic kernel; the SAC cases scale their own target critics)
  count    COUNTS; 2^24 - 2 is there for what follows it: 2^24 - 1, 2^24, and then 2^24 again (SATURATED)
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import bptt as obptt
from oracle import sac as osac


def f32(x: float) -> float:
    """The float32 nearest to x, as a Python float (widened: exact)."""
    return float(np.float32(x))


# optax.adamw's constants as float32 arithmetic sees them: optax forms (1 - decay) in Python double and casts that
B1, B2, ONE_MINUS_B1, ONE_MINUS_B2, EPS = f32(0.9), f32(0.999), f32(0.1), f32(0.001), f32(1e-8)
ADAM = dict(b1=B1, b2=B2, eps=EPS, one_minus_b1=ONE_MINUS_B1, one_minus_b2=ONE_MINUS_B2)


def adam_in(dtype, **override) -> dict:
    """ADAM as 0-dim tensors of `dtype`, for the oracles' `adam` keyword.  As Python floats the constants would leave b^count and
    1 - b^count to Python's double whatever the state's dtype; as tensors the float32 oracle forms them in float32 with the host's
    powf, which is what float32 arithmetic (optax's, and the kernels' `1.f - powf(b, count)`) does.  That matters at early counts:
    1 - 0.999^2 = 0.002 cancels seven bits, so half an ulp of the power is 1.5e-5 of the correction and 7.5e-6 of the update.  It is
    the reference's OWN float32 error and belongs in the measured tolerance; the float64 oracle, the reference, is not touched."""
    return {k: torch.tensor(v, dtype=dtype) for k, v in dict(ADAM, **override).items()}


COUNTS = (0, 1, 9, 999, 99_999, 2 ** 24 - 2)
SATURATED = 2 ** 24          # float32: SATURATED + 1 == SATURATED
LR = f32(1e-2)               # every group of every path
GENERIC_WD, NET_WD, TAU = f32(1e-1), f32(1e-2), f32(0.005)
GENERIC_NS = (1, 255, 1027)  # 1027 = 256 quads + a scalar tail of 3
GENERIC_STEPS = 3
GENERIC_P_MAX = 1e-2
NET_SCALE = 2.0 ** -4
N_SPECIAL = 4
FACTOR = 4.0                 # the kernel's allowance over the float32 oracle's own error (FMA contraction, 1-2 ulp in powf)
TENSORS = ("params", "target", "m", "v")


def _uniform(gen, n, lo, hi):
    return lo + (hi - lo) * torch.rand(n, generator=gen, dtype=torch.float64)


def special_indices(n: int):
    """(indices with v = 0, indices with v ~ 1e-30): none below 32 elements; spread over the vector, the last element a zero."""
    if n < 32:
        return [], []
    k = N_SPECIAL
    zeros = [(j * n) // k + (n // (2 * k)) for j in range(k - 1)] + [n - 1]
    tiny = [(j * n) // k + (n // (4 * k)) for j in range(k)]
    assert len(set(zeros) | set(tiny)) == 2 * k
    return zeros, tiny


def trained_state(n: int, c: int, seed: int = 0, params: torch.Tensor = None):
    """(params, m, v, target, count) of n float32 elements at count c (module docstring).  `params` given: kept as they are."""
    gen = torch.Generator().manual_seed(1_000_003 * seed + 7919 * n + c % 65_521)
    mag = 10.0 ** _uniform(gen, n, -6.0, 1.0)
    sign = torch.where(torch.rand(n, generator=gen, dtype=torch.float64) < 0.5, -1.0, 1.0)
    k = torch.exp(_uniform(gen, n, float(np.log(0.3)), float(np.log(30.0))))
    tiny_v = 1e-30 * _uniform(gen, n, 0.5, 2.0)
    p_draw, t_draw = _uniform(gen, n, -1.0, 1.0), _uniform(gen, n, -1.0, 1.0)
    zeros, tiny = special_indices(n)
    for i in zeros:
        mag[i] = 0.0
    for i in tiny:
        mag[i] = torch.sqrt(tiny_v[i]) / k[i]
    m = sign * mag
    v = (k * m) ** 2
    for i in zeros:
        v[i] = 0.0
    for i in tiny:
        v[i] = tiny_v[i]
    if params is None:
        p = (GENERIC_P_MAX * p_draw).float()
        scale = GENERIC_P_MAX
    else:
        assert params.numel() == n and params.dtype == torch.float32
        p = params.clone()
        scale = float(p.abs().max())
    target = (p.double() + 0.2 * scale * t_draw).float()
    return p, m.float(), v.float(), target, int(c)


def network_params(p: torch.Tensor) -> torch.Tensor:
    """A network's usual initialisation, scaled exactly (module docstring)."""
    return (p * NET_SCALE).float()


def generic_grads(n: int, c: int, steps: int = GENERIC_STEPS, seed: int = 0):
    """Gradients of mixed sign and scale, randn * 10^U(-3, 0): `steps` vectors of n."""
    gen = torch.Generator().manual_seed(15_485_863 * (seed + 1) + 104_729 * n + c % 65_521)
    return [(torch.randn(n, generator=gen, dtype=torch.float64) * 10.0 ** _uniform(gen, n, -3.0, 0.0)).float() for _ in range(steps)]


def ulp_over_lr(p: torch.Tensor, lr: float = LR) -> float:
    """max over the elements of ulp(p) / lr."""
    return float(np.spacing(np.abs(p.numpy()).astype(np.float32)).max()) / lr


def stored_count(c: int, steps_taken: int) -> float:
    """What the device's float32 counter holds `steps_taken` steps after c: it stops at 2^24."""
    return float(min(c + steps_taken, SATURATED))


# ------------------------------------------------------------------------------------------------------------ error units
def errors(got: dict, ref64: dict, lr: float = LR) -> dict:
    """Per tensor, over EVERY element: params and target |d| / lr; m |d| / max |m|; v |d| / max |v| (maxima of the float64 reference).
    A NaN or an infinity in `got` where the reference is finite gives inf."""
    out = {}
    for k in TENSORS:
        if k not in ref64 or ref64[k] is None:
            continue
        g, r = got[k].detach().cpu().double(), ref64[k].double()
        assert g.shape == r.shape, (k, g.shape, r.shape)
        unit = lr if k in ("params", "target") else float(r.abs().max())
        d = (g - r).abs() / unit
        out[k] = float("inf") if not bool(torch.isfinite(d).all()) else float(d.max())
    return out


def worst_element(got: dict, ref64: dict, k: str) -> str:
    """For a failure message: where tensor k is farthest from the reference, and what stands there."""
    g, r = got[k].detach().cpu().double(), ref64[k].double()
    d = torch.nan_to_num((g - r).abs(), nan=float("inf"))
    i = int(d.argmax())
    return f"{k}[{i}] of {g.numel()}: got {float(g[i])!r}, float64 oracle {float(r[i])!r}"


def pool(into: dict, e: dict) -> dict:
    for k, x in e.items():
        into[k] = max(into.get(k, 0.0), x)
    return into


def within(e: dict, measured: dict):
    """(ok, the tensors beyond FACTOR x the float32 oracle's measured error).  NaN fails."""
    bad = {k: (x, FACTOR * measured[k]) for k, x in e.items() if not x <= FACTOR * measured[k]}
    return not bad, bad


# ------------------------------------------------------------------------------------------------- generic optimizer oracle
def generic_oracle(dtype, state, grads, with_target: bool, apply_if_finite: bool, lr=LR, wd=GENERIC_WD, tau=TAU, adam=None,
                   polyak_on_old: bool = False, count_shift: int = 0):
    """optax [apply_if_finite(] adamw [)] + soft_update from `state` over `grads`, in `dtype`, with the TRUE integer count.  One dict
    per step: params, m, v, target (None without one), count.  polyak_on_old / count_shift restate two mistakes (the target fed the
    old parameter; corrections taken at another count) so that the CPU test can show the state is strong enough to expose them."""
    p, m, v, t, c = state
    p, m, v, t = p.to(dtype), m.to(dtype), v.to(dtype), t.to(dtype)
    adam = adam_in(dtype, **(adam or {}))
    out = []
    for g in grads:
        g = g.to(dtype)
        p_old = p
        if apply_if_finite and count_shift == 0:
            p, m, v, c = obptt.apply_if_finite_adamw(p, g, m, v, c, lr, wd, adam=adam)
        else:
            c = c + 1
            p, m, v = osac.adamw_step(p, g, m, v, c + count_shift, lr, wd, **adam)
        if with_target:
            t = (1 - tau) * t + tau * (p_old if polyak_on_old else p)
        out.append(dict(params=p, m=m, v=v, target=t if with_target else None, count=c))
    return out


def generic_measured(c: int, seed: int = 0):
    """The float32 oracle's error against the float64 oracle for the generic path at count c, pooled over GENERIC_NS, with and
    without a target, and the steps (apply_if_finite and the target's alignment do not change the reference).
    Returns (measured, {(n, with_target): float64 chain})."""
    measured, chains = {}, {}
    for n in GENERIC_NS:
        st, gr = trained_state(n, c, seed), generic_grads(n, c, seed=seed)
        for wt in (False, True):
            r64 = generic_oracle(torch.float64, st, gr, wt, False)
            r32 = generic_oracle(torch.float32, st, gr, wt, False)
            for a, b in zip(r32, r64):
                pool(measured, errors(a, b))
            chains[(n, wt)] = r64
    return measured, chains
