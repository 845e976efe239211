"""No GPU: the case builder of tests/test_gpu_optimizer_trained_state.py (tests/optimizer_state_cases.py) builds what that module's
docstring promises, the oracles' new constant keywords leave every old caller's numbers alone, and the built state is strong
enough: each mistake of the issue's list, restated on the float32 ORACLE, lands beyond the tolerance the GPU module would grant."""
import math

import numpy as np
import pytest
import torch

import optimizer_state_cases as oc
from oracle import bptt as obptt
from oracle import ppo as oppo
from oracle import sac as osac

NS = oc.GENERIC_NS + (32, 20_993)


@pytest.mark.parametrize("c", oc.COUNTS)
@pytest.mark.parametrize("n", NS)
def test_trained_state_is_what_the_docstring_says(n, c):
    p, m, v, t, count = oc.trained_state(n, c)
    again = oc.trained_state(n, c)
    assert all(torch.equal(a, b) for a, b in zip((p, m, v, t), again[:4])) and count == again[4] == c      # deterministic
    assert all(x.dtype == torch.float32 and x.shape == (n,) for x in (p, m, v, t))
    assert all(bool(torch.isfinite(x).all()) for x in (p, m, v, t))
    zeros, tiny = oc.special_indices(n)
    assert (len(zeros), len(tiny)) == ((0, 0) if n < 32 else (oc.N_SPECIAL, oc.N_SPECIAL))
    rest = torch.ones(n, dtype=torch.bool)
    rest[zeros + tiny] = False
    assert float(m[rest].abs().min()) >= 0.99e-6 and float(m.abs().max()) <= 10.0
    assert all(float(v[i]) == 0.0 and float(m[i]) == 0.0 for i in zeros)                   # no gradient ever: no moment either
    assert all(0.4e-30 < float(v[i]) < 2.1e-30 and 1e-17 < abs(float(m[i])) < 1e-14 for i in tiny)
    if n >= 32:
        assert zeros[-1] == n - 1
    notzero = torch.ones(n, dtype=torch.bool)
    notzero[zeros] = False
    ratio = (m.double().abs() / v.double().sqrt())[notzero]       # = 1 / k, at the ~1e-30 elements too
    assert float(ratio.min()) >= 0.999 / 30 and float(ratio.max()) <= 1.001 / 0.3
    if n >= 255:
        assert bool((m > 0).any()) and bool((m < 0).any())
        assert float(m.abs().min()) < 1e-5 and float(m.abs().max()) > 1.0          # the span, roughly 1e-6 .. 1e1
        assert bool((ratio < 0.5).any()) and bool((ratio > 2.0).any())           # both sides of 1
    assert float(p.abs().max()) <= oc.GENERIC_P_MAX and float(t.abs().max()) <= 1.2 * oc.GENERIC_P_MAX + 1e-9
    assert oc.ulp_over_lr(p) < 1e-6 and oc.ulp_over_lr(t) < 1e-6


def test_counts_and_saturation():
    assert oc.COUNTS == (0, 1, 9, 999, 99_999, 2 ** 24 - 2)
    assert np.float32(oc.SATURATED) + np.float32(1) == np.float32(oc.SATURATED)
    assert np.float32(oc.SATURATED - 1) + np.float32(1) == np.float32(oc.SATURATED)
    assert [oc.stored_count(2 ** 24 - 2, i) for i in (1, 2, 3, 4)] == [2.0 ** 24 - 1, 2.0 ** 24, 2.0 ** 24, 2.0 ** 24]
    # both corrections are exactly 1 long before: the saturated count changes nothing in the update
    for b in (oc.B1, oc.B2):
        assert np.float32(1.0 - b ** 99_999) == 1.0 and 1.0 - b ** (2 ** 24 - 1) == 1.0


def test_constants_are_the_float32_ones():
    assert oc.ONE_MINUS_B2 != 1.0 - oc.B2 and oc.ONE_MINUS_B1 != 1.0 - oc.B1
    # (1 - b2) formed in float32 is 1.29e-5 too small: 6.5e-6 of an update where v is new, which the tolerance must not swallow
    assert float(np.float32(1) - np.float32(0.999)) / oc.ONE_MINUS_B2 - 1 == pytest.approx(-1.292e-5, rel=1e-3)
    # at count 999 the float32 b2 alone moves 1 - b2^count by 4.7e-6 against Python's 0.999: forty float32 roundings
    assert abs((1 - oc.B2 ** 999) - (1 - 0.999 ** 999)) == pytest.approx(4.74e-6, rel=1e-2)


@pytest.mark.parametrize("kind", ["sac_init", "ppo_init"])
def test_network_parameters_scaled(kind):
    """The usual initialisation of the SAC / PPO cases, times 2^-4: every ulp below 1e-6 lr; unscaled it is not."""
    g = torch.Generator().manual_seed(0)
    if kind == "sac_init":
        cfg = osac.SacConfig(x_dim=1, u_dim=31, policy_dims=[1, 64, 64, 62], q_dims=[32, 64, 64, 1])
        p = osac.init_state(cfg, g, init_log_alpha=-0.3).params
    else:
        cfg = oppo.PpoConfig(x_dim=3, u_dim=1, policy_dims=[3, 64, 64, 64, 2], value_dims=[3, 64, 64, 64, 1])
        p = oppo.init_state(cfg, g).params
    p = p + 0.03 * torch.randn(p.shape, generator=g)
    s = oc.network_params(p)
    assert torch.equal(s * 16, p)                                   # exact
    assert oc.ulp_over_lr(s) < 1e-6 < oc.ulp_over_lr(p)
    ps, m, v, t, _ = oc.trained_state(p.numel(), 999, params=s)
    assert torch.equal(ps, s) and oc.ulp_over_lr(t) < 1e-6


def test_oracle_keywords_leave_old_callers_alone():
    g = torch.Generator().manual_seed(3)
    p, gr, m, v = (torch.randn(300, generator=g, dtype=torch.float64) for _ in range(4))
    v = v * v
    old = (lambda b1=0.9, b2=0.999, eps=1e-8: (
        (lambda m2, v2: (p - 1e-3 * ((m2 / (1 - b1 ** 7)) / (torch.sqrt(v2 / (1 - b2 ** 7)) + eps) + 0.1 * p), m2, v2))(
            b1 * m + (1 - b1) * gr, b2 * v + (1 - b2) * gr * gr)))()
    new = osac.adamw_step(p, gr, m, v, 7, 1e-3, 0.1)
    assert all(torch.equal(a, b) for a, b in zip(old, new))
    a = obptt.apply_if_finite_adamw(p, gr, m, v, 6, 1e-3, 0.1)
    assert all(torch.equal(x, y) for x, y in zip(a[:3], new)) and a[3] == 7
    b = obptt.apply_if_finite_adamw(p, gr, m, v, 6, 1e-3, 0.1, adam=oc.adam_in(torch.float64))
    assert not torch.equal(b[2], new[2])                             # the float32 constants do change v


@pytest.mark.parametrize("c", oc.COUNTS)
def test_generic_tolerance_is_small_and_the_listed_mistakes_exceed_it(c):
    """The measured float32-oracle error (what the GPU module multiplies by FACTOR) is of the order of float32 rounding, and the
    float32 oracle WITH one of the listed mistakes is beyond FACTOR x it: the state exposes the mistake, the tolerance does not
    swallow it.  (Corrections at another count cannot show once both are exactly 1: counts >= 99 999.)"""
    measured, chains = oc.generic_measured(c)
    print(f"generic c={c}: " + "  ".join(f"{k} {measured[k]:.2e}" for k in oc.TENSORS))
    assert set(measured) == set(oc.TENSORS)
    assert all(0 < measured[k] < 1e-4 for k in oc.TENSORS), measured
    n = 1027
    st, gr = oc.trained_state(n, c), oc.generic_grads(n, c)
    ref = chains[(n, True)]

    def worst(**kw):
        run = oc.generic_oracle(torch.float32, st, gr, True, False, **kw)
        e = {}
        for a, b in zip(run, ref):
            oc.pool(e, oc.errors(a, b))
        return e

    ok, _ = oc.within(worst(), measured)
    assert ok
    ok, bad = oc.within(worst(polyak_on_old=True), measured)
    assert not ok and set(bad) == {"target"}, bad
    ok, bad = oc.within(worst(adam=dict(one_minus_b2=float(np.float32(1) - np.float32(0.999)))), measured)
    if c >= 9:
        # (at counts 2 and 3 float32's own 1 - 0.999^count, seven bits cancelled, is 1e-5 of an update off and hides these 6.5e-6:
        # the late counts are where this mistake shows)
        assert not ok and "params" in bad, bad
    if c >= 1:
        ok, bad = oc.within(worst(count_shift=-1), measured)
        assert ok == (c >= 99_999), (c, bad)


def test_errors_see_every_element_and_nan():
    ref = dict(params=torch.zeros(5, dtype=torch.float64), m=torch.ones(5, dtype=torch.float64), v=torch.ones(5, dtype=torch.float64), target=None)
    got = dict(params=torch.zeros(5), m=torch.ones(5), v=torch.ones(5))
    assert oc.errors(got, ref) == dict(params=0.0, m=0.0, v=0.0)
    got["params"][4] = 1e-2 * oc.LR
    assert oc.errors(got, ref)["params"] == pytest.approx(1e-2)
    got["m"][0] = float("nan")
    e = oc.errors(got, ref)
    assert math.isinf(e["m"]) and not oc.within(e, dict(params=1.0, m=1.0, v=1.0))[0]
