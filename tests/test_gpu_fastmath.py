"""GPU accuracy of the hardware-transcendental helpers (csrc/fast_math.hpp) that every elementwise section uses: NormalTanh sampling and
log-probs (SAC, PPO, rollout), BPTT's log-prob gradient and the swish activations.  Each helper runs elementwise through the test hook
mbpo_debug_eval_fastmath over a dense grid (signed zeros, denormals, +-inf, NaN, the kernels' clamp points) and is compared with fp64.

Bounds hold on the ranges the kernels use: softplus relative 1e-6 on [-80, 80] (collapsed policy stds sit at softplus(x << 0));
tanh relative 1e-6 on 1e-6 <= |x| <= 15 and exactly +-1 beyond; atanh relative 1e-6 on 1e-6 <= |a| <= 0.999; sigmoid, swish and
swish' relative 2e-6 on |v| <= 20, finite with the right sign everywhere.  The plain forms SAC, PPO and the rollout keep
(fm_softplus_fast, fm_tanh_fast) are pinned to their documented absolute accuracy."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EXP, LOG, SOFTPLUS, TANH, ATANH, SIGMOID, SWISH, SWISH_GRAD, SOFTPLUS_FAST, TANH_FAST = range(10)
F32 = np.float32
TINY = float(np.finfo(np.float32).tiny)


def _eval(fn, x):
    from mbpo import _hip
    lib = _hip.load()
    lib.mbpo_debug_eval_fastmath.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.mbpo_debug_eval_fastmath.restype = C.c_int
    xd = torch.as_tensor(np.asarray(x, F32)).cuda()
    yd = torch.full_like(xd, 12345.0)
    assert lib.mbpo_debug_eval_fastmath(fn, C.c_void_p(xd.data_ptr()), C.c_void_p(yd.data_ptr()), xd.numel(), None) == 0, \
        lib.mbpo_last_error()
    torch.cuda.synchronize()
    return yd.cpu().numpy().astype(np.float64)


def _grid(lo, hi, n=200_001, extra=()):
    """Dense linear grid plus log-spaced magnitudes of both signs, the listed points and their fp32 neighbours, as fp32."""
    mags = np.logspace(-45, np.log10(max(abs(lo), abs(hi))), 20_001)
    g = np.concatenate([np.linspace(lo, hi, n), mags, -mags, np.asarray(extra, np.float64)]).astype(F32)
    g = g[(g >= F32(lo)) & (g <= F32(hi))]
    g = np.concatenate([g, np.nextafter(g, F32(np.inf)), np.nextafter(g, F32(-np.inf))])
    return np.unique(g[(g >= F32(lo)) & (g <= F32(hi))])


SPECIAL = np.array([0.0, -0.0, TINY, -TINY, 1e-40, -1e-40, 1.4e-45, -1.4e-45, np.inf, -np.inf, np.nan], F32)


def _rel(y, ref):
    return np.abs(y - ref) / np.abs(ref)


def _softplus64(x):
    return np.logaddexp(x, 0.0)


def _report(name, x, err, bound):
    i = int(np.nanargmax(err))
    assert err[i] <= bound, f"{name}: relative error {err[i]:.3g} > {bound:g} at x = {x[i]!r}"


def test_unknown_helper_is_refused(dev):
    from mbpo import _hip
    lib = _hip.load()
    lib.mbpo_debug_eval_fastmath.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.mbpo_debug_eval_fastmath.restype = C.c_int
    x = torch.zeros(4, device=dev)
    assert lib.mbpo_debug_eval_fastmath(10, C.c_void_p(x.data_ptr()), C.c_void_p(x.data_ptr()), 4, None) < 0
    assert b"unknown helper" in lib.mbpo_last_error()


def test_softplus(dev):
    """Relative 1e-6 on [-80, 80], including the 1e-6 and 1e2 points of BPTT's clip(softplus(raw + c0), 1e-6, 1e2); 0 / inf at -+inf,
    NaN propagates, never negative."""
    inv_1e6, inv_1e2 = np.log(np.expm1(1e-6)), np.log(np.expm1(1e2))
    x = _grid(-80.0, 80.0, extra=[inv_1e6, inv_1e2, -13.8, -13.816, -17.0, -5.0, 8.0, 30.0])
    y = _eval(SOFTPLUS, x)
    _report("softplus", x, _rel(y, _softplus64(x.astype(np.float64))), 1e-6)
    assert np.all(y >= 0.0)
    # the clamp decision of BPTT: (softplus(x) > 1e-6) agrees with fp64's wherever fp32 x is not within 1e-3 of the crossing
    far = np.abs(x - inv_1e6) > 1e-3
    assert np.array_equal((y > F32(1e-6))[far], (_softplus64(x.astype(np.float64)) > float(F32(1e-6)))[far])
    ys = _eval(SOFTPLUS, SPECIAL)
    assert ys[8] == np.inf and ys[9] == 0.0 and np.isnan(ys[10])
    np.testing.assert_allclose(ys[:8], np.log(2.0), rtol=1e-6)
    # beyond +-80: finite where the result is, never negative, never NaN
    big = _eval(SOFTPLUS, np.array([-1e4, -120.0, -104.0, -88.0, 88.0, 1e4, 3e38, -3e38], F32))
    assert np.all(big >= 0.0) and not np.any(np.isnan(big))
    np.testing.assert_allclose(big[4:7], [88.0, 1e4, float(F32(3e38))], rtol=1e-6)
    assert big[7] == 0.0


def test_tanh(dev):
    """Relative 1e-6 on 1e-6 <= |x| <= 15 (the kernels' clamp point), exactly +-1 beyond, odd, sign of zero kept."""
    x = _grid(-40.0, 40.0, extra=[15.0, -15.0, 0.5, -0.5, 1e-6, -1e-6, 9.0, -9.0])
    y = _eval(TANH, x)
    x64 = x.astype(np.float64)
    m = (np.abs(x64) >= 1e-6) & (np.abs(x64) <= 15.0)
    _report("tanh", x[m], _rel(y[m], np.tanh(x64[m])), 1e-6)
    tiny = (np.abs(x64) < 1e-6) & (np.abs(x64) >= TINY)
    _report("tanh (|x| < 1e-6)", x[tiny], _rel(y[tiny], np.tanh(x64[tiny])), 1e-6)
    assert np.all(y[x64 >= 15.0] == 1.0) and np.all(y[x64 <= -15.0] == -1.0)
    assert np.all(np.abs(y) <= 1.0)
    assert np.array_equal(np.sign(y), np.sign(x64))
    np.testing.assert_array_equal(_eval(TANH, -x), -y)                      # odd, bit for bit
    ys = _eval(TANH, SPECIAL)
    assert ys[0] == 0.0 and not np.signbit(ys[0]) and ys[1] == 0.0 and np.signbit(ys[1])
    assert ys[8] == 1.0 and ys[9] == -1.0


def test_atanh(dev):
    """Relative 1e-6 on 1e-6 <= |a| <= 0.999 (BPTT's squash clamp), odd; NaN outside [-1, 1]."""
    a = _grid(-0.999, 0.999, extra=[0.999, -0.999, 0.5, -0.5, 1e-6, -1e-6])
    y = _eval(ATANH, a)
    a64 = a.astype(np.float64)
    m = np.abs(a64) >= 1e-6
    _report("atanh", a[m], _rel(y[m], np.arctanh(a64[m])), 1e-6)
    nz = (~m) & (np.abs(a64) >= TINY)
    _report("atanh (|a| < 1e-6)", a[nz], _rel(y[nz], np.arctanh(a64[nz])), 1e-6)
    assert np.array_equal(np.sign(y), np.sign(a64))
    np.testing.assert_array_equal(_eval(ATANH, -a), -y)
    assert np.all(np.isnan(_eval(ATANH, np.array([1.5, -1.5, 2.0, np.nan], F32))))


def _sigmoid64(v):
    return 0.5 * (1.0 + np.tanh(0.5 * v))


def test_sigmoid_swish_and_grad(dev):
    """sigmoid, swish = v sigmoid(v) (act_apply) and swish' = s (1 + v (1 - s)) (act_grad): relative 2e-6 on |v| <= 20.  swish'
    crosses zero at v ~ -1.28, so its error is taken relative to the magnitude of its terms, s (1 + |v| (1 - s)).  Over |v| <= 1e4
    and at the fp32 extremes every value is finite, in range and of the right sign (no inf * 0)."""
    v = _grid(-1e4, 1e4, extra=[20.0, -20.0, 88.0, -88.0, 89.0, -89.0, 104.0, -104.0])
    v64 = v.astype(np.float64)
    s64 = _sigmoid64(v64)
    sg, sw, sd = _eval(SIGMOID, v), _eval(SWISH, v), _eval(SWISH_GRAD, v)
    m = np.abs(v64) <= 20.0
    _report("sigmoid", v[m], _rel(sg[m], s64[m]), 2e-6)
    mz = m & (np.abs(v64) >= TINY)                                          # (v * 0.5 of a denormal v rounds)
    _report("swish", v[mz], _rel(sw[mz], v64[mz] * s64[mz]), 2e-6)
    grad64 = s64 * (1.0 + v64 * (1.0 - s64))
    scale = s64 * (1.0 + np.abs(v64) * (1.0 - s64))
    _report("swish'", v[m], np.abs(sd[m] - grad64[m]) / scale[m], 2e-6)
    for name, y in (("sigmoid", sg), ("swish", sw), ("swish'", sd)):
        assert np.all(np.isfinite(y)), name
    assert np.all((sg >= 0.0) & (sg <= 1.0))
    assert np.all(sw[v64 > 0] >= 0) and np.all(sw[v64 < 0] <= 0) and np.all(sw[v64 < -20] >= v64[v64 < -20] * 1e-7 - 1e-30)
    assert np.all(sw >= -0.2785)                                             # min swish = -0.27846 at v = -1.2785
    assert np.all(sd[v64 > 20] > 0.99) and np.all(sd[v64 < -20] <= 0) and np.all(sd[v64 < -20] > -1e-6)
    ext = np.array([3e38, -3e38, np.inf, -np.inf], F32)
    sge, swe, sde = _eval(SIGMOID, ext), _eval(SWISH, ext[:2]), _eval(SWISH_GRAD, ext[:2])
    np.testing.assert_array_equal(sge, [1.0, 0.0, 1.0, 0.0])
    assert swe[0] == float(F32(3e38)) and swe[1] == 0.0 and np.all(np.isfinite(sde)) and sde[0] == 1.0 and sde[1] == 0.0


def test_exp_and_log(dev):
    """fm_exp (PPO's ratio, the softplus-free exps) and fm_log: the v_exp_f32 / v_log_f32 forms, relative error within a few ulp plus
    the rounding of x * log2(e), an absolute error in the exponent of at most 6e-8 |x|."""
    x = _grid(-87.0, 88.0, extra=[0.0, 1.0, -1.0])
    y = _eval(EXP, x)
    _report("exp", x, _rel(y, np.exp(x.astype(np.float64))) / (3e-7 + 8e-8 * np.abs(x.astype(np.float64))), 1.0)
    p = _grid(TINY, 3e38, extra=[1.0, 2.0, 0.5])
    p = p[p > 0]
    lg = _eval(LOG, p)
    ref = np.log(p.astype(np.float64))
    away = np.abs(p.astype(np.float64) - 1.0) > 1e-3          # near 1 log is ~0: absolute error there
    _report("log", p[away], _rel(lg[away], ref[away]), 1e-6)
    assert np.all(np.abs(lg[~away] - ref[~away]) <= 1e-7)
    sp = _eval(LOG, np.array([0.0, -1.0, np.inf], F32))
    assert sp[0] == -np.inf and np.isnan(sp[1]) and sp[2] == np.inf


def test_plain_softplus_and_tanh(dev):
    """fm_softplus_fast = max(x,0) + log(1 + exp(-|x|)) and fm_tanh_fast = (e - 1) / (e + 1): absolute 2e-7 + 1e-6 |softplus| and 3e-7;
    the plain softplus is exactly 0 below x ~ -17.3, and sigma = softplus + 0.001 (SAC, PPO, rollout) stays within 1e-4 relative."""
    x = _grid(-80.0, 80.0, extra=[-17.0, -17.5, -13.8, -8.0, -5.0])
    x64 = x.astype(np.float64)
    sp, ref = _eval(SOFTPLUS_FAST, x), _softplus64(x64)
    _report("softplus_fast (absolute)", x, np.abs(sp - ref) / (2e-7 + 1e-6 * ref), 1.0)
    assert np.all(sp >= 0.0) and np.all(sp[x64 <= -17.5] == 0.0)
    _report("softplus_fast + 0.001", x, _rel(sp + float(F32(0.001)), ref + float(F32(0.001))), 1e-4)
    t = _grid(-40.0, 40.0, extra=[15.0, -15.0, 1e-6, -1e-6])
    t64 = t.astype(np.float64)
    th = _eval(TANH_FAST, t)
    _report("tanh_fast (absolute)", t, np.abs(th - np.tanh(t64)) / 3e-7, 1.0)
    assert np.all(np.abs(th) <= 1.0 + 2.0 ** -23)                          # (one ulp over: v_rcp_f32's rounding)
