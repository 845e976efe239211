"""GPU parity in the regimes trained networks reach and init-like networks never do: collapsed policy stds (raw std head far below 0),
saturated squashes (|pre-squash| past tanh's rounding to +-1), large stds (BPTT's upper clamp) and saturated hidden layers.  The
values are placed with the output-layer biases, and the output-layer weights are scaled down so that every row stays near the
chosen value (hidden layers are scaled up for the saturated-hidden regime).

Tolerance rule.  Parts of these regimes are ill-conditioned in exact arithmetic (BPTT's q = (atanh(tanh(mu + eps sg)) - mu) / sg with
sg ~ 1e-6 amplifies the rounding of mu + eps sg by 1/sg), so a fixed tolerance against the fp32 oracle says nothing.  Each result is
compared with the fp64 oracle (oracle/* fed .double() on the same fp32 inputs), elementwise:

    |hip - fp64| <= 4 |fp32_oracle - fp64| + atol + rtol |fp64|

with the family's existing atol / rtol against fp64 (tests/test_gpu_bptt.py, tests/test_gpu_sac.py, tests/test_gpu_ppo.py,
tests/test_gpu_rollout.py, tests/test_gpu_ensemble_train.py).  Where a pair of kernels is defined to agree bit for bit (SAC lean and
generic, rollout lean and generic, BPTT z store and recompute) it must in every regime; PPO's lean kernel sums tiles in another order
and keeps test_gpu_ppo.py's tolerance against the generic one.  Where elementwise is meaningless (sums that cancel: BPTT's tiny-loc
cases, ens_nll_grads) the rule is applied to norms, as each test says.

Covered: BPTT fused ('mean' mode, z store and recompute) and the wide path (BpttActorGradGeneric) against the fused kernel; SAC generic,
lean, thin-layer variant and layered path (swish, relu and tanh hidden layers); PPO generic, lean and layered, the ratio clip driven
from both sides with the entropy term on; the rollout generic and lean with ppo_extras, deterministic and sampled; ens_nll_grads with
member sigma at min_std and large residuals.  Not covered here: BPTT's 'ts1' mode (its elementwise section is the 'mean' mode's, with
the sampled member's output; tests/test_gpu_bptt_stochastic.py runs it at init-like values) and the ensemble forward / rollout at
min_std (libm, like ens_nll_grads).
"""
import math

import pytest
import torch

from oracle import bptt as obptt
from oracle import nets as onets
from oracle import sac as osac
from test_gpu_bptt import _run_hip, _set_zstore, _setup
from test_gpu_sac import _make, _updater
from test_gpu_sac_lean import _run as _sac_run, _set_lean, _slab_floats

pytestmark = pytest.mark.gpu

SP_1E6 = math.log(math.expm1(1e-6))          # raw + c0 where softplus crosses BPTT's lower clamp: -13.8155


def _assert_rule(name, hip, f32, f64, atol, rtol):
    hip, f32, f64 = (torch.as_tensor(t).double().reshape(-1) for t in (hip, f32, f64))
    bound = 4.0 * (f32 - f64).abs() + atol + rtol * f64.abs()
    err = (hip - f64).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = int(torch.argmax(torch.where(bad, err - bound, torch.zeros_like(err))))
        raise AssertionError(f"{name}: {int(bad.sum())} of {err.numel()} elements outside 4|fp32 - fp64| + {atol:g} + {rtol:g}|fp64|; "
                             f"worst [{i}]: hip {float(hip[i]):.9g}, fp32 oracle {float(f32[i]):.9g}, fp64 {float(f64[i]):.9g}")


def _place(params, dims, off, U, loc=None, raw=None, w_loc=1e-3, w_raw=1e-5, hidden_scale=None):
    """Output layer [dims[-2], 2U] at params[off:]: scale its loc / raw-std columns by w_loc / w_raw, set the biases to loc / raw;
    hidden_scale multiplies every hidden layer's weights.  Returns a new tensor."""
    p = params.clone()
    n_out = onets.n_params(dims)
    o = off + n_out - (dims[-2] * dims[-1] + dims[-1])
    W = p[o:o + dims[-2] * dims[-1]].view(dims[-2], dims[-1])
    b = p[o + dims[-2] * dims[-1]:off + n_out]
    W[:, :U] *= w_loc
    W[:, U:] *= w_raw
    if loc is not None:
        b[:U] = loc
    if raw is not None:
        b[U:] = raw
    if hidden_scale is not None:
        q = off
        for i in range(len(dims) - 2):
            n_w = dims[i] * dims[i + 1]
            if i > 0:
                p[q:q + n_w] *= hidden_scale
            q += n_w + dims[i + 1]
    return p


# ------------------------------------------------------------------------------------------------ BPTT (k_bptt_actor)
def _bptt_case(X, U, H, n, system, E, raw, loc=0.0, seed=0, hidden_scale=None):
    cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, tsys, extra = _setup(X, U, H, n, system, E, seed)
    c0 = obptt.inv_softplus(cfg.init_stddev)
    ap = _place(ap, cfg.actor_dims, 0, U, loc=loc, raw=raw - c0, hidden_scale=hidden_scale)
    g_ref, loss32, aux = obptt.actor_grads(cfg, tsys, ap, cp, x0, noise, s_mean, s_std, r_ms[0], r_ms[1])
    d = lambda t: t.double()
    tsys64 = obptt.TorchPendulumSystem() if system == "pendulum" else obptt.TorchEnsembleSystem(
        d(extra["dp"]), extra["dd"], E, X, U, d(extra["tgt"]), d(extra["q"]), d(extra["r"]))
    g64, loss64, aux64 = obptt.actor_grads(cfg, tsys64, d(ap), d(cp), d(x0), d(noise), d(s_mean), d(s_std), d(r_ms[0]), d(r_ms[1]))
    refs = (g_ref, aux, g64, loss64, aux64)
    return cfg, (ap, cp, x0, noise, s_mean, s_std, r_ms, extra), refs, (loss32, float(aux["entropy_loss"]))


def _bptt_assert(op, refs, m32, X, U, H, n, tag, normwise_grad=False):
    g_ref, aux, g64, loss64, aux64 = refs
    rows = op.transitions.cpu().reshape(n, H, -1)
    _assert_rule(f"{tag} action", rows[..., X:X + U], aux["action"], aux64["action"], 2e-6, 2e-6)
    _assert_rule(f"{tag} observation", rows[..., :X], aux["observation"], aux64["observation"], 2e-4, 2e-4)
    m = op.metrics.cpu()
    _assert_rule(f"{tag} actor loss", m[0:1], torch.tensor([m32[0]]), torch.tensor([loss64]), 2e-5, 1e-4)
    _assert_rule(f"{tag} entropy", m[1:2], torch.tensor([m32[1]]), torch.tensor([float(aux64["entropy_loss"])]), 2e-5, 1e-4)
    if normwise_grad:      # the rule on max-norms: see test_bptt_regimes_zstore_and_recompute
        g = op.grads.cpu().double()
        e_hip, e32, scale = float((g - g64).abs().max()), float((g_ref.double() - g64).abs().max()), float(g64.abs().max())
        assert e_hip <= 4.0 * e32 + 5e-6 + 1e-3 * scale, f"{tag} actor grad (normwise): |hip - fp64| {e_hip:.3g}, |fp32 - fp64| {e32:.3g}, |fp64| {scale:.3g}"
        return
    _assert_rule(f"{tag} actor grad", op.grads.cpu(), g_ref, g64, 5e-6, 1e-3)


def _bptt_band():
    """raw + c0 on a 0.005 grid across [-14.2, -13.4] (BPTT's lower clamp at softplus = 1e-6), less the 1e-3 around the crossing where
    fp32 cannot decide the side, plus the rest of the collapsed range."""
    band = [round(-14.2 + 0.005 * k, 3) for k in range(161)]
    pts = [-17.0, -16.0, -15.0, -12.0, -11.0, -10.0, -8.0, -6.0, -5.0] + band
    return [v for v in pts if abs(v - SP_1E6) > 1e-3 + 2e-4]      # (+ the rows' spread about the bias, ~1e-4)


def test_bptt_collapsed_std_band(dev):
    """Pendulum, H = 6: the std head's raw + c0 from -17 to -5, densely through the clamp band."""
    X, U, H, n = 3, 1, 6, 20
    failures = []
    for v in _bptt_band():
        cfg, ins, refs, m32 = _bptt_case(X, U, H, n, "pendulum", 0, raw=v, loc=0.0)
        ap, cp, x0, noise, s_mean, s_std, r_ms, extra = ins
        op = _run_hip(dev, cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, "pendulum", extra, n)
        try:
            _bptt_assert(op, refs, m32, X, U, H, n, f"raw+c0={v}")
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, f"{len(failures)} of {len(_bptt_band())} band points fail; first: {failures[:3]}"


@pytest.mark.parametrize("raw,loc,hidden_scale", [
    (-13.0, 1e-3, None),      # tiny loc with a collapsed std
    (-15.5, 1e-3, None),
    (0.0, 4.0, None),         # saturated squash: past the +-0.999 clamp
    (0.0, -8.0, None),
    (0.0, 12.0, None),        # tanh rounds to 1 in fp32
    (8.0, 0.0, None),         # large std
    (30.0, 0.0, None),
    (120.0, 0.0, None),       # raw + c0 > 100: the upper clamp
    (0.0, 0.3, 8.0),          # saturated hidden layers (swish)
])
def test_bptt_regimes_zstore_and_recompute(dev, raw, loc, hidden_scale):
    """Ensemble (4, 1, H = 5, n = 48, E = 5): parity by the rule with the z store and with recompute, and the two agree bit for bit.
    Tiny loc with a collapsed std makes q = (atanh(a) - mu) / sg carry mu's rounding times 1/sg into every row, and the gradient's
    small elements are sums that cancel: there the actor gradient is held to the rule on max-norms, not elementwise."""
    X, U, H, n, E = 4, 1, 5, 48, 5
    cfg, ins, refs, m32 = _bptt_case(X, U, H, n, "ensemble", E, raw=raw, loc=loc, hidden_scale=hidden_scale)
    ap, cp, x0, noise, s_mean, s_std, r_ms, extra = ins
    res = {}
    try:
        for mode in (-1, 0):
            _set_zstore(mode)
            op = _run_hip(dev, cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, "ensemble", extra, n)
            _bptt_assert(op, refs, m32, X, U, H, n, f"zstore={mode}", normwise_grad=(loc == 1e-3))
            res[mode] = (op.grads.clone(), op.metrics.clone(), op.transitions.clone())
    finally:
        _set_zstore(-1)
    for a, b in zip(res[-1], res[0]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ SAC (k_sac_fwd_bwd / k_sac_lean)
SAC_REGIMES = [
    dict(raw=-17.0), dict(raw=-13.8), dict(raw=-10.0), dict(raw=-5.0),           # collapsed std (sigma -> the 0.001 floor)
    dict(loc=4.0), dict(loc=-8.0), dict(loc=12.0),                               # saturated squash
    dict(loc=1e-3, raw=-14.0),                                                   # tiny loc with a collapsed std
    dict(raw=8.0), dict(raw=30.0),                                               # large std
    dict(loc=0.3, hidden_scale=8.0),                                             # saturated hidden layers
]


def _sac_case(X, U, hidden, B, reg, seed=0, q_hidden=None):
    cfg, st, batch, noise, nm, ns = _make(X, U, hidden, B, seed, True, q_hidden=q_hidden, discounting=0.99, reward_scaling=1.5)
    st.params = _place(st.params, cfg.policy_dims, 0, U, loc=reg.get("loc"), raw=reg.get("raw"), hidden_scale=reg.get("hidden_scale"))
    g32, l32 = osac.grads(cfg, st.params, st.target_q, batch, *noise, nm, ns)
    to64 = lambda t: None if t is None else t.double()
    g64, l64 = osac.grads(cfg, st.params.double(), st.target_q.double(), batch.double(), *[t.double() for t in noise], to64(nm), to64(ns))
    return cfg, st, batch, noise, nm, ns, (g32, torch.tensor([float(v) for v in l32])), (g64, torch.tensor([float(v) for v in l64]))


def _sac_assert(g, metrics, r32, r64, cfg, tag):
    """Gradients (tests/test_gpu_sac.py's atol / rtol against fp64) and the critic, actor and alpha losses."""
    (g32, l32), (g64, l64) = r32, r64
    _assert_rule(f"{tag} losses", metrics[:3], l32, l64, 2e-6, 2e-5)
    P, Q = cfg.P, cfg.Q
    for name, sl in (("policy", slice(0, P)), ("critic", slice(P, P + 2 * Q)), ("alpha", slice(P + 2 * Q, None))):
        _assert_rule(f"{tag} {name} grad", g[sl], g32[sl], g64[sl], 2e-6, 1e-4)


@pytest.mark.parametrize("reg", SAC_REGIMES, ids=lambda r: ",".join(f"{k}={v}" for k, v in r.items()))
def test_sac_regimes_generic_and_lean(dev, reg):
    """The benchmark networks (4, 1, 64 x 3, B = 64): the generic kernel and the lean kernel, parity by the rule, bit for bit equal."""
    X, U, hidden, B = 4, 1, (64, 64, 64), 64
    cfg, st, batch, noise, nm, ns, r32, r64 = _sac_case(X, U, hidden, B, reg)
    try:
        ups = {lean: _sac_run(dev, lean, cfg, st, batch, noise, nm, ns, B) for lean in (False, True)}
    finally:
        _set_lean(-1)
    (up_g, s_g), (up_l, s_l) = ups[False], ups[True]
    _sac_assert(s_g["grads"].cpu(), s_g["metrics"].cpu(), r32, r64, cfg, "generic")
    n = _slab_floats(up_g)
    assert torch.equal(s_g["workspace"][:n], s_l["workspace"][:n])
    for k in ("grads", "params", "target_q", "metrics"):
        assert torch.equal(s_g[k], s_l[k]), k


@pytest.mark.parametrize("reg", [dict(raw=-13.8), dict(loc=12.0), dict(raw=30.0), dict(loc=0.3, hidden_scale=8.0)],
                         ids=lambda r: ",".join(f"{k}={v}" for k, v in r.items()))
def test_sac_regimes_layered_path(dev, reg):
    """Unequal hidden widths, outside the fused kernels' range, take the layered path (tests/test_gpu_sac.py): parity by the rule."""
    X, U, B = 4, 2, 100
    cfg, st, batch, noise, nm, ns, r32, r64 = _sac_case(X, U, (48, 80), B, reg, q_hidden=(200, 72, 40))
    up = _updater(dev, cfg, B)
    up.load_state(st.params.to(dev), st.target_q.to(dev))
    up.sgd_step(batch.to(dev), nm.to(dev), ns.to(dev), *[t.to(dev) for t in noise])
    torch.cuda.synchronize()
    up.finalize()
    torch.cuda.synchronize()
    _sac_assert(up.grads.cpu(), up.metrics.cpu(), r32, r64, cfg, "layered")


@pytest.mark.parametrize("reg", [dict(raw=-13.8), dict(loc=-8.0), dict(loc=0.3, hidden_scale=8.0)],
                         ids=lambda r: ",".join(f"{k}={v}" for k, v in r.items()))
def test_sac_regimes_thin_layer_variant(dev, monkeypatch, reg):
    """k_sac_fwd_bwd's thin-layer variant (critic input x + u = 8, tests/test_gpu_sac.py): parity by the rule."""
    X, U, B = 7, 1, 64
    cfg, st, batch, noise, nm, ns, r32, r64 = _sac_case(X, U, (64, 64), B, reg)
    monkeypatch.setenv("MBPO_SAC_THIN", "1")
    up = _updater(dev, cfg, B)
    up.load_state(st.params.to(dev), st.target_q.to(dev))
    up.sgd_step(batch.to(dev), nm.to(dev), ns.to(dev), *[t.to(dev) for t in noise])
    up.finalize()
    torch.cuda.synchronize()
    _sac_assert(up.grads.cpu(), up.metrics.cpu(), r32, r64, cfg, "thin")


@pytest.mark.parametrize("act,scale", [("relu", 10.0), ("tanh", 6.0), ("swish", 8.0)])
def test_sac_saturated_hidden_layers_every_activation(dev, act, scale):
    """Hidden weights scaled by 6-10 (many |pre-activations| > 20) with relu, tanh and swish policy and critic layers, on widths
    (40, 72) / (136, 24) that sac_plan sends to the layered path.  Every path honours the activation (the fused kernels under relu and
    tanh: tests/test_gpu_activations.py); only the lean kernels refuse anything but swish and fall back to the generic ones."""
    X, U, B = 5, 2, 70
    cfg, st, batch, noise, nm, ns = _make(X, U, (40, 72), B, 21, True, q_hidden=(136, 24), policy_act=act, q_act=act, reward_scaling=1.5)
    st.params = _place(st.params, cfg.policy_dims, 0, U, loc=0.3, hidden_scale=scale)
    assert float((st.params[:cfg.P].abs()).max()) > 1.0
    g32, l32 = osac.grads(cfg, st.params, st.target_q, batch, *noise, nm, ns)
    to64 = lambda t: t.double()
    g64, l64 = osac.grads(cfg, st.params.double(), st.target_q.double(), batch.double(), *[t.double() for t in noise], to64(nm), to64(ns))
    up = _updater(dev, cfg, B, policy_activation=act, q_activation=act)
    up.load_state(st.params.to(dev), st.target_q.to(dev))
    up.sgd_step(batch.to(dev), nm.to(dev), ns.to(dev), *[t.to(dev) for t in noise])
    up.finalize()
    torch.cuda.synchronize()
    _sac_assert(up.grads.cpu(), up.metrics.cpu(), (g32, torch.tensor([float(v) for v in l32])),
                (g64, torch.tensor([float(v) for v in l64])), cfg, f"layered {act}")


# ------------------------------------------------------------------------------------------------ PPO (k_ppo_fwd_bwd / k_ppo_lean / layered)
PPO_REGIMES = [dict(raw=-17.0), dict(raw=-13.8), dict(raw=-8.0), dict(loc=8.0), dict(loc=-12.0), dict(raw=8.0), dict(raw=30.0),
               dict(loc=0.3, hidden_scale=8.0)]


def _ppo_case(X, U, hidden, B, T, reg, v_hidden=None, seed=0):
    """PPO minibatch with the policy placed in the regime; the stored raw actions are drawn around the policy's own loc at its own std
    (so the log-probs are finite), and the behaviour log-probs are the target ones shifted by N(0, 1.5): rho falls on both sides of
    the clip.  The entropy term is on (entropy_cost 1e-2)."""
    from oracle import ppo as oppo
    from test_gpu_ppo import _make as _ppo_make
    cfg, st, data, noise, _, _ = _ppo_make(X, U, hidden, B, T, seed, False, v_hidden=v_hidden, entropy_cost=1e-2, discounting=0.99,
                                           reward_scaling=0.5, gae_lambda=0.95, clipping_epsilon=0.2, normalize_advantage=True,
                                           lr=3e-4, wd=1e-5)
    st.params = torch.cat([_place(st.params[:cfg.P], cfg.policy_dims, 0, U, loc=reg.get("loc"), raw=reg.get("raw"),
                                  hidden_scale=reg.get("hidden_scale")), st.params[cfg.P:]])
    g = torch.Generator().manual_seed(seed + 100)
    o = X + U
    logits = onets.mlp_forward(st.params[:cfg.P], cfg.policy_dims, data[..., :X], cfg.policy_act)
    loc, scale = onets.split_logits(logits)
    z = loc + scale * torch.randn(B, T, U, generator=g)
    data[..., o + 3 + X:o + 3 + X + U] = z
    data[..., X:o] = torch.tanh(z)
    data[..., o + 2 + X] = onets.log_prob(logits, z) + 1.5 * torch.randn(B, T, generator=g)
    g32, t32, _, _ = oppo.grads(cfg, st.params, data, noise)
    g64, t64, _, _ = oppo.grads(cfg, st.params.double(), data.double(), noise.double())
    keys = ("total_loss", "policy_loss", "v_loss", "entropy_loss")
    return cfg, st, data, noise, (g32, torch.tensor([float(t32[k]) for k in keys])), (g64, torch.tensor([float(t64[k]) for k in keys]))


def _ppo_run(dev, cfg, st, data, noise, B, T, lean=None):
    import ctypes as C
    from mbpo import _hip
    from test_gpu_ppo import _updater as _ppo_updater
    lib = _hip.load()
    lib.mbpo_debug_set_ppo_lean.argtypes = [C.c_int]
    try:
        if lean is not None:
            lib.mbpo_debug_set_ppo_lean(lean)
        up = _ppo_updater(dev, cfg, B, T)
        up.load_state(st.params.to(dev))
        up.minibatch_step(data.to(dev), None, None, noise.to(dev))
        torch.cuda.synchronize()
    finally:
        lib.mbpo_debug_set_ppo_lean(-1)
    return up.grads.cpu().clone(), up.metrics.cpu().clone()


def _ppo_assert(g, m, r32, r64, tag, P=None):
    """P given (the lean kernel): its atol is 2e-6 times each network's largest gradient, test_gpu_ppo.py's lean-against-generic
    tolerance: it sums the tiles in another order, and at a collapsed std the policy's loc gradients are sums of ~1/sigma terms."""
    (g32, m32), (g64, m64) = r32, r64
    if P is None:
        _assert_rule(f"{tag} grad", g, g32, g64, 2e-6, 2e-4)              # tests/test_gpu_ppo.py against fp64
    else:
        for name, sl in (("policy", slice(0, P)), ("value", slice(P, None))):
            _assert_rule(f"{tag} {name} grad", g[sl], g32[sl], g64[sl], 2e-6 * max(float(g64[sl].abs().max()), 1e-3), 2e-4)
    _assert_rule(f"{tag} loss terms", m, m32, m64, 1e-5, 2e-5)


@pytest.mark.parametrize("reg", PPO_REGIMES, ids=lambda r: ",".join(f"{k}={v}" for k, v in r.items()))
def test_ppo_regimes_generic_and_lean(dev, reg):
    """The 64 x 3 networks (x = 4, B = 32, T = 8): the generic and the lean loss kernels, both by the rule; lean against generic with
    test_gpu_ppo.py's tolerance (another cross-tile summation order)."""
    X, U, B, T = 4, 1, 32, 8
    cfg, st, data, noise, r32, r64 = _ppo_case(X, U, (64, 64, 64), B, T, reg)
    rho = torch.exp(onets.log_prob(onets.mlp_forward(st.params[:cfg.P], cfg.policy_dims, data[..., :X]), data[..., X + U + 3 + X:X + U + 3 + X + U])
                    - data[..., X + U + 2 + X])
    assert bool((rho < 0.8).any()) and bool((rho > 1.2).any())                 # the clip is driven from both sides
    g0, m0 = _ppo_run(dev, cfg, st, data, noise, B, T, lean=0)
    g1, m1 = _ppo_run(dev, cfg, st, data, noise, B, T, lean=1)
    _ppo_assert(g0, m0, r32, r64, "generic")
    _ppo_assert(g1, m1, r32, r64, "lean", P=cfg.P)
    P = cfg.P
    for name, sl in (("policy", slice(0, P)), ("value", slice(P, None))):
        scale = float(g0[sl].abs().max())
        torch.testing.assert_close(g1[sl], g0[sl], atol=2e-6 * max(scale, 1e-3), rtol=2e-5, msg=lambda m: f"{name}: {m}")
    torch.testing.assert_close(m1, m0, rtol=2e-5, atol=1e-6)


@pytest.mark.parametrize("reg", [dict(raw=-13.8), dict(loc=8.0), dict(raw=30.0), dict(loc=0.3, hidden_scale=8.0)],
                         ids=lambda r: ",".join(f"{k}={v}" for k, v in r.items()))
def test_ppo_regimes_layered_path(dev, reg):
    """Unequal hidden widths (tests/test_gpu_ppo.py's layered case) take the layered path: parity by the rule."""
    X, U, B, T = 4, 2, 20, 7
    cfg, st, data, noise, r32, r64 = _ppo_case(X, U, (48, 80), B, T, reg, v_hidden=(200, 72, 40))
    g, m = _ppo_run(dev, cfg, st, data, noise, B, T)
    _ppo_assert(g, m, r32, r64, "layered")


# ------------------------------------------------------------------------------------------------ rollout (k_model_rollout64 / k_rollout_lean)
ROLLOUT_REGIMES = [dict(raw=-17.0), dict(raw=-13.8), dict(raw=-8.0), dict(loc=8.0), dict(loc=-12.0), dict(loc=1e-3, raw=-14.0),
                   dict(raw=8.0), dict(raw=30.0), dict(loc=0.3, hidden_scale=8.0)]


def _rollout_case(dev, reg, deterministic, N=77, S=4, L=5, X=4, U=1, E=5, hidden=(64, 64, 64), seed=0):
    """Ensemble system ('mean' mode), ppo_extras on (the z and log-prob columns): rows by the rule against oracle/rollout.py in fp32 and
    fp64 on the same inputs."""
    from mbpo import _hip, ops
    from oracle import rollout as oro
    from oracle import systems as osys
    g = torch.Generator().manual_seed(seed)
    pdims, ddims = [X, *hidden, 2 * U], [X + U, *hidden, 2 * X]
    ppar = onets.init_mlp_flat(pdims, g) + 0.02 * torch.randn(onets.n_params(pdims), generator=g)
    ppar = _place(ppar, pdims, 0, U, loc=reg.get("loc"), raw=reg.get("raw"), hidden_scale=reg.get("hidden_scale"))
    dpar = torch.cat([onets.init_mlp_flat(ddims, g) * 0.5 + 0.01 * torch.randn(onets.n_params(ddims), generator=g) for _ in range(E)])
    obs0, first = torch.randn(N, X, generator=g), torch.randn(N, X, generator=g)
    steps0 = torch.randint(0, L, (N,), generator=g).float()
    done0 = (torch.rand(N, generator=g) < 0.2).float()
    pnoise = torch.randn(S, N, U, generator=g)
    tgt, q, r = torch.randn(X, generator=g), torch.rand(X, generator=g), torch.rand(U, generator=g) * 0.1
    outs = []
    for dt in (torch.float32, torch.float64):
        c = lambda t: t.to(dt)
        osystem = osys.EnsembleSystem(c(dpar), ddims, E, X, U, mode="mean", predict_delta=True, min_std=1e-3,
                                      reward_fn=lambda x, u: osys.quadratic_reward(x, u, c(tgt), c(q), c(r)))
        _, rows = oro.rollout(osystem, c(ppar), pdims, oro.EnvState(c(obs0), c(first), c(steps0), c(done0)), S, L, 1,
                              policy_noise=c(pnoise), deterministic=deterministic, ppo_extras=True)
        outs.append(rows)
    rows = ops.model_rollout(policy_params=ppar.to(dev), policy_spec=ops.MlpSpec(pdims, "swish", 1), x_dim=X, u_dim=U,
                             obs=obs0.to(dev), first_obs=first.to(dev), steps=steps0.to(dev), done=done0.to(dev), n_steps=S,
                             episode_length=L, action_repeat=1, reward_params=torch.cat([tgt, q, r]).to(dev), deterministic=deterministic,
                             ppo_extras=True, policy_noise=pnoise.to(dev), system_kind=_hip.SYS_ENSEMBLE, dyn_params=dpar.to(dev),
                             dyn_spec=ops.MlpSpec(ddims, "swish", E), ens_mode=_hip.ENS_MEAN, ens_predict_delta=True,
                             ens_sample_noise=False, ens_min_std=1e-3, reward_kind=_hip.REWARD_QUADRATIC)
    torch.cuda.synchronize()
    return rows.cpu(), outs[0], outs[1]


@pytest.mark.parametrize("deterministic", [False, True], ids=["sampled", "deterministic"])
@pytest.mark.parametrize("reg", ROLLOUT_REGIMES, ids=lambda r: ",".join(f"{k}={v}" for k, v in r.items()))
def test_rollout_regimes_generic_and_lean(dev, reg, deterministic):
    """Rows (observation, action, reward, next observation, z and log-prob) by the rule with tests/test_gpu_rollout.py's 2e-4; the lean
    kernel (one and two tiles in flight) equal to the generic kernel bit for bit."""
    from test_gpu_rollout import _set_rollout_lean
    res = {}
    try:
        for mode in (0, 3, 2):
            _set_rollout_lean(mode)
            res[mode], r32, r64 = _rollout_case(dev, reg, deterministic)
    finally:
        _set_rollout_lean(-1)
    _assert_rule("rows", res[0], r32, r64, 2e-4, 2e-4)
    assert torch.equal(res[0], res[3]) and torch.equal(res[0], res[2])


# ------------------------------------------------------------------------------------------------ BPTT wide path
@pytest.mark.parametrize("raw,loc", [(-13.81, 0.0), (-15.0, 0.0), (0.0, 12.0), (120.0, 0.0)])
def test_bptt_wide_path_regimes_against_fused(dev, raw, loc):
    """BpttActorGradGeneric (a user torch System, the non-fused path) and the fused kernel on the same placed actor: both by the rule,
    and each within the rule's bound of the other."""
    from mbpo import ops
    from test_gpu_bptt_generic import _user_pendulum_system
    X, U, H, n = 3, 1, 6, 20
    cfg, ins, refs, m32 = _bptt_case(X, U, H, n, "pendulum", 0, raw=raw, loc=loc)
    ap, cp, x0, noise, s_mean, s_std, r_ms, extra = ins
    user = _user_pendulum_system()
    op = ops.BpttActorGradGeneric(x_dim=X, u_dim=U, horizon=H, actor_dims=cfg.actor_dims, critic_dims=cfg.critic_dims, n=n, device=dev,
                                  init_stddev=cfg.init_stddev, discount=cfg.discount, lambda_=cfg.lambda_, ent_coef=cfg.ent_coef)
    op(actor_params=ap.to(dev), target_critic_params=cp.to(dev), init_states=x0.to(dev), state_mean=s_mean.to(dev), state_std=s_std.to(dev),
       reward_mean_std=r_ms.to(dev), system=user, system_params=user.init_params(0), act_noise=noise.to(dev))
    torch.cuda.synchronize()
    _bptt_assert(op, refs, m32, X, U, H, n, "wide")
    fused = _run_hip(dev, cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, "pendulum", extra, n)
    _bptt_assert(fused, refs, m32, X, U, H, n, "fused")
    g_ref, _, g64, _, _ = refs
    bound = 2 * (4 * (g_ref.double() - g64).abs() + 5e-6 + 1e-3 * g64.abs())
    assert bool(((op.grads.cpu().double() - fused.grads.cpu().double()).abs() <= bound).all())


# ------------------------------------------------------------------------------------------------ ens_nll_grads
@pytest.mark.parametrize("raw,resid", [(-20.0, 5.0), (-8.0, 20.0), (-30.0, 1.0)])
def test_ens_nll_grads_at_min_std_and_large_residuals(dev, raw, resid):
    """Member sigma = softplus(raw) + min_std pinned at min_std (raw << 0) with residuals of 1-20 (so (r / sigma)^2 ~ 1e6-4e8): libm
    softplus / log in the kernel.  Losses by the rule; the gradient by the rule in the L2 norm, tests/test_gpu_ensemble_train.py's
    measure against fp64 (its elements are batch sums of terms ~1/sigma^2 = 1e6 that cancel to O(1), so a few elements land outside
    an elementwise bound in either precision)."""
    from mbpo import ops
    from oracle import ensemble as oens
    X, U, E, B, hidden = 4, 1, 3, 64, (64, 64, 64)
    g = torch.Generator().manual_seed(7)
    dims = [X + U, *hidden, 2 * X]
    P = onets.n_params(dims)
    members = []
    for _ in range(E):
        p = onets.init_mlp_flat(dims, g) + 0.02 * torch.randn(P, generator=g)
        members.append(_place(p, dims, 0, X, raw=raw, w_loc=1.0, w_raw=1e-3))
    params = torch.cat(members)
    R, D = 200, 2 * X + U + 2
    rows = torch.randn(R, D, generator=g)
    rows[:, X + U + 2:] = rows[:, :X] + resid * torch.randn(R, X, generator=g)
    idx = torch.randint(0, R, (E, B), generator=g)
    g32, l32 = oens.nll_grads(params, dims, E, rows, idx, X, U, True, 1e-3)
    g64, l64 = oens.nll_grads(params.double(), dims, E, rows.double(), idx, X, U, True, 1e-3)
    op = ops.EnsembleNllGrad(x_dim=X, u_dim=U, spec=ops.MlpSpec(dims, "swish", E), batch=B, device=dev, predict_delta=True)
    got = op(params.to(dev), rows.to(dev), idx.to(torch.int32).to(dev))
    torch.cuda.synchronize()
    _assert_rule("nll losses", op.metrics.cpu(), l32, l64, 2e-5, 2e-5)
    e_hip, e32 = float((got.cpu().double() - g64).norm() / g64.norm()), float((g32.double() - g64).norm() / g64.norm())
    assert e_hip <= 4.0 * e32 + 5e-5, f"nll grads: relative L2 error {e_hip:.3g}, fp32 oracle {e32:.3g}"
