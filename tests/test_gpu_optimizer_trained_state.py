"""GPU: the four places that form the AdamW update, handed a learner that is thousands of steps old.

  csrc/optim.hip k_adamw_step              the generic optimizer (BPTT actor and critic, EnsembleDynamics.fit), with its Polyak target
  csrc/sac_shared.hpp sac_adam             from k_sac_apply (three launches), k_sac_reduce_apply (two launches) and sac_clip_fixup
                                           (a clipped group's step redone from the undo log, bias corrections from undo_count[2..3])
  csrc/ppo.hip ppo_adamw                   from k_ppo_reduce (fused apply), k_ppo_clip_apply and k_ppo_apply (split path)

Every other optimizer test starts at count 0 with zero moments and takes at most ten steps, where the update is +-1 whatever the bias
corrections are.  Here the state is tests/optimizer_state_cases.py's: moments of mixed sign over seven decades, m / sqrt(v) on both
sides of 1, a few v exactly 0 and a few ~1e-30, parameters whose ulp is below 1e-6 lr, and counts 0, 1, 9, 999, 99 999 and 2^24 - 2
(from which the float32 counter reaches 2^24 and stays: the stored count is pinned, the update is checked against the oracle run
with the true integer count).

Reference: the float64 oracles (oracle/sac.py adamw_step / sgd_step, oracle/bptt.py apply_if_finite_adamw, oracle/ppo.py
minibatch_step) with optax's constants as float32 arithmetic sees them, widened: f32(0.9), f32(0.999), f32(0.1), f32(0.001),
f32(1e-8).  SAC and PPO gradients are the device's own (grad_override): the optimizer is under test, not the backward pass.

Tolerance: measured, at run time.  The same steps run through the same oracle in float32; its largest error against the float64
oracle, per tensor and per (path, count) — pooled over the path's sizes, variants and steps — in the units
    params, target: |d| / lr          m: |d| / max |m|          v: |d| / max |v|
times 4 (FMA contraction, 1-2 ulp of the device powf) is what the kernel is allowed, over EVERY element.  step_count is exact.
The float32 oracle is float32 throughout: its constants are float32 tensors (optimizer_state_cases.adam_in), so it forms b^count with
the host's powf and 1 - b^count in float32, as optax in float32 and the kernels do.  At counts 2 and 3 that subtraction cancels
seven bits of 0.999^count and the float32 result is up to 1.2e-5 of an update off: the early columns of the table show it.  That
is float32's error, the reference's as much as the kernel's, not a kernel mistake; a correction formed as -expm1(count ln b)
would be 100 times closer, but it changes the last bits of every early step and with them which seeds of the chaotic learning
tests (test_gpu_host_api.py) end above their thresholds, so the kernels keep optax's form.
The float32 oracle's error at these cases (what is multiplied by 4), on an MI355X's own SAC and PPO gradients (the test prints each
as it runs; `sac/<shape>/median` is the run whose max_grad_norm clips some steps, `ppo/clipped` the one that clips every step):

  path                                          count:          0         1         9       999    99 999  2^24 - 2
  generic (n 1, 255, 1027)                      params    1.0e-05   1.2e-05   1.1e-06   1.5e-06   1.8e-06   1.7e-06
                                                target    2.1e-07   2.2e-07   2.0e-07   2.3e-07   1.6e-07   1.6e-07
                                                m         1.6e-07   1.6e-07   1.0e-07   1.4e-07   8.5e-08   1.1e-07
                                                v         1.4e-07   7.0e-08   9.2e-08   6.0e-08   9.7e-08   4.9e-08
  sac/last_element_alone_one_tile/never clips   params    1.5e-05   1.6e-05   1.8e-06   2.1e-06   2.6e-06   2.4e-06
                                                target    4.8e-07   4.9e-07   4.6e-07   4.8e-07   4.7e-07   5.2e-07
                                                m         1.2e-07   1.1e-07   1.7e-07   1.6e-07   1.5e-07   1.9e-07
                                                v         8.7e-08   1.1e-07   8.2e-08   1.2e-07   1.0e-07   8.4e-08
  sac/last_element_alone_one_tile/median        params    1.5e-05   1.6e-05   1.7e-06   2.7e-06   2.6e-06   2.8e-06
                                                target    4.8e-07   5.0e-07   4.6e-07   5.1e-07   4.7e-07   5.1e-07
                                                m         1.2e-07   1.1e-07   1.7e-07   1.6e-07   1.5e-07   1.9e-07
                                                v         8.7e-08   1.1e-07   8.2e-08   1.2e-07   1.0e-07   8.4e-08
  sac/seventeen_tiles/never clips               params    1.4e-05   1.6e-05   1.7e-06   1.7e-06   2.8e-06   2.6e-06
                                                target    9.3e-07   9.2e-07   9.0e-07   1.0e-06   9.2e-07   1.0e-06
                                                m         1.6e-07   1.6e-07   1.8e-07   1.5e-07   1.7e-07   1.8e-07
                                                v         8.7e-08   9.3e-08   1.5e-07   1.1e-07   8.0e-08   9.9e-08
  sac/seventeen_tiles/median                    params    1.5e-05   1.6e-05   1.7e-06   2.0e-06   2.3e-06   2.5e-06
                                                target    9.3e-07   9.2e-07   9.0e-07   1.0e-06   9.2e-07   1.0e-06
                                                m         1.6e-07   1.6e-07   1.8e-07   1.5e-07   1.7e-07   1.8e-07
                                                v         8.7e-08   9.3e-08   1.5e-07   1.1e-07   8.0e-08   9.9e-08
  ppo/unclipped                                 params    1.1e-05   1.2e-05   1.2e-06   1.8e-06   2.0e-06   1.8e-06
                                                m         1.3e-07   1.8e-07   1.4e-07   1.2e-07   1.3e-07   1.2e-07
                                                v         1.2e-07   5.0e-08   9.0e-08   4.2e-08   5.6e-08   6.0e-08
  ppo/clipped                                   params    1.1e-05   1.2e-05   1.3e-06   1.5e-06   1.8e-06   1.6e-06
                                                m         1.1e-07   1.3e-07   1.2e-07   9.8e-08   1.1e-07   1.1e-07
                                                v         1.2e-07   5.0e-08   9.0e-08   4.2e-08   5.6e-08   6.0e-08

Arms that must agree bit for bit do: SAC three-launch == two-launch (clip check deferred and resolved every step) == the same with
the generic forward/backward kernel where the default dispatch takes k_sac_lean; PPO fused == split == clip-above-the-norm, and
fused clipped == split clipped.
"""
import statistics

import pytest
import torch

import optimizer_state_cases as oc
import stream_cases as sc
from oracle import ppo as oppo
from oracle import sac as osac
from ppo_brax_env_ref import clip_by_global_norm as ppo_clip
from test_gpu_ppo import _make as _ppo_make, _updater as _ppo_updater
from test_gpu_sac_lean import _set_lean
from test_gpu_sac_reduce_apply import CASES as SAC_CASES, _case, _updater

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32


def _report(path, c, measured):
    print(f"TOL {path} c={c}: " + "  ".join(f"{k} {measured[k]:.1e}" for k in oc.TENSORS if k in measured))


def _check(got, ref64, measured, what):
    ok, bad = oc.within(oc.errors(got, ref64), measured)
    assert ok, (what, "error, allowed:", bad, [oc.worst_element(got, ref64, k) for k in bad])


# ------------------------------------------------------------------------------------------------------------- generic AdamW
@pytest.mark.parametrize("c", oc.COUNTS)
def test_generic_adamw_from_a_trained_state(dev, c):
    """ops.AdamW at n = 1, 255 and 1027 (a vector body and a scalar tail), without a target, with one, and with one 4 bytes off
    16-byte alignment (scalars only), apply_if_finite on and off: three chained steps, every step against the float64 oracle."""
    from mbpo import ops
    measured, chains = oc.generic_measured(c)
    _report("generic", c, measured)
    for n in oc.GENERIC_NS:
        p0, m0, v0, t0, _ = oc.trained_state(n, c)
        grads = oc.generic_grads(n, c)
        for target_k in (None, 0, 1):
            for aif in (False, True):
                what = ("generic", c, n, target_k, aif)
                opt = ops.AdamW(n, dev, lr=oc.LR, weight_decay=oc.GENERIC_WD, apply_if_finite=aif)
                opt.load_state(m0.to(dev), v0.to(dev), float(c))
                dp = p0.to(dev)
                dt = None if target_k is None else sc.misaligned(t0.to(dev), target_k)
                assert all(sc.aligned16(t) for t in (dp, opt.m, opt.v))
                if dt is not None:
                    assert dt.data_ptr() % 16 == 4 * target_k
                ref = chains[(n, target_k is not None)]
                for i, g in enumerate(grads):
                    dg = g.to(dev)
                    assert sc.aligned16(dg)
                    opt.step(dp, dg, target=dt, tau=oc.TAU)
                    torch.cuda.synchronize()
                    got = dict(params=dp, m=opt.m, v=opt.v, target=dt)
                    _check(got, ref[i], measured, what + (i,))
                    assert float(opt.count) == oc.stored_count(c, i + 1), what + (i,)
                    assert ref[i]["count"] == c + i + 1                    # the oracle ran with the true integer count
                    norm = float(g.double().norm())
                    assert abs(float(opt.grad_norm) - norm) <= 1e-5 * norm, what + (i,)
                if dt is not None:
                    assert sc.slack_untouched(dt)


@pytest.mark.parametrize("aif", [False, True])
def test_generic_adamw_squared_gradient_overflow(dev, aif):
    """A gradient of 1e20 squares to +inf in float32.  optax in float32: v = +inf, m finite, the update m_hat / (inf + eps) = 0 so the
    parameter moves by the weight-decay term alone, global_norm = +inf, and apply_if_finite does NOT skip: the gradient is finite.
    One element in the vector body, one in the scalar tail.  Properties, not the float64 oracle (which does not overflow)."""
    from mbpo import ops
    n, c = 1027, 999
    p0, m0, v0, t0, _ = oc.trained_state(n, c)
    g = oc.generic_grads(n, c)[0]
    hot = [5, n - 1]
    g[hot[0]], g[hot[1]] = 1e20, -1e20
    opt = ops.AdamW(n, dev, lr=oc.LR, weight_decay=oc.GENERIC_WD, apply_if_finite=aif)
    opt.load_state(m0.to(dev), v0.to(dev), float(c))
    dp, dt = p0.to(dev), t0.to(dev)
    opt.step(dp, g.to(dev), target=dt, tau=oc.TAU)
    torch.cuda.synchronize()
    p, m, v, t = dp.cpu(), opt.m.cpu(), opt.v.cpu(), dt.cpu()
    assert float(opt.count) == c + 1                                               # not skipped
    assert float(opt.grad_norm) == float("inf")
    for i in hot:
        assert float(v[i]) == float("inf")
        want_m = oc.B1 * float(m0[i]) + oc.ONE_MINUS_B1 * float(g[i])
        assert bool(torch.isfinite(m[i])) and abs(float(m[i]) - want_m) <= 1e-6 * abs(want_m)
        want_p = float(p0[i]) - oc.LR * oc.GENERIC_WD * float(p0[i])               # weight decay alone
        ulp = float(torch.nextafter(p0[i].abs(), torch.tensor(float("inf"))) - p0[i].abs())
        assert abs(float(p[i]) - want_p) <= ulp, (i, float(p[i]), want_p)
        assert float(p[i]) != float(p0[i])
        want_t = (1 - oc.TAU) * float(t0[i]) + oc.TAU * want_p
        assert abs(float(t[i]) - want_t) <= 2 * ulp
    # every other element took an ordinary step: the float64 oracle within the measured tolerance of this very step
    cold = torch.ones(n, dtype=torch.bool)
    cold[hot] = False
    st = (p0, m0, v0, t0, c)
    g_cold = torch.where(cold, g, torch.zeros(()))
    r64 = oc.generic_oracle(F64, st, [g_cold], True, aif)[0]
    r32 = oc.generic_oracle(F32, st, [g_cold], True, aif)[0]
    sel = lambda d: {k: d[k][cold] for k in oc.TENSORS}
    measured = oc.errors(sel(r32), sel(r64))
    _check(sel(dict(params=p, m=m, v=v, target=t)), sel(r64), measured, ("overflow, the other elements", aif))


# ----------------------------------------------------------------------------------------------------------------------- SAC
SAC_STEPS = 4
SAC_KEYS = ("params", "adam_m", "adam_v", "target_q", "grads", "metrics", "metrics_accum", "step_count")
NO_CLIP = oc.f32(1e5)


@pytest.fixture
def _lean_default():
    yield
    _set_lean(-1)


def _sac_inputs(name, c):
    B, (cfg, st, batch, _, nm, ns) = _case(name)
    cfg.lr_policy = cfg.lr_q = cfg.lr_alpha = oc.LR
    cfg.wd_q, cfg.tau = oc.NET_WD, oc.TAU
    p, m, v, _, _ = oc.trained_state(cfg.NP, c, seed=1, params=oc.network_params(st.params))
    tq = oc.network_params(st.target_q)
    assert oc.ulp_over_lr(p) < 1e-6 and oc.ulp_over_lr(tq) < 1e-6
    return B, cfg, dict(params=p, target_q=tq, adam_m=m, adam_v=v), batch, nm, ns


def _bits(t):
    return t.detach().clone().view(torch.int32)


def _sac_chain(dev, B, cfg, state, c, batch, nm, ns, two_launch, defer, max_norm, per_step=False):
    """SAC_STEPS chained sgd_steps from the trained state.  Returns (final state bits, clip events, per-step records): the records
    (the gradient, its three group norms, the state) only from the three-launch step, whose state is final after every step."""
    from mbpo import ops
    cfg.max_grad_norm = max_norm
    up = _updater(dev, cfg, B, two_launch=two_launch)
    up.load_state(state["params"].to(dev), state["target_q"].to(dev), state["adam_m"].to(dev), state["adam_v"].to(dev), float(c))
    rng = ops.make_rng(dev, 11)
    recs = []
    for i in range(SAC_STEPS):
        up.sgd_step(torch.roll(batch, i, 0).to(dev), nm.to(dev), ns.to(dev), seed=3, offset=(7 + i) << 32, rng_dev=rng, defer_clip_check=defer)
        if per_step:
            assert not two_launch
            torch.cuda.synchronize()
            g = up.grads.cpu().clone()
            recs.append(dict(grads=g, params=up.params.cpu().clone(), target=up.target_q.cpu().clone(), m=up.adam_m.cpu().clone(),
                             v=up.adam_v.cpu().clone(), count=float(up.step_count)))
    if two_launch:
        assert int(up._control[0]) == SAC_STEPS, "the two-launch step did not run k_sac_reduce_apply"
    events = up.clip_events()
    up.finalize()
    torch.cuda.synchronize()
    return {k: _bits(getattr(up, k)) for k in SAC_KEYS}, events, recs


def _sac_oracle(dtype, cfg, state, c, batch, nm, ns, recs, max_norm):
    """oracle/sac.py sgd_step in `dtype` from the same state, on the device's gradients, with the TRUE integer count."""
    cfg.max_grad_norm = max_norm
    st = osac.SacState(state["params"].to(dtype), state["target_q"].to(dtype), state["adam_m"].to(dtype), state["adam_v"].to(dtype), c)
    zero = torch.zeros(batch.shape[0], cfg.u_dim, dtype=dtype)
    out = []
    for i, r in enumerate(recs):
        st, _, _ = osac.sgd_step(cfg, st, torch.roll(batch, i, 0).to(dtype), zero, zero, zero, nm.to(dtype), ns.to(dtype),
                                 grad_override=r["grads"].to(dtype), adam=oc.adam_in(dtype))
        out.append(dict(params=st.params, target=st.target_q, m=st.adam_m, v=st.adam_v, count=st.count))
    return out


def _group_norms(cfg, g):
    P, Q = cfg.P, cfg.Q
    g = g.double()
    return [float(g[:P].norm()), float(g[P:P + 2 * Q].norm()), float(g[P + 2 * Q:].norm())]


@pytest.mark.parametrize("c", oc.COUNTS)
@pytest.mark.parametrize("name", ["last_element_alone_one_tile", "seventeen_tiles"])
def test_sac_optimizer_from_a_trained_state(dev, _lean_default, name, c):
    """Four chained SAC steps from the trained state at a max_grad_norm that never clips and at the median of the per-step norms
    (some steps clip: sac_clip_fixup redoes them from the undo log with the corrections the speculative step stored):
    the three-launch step against the float64 oracle after every step; the two-launch step, clip check deferred and resolved every
    step, and — where the default dispatch takes k_sac_lean — both forward/backward kernels, all bit for bit the same."""
    B, cfg, state, batch, nm, ns = _sac_inputs(name, c)
    lean_shape = tuple(SAC_CASES[name][:4]) == (4, 1, (64, 64, 64), (64, 64, 64))      # what csrc/sac_lean.hip is specialised for
    arms = (1, 0) if lean_shape else (-1,)
    thr = None
    for mode in ("never clips", "median"):
        if mode == "never clips":
            max_norm = NO_CLIP
        else:
            assert thr is not None
            max_norm = thr
        _set_lean(arms[0])
        ref, ev_ref, recs = _sac_chain(dev, B, cfg, state, c, batch, nm, ns, False, False, max_norm, per_step=True)
        norms = [_group_norms(cfg, r["grads"]) for r in recs]
        assert all(torch.isfinite(r["grads"]).all() and float(r["grads"].abs().sum()) > 0 for r in recs)
        if mode == "never clips":
            assert ev_ref == 0 and max(max(n) for n in norms) < 0.5 * NO_CLIP
            thr = oc.f32(statistics.median(max(n) for n in norms))        # four steps: midway between the two middle norms
        else:
            print(name, c, "per-step group norms", norms, "threshold", max_norm, "clip events", ev_ref)
            assert 0 < ev_ref < SAC_STEPS, (ev_ref, norms, max_norm)          # otherwise the fix-up path was not exercised
            # no group norm within float32 rounding of the threshold: the oracle's clip decision is the kernel's
            assert all(abs(x / max_norm - 1) > 1e-5 for n in norms for x in n), (norms, max_norm)
            assert ev_ref == sum(any(x >= max_norm for x in n) for n in norms)
        r64 = _sac_oracle(F64, cfg, state, c, batch, nm, ns, recs, max_norm)
        r32 = _sac_oracle(F32, cfg, state, c, batch, nm, ns, recs, max_norm)
        measured = {}
        for a, b in zip(r32, r64):
            oc.pool(measured, oc.errors(a, b))
        _report(f"sac/{name}/{mode}", c, measured)
        for i, (r, o) in enumerate(zip(recs, r64)):
            _check(r, o, measured, (name, c, mode, "three-launch, step", i))
            assert r["count"] == oc.stored_count(c, i + 1) and o["count"] == c + i + 1
        for lean in arms:
            _set_lean(lean)
            for two_launch, defer in ((False, False), (True, True), (True, False)):
                if lean == arms[0] and not two_launch:
                    continue                                                  # the reference run itself
                got, ev, _ = _sac_chain(dev, B, cfg, state, c, batch, nm, ns, two_launch, defer, max_norm)
                for k in SAC_KEYS:
                    assert torch.equal(got[k], ref[k]), (name, c, mode, "lean" if lean else "generic", two_launch, defer, k)
                assert ev == ev_ref
    assert float(ref["step_count"].view(torch.float32)) == oc.stored_count(c, SAC_STEPS)


# ----------------------------------------------------------------------------------------------------------------------- PPO
PPO_STEPS = 3
PPO_KEYS = ("params", "adam_m", "adam_v", "grads", "metrics", "step_count")
PPO_B, PPO_T = 32, 5


def _ppo_chain(dev, cfg, state, c, data, noise, nm, ns, **kw):
    up = _ppo_updater(dev, cfg, PPO_B, PPO_T, **kw)
    up.load_state(state["params"].to(dev), state["adam_m"].to(dev), state["adam_v"].to(dev), float(c))
    recs = []
    for i in range(PPO_STEPS):
        up.minibatch_step(torch.roll(data, i, 0).to(dev), nm.to(dev), ns.to(dev), torch.roll(noise, i, 0).to(dev))
        torch.cuda.synchronize()
        recs.append({k: getattr(up, k).cpu().clone() for k in PPO_KEYS})
    return recs


def _ppo_oracle(dtype, cfg, state, c, data, noise, nm, ns, recs, max_norm):
    st = oppo.PpoState(state["params"].to(dtype), state["adam_m"].to(dtype), state["adam_v"].to(dtype), c)
    out = []
    for i, r in enumerate(recs):
        g = ppo_clip(r["grads"].to(dtype), max_norm)
        st, _, _ = oppo.minibatch_step(cfg, st, torch.roll(data, i, 0).to(dtype), torch.roll(noise, i, 0).to(dtype), nm.to(dtype),
                                       ns.to(dtype), grad_override=g, adam=oc.adam_in(dtype))
        out.append(dict(params=st.params, m=st.adam_m, v=st.adam_v, count=st.count))
    return out


@pytest.mark.parametrize("c", oc.COUNTS)
def test_ppo_optimizer_from_a_trained_state(dev, c):
    """Three minibatch updates at B = 32, T = 5 from the trained state through ppo_adamw's three call sites: k_ppo_reduce (the fused
    apply), k_ppo_apply (the split path, with a seam where a collective would sit) and k_ppo_clip_apply (max_grad_norm > 0), once
    above every norm (bit for bit the unclipped step) and once at half the smallest norm (every step clips), fused and split."""
    cfg, st, data, noise, nm, ns = _ppo_make(3, 1, (64, 64, 64), PPO_B, PPO_T, 12, True, entropy_cost=1e-2, lr=oc.LR, wd=oc.NET_WD)
    p, m, v, _, _ = oc.trained_state(cfg.P + cfg.V, c, seed=2, params=oc.network_params(st.params))
    assert oc.ulp_over_lr(p) < 1e-6
    state = dict(params=p, adam_m=m, adam_v=v)
    seam = lambda t: None                                   # a collective's place: mbpo_ppo_grads, the hook, mbpo_ppo_apply
    fused = _ppo_chain(dev, cfg, state, c, data, noise, nm, ns)
    norms = [float(r["grads"].double().norm()) for r in fused]
    assert all(n > 0 for n in norms)
    thr = oc.f32(0.5 * min(norms))
    groups = {None: [("fused", fused), ("split", _ppo_chain(dev, cfg, state, c, data, noise, nm, ns, all_reduce=seam)),
                     ("clip above the norm", _ppo_chain(dev, cfg, state, c, data, noise, nm, ns, max_grad_norm=1e30))],
              thr: [("clipped fused", _ppo_chain(dev, cfg, state, c, data, noise, nm, ns, max_grad_norm=thr)),
                    ("clipped split", _ppo_chain(dev, cfg, state, c, data, noise, nm, ns, max_grad_norm=thr, all_reduce=seam))]}
    for max_norm, runs in groups.items():
        path = "ppo/unclipped" if max_norm is None else "ppo/clipped"
        recs = runs[0][1]
        if max_norm is not None:
            clipped_norms = [float(r["grads"].double().norm()) for r in recs]
            assert all(n > max_norm * (1 + 1e-5) for n in clipped_norms), (clipped_norms, max_norm)      # every step clips
        for arm, other in runs[1:]:
            for i in range(PPO_STEPS):
                for k in PPO_KEYS:
                    assert torch.equal(_bits(other[i][k]), _bits(recs[i][k])), (c, arm, "against", runs[0][0], "step", i, k)
        r64 = _ppo_oracle(F64, cfg, state, c, data, noise, nm, ns, recs, max_norm)
        r32 = _ppo_oracle(F32, cfg, state, c, data, noise, nm, ns, recs, max_norm)
        measured = {}
        for a, b in zip(r32, r64):
            oc.pool(measured, oc.errors(a, b))
        _report(path, c, measured)
        for i, (r, o) in enumerate(zip(recs, r64)):
            got = dict(params=r["params"], m=r["adam_m"], v=r["adam_v"])
            _check(got, o, measured, (path, c, "step", i))
            assert float(r["step_count"]) == oc.stored_count(c, i + 1) and o["count"] == c + i + 1
