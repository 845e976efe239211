"""The term reward (MBPO_REWARD_TERMS, include/mbpo_hip.h "term rewards") without a device: the constants and the packed layout against
the header, every constructor refusal, from_quadratic against the quadratic formula, mbpo_reward_eval's declaration and argument
checks, the rollout's and BPTT's refusals, and the fp32 restatement against the fp64 one on the cases' inputs."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

import term_reward_cases as tc
import term_reward_ref as tr

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "mbpo_hip.h").read_text()


def _define(name):
    m = re.search(rf"#define {name} (\d+)\s", HEADER)
    assert m, name
    return int(m.group(1))


@pytest.fixture(scope="module")
def lib():
    from mbpo import _hip
    return _hip.load()


def test_constants_match_the_header():
    from mbpo import _hip
    assert _define("MBPO_REWARD_TERMS") == _hip.REWARD_TERMS == 3
    assert _define("MBPO_REWARD_TERMS_MAX_GROUPS") == _hip.REWARD_TERMS_MAX_GROUPS == 16
    assert _define("MBPO_REWARD_TERMS_MAX_TERMS") == _hip.REWARD_TERMS_MAX_TERMS == 128
    assert _hip.REWARD_TERMS_FLOATS == 4 + 4 * 16 + 4 * 128
    assert "(4 + 4 * MBPO_REWARD_TERMS_MAX_GROUPS + 4 * MBPO_REWARD_TERMS_MAX_TERMS)" in HEADER
    for name, i in _hip.TERM_FN_IDS.items():
        assert _define(f"MBPO_TERM_FN_{name.upper()}") == i
    for name, i in _hip.TERM_LINK_IDS.items():
        assert _define(f"MBPO_TERM_LINK_{name.upper()}") == i
    assert "term rewards" in HEADER.lower()


def test_packing_layout():
    from mbpo import _hip
    rew = tc.make_reward("mixed")
    X, U, bias, groups = tc.MIXED
    v = rew.init_params(0).vector()
    assert v.dtype == torch.float32 and v.shape == (_hip.REWARD_TERMS_FLOATS,)
    n_terms = sum(len(g[2]) for g in groups)
    assert v[:4].tolist() == [len(groups), n_terms, pytest.approx(bias), 0.0]
    part_off = {"x": 0, "u": X, "x_next": X + U}
    k = 0
    for gi, (w, link, terms) in enumerate(groups):
        rec = v[4 + 4 * gi:8 + 4 * gi].tolist()
        assert rec == [pytest.approx(w), _hip.TERM_LINK_IDS[link], k, len(terms)]
        for on, idx, fn, coef, off in terms:
            t = v[4 + 64 + 4 * k:4 + 64 + 4 * k + 4].tolist()
            assert t == [part_off[on] + idx, _hip.TERM_FN_IDS[fn], pytest.approx(coef), pytest.approx(off)]
            k += 1
    assert float(v[4 + 4 * len(groups):4 + 64].abs().sum()) == 0 and float(v[4 + 64 + 4 * k:].abs().sum()) == 0      # always the full length
    assert rew.has_next_state_terms and not tc.make_reward("wide").has_next_state_terms
    # params.replace builds a new table
    p2 = rew.init_params(0).replace(bias=1.5)
    assert float(p2.vector()[2]) == 1.5 and float(v[2]) == pytest.approx(bias)
    assert torch.equal(p2.vector()[4:], v[4:])


def test_constructor_refusals():
    from mbpo.systems import Group, Term, TermReward
    ok = Group([Term("x", 0)])
    TermReward(3, 1, groups=[ok] * 16)
    TermReward(3, 1, groups=[Group([Term("u", 0)] * 128)])
    with pytest.raises(ValueError, match="group 1 term 0.*index 3"):
        TermReward(3, 1, groups=[ok, Group([Term("x", 3)])])
    with pytest.raises(ValueError, match="group 0 term 1.*index 1"):
        TermReward(3, 1, groups=[Group([Term("u", 0), Term("u", 1)])])
    with pytest.raises(ValueError, match="group 0 term 0.*index -1"):
        TermReward(3, 1, groups=[Group([Term("x_next", -1)])])
    with pytest.raises(ValueError, match="group 0 term 0.*unknown fn 'cube'"):
        TermReward(3, 1, groups=[Group([Term("x", 0, fn="cube")])])
    with pytest.raises(ValueError, match="group 2.*unknown link 'log'"):
        TermReward(3, 1, groups=[ok, ok, Group([Term("x", 0)], link="log")])
    with pytest.raises(ValueError, match="group 0 term 0.*unknown part 'xn'"):
        TermReward(3, 1, groups=[Group([Term("xn", 0)])])
    with pytest.raises(ValueError, match="17 groups"):
        TermReward(3, 1, groups=[ok] * 17)
    with pytest.raises(ValueError, match="129 terms"):
        TermReward(3, 1, groups=[Group([Term("x", 0)] * 100), Group([Term("x", 1)] * 29)])
    with pytest.raises(ValueError, match="group 1 is empty"):
        TermReward(3, 1, groups=[ok, Group([])])
    with pytest.raises(ValueError, match="group 0 term 0"):
        TermReward(3, 1, groups=[ok]).init_params(0).replace(groups=(Group([Term("x", 7)]),))      # `replace` validates too


def test_from_quadratic_equals_the_quadratic_formula():
    from mbpo.systems import TermReward
    rew = TermReward.from_quadratic(tc.QUAD_TARGET, tc.QUAD_Q, tc.QUAD_R)
    assert (rew.x_dim, rew.u_dim) == (5, 2) and not rew.has_next_state_terms
    assert torch.equal(rew.init_params(0).vector(), tc.make_reward("quadratic").init_params(0).vector())
    x, u, _ = (t.double() for t in tc.eval_inputs("quadratic"))
    want = tr.quadratic(x, u, tc.QUAD_TARGET, tc.QUAD_Q, tc.QUAD_R)
    torch.testing.assert_close(tr.reward(tc.QUADRATIC, x, u, None), want, atol=1e-13, rtol=1e-13)
    torch.testing.assert_close(rew.torch_reward(x, u, rew.init_params(0)), want, atol=1e-6, rtol=1e-6)      # (python-float coefficients)


@pytest.mark.parametrize("name", sorted(tc.CASES))
def test_torch_form_and_fp32_restatement_against_fp64(name):
    """The fp32 restatement (the kernel's order) stays within 5e-6 (absolute plus relative) of the fp64 one on the cases' inputs: a
    quarter of the GPU comparison's 2e-5, so the inputs themselves cannot eat it.  The cases keep |term| <= 2 and |s_g| <= 4."""
    x, u, xn = tc.eval_inputs(name)
    rec = {}
    r64 = tr.reward(tc.CASES[name], x.double(), u.double(), xn.double(), record=rec)
    assert rec["term"] <= 2.0 and rec["s"] <= 4.0, rec
    r32 = tr.reward(tc.CASES[name], x, u, xn)
    assert r32.dtype == torch.float32
    err = (r32.double() - r64).abs() - 5e-6 * r64.abs()
    print(f"{name}: max |fp32 - fp64| = {float((r32.double() - r64).abs().max()):.3e}")
    assert float(err.max()) <= 5e-6
    # the product's own torch form (the wide BPTT path's reward) is the same function
    rew = tc.make_reward(name)
    got = rew.torch_reward(x.double(), u.double(), rew.init_params(0), xn.double())
    torch.testing.assert_close(got, r64, atol=1e-6, rtol=1e-6)
    # the non-finite rule: a row whose next state is not finite reads x there
    bad = xn.double().clone()
    bad[::7, 0] = float("inf")
    bad[3::7, -1] = float("nan")
    fixed = torch.where(torch.isfinite(bad).all(dim=1, keepdim=True), bad, x.double())
    torch.testing.assert_close(tr.reward(tc.CASES[name], x.double(), u.double(), bad), tr.reward(tc.CASES[name], x.double(), u.double(), fixed),
                               atol=0, rtol=0)
    assert bool(torch.isfinite(rew.torch_reward(x.double(), u.double(), rew.init_params(0), bad)).all())


def test_reward_eval_is_declared_exported_and_checks_its_arguments(lib):
    from mbpo import _hip
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    m = re.search(r"int mbpo_reward_eval\(([^;]*?)\);", code, re.S)
    assert m and [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")] == [
        "reward_kind", "reward_params", "x", "u", "x_next", "n", "x_dim", "u_dim", "out", "stream"]
    assert hasattr(lib, "mbpo_reward_eval")
    ev = lambda kind, rp, x, u, xn, n, X, U, out: lib.mbpo_reward_eval(kind, rp, x, u, xn, n, X, U, out, None)
    for kind in (_hip.REWARD_PENDULUM, _hip.REWARD_LEARNED, 4, -1):
        assert ev(kind, 16, 16, 16, 16, 4, 3, 1, 16) == -2 and b"reward_kind" in lib.mbpo_last_error()      # MBPO_ERR_UNSUPPORTED
    for kind in (_hip.REWARD_TERMS, _hip.REWARD_QUADRATIC):
        assert ev(kind, 16, 16, 16, None, -1, 3, 1, 16) < 0 and b"n < 0" in lib.mbpo_last_error()
        assert ev(kind, 16, 16, 16, None, 4, 0, 1, 16) < 0 and ev(kind, 16, 16, 16, None, 4, 3, 0, 16) < 0
        for args in ((None, 16, 16, 16), (16, None, 16, 16), (16, 16, None, 16), (16, 16, 16, None)):
            rp, x, u, out = args
            assert ev(kind, rp, x, u, None, 4, 3, 1, out) < 0 and b"null" in lib.mbpo_last_error()
        assert ev(kind, None, None, None, None, 0, 3, 1, None) == 0      # nothing to do: no pointer is read


def test_unsupported_code():
    assert re.search(r"#define MBPO_ERR_UNSUPPORTED \(-2\)", HEADER)


def test_model_rollout_takes_the_kind_on_an_ensemble_only(lib):
    """The argument checks run before any device work (an empty rollout returns after them)."""
    from mbpo import _hip
    X, U, E = 5, 2, 3
    d = _hip.RolloutDesc()
    d.x_dim, d.u_dim, d.n_envs, d.n_steps, d.episode_length, d.action_repeat = X, U, 0, 0, 5, 1
    d.row_len, d.actions, d.reward_params = 2 * X + U + 3, 16, 16
    d.system_kind, d.reward_kind = _hip.SYS_ENSEMBLE, _hip.REWARD_TERMS
    m = d.dynamics
    m.params, m.n_nets, m.n_layers, m.activation = 16, E, 4, _hip.ACT_IDS["swish"]
    for i, v in enumerate([X + U, 64, 64, 64, 2 * X]):
        m.dims[i] = v
    m.net_stride = sum(m.dims[i] * m.dims[i + 1] + m.dims[i + 1] for i in range(4))
    assert lib.mbpo_model_rollout(C.byref(d), None) == 0
    d.reward_params = None
    assert lib.mbpo_model_rollout(C.byref(d), None) != 0 and b"reward_params" in lib.mbpo_last_error()
    d.reward_params, d.reward_kind = 16, 4
    assert lib.mbpo_model_rollout(C.byref(d), None) != 0 and b"unknown reward_kind" in lib.mbpo_last_error()
    p = _hip.RolloutDesc()
    p.x_dim, p.u_dim, p.n_envs, p.n_steps, p.episode_length, p.action_repeat = 3, 1, 0, 0, 5, 1
    p.row_len, p.actions, p.reward_params, p.sys_params = 10, 16, 16, 16
    p.system_kind, p.reward_kind = _hip.SYS_PENDULUM, _hip.REWARD_TERMS
    assert lib.mbpo_model_rollout(C.byref(p), None) != 0 and b"term reward needs system_kind ENSEMBLE" in lib.mbpo_last_error()


def test_host_api_wiring_and_spec_cache():
    from mbpo import _hip
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, PendulumSystem, TermReward
    rew = tc.make_reward("mixed")
    dyn = EnsembleDynamics(5, 2, n_members=3, device="cpu")
    system = EnsembleSystem(dyn, rew, mode="ts1", sample_noise=True)
    sp = system.init_params(0)
    spec = system.rollout_spec(sp, torch.device("cpu"))
    assert spec["reward_kind"] == _hip.REWARD_TERMS and torch.equal(spec["reward_params"], sp.reward_params.vector())
    assert system.rollout_spec(sp, torch.device("cpu"))["reward_params"] is spec["reward_params"]      # cached: a captured step replays it
    assert rew.kernel_spec(sp.reward_params, torch.device("cpu"))[1] is spec["reward_params"]
    sp2 = sp.replace(reward_params=sp.reward_params.replace(bias=2.0))
    assert float(system.rollout_spec(sp2, torch.device("cpu"))["reward_params"][2]) == 2.0
    with pytest.raises(ValueError, match="x_next"):
        rew(torch.zeros(4, 5), torch.zeros(4, 2), sp.reward_params)      # next-state terms and no x_next: refused before the device
    with pytest.raises(ValueError, match="not a term table"):
        rew.kernel_spec(tc.make_reward("wide").init_params(0), torch.device("cpu"))
    assert type(PendulumSystem().reward).__name__ == "PendulumReward" and not isinstance(PendulumSystem().reward, TermReward)


def test_bptt_refuses_next_state_terms_before_the_device():
    """Fused and wide alike (both start at BPTTOptimizer's refusal): raised from the constructor, set_system and the per-step spec,
    before the library is loaded or a tensor is made."""
    from mbpo.optimizers.policy_optimizers.bptt_optimizer import BPTTOptimizer
    from mbpo.systems import EnsembleDynamics, EnsembleSystem
    dyn = EnsembleDynamics(5, 2, n_members=3, device="cpu")
    bad = EnsembleSystem(dyn, tc.make_reward("mixed"))
    for kw in ({}, dict(actor_features=(128, 128))):
        with pytest.raises(ValueError, match="gradient through next-state terms is not built"):
            BPTTOptimizer(obs_dim=5, action_dim=2, device="cpu", system=bad, **kw)
    opt = BPTTOptimizer.__new__(BPTTOptimizer)
    opt.system = None
    with pytest.raises(ValueError, match="next-state terms"):
        opt.set_system(bad)
    # a table that gains a next-state term through `replace` is refused where the step's spec is formed
    good = EnsembleSystem(EnsembleDynamics(17, 6, n_members=3, device="cpu"), tc.make_reward("wide"))
    opt.system, opt.device = good, torch.device("cpu")
    sp = good.init_params(0)
    from mbpo.systems import Group, Term
    worse = sp.reward_params.replace(groups=sp.reward_params.groups + (Group([Term("x_next", 0)]),))
    with pytest.raises(ValueError, match="next-state terms"):
        opt._system_kwargs(sp.replace(reward_params=worse))
    spec, kw = opt._system_kwargs(sp)
    from mbpo import _hip
    assert kw["reward_kind"] == _hip.REWARD_TERMS


def test_bptt_plan_takes_the_kind_on_an_ensemble(lib):
    from mbpo import _hip
    import test_cpu_bptt_stochastic as tb
    ws = lambda d: lib.mbpo_bptt_workspace_floats(C.byref(d))
    d = tb._desc(system="ensemble")
    d.reward_kind = _hip.REWARD_TERMS
    assert ws(d) > 0
    p = tb._desc(system="pendulum", dyn_out=0, x=3, u=1)
    p.reward_kind = _hip.REWARD_TERMS
    assert ws(p) < 0 and b"reward_kind" in lib.mbpo_last_error()


def test_differentiable_step_uses_the_term_rewards_torch_form():
    """torch_steps.DifferentiableBuiltin (the wide BPTT path) with REWARD_TERMS: TermReward's own torch form on (x, u), through a
    stand-in MLP node."""
    from mbpo import _hip, ops
    from mbpo.systems import EnsembleDynamics, EnsembleSystem
    from mbpo.systems.torch_steps import DifferentiableBuiltin
    X, U, E, n = 17, 6, 3, 9
    rew = tc.make_reward("wide")
    system = EnsembleSystem(EnsembleDynamics(X, U, n_members=E, device="cpu"), rew)
    sp = system.init_params(0)
    spec = system.rollout_spec(sp, torch.device("cpu"))
    g = torch.Generator().manual_seed(5)
    y = torch.randn(E, n, 2 * X, generator=g)
    x, u = torch.rand(n, X, generator=g) * 2 - 1, torch.rand(n, U, generator=g) * 2 - 1

    class FakeMlp:
        @staticmethod
        def apply(*a):
            return y

    real, ops.HipMlp = ops.HipMlp, FakeMlp
    try:
        st = DifferentiableBuiltin(system, spec).step(x, u, sp)
    finally:
        ops.HipMlp = real
    torch.testing.assert_close(st.reward, tr.reward(tc.WIDE, x, u, None), atol=1e-6, rtol=1e-6)
    torch.testing.assert_close(st.x_next, x + y[..., :X].mean(0))
