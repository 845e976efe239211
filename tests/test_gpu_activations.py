"""GPU parity of every fused kernel family under relu and tanh (tests/activation_cases.py): each case against the fp32 and the fp64
oracle, elementwise, at the tolerance of the module that owns the kernel (activation_cases.TOL names them), the optimizer step GIVEN
the device gradient.  Networks that meet in one launch carry different activations.  The inputs of every case that differentiates a
relu network are clear of relu's kink (tests/test_cpu_activation_cases.py), so no row, unit or element is left out of a comparison."""
import numpy as np
import pytest
import torch

import activation_cases as ac
import many_tiles_cases as mt

pytestmark = pytest.mark.gpu

_d = lambda t, dev: None if t is None else t.to(dev)


def _names(family):
    return [n for n, c in ac.ALL.items() if c["family"] == family]


# ---------------------------------------------------------------------------------------------------------------------- SAC
def _sac_run(dev, name):
    from test_gpu_sac import _updater
    c = ac.CASES[name]
    cfg, st, batch, noise, nm, ns = ac.inputs(name)
    up = _updater(dev, cfg, c["B"], policy_activation=c["acts"][0], q_activation=c["acts"][1])
    up.load_state(st.params.to(dev), st.target_q.to(dev))
    up.sgd_step(batch.to(dev), _d(nm, dev), _d(ns, dev), *[n.to(dev) for n in noise])
    up.finalize()
    torch.cuda.synchronize()
    return up


def _sac_check(name, up):
    from oracle import sac as osac
    cfg, st, batch, noise, nm, ns = ac.inputs(name)
    o32, o64 = ac.oracle(name, torch.float32), ac.oracle(name, torch.float64)
    g = up.grads.cpu()
    P, Q = cfg.P, cfg.Q
    for gname, sl in (("policy", slice(0, P)), ("critic", slice(P, P + 2 * Q)), ("alpha", slice(P + 2 * Q, None))):
        torch.testing.assert_close(g[sl], o32["main"][sl], msg=lambda m: f"{name} {gname} grad vs fp32 oracle: {m}", **ac.TOL["sac"]["tol32"])
        torch.testing.assert_close(g[sl].double(), o64["main"][sl], msg=lambda m: f"{name} {gname} grad vs fp64 oracle: {m}",
                                   **ac.TOL["sac"]["tol64"])
    m = up.metrics.cpu().tolist()
    np.testing.assert_allclose(m[:3], o64["losses"], rtol=2e-5, atol=2e-6)
    st_new, met, _ = osac.sgd_step(cfg, st, batch, *noise, nm, ns, grad_override=g)
    np.testing.assert_allclose(m[3], met["alpha"], rtol=1e-6)
    torch.testing.assert_close(up.params.cpu(), st_new.params, atol=1e-7, rtol=1e-6)
    torch.testing.assert_close(up.target_q.cpu(), st_new.target_q, atol=1e-7, rtol=1e-6)
    torch.testing.assert_close(up.adam_m.cpu(), st_new.adam_m, atol=1e-9, rtol=1e-5)
    torch.testing.assert_close(up.adam_v.cpu(), st_new.adam_v, atol=1e-12, rtol=1e-5)


@pytest.mark.parametrize("name", _names("sac"))
def test_sac_fused_kernels(dev, name):
    """k_sac_fwd_bwd's variants (thin + JVP, reverse-mode actor at u = 2, wide, 128) with policy and critics under different
    activations: gradients, losses and the optimizer step; tolerances of test_sac_gradients_and_step."""
    _sac_check(name, _sac_run(dev, name))


@pytest.mark.parametrize("name", ["sac_thin_rt", "sac_thin_tr"])
def test_sac_forward_mode_actor_without_thin_layers(dev, monkeypatch, name):
    """MBPO_SAC_THIN=0 (re-read per call): the same shapes on k_sac_fwd_bwd<64,4,false,2> — the forward-mode tangent epilogue of the
    actor role with every layer on MFMA (chain_run.hpp's non-swish branch)."""
    monkeypatch.setenv("MBPO_SAC_THIN", "0")
    up = _sac_run(dev, name)
    _sac_check(name, up)
    monkeypatch.setenv("MBPO_SAC_THIN", "1")
    thin = _sac_run(dev, name)
    torch.testing.assert_close(thin.grads, up.grads, atol=5e-7, rtol=2e-5)      # test_sac_thin_layer_variant_matches_mfma_layers


# ---------------------------------------------------------------------------------------------------------------------- PPO
@pytest.mark.parametrize("name", _names("ppo"))
def test_ppo_kernels(dev, name):
    """k_ppo_values_gae / k_ppo_values + k_ppo_fwd_bwd's variants and the layered path with policy and value net under different
    activations; tolerances of test_ppo_gradients_and_step (layered: test_ppo_layered_path_any_widths)."""
    from oracle import ppo as oppo
    from test_gpu_ppo import _updater
    c = ac.CASES[name]
    cus = None
    if name == "ppo_sp2_rt":       # sized from this device's CU count, as tests/many_tiles_cases.py sizes its cases
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        c = dict(c, B=ac.ppo_sp2_shape(cus)[0])
        assert mt.tiles_of(c["B"] * c["T"]) == cus + 1
    cfg, st, data, noise, nm, ns = ac.inputs(name, cus=cus)
    assert data.shape[:2] == (c["B"], c["T"])
    o32, o64 = ac.oracle(name, torch.float32, cus=cus), ac.oracle(name, torch.float64, cus=cus)
    up = _updater(dev, cfg, c["B"], c["T"], policy_activation=c["acts"][0], value_activation=c["acts"][1])
    up.load_state(st.params.to(dev))
    up.minibatch_step(data.to(dev), _d(nm, dev), _d(ns, dev), noise.to(dev))
    torch.cuda.synchronize()
    g = up.grads.cpu()
    layered = c["v_hidden"] is not None
    tol32, tol64 = dict(ac.TOL["ppo"]["tol32"]), dict(ac.TOL["ppo"]["tol64"])
    if layered:
        tol64 = dict(atol=2e-6 + 2e-6 * float(o64["main"].abs().max()), rtol=5e-4)
        tol32 = dict(tol64)
    torch.testing.assert_close(g, o32["main"], msg=lambda m: f"{name} grad vs fp32 oracle: {m}", **tol32)
    torch.testing.assert_close(g.double(), o64["main"], msg=lambda m: f"{name} grad vs fp64 oracle: {m}", **tol64)
    t64 = o64["terms"]
    np.testing.assert_allclose(up.metrics.cpu().tolist(), [t64[k] for k in ("total_loss", "policy_loss", "v_loss", "entropy_loss")],
                               rtol=5e-5 if layered else 2e-5, atol=1e-5)
    st_new, _, _ = oppo.minibatch_step(cfg, st, data, noise, nm, ns, grad_override=g)
    torch.testing.assert_close(up.params.cpu(), st_new.params, atol=1e-7, rtol=1e-6)
    torch.testing.assert_close(up.adam_m.cpu(), st_new.adam_m, atol=1e-9, rtol=1e-5)
    torch.testing.assert_close(up.adam_v.cpu(), st_new.adam_v, atol=1e-12, rtol=1e-5)


# ----------------------------------------------------------------------------------------------------------------- rollouts
@pytest.mark.parametrize("name", list(ac.ROLLOUT_CASES))
def test_model_rollout_kernels(dev, name):
    """k_model_rollout64 / k_model_rollout<128|256> (k_rollout_lean refuses non-swish) with policy and members under different
    activations, against the fp32 and the fp64 oracle at test_gpu_rollout's row tolerance."""
    from test_gpu_rollout import _run_rollout_case
    rows = _run_rollout_case(dev, **ac.ROLLOUT_CASES[name])
    assert bool(torch.isfinite(rows).all())


@pytest.mark.parametrize("name", _names("ensfwd"))
def test_ensemble_forward_64(dev, name):
    """k_ensemble_forward<64> at the lean kernel's own shape: under relu / tanh the generic kernel must take it (the result says so)."""
    from mbpo import ops
    c, i = ac.ALL[name], ac.inputs(name)
    y = ops.ensemble_mlp_forward(i["params"].to(dev), ops.MlpSpec(c["dims"], i["act"], c["E"]), i["x"].to(dev)).cpu()
    torch.testing.assert_close(y, ac.oracle(name, torch.float32)["main"], **ac.TOL["ensfwd"]["tol32"])
    torch.testing.assert_close(y.double(), ac.oracle(name, torch.float64)["main"], **ac.TOL["ensfwd"]["tol64"])


@pytest.mark.parametrize("name", _names("policy_act"))
def test_policy_act(dev, name):
    from mbpo import ops
    c, i = ac.ALL[name], ac.inputs(name)
    spec = ops.MlpSpec(c["dims"], i["act"], 1)
    o32, o64 = ac.oracle(name, torch.float32), ac.oracle(name, torch.float64)
    a, raw, lp = ops.policy_act(i["params"].to(dev), spec, i["obs"].to(dev), i["mean"].to(dev), i["std"].to(dev), noise=i["noise"].to(dev),
                                want_extras=True)
    mode = ops.policy_act(i["params"].to(dev), spec, i["obs"].to(dev), i["mean"].to(dev), i["std"].to(dev), deterministic=True)
    for got, key in ((a, "main"), (raw, "raw"), (mode, "mode")):
        torch.testing.assert_close(got.cpu(), o32[key], **ac.TOL["policy_act"]["tol32"])
        torch.testing.assert_close(got.cpu().double(), o64[key], **ac.TOL["policy_act"]["tol64"])
    torch.testing.assert_close(lp.cpu().double(), o64["log_prob"], atol=2e-4, rtol=2e-4)      # test_gpu_rollout's row tolerance


@pytest.mark.parametrize("name", _names("ens_eval"))
def test_ens_eval(dev, name):
    from mbpo import ops
    c, i = ac.ALL[name], ac.inputs(name)
    op = ops.EnsembleEval(x_dim=c["X"], u_dim=c["U"], spec=ops.MlpSpec(i["dims"], i["act"], c["E"]), device=dev)
    got = op(i["params"].to(dev), i["rows"].to(dev), i["idx"].to(torch.int32).to(dev)).cpu()
    torch.testing.assert_close(got, ac.oracle(name, torch.float32)["main"], **ac.TOL["ens_eval"]["tol32"])
    torch.testing.assert_close(got.double(), ac.oracle(name, torch.float64)["main"], **ac.TOL["ens_eval"]["tol64"])


# --------------------------------------------------------------------------------------------------------------------- BPTT
def _bptt_refs(name):
    o32, o64 = ac.oracle(name, torch.float32), ac.oracle(name, torch.float64)
    return o32["main"], o32["aux"], o64["main"], o64["loss"], o64["aux"]


@pytest.mark.parametrize("name", _names("bptt"))
def test_bptt_actor(dev, name):
    """k_bptt_actor with actor, critics and members each under their own activation; test_gpu_bptt's comparison and tolerances."""
    from test_gpu_bptt import _assert_matches_oracle, _run_hip
    c = ac.CASES[name]
    cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, tsys, extra = ac.inputs(name)
    op = _run_hip(dev, cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, "ensemble", extra, c["n"])
    _assert_matches_oracle(op, _bptt_refs(name), c["X"], c["U"], c["H"], c["n"])


def test_bptt_actor_ts1_with_sampled_noise(dev):
    """k_bptt_actor in 'ts1' with model noise (test_gpu_bptt_stochastic's run and oracle) under three different activations."""
    from test_gpu_bptt import _assert_matches_oracle
    from test_gpu_bptt_stochastic import _run_ts
    name = "bptt_ts1_noise"
    c = ac.CASES[name]
    cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, extra, members, eps = ac.inputs(name)
    op = _run_ts(dev, cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, extra, c["n"], "ts1", True, True, members=members, eps=eps)
    _assert_matches_oracle(op, _bptt_refs(name), c["X"], c["U"], c["H"], c["n"])


@pytest.mark.parametrize("name", ["bptt_x4_b", "bptt_wide", "bptt_x4_a"])
def test_bptt_zstore_and_recompute(dev, name):
    """The backward sweep's two sources of the MEMBERS' pre-activations (the store holds only theirs; actor and critic are always
    recomputed): bptt_x4_b has relu members (act' at the kink-free pre-activations), bptt_wide tanh members, bptt_x4_a swish members
    under a relu actor.  Each mode against the oracle, the two bit for bit (as test_bptt_zstore_equals_recompute)."""
    import os
    from test_gpu_bptt import _assert_matches_oracle, _run_hip, _set_zstore
    assert os.environ.get("MBPO_BPTT_ZSTORE_MAX_MB") is None, "MBPO_BPTT_ZSTORE_MAX_MB caps the z store in this process"
    c = ac.CASES[name]
    cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, tsys, extra = ac.inputs(name)
    res = {}
    try:
        for mode in (-1, 0):
            _set_zstore(mode)
            op = _run_hip(dev, cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, "ensemble", extra, c["n"])
            _assert_matches_oracle(op, _bptt_refs(name), c["X"], c["U"], c["H"], c["n"])
            res[mode] = (op.workspace.numel(), op.grads.clone(), op.metrics.clone(), op.transitions.clone(), op.lambda_values.clone())
    finally:
        _set_zstore(-1)
    tiles, hidden_layers = (c["n"] + 15) // 16, len(extra["dd"]) - 2
    assert res[-1][0] - res[0][0] == tiles * c["H"] * c["E"] * hidden_layers * 1024      # the store path really ran
    for a, b in zip(res[-1][1:], res[0][1:]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", _names("critic"))
def test_critic_grad(dev, name):
    """k_critic_fwd_bwd; tolerances of test_critic_grads_parity."""
    from mbpo import ops
    c, i = ac.CASES[name], ac.inputs(name)
    o32, o64 = ac.oracle(name, torch.float32), ac.oracle(name, torch.float64)
    op = ops.CriticGrad(x_dim=c["X"], critic_dims=i["cfg"].critic_dims, batch=c["batch"], device=dev, activation=c["acts"][0])
    got = op(i["cp"].to(dev), i["rows"].to(dev), i["lam"].to(dev), i["idx"].to(dev), i["mean"].to(dev), i["std"].to(dev)).cpu()
    assert abs(float(op.metrics[0]) - o32["loss"]) <= 1e-5 + 2e-5 * abs(o32["loss"])
    torch.testing.assert_close(got, o32["main"], **ac.TOL["critic"]["tol32"])
    torch.testing.assert_close(got.double(), o64["main"], **ac.TOL["critic"]["tol32"])
    assert ac.rel_l2(got, o64["main"]) < ac.TOL["critic"]["rel64"]


@pytest.mark.parametrize("name", _names("mlp"))
def test_hip_mlp_against_autograd(dev, name):
    """ops.HipMlp as an autograd node: k_mlp_vjp ([3, 64, 64, 2]) and mbpo_mlp_layered_vjp ([3, 128, 128, 2]); tolerances of
    test_mlp_vjp_matches_autograd."""
    from mbpo import ops
    c, i = ac.CASES[name], ac.inputs(name)
    o32, o64 = ac.oracle(name, torch.float32), ac.oracle(name, torch.float64)
    p, x = i["params"].to(dev).requires_grad_(True), i["x"].to(dev).requires_grad_(True)
    y = ops.HipMlp.apply(p, x, ops.MlpSpec(c["dims"], i["act"], 1), i["mean"].to(dev), i["std"].to(dev))
    (y * i["dy"].to(dev)).sum().backward()
    torch.cuda.synchronize()
    T = ac.TOL["mlp"]
    for ref in (o32, o64):
        f = lambda t: t.detach().cpu().to(ref["main"].dtype)
        torch.testing.assert_close(f(y)[0], ref["y"], **T["y"])
        torch.testing.assert_close(f(x.grad), ref["dx"], **T["dx"])
        scale = max(float(ref["main"].abs().max()), 1.0)
        torch.testing.assert_close(f(p.grad), ref["main"], atol=T["dw"]["atol"] * scale, rtol=T["dw"]["rtol"])


# ------------------------------------------------------------------------------------------------------- ensemble learning
@pytest.mark.parametrize("name", _names("nll"))
def test_ens_nll_grads(dev, name):
    """k_ens_nll_fwd_bwd and its layered form; tolerances of test_ens_nll_grads_parity."""
    from mbpo import ops
    c, i = ac.CASES[name], ac.inputs(name)
    o32, o64 = ac.oracle(name, torch.float32), ac.oracle(name, torch.float64)
    op = ops.EnsembleNllGrad(x_dim=c["X"], u_dim=c["U"], spec=ops.MlpSpec(i["dims"], i["act"], c["E"]), batch=c["B"], device=dev)
    got = op(i["params"].to(dev), i["rows"].to(dev), i["idx"].to(torch.int32).to(dev)).cpu()
    np.testing.assert_allclose(op.metrics.cpu().numpy(), o32["losses"].numpy(), rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(got, o32["main"], **ac.TOL["nll"]["tol32"])
    torch.testing.assert_close(got.double(), o64["main"], **ac.TOL["nll"]["tol32"])
    assert ac.rel_l2(got, o64["main"]) < ac.TOL["nll"]["rel64"]


# --------------------------------------------------------------------------------------------------------- terminal values
@pytest.mark.parametrize("name", _names("tv"))
def test_terminal_value_mixed_widths_and_activations(dev, name):
    """Kind Q with a policy narrower (wave_dense_fwd's partial-tile paths, csrc/terminal_value.hip header) and wider than the critics,
    two different `act` fields in one launch; terminal_value_cases.TOL32 / TOL64."""
    import terminal_value_cases as tvc
    from mbpo.optimizers import TerminalValue
    i = ac.inputs(name)
    tv = TerminalValue(ac.ALL[name]["X"], i["critic"].to(dev), i["cdims"], n_critics=2, activation=i["acts"][1],
                       policy_params=i["policy"].to(dev), policy_dims=i["pdims"], policy_activation=i["acts"][0],
                       norm_mean=i["mean"].to(dev), norm_std=i["std"].to(dev))
    v32, v64 = ac.oracle(name, torch.float32)["main"], ac.oracle(name, torch.float64)["main"]
    for n in (1, 17, i["x"].shape[0]):
        got = tv(i["x"][:n].to(dev)).cpu()
        torch.testing.assert_close(got, v32[:n], atol=tvc.TOL32, rtol=tvc.TOL32)
        torch.testing.assert_close(got.double(), v64[:n], atol=tvc.TOL64, rtol=tvc.TOL64)


# ---------------------------------------------------------------------------------------------------------------- trainers
@pytest.mark.parametrize("which,act", [("sac", "relu"), ("ppo", "tanh"), ("bptt", "relu")])
def test_trainer_activation_string_reaches_the_launch(dev, which, act):
    """SAC, PPO and BPTTOptimizer built with a non-swish policy: the deterministic act() on 5 observations is oracle.nets.mlp_forward
    under that activation (and not under swish)."""
    from oracle import nets as onets
    obs = torch.randn(5, 3, generator=torch.Generator().manual_seed(9))
    if which == "bptt":
        from mbpo.optimizers import BPTTOptimizer
        from test_gpu_host_api import _bptt_pendulum_setup
        system, _, sbs = _bptt_pendulum_setup(dev, buffer_rows=64)
        opt = BPTTOptimizer(action_dim=1, obs_dim=3, horizon=4, num_samples_per_gradient_update=16, train_steps=1, sampling_buffer_size=256,
                            policy_activation=act, critic_activation="tanh")
        opt.set_system(system)
        st = opt.init(key=3, true_buffer_state=sbs)
        ns = st.state_normalizer_state
        pol, dims, mean, std = st.actor_params, opt.actor_dims, ns.mean, ns.std
        head = lambda out: torch.clamp(torch.tanh(out[:, :1]), -0.999, 0.999)
    else:
        from mbpo.optimizers import PPOOptimizer, SACOptimizer
        from mbpo.replay import UniformSamplingQueue
        from mbpo.systems import PendulumSystem
        from mbpo.types import Transition
        system = PendulumSystem()
        s0 = system.reset()
        dummy = Transition(observation=s0.x_next, action=torch.zeros(1, device=dev), reward=s0.reward, discount=torch.tensor(0.99, device=dev),
                           next_observation=s0.x_next)
        buf = UniformSamplingQueue(10, dummy, 1, device=dev)
        kw = dict(num_timesteps=1000, episode_length=20, num_envs=4, normalize_observations=True, policy_hidden_layer_sizes=(64, 64),
                  critic_hidden_layer_sizes=(64, 64), policy_activation=act, critic_activation="relu" if act == "tanh" else "tanh")
        if which == "sac":
            opt = SACOptimizer(system=system, true_buffer=buf, batch_size=16, **kw)
        else:
            opt = PPOOptimizer(system=system, true_buffer=buf, batch_size=4, num_minibatches=1, unroll_length=5, **kw)
        st = opt.init(key=7)
        norm, pol = st.policy_params
        norm.vec[1:4] = torch.tensor([0.1, -0.2, 0.3], device=dev)
        norm.vec[7:10] = torch.tensor([0.7, 1.3, 2.0], device=dev)
        dims, mean, std = opt.dummy_trainer.policy_dims, norm.mean, norm.std
        head = onets.mode
    a, _ = opt.act(obs.to(dev), st, evaluate=True)
    xn = onets.normalize(obs, mean.cpu(), std.cpu())
    want = head(onets.mlp_forward(pol.cpu(), dims, xn, act))
    torch.testing.assert_close(a.cpu(), want, atol=2e-5, rtol=2e-5)
    assert float((head(onets.mlp_forward(pol.cpu(), dims, xn, "swish")) - want).abs().max()) > 1e-3
