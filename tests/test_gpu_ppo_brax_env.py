"""GPU parity: PPO with the brax-env options (ppo/ppo_brax_env.py, ppo/losses_new.py) — the per-sample discount of
non_equidistant_time on every values/GAE path, clip_by_global_norm before AdamW, return_best_model — against the restatement in
tests/ppo_brax_env_ref.py.  Tolerances are tests/test_gpu_ppo.py's."""
import types

import numpy as np
import pytest
import torch

import ppo_brax_env_ref as ref
from oracle import ppo as oppo
from test_gpu_ppo import _make, _updater

pytestmark = pytest.mark.gpu

# t = (1 - 0)/2 * a + 1/2 on the grid a = 2 (k + 0.5) 0.1 - 1: t = 0.05, 0.15, ..., 0.95, far from the floor's steps in fp32 and fp64
# alike, so the floor gives ten distinct discounts exp(-0.5 * 0.1 k)
NEQ = ref.Neq(0.5, 0.0, 1.0, 0.1)
NEQ_KW = dict(non_equidistant_time=True, continuous_discounting=0.5, min_time_between_switches=0.0, max_time_between_switches=1.0,
              env_dt=0.1)


def _with_switch_times(data, X, U, seed):
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(0, 10, data.shape[:2], generator=g)
    data[..., X + U - 1] = 2 * (k.to(data.dtype) + 0.5) * 0.1 - 1
    return data


def _r4(n):
    return (n + 3) & ~3


def _vs_adv(up, B, T):
    """vs and the raw advantages from the workspace (ppo.hip's layout: baseline [M], boot [B], trunc, term, rew [M], vs [M], adv [M])."""
    M = B * T
    o = _r4(M) + _r4(B) + 3 * _r4(M)
    ws = up.workspace.cpu()
    return ws[o:o + M].reshape(B, T), ws[o + _r4(M):o + _r4(M) + M].reshape(B, T)


CASES = [
    # X, U, hidden, v_hidden, B, T, norm_adv          path
    (3, 1, (64, 64, 64), None, 32, 10, True),         # k_ppo_vg_lean, 64 x 3
    (3, 1, (64, 64), None, 128, 40, False),           # k_ppo_vg_lean, 64 x 2
    (4, 2, (64, 64, 64), None, 24, 7, True),          # k_ppo_values_gae<64>, u = 2
    (4, 1, (128, 128), None, 16, 9, False),           # k_ppo_values_gae<128>
    (3, 1, (64, 64), (256, 256), 20, 6, True),        # layered: k_ppol_prep + mbpo_gae_scan_discounts
    (3, 1, (64, 64), None, 2, 1030, False),           # k_ppo_values + mbpo_gae_scan_discounts (too long for the fused launch)
]


@pytest.mark.parametrize("X,U,hidden,v_hidden,B,T,norm_adv", CASES)
def test_per_sample_discount_gradients(dev, X, U, hidden, v_hidden, B, T, norm_adv):
    cfg, st, data, noise, nm, ns = _make(X, U, hidden, B, T, 0, True, v_hidden=v_hidden, entropy_cost=1e-2, discounting=0.99,
                                          reward_scaling=0.5, gae_lambda=0.95, clipping_epsilon=0.3, normalize_advantage=norm_adv,
                                          lr=3e-4, wd=1e-5)
    data = _with_switch_times(data, X, U, 1)
    assert len(torch.unique(data[..., X + U - 1])) >= 5
    g_ref, terms, vs_ref, adv_ref = ref.grads(cfg, st.params, data, noise, nm, ns, neq=NEQ)
    g64, terms64, vs64, adv64 = ref.grads(cfg, st.params.double(), data.double(), noise.double(), nm.double(), ns.double(), neq=NEQ)
    up = _updater(dev, cfg, B, T, **NEQ_KW)
    up.fused_step = False
    up.load_state(st.params.to(dev))
    up.minibatch_step(data.to(dev), nm.to(dev), ns.to(dev), noise.to(dev))
    torch.cuda.synchronize()
    vs, adv = _vs_adv(up, B, T)
    torch.testing.assert_close(vs, vs64.T.float(), atol=2e-5, rtol=1e-4)
    torch.testing.assert_close(adv, adv64.T.float(), atol=2e-5, rtol=1e-4)
    g = up.grads.cpu()
    scale = float(g64.abs().max())
    if v_hidden is None:
        torch.testing.assert_close(g, g_ref, atol=2e-6, rtol=5e-4)
        torch.testing.assert_close(g.double(), g64, atol=2e-6, rtol=2e-4)
    else:
        torch.testing.assert_close(g.double(), g64, atol=2e-6 + 2e-6 * scale, rtol=5e-4)
    np.testing.assert_allclose(up.metrics.cpu().tolist(), [terms64[k] for k in ("total_loss", "policy_loss", "v_loss", "entropy_loss")],
                               rtol=5e-5 if v_hidden else 2e-5, atol=1e-5)
    # the per-sample discount matters here: the constant-discount loss is a different one
    g_plain, _, _, _ = oppo.grads(cfg, st.params.double(), data.double(), noise.double(), nm.double(), ns.double())
    assert float((g_plain - g64).abs().max()) > 10 * (2e-6 + 2e-4 * scale)


@pytest.mark.parametrize("X,U,hidden", [(3, 1, (64, 64, 64)), (4, 2, (64, 64, 64))])
def test_zero_continuous_discounting_is_bitwise_the_constant_discount_one(dev, X, U, hidden):
    """exp(-0 * t) == 1.0f exactly: the NEQ instantiations (lean and generic) give the constant-discount launch's bits at discounting = 1."""
    cfg, st, data, noise, nm, ns = _make(X, U, hidden, 48, 12, 3, True, discounting=1.0, entropy_cost=1e-2)
    data = _with_switch_times(data, X, U, 4)
    outs = []
    for kw in ({}, dict(NEQ_KW, continuous_discounting=0.0)):
        up = _updater(dev, cfg, 48, 12, **kw)
        up.load_state(st.params.to(dev))
        up.minibatch_step(data.to(dev), nm.to(dev), ns.to(dev), noise.to(dev))
        torch.cuda.synchronize()
        outs.append((up.grads.cpu(), up.metrics.cpu(), up.params.cpu()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_clip_far_below_the_norm_matches_the_restatement(dev):
    cfg, st, data, noise, nm, ns = _make(3, 1, (64, 64, 64), 64, 10, 5, True, entropy_cost=1e-2, lr=3e-4, wd=1e-5)
    g_ref, _, _, _ = ref.grads(cfg, st.params, data, noise, nm, ns)
    max_norm = 1e-3 * float(g_ref.norm())
    for fused in (True, False):
        up = _updater(dev, cfg, 64, 10, max_grad_norm=max_norm)
        up.fused_step = fused
        up.load_state(st.params.to(dev))
        up.minibatch_step(data.to(dev), nm.to(dev), ns.to(dev), noise.to(dev))
        torch.cuda.synchronize()
        g = up.grads.cpu()
        torch.testing.assert_close(g, g_ref, atol=2e-6, rtol=5e-4)
        st_new, _, _ = ref.minibatch_step(cfg, st, data, noise, nm, ns, max_grad_norm=max_norm, grad_override=g)
        torch.testing.assert_close(up.params.cpu(), st_new.params, atol=1e-7, rtol=1e-6)
        torch.testing.assert_close(up.adam_m.cpu(), st_new.adam_m, atol=1e-12, rtol=1e-5)
        torch.testing.assert_close(up.adam_v.cpu(), st_new.adam_v, atol=1e-16, rtol=1e-5)
        assert float(up.adam_m.cpu().norm()) < 0.11 * max_norm          # the moments saw the clipped gradient


def test_clip_above_the_norm_is_bitwise_no_clip(dev):
    cfg, st, data, noise, nm, ns = _make(3, 1, (64, 64), 64, 10, 6, True, entropy_cost=1e-2, lr=1e-3, wd=1e-5)
    for fused in (True, False):
        outs = []
        for kw in ({}, dict(max_grad_norm=1e30)):
            up = _updater(dev, cfg, 64, 10, **kw)
            up.fused_step = fused
            up.load_state(st.params.to(dev))
            for it in range(2):
                up.minibatch_step(data.to(dev), nm.to(dev), ns.to(dev), noise.to(dev))
            torch.cuda.synchronize()
            outs.append([getattr(up, n).cpu() for n in ("params", "adam_m", "adam_v", "grads", "metrics", "step_count")])
        for a, b in zip(*outs):
            assert torch.equal(a, b), fused


@pytest.mark.parametrize("hidden,v_hidden,B,T", [((64, 64, 64), None, 512, 40), ((64, 64), (256, 256), 64, 10)])
def test_clipped_fused_step_equals_grads_plus_apply(dev, hidden, v_hidden, B, T):
    """With clipping on (and the per-sample discount), mbpo_ppo_step == mbpo_ppo_grads + mbpo_ppo_apply bit for bit over three chained
    steps, at C3's shape (B = 512, T = 40) and on the layered path."""
    cfg, st, data, noise, nm, ns = _make(3, 1, hidden, B, T, 7, True, v_hidden=v_hidden, entropy_cost=1e-2, lr=1e-3, wd=1e-4)
    g_ref, _, _, _ = ref.grads(cfg, st.params, data, noise, nm, ns)
    ups = []
    for fused in (True, False):
        up = _updater(dev, cfg, B, T, max_grad_norm=0.1 * float(g_ref.norm()), **NEQ_KW)
        up.fused_step = fused
        up.load_state(st.params.to(dev))
        ups.append(up)
    g = torch.Generator().manual_seed(8)
    for it in range(3):
        d = _with_switch_times(data + 0.1 * torch.randn(data.shape, generator=g), 3, 1, 10 + it).to(dev)
        for up in ups:
            up.minibatch_step(d, nm.to(dev), ns.to(dev), seed=9, offset=it << 32)
    torch.cuda.synchronize()
    a, b = ups
    for name in ("params", "adam_m", "adam_v", "grads", "metrics", "step_count"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


def test_apply_clips_the_reduced_gradient(dev):
    """Two ranks' exchange, in process: the all-reduce hook adds the other rank's gradient, grad_scale = 1/2; the clip norm is that of
    the reduced, scaled gradient (the pmean), and the step equals the restatement on it."""
    cfg, st, data, noise, nm, ns = _make(3, 1, (64, 64), 32, 8, 9, True, entropy_cost=1e-2, lr=1e-3, wd=1e-4)
    other = torch.randn(cfg.P + cfg.V, generator=torch.Generator().manual_seed(1)) * 1e-2
    max_norm = 2e-3
    up = _updater(dev, cfg, 32, 8, max_grad_norm=max_norm, world_size=2, all_reduce=lambda t: t.add_(other.to(dev)))
    up.load_state(st.params.to(dev))
    up.minibatch_step(data.to(dev), nm.to(dev), ns.to(dev), noise.to(dev))
    torch.cuda.synchronize()
    reduced = up.grads.cpu()                     # own + other, as the all-reduce left it
    pmean = reduced * 0.5
    assert float(pmean.norm()) > 10 * max_norm
    st_new, _, _ = ref.minibatch_step(cfg, st, data, noise, nm, ns, max_grad_norm=max_norm, grad_override=pmean)
    torch.testing.assert_close(up.params.cpu(), st_new.params, atol=1e-7, rtol=1e-6)
    torch.testing.assert_close(up.adam_m.cpu(), st_new.adam_m, atol=1e-12, rtol=1e-5)
    torch.testing.assert_close(up.adam_v.cpu(), st_new.adam_v, atol=1e-16, rtol=1e-5)


# ------------------------------------------------------------------------------------------------ trainer
def _trainer_kw():
    from test_gpu_trainer_parity import PPO_KW
    return dict(PPO_KW, max_grad_norm=0.05, non_equidistant_time=True, continuous_discounting=0.9, min_time_between_switches=0.0,
                max_time_between_switches=0.5, env_dt=0.05)


def test_trainer_graph_equals_eager_with_options(dev):
    from mbpo.optimizers.policy_optimizers.ppo.ppo import PPO
    from mbpo.systems.brax_wrapper import BraxWrapper
    from test_gpu_trainer_parity import _make_system, _true_buffer
    kw = _trainer_kw()
    out = {}
    for use_graph in (False, True):
        system, sp, _, X, U = _make_system(dev, "pendulum")
        tb, tbs = _true_buffer(dev, X, U, 256)
        env = BraxWrapper(system, sp, tbs, tb)
        tr = PPO(environment=env, num_timesteps=5 * 16 * 8 * 4, use_graph=use_graph, **kw)
        ts = tr.init_training_state(5)
        es = env.reset([101 + i for i in range(kw["num_envs"])])
        metrics = None
        for key in (19, 31):
            ts, es, metrics = tr.training_epoch(ts, es, key)
        torch.cuda.synchronize()
        assert (tr._graph is not None) == use_graph
        u = tr.updater
        out[use_graph] = dict(params=u.params.clone(), m=u.adam_m.clone(), v=u.adam_v.clone(), count=u.step_count.clone(),
                              obs=es.obs.clone(), steps=es.info["steps"].clone(), done=es.done.clone(), stats=tr._stats_vec.clone(),
                              data=tr._data.clone(), perm=tr._perm.clone(), rng=tr._rng.clone(), metrics=metrics)
        tr.close()
    for name, eager in out[False].items():
        if name == "metrics":
            assert eager == out[True][name]
        else:
            assert torch.equal(eager, out[True][name]), name


def test_trainer_training_step_matches_restated_cpu_loop(dev, monkeypatch):
    from mbpo.optimizers.policy_optimizers.ppo.ppo import PPO
    from mbpo.systems.brax_wrapper import BraxWrapper
    from oracle import trainer as otr
    from test_gpu_trainer_parity import _make_system, _rel, _true_buffer
    kw = _trainer_kw()
    system, sp, osystem, X, U = _make_system(dev, "pendulum")
    tb, tbs = _true_buffer(dev, X, U, 256)
    env = BraxWrapper(system, sp, tbs, tb)
    tr = PPO(environment=env, num_timesteps=3 * 16 * 8 * 4, **kw)
    ts = tr.init_training_state(5)
    es = env.reset([101 + i for i in range(kw["num_envs"])])
    cfg = oppo.PpoConfig(X, U, tr.policy_dims, tr.value_dims, entropy_cost=kw["entropy_cost"], discounting=kw["discounting"],
                         gae_lambda=kw["gae_lambda"], clipping_epsilon=kw["clipping_epsilon"], lr=kw["lr"], wd=kw["wd"])
    neq = ref.Neq(kw["continuous_discounting"], kw["min_time_between_switches"], kw["max_time_between_switches"], kw["env_dt"])
    shim = types.SimpleNamespace(**{k: getattr(oppo, k) for k in dir(oppo) if not k.startswith("__")})
    shim.minibatch_step = lambda c, s, d, e, nm, ns: ref.minibatch_step(c, s, d, e, nm, ns, neq=neq, max_grad_norm=kw["max_grad_norm"])
    monkeypatch.setattr(otr, "ppo", shim)
    loop = otr.CpuPpoLoop(cfg, osystem, kw["num_envs"], kw["unroll_length"], kw["episode_length"], kw["batch_size"],
                          kw["num_minibatches"], kw["num_updates_per_batch"], True, init_params=tr.updater.params.cpu().clone(),
                          init_obs=es.obs.cpu().clone())
    tr.rekey(23)
    loop.rekey(23)
    ts, es, _ = tr.training_step(ts, es)
    terms = loop.training_step()
    torch.cuda.synchronize()
    torch.testing.assert_close(tr._data.cpu(), loop.last_data, atol=2e-4, rtol=2e-4)
    P = tr.updater.P
    assert _rel(tr.updater.params[:P], loop.state.params[:P]) < 1e-3
    assert _rel(tr.updater.params[P:], loop.state.params[P:]) < 1e-3
    assert _rel(tr.updater.adam_m, loop.state.adam_m) < 1e-2
    assert float(tr.updater.step_count) == loop.state.count == 8
    for got, key in zip(tr.updater.metrics.cpu().tolist(), ("total_loss", "policy_loss", "v_loss", "entropy_loss")):
        assert abs(got - terms[key]) <= 2e-3 * max(1.0, abs(terms[key])), key
    tr.close()


@pytest.mark.parametrize("return_best_model", [True, False])
def test_return_best_model(dev, monkeypatch, return_best_model):
    """ppo_brax_env.py:315-367: the snapshot at the highest eval/episode_reward among the evaluations after training epochs (the
    initial evaluation is not a candidate), else the last one."""
    from mbpo.optimizers.policy_optimizers.ppo import ppo as ppo_mod
    from mbpo.systems.brax_wrapper import BraxWrapper
    from test_gpu_trainer_parity import _make_system, _true_buffer
    rewards = iter([1e9, -50.0, -10.0, -30.0])          # initial, then after epochs 1..3: the best is after epoch 2
    seen = []

    class FakeEvaluator:
        def __init__(self, *a, **k):
            pass

        def run_evaluation(self, params, training_metrics, **k):
            seen.append((params[0].vec.clone(), params[1].clone()))
            return {"eval/episode_reward": next(rewards), **training_metrics}

    monkeypatch.setattr(ppo_mod, "Evaluator", FakeEvaluator)
    kw = _trainer_kw()
    system, sp, _, X, U = _make_system(dev, "pendulum")
    tb, tbs = _true_buffer(dev, X, U, 256)
    env = BraxWrapper(system, sp, tbs, tb)
    tr = ppo_mod.PPO(environment=env, num_timesteps=3 * 16 * 8 * 4, num_evals=4, return_best_model=return_best_model, **kw)
    (norm, pol), metrics = tr.run_training(key=3)
    tr.close()
    assert len(seen) == 4 and len(metrics) == 4
    want = seen[2] if return_best_model else seen[3]
    assert torch.equal(norm.vec, want[0]) and torch.equal(pol, want[1])
    assert not torch.equal(seen[2][1], seen[3][1])         # the epochs did move the policy


def test_validation_and_optimizer_facade(dev):
    from mbpo import ops, _hip
    from mbpo.optimizers import PPOOptimizer
    from mbpo.optimizers.policy_optimizers.ppo.ppo import PPO
    from mbpo.systems.brax_wrapper import BraxWrapper
    from test_gpu_host_api import _one_row_true_buffer
    from test_gpu_trainer_parity import _make_system, _true_buffer
    base = dict(x_dim=3, u_dim=1, policy_dims=[3, 64, 64, 2], value_dims=[3, 64, 64, 1], batch_size=8, unroll_length=4, device=dev)
    with pytest.raises(ValueError):
        ops.PpoUpdater(**base, non_equidistant_time=True)
    with pytest.raises(ValueError):
        ops.PpoUpdater(**base, max_grad_norm=0.0)
    up = ops.PpoUpdater(**base, **NEQ_KW)
    up.desc.env_dt = 0.0                                          # the library checks it too
    with pytest.raises(_hip.MbpoHipError):
        up.minibatch_step(torch.zeros(8, 4, 12, device=dev))
    system, sp, _, X, U = _make_system(dev, "pendulum")
    tb, tbs = _true_buffer(dev, X, U, 64)
    with pytest.raises(ValueError):
        PPO(environment=BraxWrapper(system, sp, tbs, tb), num_timesteps=1000, episode_length=20, env_dt=-1.0, non_equidistant_time=True)
    system, buf, sbs = _one_row_true_buffer(dev)
    opt = PPOOptimizer(system=system, true_buffer=buf, num_timesteps=16 * 8 * 4, episode_length=20, num_envs=32, num_eval_envs=2,
                       unroll_length=8, batch_size=16, num_minibatches=4, num_updates_per_batch=1, num_evals=1,
                       policy_hidden_layer_sizes=(64, 64), critic_hidden_layer_sizes=(64, 64), max_grad_norm=0.5,
                       non_equidistant_time=True, continuous_discounting=0.5, max_time_between_switches=0.5, env_dt=0.05)
    assert opt.dummy_trainer.updater.desc.non_equidistant_time == 1
    assert opt.dummy_trainer.updater.desc.max_grad_norm == pytest.approx(0.5)
    out = opt.train(opt.init(key=0, true_buffer_state=sbs))
    assert np.isfinite(out.summary[-1]["training/total_loss"])
    assert float(out.optimizer_state.policy_params[1].abs().sum()) > 0
