"""GPU parity: BPTT through a trajectory-sampling ensemble ('ts1' / 'tsinf', with and without sampled model noise) — the fused
kernel (k_bptt_actor), the host-walked wide path (ops.BpttActorGradGeneric + torch_steps.DifferentiableBuiltin) and BPTTOptimizer,
against torch autograd through a test-local differentiable system that takes the same draws (pathwise gradient through the selected
member: mu_m and sigma_m * eps; the member draw itself is not differentiated).  Tolerances are those of tests/test_gpu_bptt.py."""
import numpy as np
import pytest
import torch

from oracle import bptt as obptt
from oracle import nets as onets
from oracle import philox

from test_gpu_bptt import _assert_matches_oracle, _set_zstore, _setup

pytestmark = pytest.mark.gpu

MIN_STD = 1e-3


class TsEnsembleSystem:
    """Differentiable trajectory-sampling ensemble with a quadratic reward: row i at horizon step t takes member members[i, t]
    (x' = [x +] mu_m (+ (softplus(raw_m) + min_std) * eps[i, t])).  A step counter walks the horizon; set_draws rewinds it."""

    def __init__(self, params, dims, E, X, U, tgt, q, r, predict_delta=True, min_std=MIN_STD, act="swish"):
        self.params, self.dims, self.E, self.X, self.U, self.act = params, list(dims), E, X, U, act
        self.tgt, self.q, self.r, self.predict_delta, self.min_std = tgt, q, r, predict_delta, min_std
        self.members = self.eps = None
        self.t = 0

    def set_draws(self, members, eps):
        self.members, self.eps, self.t = members, eps, 0
        return self

    def step(self, x, u):
        X, n = self.X, x.shape[0]
        y = onets.ensemble_forward(self.params, self.dims, self.E, torch.cat([x, u], dim=1), self.act)
        ym = y[self.members[:, self.t].long(), torch.arange(n)]
        nxt = ym[:, :X] + x if self.predict_delta else ym[:, :X]
        if self.eps is not None:
            nxt = nxt + (torch.nn.functional.softplus(ym[:, X:2 * X]) + self.min_std) * self.eps[:, self.t].to(x.dtype)
        self.t += 1
        rew = -(self.q * (x - self.tgt) ** 2).sum(1) - (self.r * u ** 2).sum(1)
        return nxt, rew


def _ts_setup(X, U, H, n, E, seed=0, **setup_kw):
    """tests/test_gpu_bptt.py's setup; the members' raw-std output bias is shifted to -2 (sigma ~ 0.13: a fitted model's aleatoric
    noise, so that H-step noisy rollouts stay in the range the tolerances were set for)."""
    cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, _, extra = _setup(X, U, H, n, "ensemble", E, seed, **setup_kw)
    dd, dp = extra["dd"], extra["dp"].clone()
    P = onets.n_params(dd)
    for e in range(E):
        dp[(e + 1) * P - X:(e + 1) * P] -= 2.0
    extra = dict(extra, dp=dp)
    g = torch.Generator().manual_seed(seed + 100)
    members = torch.randint(0, E, (n, H), generator=g, dtype=torch.int32)
    eps = torch.randn(n, H, X, generator=g)
    return cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, extra, members, eps


def _mode_id(mode):
    from mbpo import _hip
    return {"ts1": _hip.ENS_TS1, "tsinf": _hip.ENS_TSINF, "mean": _hip.ENS_MEAN}[mode]


def _run_ts(dev, cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, extra, n, mode, with_noise, delta, members=None, eps=None, seed=0,
            offset=0, rng_dev=None):
    from mbpo import _hip, ops
    op = ops.BpttActorGrad(x_dim=cfg.x_dim, u_dim=cfg.u_dim, horizon=cfg.horizon, actor_dims=cfg.actor_dims, critic_dims=cfg.critic_dims,
                           n=n, device=dev, init_stddev=cfg.init_stddev, discount=cfg.discount, lambda_=cfg.lambda_, ent_coef=cfg.ent_coef,
                           seed=seed, actor_activation=cfg.actor_act, critic_activation=cfg.critic_act)
    E = extra["dp"].numel() // onets.n_params(extra["dd"])
    op(actor_params=ap.to(dev), target_critic_params=cp.to(dev), init_states=x0.to(dev), state_mean=s_mean.to(dev), state_std=s_std.to(dev),
       reward_mean_std=r_ms.to(dev), act_noise=noise.to(dev), offset=offset, rng_dev=rng_dev, system_kind=_hip.SYS_ENSEMBLE,
       reward_kind=_hip.REWARD_QUADRATIC, reward_params=torch.cat([extra["tgt"], extra["q"], extra["r"]]).to(dev),
       dyn_params=extra["dp"].to(dev), dyn_spec=ops.MlpSpec(extra["dd"], extra["act"], E), ens_predict_delta=delta, ens_mode=_mode_id(mode),
       ens_sample_noise=with_noise, ens_min_std=MIN_STD, member_idx=None if members is None else members.to(dev).contiguous(),
       model_noise=None if eps is None else eps.to(dev).contiguous())
    torch.cuda.synchronize()
    return op


def _ts_oracle(cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, extra, E, members, eps, delta):
    X, U = cfg.x_dim, cfg.u_dim
    sys32 = TsEnsembleSystem(extra["dp"], extra["dd"], E, X, U, extra["tgt"], extra["q"], extra["r"], delta, act=extra["act"]).set_draws(members, eps)
    g_ref, _, aux = obptt.actor_grads(cfg, sys32, ap, cp, x0, noise, s_mean, s_std, r_ms[0], r_ms[1])
    d = lambda t: t.double()
    sys64 = TsEnsembleSystem(d(extra["dp"]), extra["dd"], E, X, U, d(extra["tgt"]), d(extra["q"]), d(extra["r"]), delta, act=extra["act"])
    sys64.set_draws(members, None if eps is None else d(eps))
    g64, loss64, aux64 = obptt.actor_grads(cfg, sys64, d(ap), d(cp), d(x0), d(noise), d(s_mean), d(s_std), d(r_ms[0]), d(r_ms[1]))
    assert sys32.t == sys64.t == cfg.horizon
    return g_ref, aux, g64, loss64, aux64


def _members_for(mode, members, n, H, E):
    return members if mode == "ts1" else (torch.arange(n, dtype=torch.int32) % E)[:, None].expand(n, H).contiguous()


@pytest.mark.parametrize("X,U,H,n,E,mode,with_noise,delta", [
    (4, 1, 5, 48, 5, "ts1", True, True),          # two member rounds (4 + 1), three tiles
    (4, 1, 5, 48, 5, "ts1", False, False),
    (4, 1, 5, 48, 5, "tsinf", True, False),
    (4, 1, 5, 48, 5, "tsinf", False, True),
    (4, 2, 6, 17, 3, "ts1", True, False),         # one round of 3, ragged n, u = 2
    (4, 2, 6, 17, 3, "tsinf", True, True),
    (17, 6, 32, 16, 10, "ts1", True, True),       # BASELINE config 5 shape at its full horizon
    (17, 6, 32, 16, 10, "tsinf", False, True),
])
def test_ts_actor_grad_parity(dev, X, U, H, n, E, mode, with_noise, delta):
    cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, extra, members, eps = _ts_setup(X, U, H, n, E)
    m = _members_for(mode, members, n, H, E)
    refs = _ts_oracle(cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, extra, E, m, eps if with_noise else None, delta)
    op = _run_ts(dev, cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, extra, n, mode, with_noise, delta, members=members, eps=eps)
    _assert_matches_oracle(op, refs, X, U, H, n)


def test_ts_differs_from_mean(dev):
    """The TS modes are not the mean: the same inputs give other transitions (guards against a silently ignored ens_mode)."""
    X, U, H, n, E = 4, 1, 5, 48, 5
    cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, extra, members, eps = _ts_setup(X, U, H, n, E)
    mean = _run_ts(dev, cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, extra, n, "mean", True, True, members=members, eps=eps)
    ts = _run_ts(dev, cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, extra, n, "ts1", False, True, members=members, eps=eps)
    assert float((mean.transitions - ts.transitions).abs().max()) > 1e-2


@pytest.mark.parametrize("X,U,H,n,E,mode", [
    (4, 1, 5, 48, 5, "ts1"),
    (4, 2, 6, 17, 3, "tsinf"),
    (17, 6, 32, 16, 10, "ts1"),
])
def test_ts_zstore_equals_recompute(dev, X, U, H, n, E, mode):
    """As tests/test_gpu_bptt.py::test_bptt_zstore_equals_recompute, in the TS modes with noise: the backward sweep reads the member,
    eps and raw_m checkpoints on both sources of the members' pre-activations, so the two agree bit for bit; the workspace differs by
    the z store alone."""
    import os
    if os.environ.get("MBPO_BPTT_ZSTORE_MAX_MB") is not None:
        pytest.skip("MBPO_BPTT_ZSTORE_MAX_MB caps the z store in this process: the store path may not run")
    cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, extra, members, eps = _ts_setup(X, U, H, n, E, seed=1)
    res = {}
    try:
        for zmode in (-1, 0):
            _set_zstore(zmode)
            op = _run_ts(dev, cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, extra, n, mode, True, True, members=members, eps=eps)
            res[zmode] = (op.workspace.numel(), op.grads.clone(), op.metrics.clone(), op.transitions.clone(), op.lambda_values.clone())
    finally:
        _set_zstore(-1)
    tiles, hidden_layers = (n + 15) // 16, len(extra["dd"]) - 2
    assert res[-1][0] - res[0][0] == tiles * H * E * hidden_layers * 1024
    for a, b in zip(res[-1][1:], res[0][1:]):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(res[-1][1]).all())


def _ts_checkpoint_members(op, n, H, X, U):
    """The member checkpoints inside the workspace (bptt_plan: x_t, a_t, eps_t, r_t, V_t, argmin, then the TS block)."""
    up4 = lambda v: (v + 3) & ~3
    o = up4(n * (H + 1) * X) + 2 * up4(n * H * U) + 3 * up4(n * H)
    return op.workspace[o:o + n * H].view(torch.int32).reshape(n, H).cpu()


@pytest.mark.parametrize("use_rng_dev", [False, True])
def test_ts_in_kernel_draws_are_the_philox_streams(dev, use_rng_dev):
    """Without member_idx / model_noise the kernel draws members (stream MEMBER, element i*H + t) and eps (stream MODEL_NOISE,
    element (i*H + t)*x + c) under (seed, offset [+ rng_dev]): members bit-exact with oracle.philox, the result equal to the run on
    the explicit oracle draws."""
    from mbpo import ops
    X, U, H, n, E = 4, 1, 5, 48, 5
    cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, extra, _, _ = _ts_setup(X, U, H, n, E, seed=2)
    seed, offset = 4242, 7
    rng = ops.make_rng(dev, seed=91, counter=5) if use_rng_dev else None
    s_eff, o_eff = (seed + 91, offset + 5) if use_rng_dev else (seed, offset)
    members = torch.from_numpy(philox.philox_randint(s_eff, o_eff, philox.STREAM_MEMBER, np.arange(n * H, dtype=np.uint64), 0, E)).reshape(n, H)
    eps = torch.from_numpy(philox.philox_normal(s_eff, o_eff, philox.STREAM_MODEL_NOISE, np.arange(n * H * X, dtype=np.uint64))).reshape(n, H, X)
    a = _run_ts(dev, cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, extra, n, "ts1", True, True, members=members, eps=eps)
    b = _run_ts(dev, cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, extra, n, "ts1", True, True, seed=seed, offset=offset, rng_dev=rng)
    assert torch.equal(_ts_checkpoint_members(b, n, H, X, U), members)
    assert torch.equal(_ts_checkpoint_members(a, n, H, X, U), members)
    torch.testing.assert_close(a.grads, b.grads, atol=1e-6, rtol=1e-4)
    torch.testing.assert_close(a.transitions, b.transitions, atol=1e-6, rtol=1e-4)
    refs = _ts_oracle(cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, extra, E, members, eps, True)
    _assert_matches_oracle(b, refs, X, U, H, n)


def test_philox_randint_is_the_oracle(dev):
    from mbpo import ops
    for seed, offset, lo, hi, base, rng in ((7, 0, 0, 5, 0, None), (2 ** 40 + 3, 11, -3, 10, 1000, (5, 2 ** 33)), (1, 2 ** 34, 0, 1, 0, None)):
        rng_dev = ops.make_rng(dev, seed=rng[0], counter=rng[1]) if rng else None
        got = ops.philox_randint(1000, lo, hi, seed, offset, philox.STREAM_MEMBER, rng_dev=rng_dev, elem_base=base, device=dev).cpu()
        s_eff, o_eff = philox.resolve(seed, offset, rng)
        ref = philox.philox_randint(s_eff, o_eff, philox.STREAM_MEMBER, np.arange(base, base + 1000, dtype=np.uint64), lo, hi)
        assert got.dtype == torch.int32 and torch.equal(got, torch.from_numpy(ref))
        assert int(got.min()) >= lo and int(got.max()) < hi


def _ensemble_system(dev, X, U, E, mode, sample_noise, seed=3):
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, QuadraticReward
    dyn = EnsembleDynamics(X, U, n_members=E, device=dev)
    return EnsembleSystem(dyn, QuadraticReward(X, U, target=[0.1] + [0.0] * (X - 1), q=[1.0, 2.0, 0.5, 0.1][:X], r=[0.3] * U),
                          mode=mode, sample_noise=sample_noise)


def test_wide_path_matches_the_fused_kernel(dev):
    """ops.BpttActorGradGeneric through torch_steps.DifferentiableBuiltin (the path of networks wider than 64) at width 64, 'ts1' with
    noise and no explicit draws: it draws the kernel's members and eps, so it matches the fused kernel on the same seeds."""
    from mbpo import _hip, ops
    from mbpo.systems.torch_steps import DifferentiableBuiltin
    X, U, H, n, E = 4, 1, 6, 40, 5
    system = _ensemble_system(dev, X, U, E, "ts1", True)
    sp = system.init_params(5)
    spec = system.rollout_spec(sp, dev)
    cfg, ap, cp, x0, _, s_mean, s_std, r_ms, _, _ = _setup(X, U, H, n, "ensemble", E, 4)
    kw = dict(x_dim=X, u_dim=U, horizon=H, actor_dims=cfg.actor_dims, critic_dims=cfg.critic_dims, n=n, device=dev,
              init_stddev=cfg.init_stddev, discount=cfg.discount, lambda_=cfg.lambda_, ent_coef=cfg.ent_coef, seed=77)
    common = dict(actor_params=ap.to(dev), target_critic_params=cp.to(dev), init_states=x0.to(dev), state_mean=s_mean.to(dev),
                  state_std=s_std.to(dev), reward_mean_std=r_ms.to(dev), offset=3, rng_dev=ops.make_rng(dev, seed=0, counter=2))
    fused = ops.BpttActorGrad(**kw)
    fused(**common, system_kind=spec["system_kind"], reward_kind=spec["reward_kind"], reward_params=spec["reward_params"],
          dyn_params=spec["dyn_params"], dyn_spec=spec["dyn_spec"], ens_predict_delta=spec["ens_predict_delta"], ens_mode=spec["ens_mode"],
          ens_sample_noise=spec["ens_sample_noise"], ens_min_std=spec["ens_min_std"])
    diff = DifferentiableBuiltin(system, spec)
    assert diff.ens_mode == _hip.ENS_TS1 and diff.sample_noise and diff.n_members == E
    wide = ops.BpttActorGradGeneric(**kw)
    wide(**common, system=diff, system_params=sp)
    torch.cuda.synchronize()
    torch.testing.assert_close(wide.transitions, fused.transitions, atol=2e-4, rtol=2e-4)
    torch.testing.assert_close(wide.lambda_values, fused.lambda_values, atol=5e-4, rtol=5e-4)
    torch.testing.assert_close(wide.metrics, fused.metrics, atol=2e-5, rtol=1e-4)
    torch.testing.assert_close(wide.grads, fused.grads, atol=5e-6, rtol=2e-3)
    # and it is not the mean model
    mean = ops.BpttActorGradGeneric(**kw)
    mean(**common, system=DifferentiableBuiltin(system, dict(spec, ens_mode=_hip.ENS_MEAN)), system_params=sp)
    assert float((mean.transitions - wide.transitions).abs().max()) > 1e-3


def _true_buffer(dev, X, U, rows=16, seed=3):
    from mbpo.replay import UniformSamplingQueue
    from mbpo.types import Transition
    g = torch.Generator().manual_seed(seed)
    q = UniformSamplingQueue(rows, Transition(observation=torch.zeros(X), action=torch.zeros(U), reward=torch.zeros(1),
                                              discount=torch.zeros(1), next_observation=torch.zeros(X)), 1, device=dev)
    return q.insert_rows(q.init(0), torch.randn(rows, 2 * X + U + 2, generator=g).to(dev))


def test_bptt_optimizer_trains_wide_networks_on_ts_noise(dev):
    from mbpo.optimizers import BPTTOptimizer
    X, U, E = 4, 1, 3
    system = _ensemble_system(dev, X, U, E, "ts1", True)
    opt = BPTTOptimizer(action_dim=U, obs_dim=X, horizon=6, num_samples_per_gradient_update=24, train_steps=3,
                        critic_updates_per_policy_update=2, sampling_buffer_size=4096, actor_features=(128, 128), critic_features=(128, 128))
    opt.set_system(system)
    st = opt.init(key=11, true_buffer_state=_true_buffer(dev, X, U))
    assert opt.wide
    out = opt.train(bptt_state=st)
    s = out.bptt_summary
    assert bool(torch.isfinite(s.actor_loss).all()) and bool(torch.isfinite(s.critic_loss).all())
    assert bool(torch.isfinite(out.optimizer_state.actor_params).all())
    assert float(out.optimizer_state.actor_opt_state.count) == 3


@pytest.mark.parametrize("mode,sample_noise", [("ts1", True), ("tsinf", False)])
def test_bptt_optimizer_ts_train_step_matches_cpu_oracle(dev, mode, sample_noise):
    """One whole train step of BPTTOptimizer on a trajectory-sampling EnsembleSystem vs oracle.bptt.CpuBpttLoop driven by
    opt._last_seeds, with the test-local system taking the oracle's Philox draws at offset = train-step index (the checks of
    tests/test_gpu_host_api.py::test_bptt_train_steps_match_cpu_oracle)."""
    from mbpo.optimizers import BPTTOptimizer
    X, U, E, n, H, kc = 4, 1, 3, 24, 6, 2
    system = _ensemble_system(dev, X, U, E, mode, sample_noise)
    sbs = _true_buffer(dev, X, U)
    opt = BPTTOptimizer(action_dim=U, obs_dim=X, horizon=H, num_samples_per_gradient_update=n, train_steps=1, init_stddev=1.5,
                        critic_updates_per_policy_update=kc, sampling_buffer_size=4096)
    opt.set_system(system)
    st0 = opt.init(key=11, true_buffer_state=sbs)
    out1 = opt.train(bptt_state=st0)
    sp = st0.system_params
    rp = sp.reward_params
    tsys = TsEnsembleSystem(sp.dynamics_params.params.cpu().clone(), system.dynamics.dims, E, X, U, torch.tensor(rp.target),
                            torch.tensor(rp.q), torch.tensor(rp.r), True, system.min_std)
    act_seed = opt._last_seeds[1]

    def draws(step):
        if mode == "ts1":
            m = philox.philox_randint(act_seed, step, philox.STREAM_MEMBER, np.arange(n * H, dtype=np.uint64), 0, E)
            m = torch.from_numpy(m).reshape(n, H)
        else:
            m = (torch.arange(n, dtype=torch.int32) % E)[:, None].expand(n, H)
        e = None
        if sample_noise:
            e = torch.from_numpy(philox.philox_normal(act_seed, step, philox.STREAM_MODEL_NOISE,
                                                      np.arange(n * H * X, dtype=np.uint64))).reshape(n, H, X)
        return m, e

    cfg = obptt.BpttConfig(x_dim=X, u_dim=U, actor_dims=opt.actor_dims, critic_dims=opt.critic_dims, horizon=H, init_stddev=1.5)
    loop = obptt.CpuBpttLoop(cfg, tsys, st0.actor_params.cpu(), st0.critic_params.cpu(), sbs.data.cpu(), n, kc, opt._last_seeds,
                             buffer_size=4096)
    tsys.set_draws(*draws(loop.step_idx))
    r = loop.step()
    assert tsys.t == H
    s1, o1 = out1.bptt_summary, out1.optimizer_state
    assert abs(float(s1.actor_loss[0]) - r["actor_loss"]) <= 2e-5 * max(1.0, abs(r["actor_loss"]))
    assert abs(float(s1.critic_loss[0]) - r["critic_loss"]) <= 1e-4 * max(1.0, abs(r["critic_loss"]))
    assert abs(float(s1.actor_grad_norm[0]) - r["actor_grad_norm"]) <= 2e-3 * r["actor_grad_norm"]
    assert abs(float(s1.critic_grad_norm[0]) - r["critic_grad_norm"]) <= 2e-3 * r["critic_grad_norm"]
    torch.testing.assert_close(o1.state_normalizer_state.mean.cpu(), loop.s_mean, atol=1e-5, rtol=1e-4)
    torch.testing.assert_close(o1.state_normalizer_state.std.cpu(), loop.s_std, atol=1e-5, rtol=1e-4)
    torch.testing.assert_close(o1.reward_normalizer_state.std.cpu(), loop.r_std, atol=1e-5, rtol=1e-4)
    rel = lambda a, b: float((a.cpu() - b).norm() / b.norm())
    assert rel(o1.actor_params, loop.ap) < 2e-4 and rel(o1.critic_params, loop.cp) < 2e-4
    assert rel(o1.target_critic_params, loop.tp) < 1e-5


@pytest.mark.parametrize("mode,sample_noise", [("ts1", True), ("tsinf", True)])
def test_bptt_optimizer_ts_graph_replay_equals_eager(dev, mode, sample_noise):
    """The hipGraph-replayed train steps equal eagerly issued ones bit for bit over 4 steps: the members and the model noise are
    drawn under rng_dev, so every replay draws the step's own numbers."""
    from mbpo.optimizers import BPTTOptimizer
    X, U, E = 4, 1, 3
    system = _ensemble_system(dev, X, U, E, mode, sample_noise)
    sbs = _true_buffer(dev, X, U)
    outs = []
    for use_graph in (True, False):
        opt = BPTTOptimizer(action_dim=U, obs_dim=X, horizon=6, num_samples_per_gradient_update=24, train_steps=4,
                            critic_updates_per_policy_update=2, sampling_buffer_size=4096, use_graph=use_graph)
        opt.set_system(system)
        out = opt.train(bptt_state=opt.init(key=5, true_buffer_state=sbs))
        assert opt._last_train_captured == use_graph
        outs.append(out)
    g, e = outs
    for a, b in ((g.optimizer_state.actor_params, e.optimizer_state.actor_params),
                 (g.optimizer_state.critic_params, e.optimizer_state.critic_params),
                 (g.bptt_summary.actor_loss, e.bptt_summary.actor_loss), (g.bptt_summary.critic_loss, e.bptt_summary.critic_loss)):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(g.bptt_summary.actor_loss).all())
    assert len(set(g.bptt_summary.actor_loss.tolist())) == 4
