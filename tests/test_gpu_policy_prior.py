"""Policy priors on the device (include/mbpo_hip.h "policy priors").  mbpo_icem_seed_candidates against the torch restatement of
tests/policy_prior_ref.py — every float of actions, candidates and mean, the poison outside the seeded slots included —, dropped proposals,
a captured launch; then the prior inside iCemTO: iteration 0's candidates against a direct ops.model_rollout call with the same
descriptor (that kernel is unchanged and has its own oracle parity in test_gpu_rollout.py), batched against single calls, a problem plain
sampling cannot solve, every_iteration, policy_prior=None, a user-defined System and a policy narrower than the ensemble.

Every comparison is bit for bit: the new kernel copies and clips."""

import numpy as np
import pytest
import torch

import policy_prior_cases as cases
import policy_prior_ref as pref
from test_gpu_icem_batched import _compare_with_single_calls, _same

pytestmark = pytest.mark.gpu

X = cases.X_DIM
DIMS = [3, 64, 64, 2]


# ------------------------------------------------------------------------------------------------ 1-3: the launch
def _launch(c, dev, rows=None, actions=True, mean=True):
    """One launch on device copies of the case; (actions, candidates, mean) on the host, None where not passed."""
    from mbpo import ops
    d = lambda t: t.to(dev).contiguous()
    src = d(c.rows if rows is None else rows)
    act, cand = (d(c.actions), d(c.candidates)) if actions else (None, None)
    mu = d(c.mean) if mean else None
    ops.icem_seed_candidates(src, c.offset, c.step_stride, c.traj_stride, c.B, c.K, c.NC, c.H, c.A, c.P, d(c.u_min), d(c.u_max),
                             actions=act, candidates=cand, mean=mu)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu() for t in (act, cand, mu))


def _want(c, rows=None, actions=True, mean=True):
    p = pref.gather_proposals(c.rows if rows is None else rows, c.offset, c.step_stride, c.traj_stride, c.B, c.K, c.H, c.A)
    return pref.seed(p, c.u_min, c.u_max, c.NC, c.P, actions=c.actions if actions else None, candidates=c.candidates if actions else None,
                     mean=c.mean if mean else None)


def _assert_same3(got, want, what):
    for name, g, w in zip(("actions", "candidates", "mean"), got, want):
        assert (g is None) == (w is None), f"{what}: {name}"
        if g is not None:
            assert _same(g.reshape(-1), w.reshape(-1)), f"{what}: {name}"


@pytest.mark.parametrize("shape", cases.SHAPES + [cases.LONG], ids=lambda s: "B{}K{}H{}A{}P{}".format(*s))
def test_seed_launch_equals_the_restatement(dev, shape):
    """Strided as iCEM passes it (the action columns of [H * B * K, 2x + A + 3] rows, every other column NaN), outputs poisoned: all of
    actions, candidates and mean, the floats outside the seeded slots included.  K < n_samples and K == n_samples; the full call, the
    mean-only call and the call without a mean.  Per-dimension bounds, u_min == u_max (A = 3), values outside the bounds, a -0.0."""
    for k_equals_samples in (False, True):
        c = cases.make_seed_case(shape, k_equals_samples)
        assert c.NC == c.n_samples + cases.N_PREV and (c.K == c.n_samples) == k_equals_samples
        for actions, mean in ((True, True), (False, True), (True, False)):
            got, want = _launch(c, dev, actions=actions, mean=mean), _want(c, actions=actions, mean=mean)
            _assert_same3(got, want, f"K == n_samples {k_equals_samples}, actions {actions}, mean {mean}")
        act, cand, mu = _launch(c, dev)
        assert _same(cand[:, c.K:], c.candidates[:, c.K:])                                  # the poison stays
        assert not _same(cand[:, :c.K], c.candidates[:, :c.K]) and bool(torch.isfinite(cand[:, :c.K]).all())
        assert bool((cand[:, :c.K] >= c.u_min).all()) and bool((cand[:, :c.K] <= c.u_max).all())
        assert _same(mu, cand[:, 0])
    # the -0.0 of the case survives the clip with its sign
    c = cases.make_seed_case(shape, False)
    _, cand, _ = _launch(c, dev)
    i = (c.H * c.B * c.K) // 2
    t, e = divmod(i, c.B * c.K)
    b, k = divmod(e, c.K)
    lo, hi = float(c.u_min[0]), float(c.u_max[0])
    assert lo < 0.0 < hi and _same(cand[b, k, t, 0], torch.tensor(-0.0))


def test_the_wrapper_refuses_a_source_that_is_too_short(dev):
    from mbpo import ops
    c = cases.make_seed_case((3, 5, 7, 3, 4), False)
    d = lambda t: t.to(dev).contiguous()
    with pytest.raises(ValueError, match="src holds"):
        ops.icem_seed_candidates(d(c.rows.reshape(-1)[:-c.traj_stride]), c.offset, c.step_stride, c.traj_stride, c.B, c.K, c.NC, c.H, c.A,
                                 c.P, d(c.u_min), d(c.u_max), actions=d(c.actions), candidates=d(c.candidates))
    with pytest.raises(ValueError, match="candidates holds"):
        ops.icem_seed_candidates(d(c.rows), c.offset, c.step_stride, c.traj_stride, c.B, c.K, c.NC, c.H, c.A, c.P, d(c.u_min), d(c.u_max),
                                 actions=d(c.actions), candidates=d(c.candidates.reshape(-1)[1:]))


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")], ids=["nan", "pinf", "ninf"])
def test_a_proposal_that_is_not_finite_is_dropped(dev, value):
    """One bad element in one (b, k): that slot's H * A candidate floats and H * P * A action floats keep the poison, every other slot is
    written; a non-finite k = 0 leaves mean[b] untouched."""
    shape = (3, 5, 7, 3, 4)
    B, K, H, A, P = shape
    for (b, k, t, a) in ((1, 2, 3, 1), (2, 0, H - 1, A - 1), (0, 0, 0, 0)):
        c = cases.make_seed_case(shape, False, seed=1)
        rows = c.rows.clone()
        rows[t * B * K + b * K + k, X + a] = value
        act, cand, mu = _launch(c, dev, rows=rows)
        _assert_same3((act, cand, mu), _want(c, rows=rows), f"({b}, {k})")
        assert _same(cand[b, k], c.candidates[b, k])
        a5, p5 = act.reshape(H, B, c.NC, P, A), c.actions.reshape(H, B, c.NC, P, A)
        assert _same(a5[:, b, k], p5[:, b, k])
        written = torch.ones(B, K, dtype=torch.bool)
        written[b, k] = False
        for bb in range(B):
            for kk in range(K):
                if written[bb, kk]:
                    assert bool(torch.isfinite(cand[bb, kk]).all()) and not _same(cand[bb, kk], c.candidates[bb, kk])
                    assert _same(a5[:, bb, kk, P - 1], cand[bb, kk])
        assert _same(mu[b], c.mean[b]) == (k == 0)
        # the mean-only call drops it alike
        _, _, m2 = _launch(c, dev, rows=rows, actions=False)
        assert _same(m2, mu)


def test_captured_launch_follows_a_refilled_source(dev):
    from mbpo import ops
    c = cases.make_seed_case((3, 5, 7, 3, 4), False)
    other = cases.make_seed_case((3, 5, 7, 3, 4), False, seed=2)
    other.rows[5, X + 1] = float("nan")                                     # the replay drops a proposal the capture wrote
    assert not torch.equal(c.rows[:, X:X + 3], other.rows[:, X:X + 3])
    d = lambda t: t.to(dev).contiguous()
    src, lo, hi = d(c.rows), d(c.u_min), d(c.u_max)
    act, cand, mu = d(c.actions), d(c.candidates), d(c.mean)
    call = lambda: ops.icem_seed_candidates(src, c.offset, c.step_stride, c.traj_stride, c.B, c.K, c.NC, c.H, c.A, c.P, lo, hi,
                                            actions=act, candidates=cand, mean=mu)
    call()                                                                  # (one eager call first: the code object)
    torch.cuda.synchronize()
    _assert_same3((act.cpu(), cand.cpu(), mu.cpu()), _want(c), "eager")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for t, p in ((act, c.actions), (cand, c.candidates), (mu, c.mean)):
        t.copy_(p.to(dev))
    graph.replay()
    torch.cuda.synchronize()
    _assert_same3((act.cpu(), cand.cpu(), mu.cpu()), _want(c), "replay")
    src.copy_(other.rows.to(dev))                                           # refilled in place: the launch reads it
    for t, p in ((act, c.actions), (cand, c.candidates), (mu, c.mean)):
        t.copy_(p.to(dev))
    graph.replay()
    torch.cuda.synchronize()
    want = _want(c, rows=other.rows)
    _assert_same3((act.cpu(), cand.cpu(), mu.cpu()), want, "replay on the refilled source")
    assert not _same(cand.cpu()[:, :c.K], _want(c)[1][:, :c.K])


# ------------------------------------------------------------------------------------------------ 4-10: inside iCemTO
_P = dict(num_samples=8, num_elites=3, num_particles=2, num_steps=1)
H = 4


def _prior(dev, dims=DIMS, seed=0, params=None, **kw):
    from mbpo.optimizers import PolicyPrior
    g = torch.Generator().manual_seed(100 + seed)
    flat = (cases.random_policy(dims, seed=seed) if params is None else params).to(dev)
    args = dict(n_candidates=3, norm_mean=(torch.randn(dims[0], generator=g) * 0.1).to(dev),
                norm_std=(torch.rand(dims[0], generator=g) + 0.5).to(dev))
    args.update(kw)
    return PolicyPrior(dims[0], flat, dims, **args)


def _opt(system, prior, horizon=H, **kw):
    from mbpo.optimizers import iCemParams, iCemTO
    params = iCemParams(**{**_P, **kw.pop("params", {})})
    opt = iCemTO(horizon=horizon, action_dim=system.action_dim, opt_params=params, key=5, policy_prior=prior, **kw)
    opt.set_system(system)
    return opt


def _starts(dev, B, x_dim, A, horizon=H, seed=0):
    g = torch.Generator().manual_seed(seed)
    if x_dim == 3:
        ang = torch.rand(B, generator=g) * 6.28
        x0 = torch.stack([torch.cos(ang), torch.sin(ang), torch.randn(B, generator=g)], dim=1)
    else:
        x0 = torch.randn(B, x_dim, generator=g) * 0.5
    return x0.to(dev), ((torch.rand(B, horizon, A, generator=g) - 0.5) * 1.5).to(dev)


def _direct_proposals(system, system_params, prior, x0, prior_keys, horizon, dev, policy=None):
    """The clipped proposals [B, K, H, A] from a direct ops.model_rollout call: the noise of the grouped fill under prior_keys with
    proposal 0 zeroed, the system's descriptor without termination, a stochastic ensemble in ENS_MEAN without model noise."""
    from mbpo import _hip, ops
    from mbpo.systems.termination import without_termination
    B, K, A, Xd = x0.shape[0], prior.n_candidates, prior.action_dim, system.x_dim
    seeds = torch.from_numpy(np.asarray([int(k) & (2 ** 64 - 1) for k in prior_keys], dtype=np.uint64).view(np.int64)).to(dev)
    noise = torch.zeros(horizon, B * K, A, device=dev)
    _hip.check(_hip.load().mbpo_philox_fill_grouped(seeds.data_ptr(), 0, _hip.STREAM_POLICY_NOISE, horizon, B, K * A, 0, 0, 0,
                                                    noise.data_ptr(), _hip.current_stream_ptr()), "mbpo_philox_fill_grouped")
    if prior.include_mode:
        noise.view(horizon, B, K, A)[:, :, 0] = 0.0
    spec = without_termination(system.rollout_spec(system_params, dev))
    if spec.get("system_kind") == _hip.SYS_ENSEMBLE:
        spec["ens_mode"], spec["ens_sample_noise"] = _hip.ENS_MEAN, False
    obs = x0[:, None, :].expand(B, K, Xd).reshape(B * K, Xd).contiguous()
    zeros = torch.zeros(B * K, device=dev)
    dims, flat = policy if policy is not None else (prior.policy_dims, prior.policy_params)
    rows = ops.model_rollout(policy_params=flat, policy_spec=ops.MlpSpec(dims, prior.activation, 1), x_dim=Xd, u_dim=A, obs=obs,
                             first_obs=obs.clone(), steps=zeros, done=zeros.clone(), n_steps=horizon, episode_length=2 ** 30,
                             norm_mean=prior.norm_mean, norm_std=prior.norm_std, action_clip=prior.action_clip, policy_noise=noise,
                             seed=0, offset=0, **spec)
    torch.cuda.synchronize()
    p = rows.cpu().reshape(horizon, B, K, -1)[..., Xd:Xd + A].permute(1, 2, 0, 3).contiguous()
    return p


def _prior_key(state_key):
    from mbpo.utils import keys as K
    return K.split(K.split(state_key, 2)[0], 3)[2]


def _iteration0(system, prior, dev, seed=0, **kw):
    """One iteration with the prior and without, from the same state: (opt with prior, its state, x0, candidates with, candidates
    without)."""
    x0, warm = _starts(dev, 1, system.x_dim, system.action_dim, seed=seed)
    res = []
    for pr in (prior, None):
        opt = _opt(system, pr, **kw)
        st = opt.init(7).replace(best_sequence=warm[0].clone())
        new = opt.optimize(x0[0], st)
        torch.cuda.synchronize()
        res.append((opt, st, new))
    (opt, st, new), (plain, _, pnew) = res
    assert new.key == pnew.key
    return opt, st, x0, opt._bufs["cand"].cpu(), plain._bufs["cand"].cpu()


def _check_iteration0(system, prior, dev, **kw):
    opt, st, x0, cand, plain = _iteration0(system, prior, dev, **kw)
    K, A, P = prior.n_candidates, system.action_dim, opt.opt_params.num_particles
    NC = opt._bufs["NC"]
    assert cand.shape == (NC, H, A) and NC == _P["num_samples"] + opt.num_prev
    assert _same(cand[K:], plain[K:])                                       # sampled slots [K, num_samples) and the carried elites
    p = _direct_proposals(system, st.system_params, prior, x0, [_prior_key(st.key)], H, dev)
    u_min, u_max = opt._bufs["u_min"].cpu(), opt._bufs["u_max"].cpu()
    want = pref.clip(p[0], u_min, u_max)
    assert bool(torch.isfinite(p).all())
    assert _same(cand[:K], want), "slots [0, K) are the clipped proposals of the direct rollout"
    assert not _same(cand[:K], plain[:K])
    act = opt._bufs["actions"].cpu().reshape(H, NC, P, A)
    for q in range(P):
        assert _same(act[:, :, q].permute(1, 0, 2), cand), "actions is the P-fold replication of the candidates"
    return cand, p


def test_iteration_zero_on_the_pendulum(dev):
    from mbpo.systems import PendulumSystem
    prior = _prior(dev)
    cand, p = _check_iteration0(PendulumSystem(), prior, dev)
    assert not _same(cand[1], cand[0]) and not _same(cand[2], cand[1])     # the mode sequence and two noisy ones
    _check_iteration0(PendulumSystem(), _prior(dev, n_candidates=1), dev)   # K = 1: the mode sequence alone
    _check_iteration0(PendulumSystem(), _prior(dev, n_candidates=8), dev)   # K == num_samples


def test_iteration_zero_with_bounds_that_clip(dev):
    from mbpo.systems import PendulumSystem
    prior = _prior(dev, params=cases.random_policy(DIMS, seed=1, scale=4.0))
    cand, p = _check_iteration0(PendulumSystem(), prior, dev, params=dict(u_min=-0.3, u_max=0.2))
    lo, hi = torch.tensor(-0.3), torch.tensor(0.2)                         # (the bounds as the float32 the kernel reads)
    assert float(p.abs().max()) > 0.3 and bool((cand[:3] <= hi).all()) and bool((cand[:3] >= lo).all())
    assert bool((cand[:3] == hi).any()) or bool((cand[:3] == lo).any())


def _ensemble(dev, mode, noise=False, x_dim=3, u_dim=1, hidden=(64, 64), dyn=None, **kw):
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, QuadraticReward
    dyn = dyn or EnsembleDynamics(x_dim, u_dim, n_members=5, hidden_layer_sizes=hidden, device=dev)
    return EnsembleSystem(dyn, QuadraticReward(x_dim, u_dim), mode=mode, sample_noise=noise, **kw)


def test_iteration_zero_on_an_ensemble_and_ts1_proposals_equal_the_mean_modes(dev):
    from mbpo.systems import EnsembleDynamics
    dyn = EnsembleDynamics(3, 1, n_members=5, hidden_layer_sizes=(64, 64), device=dev)
    prior = _prior(dev)
    mean_cand, _ = _check_iteration0(_ensemble(dev, "mean", dyn=dyn), prior, dev)
    ts1_cand, _ = _check_iteration0(_ensemble(dev, "ts1", noise=True, dyn=dyn), prior, dev)
    assert _same(ts1_cand[:3], mean_cand[:3])                               # proposals run in ENS_MEAN without model noise


def test_iteration_zero_on_an_optimistic_ensemble(dev):
    system = _ensemble(dev, "optimistic", beta=1.5)
    A = system.action_dim
    assert A == 1 + 3
    dims = [3, 64, 64, 2 * A]
    cand, p = _check_iteration0(system, _prior(dev, dims=dims), dev)
    assert cand.shape[-1] == A and p.shape == (1, 3, H, A)


def _pendulum_value(dev):
    import terminal_value_cases as tvcases
    from test_gpu_terminal_value import _tv
    return _tv(tvcases.make_case(tvcases.SHAPES[0], "Q"), dev)


@pytest.mark.parametrize("kind", ["pendulum", "ts1", "pendulum_value_and_cost"])
def test_batched_equals_single_calls(dev, kind):
    from mbpo.systems import Group, PendulumSystem, Term, TermCost
    B = 3
    kw = {}
    if kind == "ts1":
        system = _ensemble(dev, "ts1", noise=True)
    else:
        system = PendulumSystem()
        if kind == "pendulum_value_and_cost":
            kw = dict(terminal_value=_pendulum_value(dev),
                      cost_fn=TermCost(3, 1, bias=-3.0, groups=[Group([Term("x_next", 2, "abs")])], reduce="max"))
    params = dict(num_steps=2, num_samples=30, num_elites=6, init_std=0.6, alpha=0.1, exponent=1.0)
    opt = _opt(system, _prior(dev), params=params, **kw)
    x0, warm = _starts(dev, B, 3, 1, seed=1)
    new = _compare_with_single_calls(opt, x0, warm)
    assert bool(torch.isfinite(new.best_reward).all()) and len(set(float(v) for v in new.best_reward)) == B
    # the prior took part: the batched candidates' slots [0, K) are the direct proposals of every problem under its own key
    st = opt.init(7, batch_size=B)
    keys = [_prior_key(k) for k in st.key]
    p = _direct_proposals(system, st.system_params, opt.policy_prior, x0, keys, H, dev)
    bb = opt._bbufs
    assert bb["pp_rows"].shape == (H * B * 3, 2 * 3 + 1 + 3) and bb["pp_seeds"].shape == (B,) and bb["pp_noise"].shape == (H, B * 3, 1)
    got = bb["pp_rows"].cpu().reshape(H, B, 3, -1)[..., 3:4].permute(1, 2, 0, 3)
    assert _same(got, p)
    assert _same(bb["cand"].cpu()[:, :3], pref.clip(p, bb["u_min"].cpu(), bb["u_max"].cpu()))      # every_iteration: the last one too


def _target_plan(system, dev):
    """PlanRewardParams of r = -(u - 0.8)^2"""
    from mbpo.systems import Group, PlanRewardParams, Term, TermReward
    reward = TermReward(3, 1, groups=[Group([Term("u", 0, "square", 1.0, 0.8)], weight=-1.0)])
    return PlanRewardParams.stack(reward, [[reward.init_params(0)]], dev)


def _with_plan(st, prp):
    return st.replace(system_params=st.system_params.replace(reward_params=prp))


def test_the_prior_finds_what_sampling_cannot(dev):
    """The test that fails without the feature.  r = -(u - 0.8)^2, init_std = 0.01, no warm start: every sample is clip(0.01 z) with a
    unit-variance z, so any run with |z| < 6 has |u| < 0.06 and best_reward < -(0.8 - 0.06)^2 = -0.5476.  The policy's mode is
    tanh(atanh(0.8)) at every state (all weights zero)."""
    from mbpo.systems import PendulumSystem
    system = PendulumSystem()
    prp = _target_plan(system, dev)
    params = dict(num_steps=2, init_std=0.01, warm_start=False)
    x0, _ = _starts(dev, 1, 3, 1, seed=2)
    plain = _opt(system, None, params=params)
    st = _with_plan(plain.init(7), prp)
    without = plain.optimize(x0[0], st)
    print(f"without a prior: best_reward {float(without.best_reward):.6f}, max |u| {float(without.best_sequence.abs().max()):.4f}")
    assert float(without.best_reward) < -0.5
    flat = cases.constant_policy(DIMS, 0.8, raw_scale=-10.0)
    prior = _prior(dev, params=flat, n_candidates=2, norm_mean=None, norm_std=None)
    opt = _opt(system, prior, params=params)
    new = opt.optimize(x0[0], st)
    mode = _direct_proposals(system, st.system_params.replace(reward_params=system.reward.init_params(0)), prior, x0, [_prior_key(st.key)], H, dev)[0, 0]
    print(f"with the prior: best_reward {float(new.best_reward):.3e}, mode {mode.reshape(-1).tolist()}")
    assert abs(float(mode[0, 0]) - 0.8) < 1e-6
    assert _same(new.best_sequence.cpu(), mode), "best_sequence is the mode proposal in all four steps"
    assert float(new.best_reward) > -1e-6
    assert new.key == without.key
    # init_mean: the mean the first sample launch reads is the clipped mode proposal.  With init_std = 0 a sampled slot IS that mean:
    # K = 1 of num_samples = 2, one iteration — slot 1 was sampled around the mean and slot 0 seeded.
    lo_hi = dict(u_min=-0.5, u_max=0.5)
    for init_mean, want in ((True, 0.5), (False, 0.0)):
        pr = _prior(dev, params=flat, n_candidates=1, norm_mean=None, norm_std=None, init_mean=init_mean)
        one = _opt(system, pr, params=dict(num_steps=1, init_std=0.0, warm_start=False, num_samples=2, num_elites=2, **lo_hi))
        one.optimize(x0[0], _with_plan(one.init(7), prp))
        cand = one._bufs["cand"].cpu()
        assert _same(cand[0], torch.full((H, 1), 0.5)), "slot 0: the mode proposal clipped to u_max"
        assert _same(cand[1], torch.full((H, 1), want)), f"slot 1 (sampled at std 0) is the mean: init_mean {init_mean}"


def test_every_iteration_false_seeds_the_first_iteration_only(dev, monkeypatch):
    from mbpo import ops
    from mbpo.systems import PendulumSystem
    calls = []
    real = ops.icem_seed_candidates

    def counted(*a, **kw):
        calls.append((kw.get("candidates") is not None, kw.get("mean") is not None))
        return real(*a, **kw)

    monkeypatch.setattr(ops, "icem_seed_candidates", counted)
    system = PendulumSystem()
    x0, warm = _starts(dev, 1, 3, 1)
    want = {(True, False): [(True, False)] * 3, (False, False): [(True, False)], (True, True): [(False, True)] + [(True, False)] * 3,
            (False, True): [(False, True), (True, False)]}
    cands = {}
    for (every, init_mean), seq in want.items():
        calls.clear()
        opt = _opt(system, _prior(dev, every_iteration=every, init_mean=init_mean), params=dict(num_steps=3))
        opt.optimize(x0[0], opt.init(7).replace(best_sequence=warm[0].clone()))
        assert calls == seq, (every, init_mean)
        cands[(every, init_mean)] = opt._bufs["cand"].cpu()
    # the last iteration's slots [0, K): the proposals when every iteration is seeded, sampled ones otherwise
    assert _same(cands[(True, False)][:3], cands[(True, True)][:3]) and not _same(cands[(False, False)][:3], cands[(True, False)][:3])
    calls.clear()
    opt = _opt(system, None, params=dict(num_steps=3))
    opt.optimize(x0[0], opt.init(7))
    assert calls == []


def test_policy_prior_none_changes_nothing_and_allocates_nothing(dev):
    from mbpo.optimizers import iCemParams, iCemTO
    from mbpo.systems import PendulumSystem
    params = iCemParams(**{**_P, "num_steps": 2})
    B = 3
    x0, warm = _starts(dev, B, 3, 1)
    res = []
    for kw in ({}, dict(policy_prior=None)):
        opt = iCemTO(horizon=H, action_dim=1, opt_params=params, key=5, **kw)
        opt.set_system(PendulumSystem())
        one = opt.optimize(x0[0], opt.init(7).replace(best_sequence=warm[0].clone()))
        many = opt.optimize(x0, opt.init(7, batch_size=B).replace(best_sequence=warm.clone()))
        assert not any(k.startswith("pp_") for k in list(opt._bufs) + list(opt._bbufs))
        res.append((one, many, opt._bufs["cand"].clone(), opt._bbufs["cand"].clone()))
    for a, b in zip(res[0][:2], res[1][:2]):
        assert _same(a.best_sequence, b.best_sequence) and _same(a.best_reward, b.best_reward) and a.key == b.key
    assert _same(res[0][2], res[1][2]) and _same(res[0][3], res[1][3])
    with_prior = _opt(PendulumSystem(), _prior(dev))
    with_prior.optimize(x0[0], with_prior.init(7))
    assert with_prior._bufs["pp_rows"].shape == (H * 3, 10) and with_prior._bufs["pp_obs"].shape == (3, 3)


def test_user_defined_system(dev):
    from test_gpu_generic_system import _user_pendulum
    system = _user_pendulum()()
    assert not system.fused
    Hs = 3
    prior = _prior(dev, n_candidates=2)
    x0, warm = _starts(dev, 1, 3, 1, horizon=Hs)
    opt = _opt(system, prior, horizon=Hs)
    st = opt.init(7).replace(best_sequence=warm[0].clone())
    opt.optimize(x0[0], st)
    torch.cuda.synchronize()
    cand = opt._bufs["cand"].cpu()
    p = _direct_proposals(system, st.system_params, prior, x0, [_prior_key(st.key)], Hs, dev)
    assert bool(torch.isfinite(p).all()) and not _same(p[0, 0], p[0, 1])
    assert _same(cand[:2], pref.clip(p[0], opt._bufs["u_min"].cpu(), opt._bufs["u_max"].cpu()))
    plain = _opt(system, None, horizon=Hs)
    plain.optimize(x0[0], st)
    assert _same(plain._bufs["cand"].cpu()[2:], cand[2:])


def test_a_policy_narrower_than_the_ensemble_runs_through_its_embedded_copy(dev):
    from mbpo import ops
    system = _ensemble(dev, "mean", hidden=(128, 128))
    assert system.dynamics.kernel_width == 128
    src = cases.random_policy(DIMS, seed=4).to(dev)
    prior = _prior(dev, params=src)
    x0, warm = _starts(dev, 1, 3, 1)
    opt = _opt(system, prior)
    st = opt.init(7).replace(best_sequence=warm[0].clone())

    def slots():
        opt.optimize(x0[0], st)
        torch.cuda.synchronize()
        return opt._bufs["cand"].cpu()[:3].clone()

    wide = [3, 128, 128, 2]
    first = slots()
    p = _direct_proposals(system, st.system_params, prior, x0, [_prior_key(st.key)], H, dev, policy=(wide, ops.embed_mlp_params(src, DIMS, 128)))
    assert _same(first, pref.clip(p[0], opt._bufs["u_min"].cpu(), opt._bufs["u_max"].cpu()))
    src.copy_(cases.random_policy(DIMS, seed=5).to(dev))                   # an in-place refresh of the source ...
    assert _same(slots(), first)                                            # ... is not seen by the copy
    prior.refresh()
    second = slots()
    assert not _same(second, first)
    p2 = _direct_proposals(system, st.system_params, prior, x0, [_prior_key(st.key)], H, dev, policy=(wide, ops.embed_mlp_params(src, DIMS, 128)))
    assert _same(second, pref.clip(p2[0], opt._bufs["u_min"].cpu(), opt._bufs["u_max"].cpu()))
    from mbpo.optimizers import PolicyPrior
    d256 = [3, 256, 256, 2]
    with pytest.raises(ValueError, match="exceeds the width"):
        _opt(system, PolicyPrior(3, torch.zeros(cases.n_params(d256), device=dev), d256, n_candidates=2))


# ------------------------------------------------------------------------------------------------ the example
def test_example_runs_with_a_policy_prior(dev):
    """--policy-prior with --terminal-value: one short SAC run, then the short-horizon MPC four ways."""
    import os
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    r = subprocess.run([sys.executable, str(root / "examples" / "icem_pendulum.py"), "--policy-prior", "4", "--terminal-value", "--tv-horizon",
                        "3", "--steps", "2", "--sac-steps", "1500"], capture_output=True, text=True, env=dict(os.environ), timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("horizon 3")]
    assert len(lines) == 4 and [w in ln for w, ln in zip(("plain", "critic only", "prior only", "critic and prior"), lines)] == [True] * 4
    assert "PolicyPrior(x_dim 3, action_dim 1" in r.stdout and "n_candidates 4" in r.stdout and "TerminalValue(kind Q" in r.stdout
