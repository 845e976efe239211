"""GPU parity of the learned reward (MBPO_REWARD_LEARNED): the fit's gradients, the three rollout kernels, System.step, the fused
BPTT actor gradient and an end-to-end fit, against the test restatement (tests/learned_reward_ref.py) on the oracle.  Tolerances are
those of tests/test_gpu_ensemble_train.py, tests/test_gpu_rollout.py and tests/test_gpu_bptt.py."""
import math

import numpy as np
import pytest
import torch

from oracle import bptt as obptt
from oracle import nets as onets
from oracle import rollout as oro

import learned_reward_ref as lref
from test_gpu_bptt import _assert_matches_oracle, _set_zstore, _setup
from test_gpu_rollout import _set_rollout_lean

pytestmark = pytest.mark.gpu

MIN_STD = 1e-3
MODES = {"mean": 0, "ts1": 1, "tsinf": 2}


def _lr_params(dims, E, g, scale=0.5):
    return torch.cat([onets.init_mlp_flat(dims, g) * scale + 0.01 * torch.randn(onets.n_params(dims), generator=g) for _ in range(E)])


# ---------------------------------------------------------------------------------------------------------------- 1. fit gradients
@pytest.mark.parametrize("X,U,E,B,hidden,delta,seed", [
    (4, 1, 5, 256, (64, 64, 64), True, 0),
    (3, 1, 3, 70, (64, 64, 64), True, 1),      # Pendulum shape, ragged batch
    (6, 2, 2, 48, (64, 64), False, 2),         # absolute prediction, output 14 wide
    (4, 1, 4, 16 * 150, (64,), True, 4),       # more tiles than slots
])
def test_ens_nll_grads_with_reward_head(dev, X, U, E, B, hidden, delta, seed):
    from mbpo import ops
    g = torch.Generator().manual_seed(seed)
    dims = [X + U, *hidden, 2 * X + 2]
    P = onets.n_params(dims)
    params = torch.cat([onets.init_mlp_flat(dims, g) + 0.02 * torch.randn(P, generator=g) for _ in range(E)])
    R, D = 500, 2 * X + U + 3
    rows = torch.randn(R, D, generator=g)
    rows[:, X + U + 2:2 * X + U + 2] = rows[:, :X] + 0.1 * torch.randn(R, X, generator=g)
    idx = torch.randint(0, R, (E, B), generator=g)
    roff = X + U
    ref_g, ref_l = lref.nll_grads(params, dims, E, rows, idx, X, U, delta, MIN_STD, reward_off=roff)
    op = ops.EnsembleNllGrad(x_dim=X, u_dim=U, spec=ops.MlpSpec(dims, "swish", E), batch=B, device=dev, predict_delta=delta)
    got = op(params.to(dev), rows.to(dev), idx.to(torch.int32).to(dev), reward_off=roff).clone()
    torch.cuda.synchronize()
    np.testing.assert_allclose(op.metrics.cpu().numpy(), ref_l.numpy(), rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(got.cpu(), ref_g, atol=2e-6, rtol=5e-4)
    g64, _ = lref.nll_grads(params.double(), dims, E, rows.double(), idx, X, U, delta, MIN_STD, reward_off=roff)
    rel = float((got.cpu().double() - g64).norm() / g64.norm())
    assert rel < 5e-5, rel
    # reward_off = -1 on the same net: the state terms alone, the head's weights get zero
    got0 = op(params.to(dev), rows.to(dev), idx.to(torch.int32).to(dev)).clone()
    ref0, _ = lref.nll_grads(params, dims, E, rows, idx, X, U, delta, MIN_STD, reward_off=None)
    torch.testing.assert_close(got0.cpu(), ref0, atol=2e-6, rtol=5e-4)


def test_ens_nll_reward_off_minus_one_is_the_state_nll(dev):
    """reward_off = -1 on a 2X + 2 net: the state NLL alone — its gradient on the state weights is the 2X net's (the head cut off),
    the head's own weights get exactly zero, and the loss is the same."""
    from mbpo import ops
    X, U, E, B = 4, 1, 5, 256
    g = torch.Generator().manual_seed(5)
    dims = [X + U, 64, 64, 64, 2 * X + 2]
    params = _lr_params(dims, E, g, 1.0)
    cut = lref.reward_head_params(params, dims, E)
    rows = torch.randn(400, 2 * X + U + 3, generator=g)
    idx = torch.randint(0, 400, (E, B), generator=g).to(torch.int32).to(dev)
    op2 = ops.EnsembleNllGrad(x_dim=X, u_dim=U, spec=ops.MlpSpec(dims[:-1] + [2 * X], "swish", E), batch=B, device=dev)
    g2 = op2(cut.to(dev), rows.to(dev), idx).clone().cpu()
    op4 = ops.EnsembleNllGrad(x_dim=X, u_dim=U, spec=ops.MlpSpec(dims, "swish", E), batch=B, device=dev)
    g4 = op4(params.to(dev), rows.to(dev), idx).clone().cpu()
    torch.cuda.synchronize()
    torch.testing.assert_close(op4.metrics.cpu(), op2.metrics.cpu(), atol=1e-6, rtol=1e-6)
    P = onets.n_params(dims)
    head = torch.zeros(P, dtype=torch.bool)
    for t in onets.unflatten(torch.arange(P, dtype=torch.float64), dims)[-1]:
        head[t[..., -2:].reshape(-1).long()] = True
    g4 = g4.reshape(E, P)
    assert float(g4[:, head].abs().max()) == 0.0
    torch.testing.assert_close(g4[:, ~head].reshape(-1), g2, atol=1e-6, rtol=1e-5)


# ------------------------------------------------------------------------------------------------------------- 2./3. rollouts
def _rollout_case(dev, *, N, S, L, AR, X, E, mode="mean", noise=False, ppo=False, env_major=False, hidden=(64, 64, 64), seed=0,
                  reward="learned", dpar=None, ddims=None, check=True, philox_seed=None, oracle_members=None):
    """philox_seed: the kernels draw the 'ts1' members from Philox (no member_idx); oracle_members are the draws the oracle takes."""
    from mbpo import _hip, ops
    U = 1
    g = torch.Generator().manual_seed(seed)
    pdims = [X, *hidden, 2 * U]
    ppar = onets.init_mlp_flat(pdims, g) + 0.02 * torch.randn(onets.n_params(pdims), generator=g)
    obs0, first = torch.randn(N, X, generator=g), torch.randn(N, X, generator=g)
    steps0 = torch.randint(0, L, (N,), generator=g).float()
    done0 = (torch.rand(N, generator=g) < 0.2).float()
    pnoise = torch.randn(S, N, U, generator=g)
    mnoise = torch.randn(S, AR, N, X, generator=g) if noise else None
    midx = torch.randint(0, E, (S, AR, N), generator=g, dtype=torch.int32) if mode == "ts1" else None
    if philox_seed is not None:
        midx = oracle_members
    if ddims is None:
        ddims = [X + U, *hidden, 2 * X + 2]
        dpar = _lr_params(ddims, E, g)
    kw = dict(system_kind=_hip.SYS_ENSEMBLE, dyn_params=dpar.to(dev), dyn_spec=ops.MlpSpec(ddims, "swish", E), ens_mode=MODES[mode],
              ens_predict_delta=True, ens_sample_noise=noise, ens_min_std=MIN_STD)
    if reward == "learned":
        kw.update(reward_kind=_hip.REWARD_LEARNED, reward_params=None)
    else:
        tg = torch.Generator().manual_seed(99)
        kw.update(reward_kind=_hip.REWARD_QUADRATIC,
                  reward_params=torch.cat([torch.randn(X, generator=tg), torch.rand(X, generator=tg), torch.rand(U, generator=tg)]).to(dev))
    obs_d, steps_d, done_d = obs0.to(dev), steps0.to(dev), done0.to(dev)
    rows = ops.model_rollout(policy_params=ppar.to(dev), policy_spec=ops.MlpSpec(pdims, "swish", 1), x_dim=X, u_dim=U, obs=obs_d,
                             first_obs=first.to(dev), steps=steps_d, done=done_d, n_steps=S, episode_length=L, action_repeat=AR,
                             ppo_extras=ppo, env_major=env_major, policy_noise=pnoise.to(dev),
                             model_noise=None if mnoise is None else mnoise.to(dev),
                             member_idx=None if (midx is None or philox_seed is not None) else midx.to(dev),
                             seed=0 if philox_seed is None else philox_seed, **kw).cpu()
    if check:
        osystem = lref.LearnedRewardEnsembleSystem(dpar, ddims, E, X, U, mode=mode, predict_delta=True, sample_noise=noise, min_std=MIN_STD)
        st_ref, rows_ref = oro.rollout(osystem, ppar, pdims, oro.EnvState(obs0, first, steps0, done0), S, L, AR, policy_noise=pnoise,
                                       model_noise=mnoise, member_idx=midx, ppo_extras=ppo, env_major=env_major)
        D = rows.shape[1]
        assert torch.equal(rows[:, X + U + 1], rows_ref[:, X + U + 1]) and torch.equal(rows[:, D - 1], rows_ref[:, D - 1])
        assert torch.equal(steps_d.cpu(), st_ref.steps) and torch.equal(done_d.cpu(), st_ref.done)
        torch.testing.assert_close(rows, rows_ref, atol=2e-4, rtol=2e-4)
        torch.testing.assert_close(obs_d.cpu(), st_ref.obs, atol=2e-4, rtol=2e-4)
        # the reward column is the head, not zero or a stale analytic value
        assert float(rows[:, X + U].abs().max()) > 1e-3
    return rows


CASES = [
    dict(N=512, S=5, L=5, X=4, E=5, mode="mean"),
    dict(N=77, S=6, L=4, X=4, E=5, mode="ts1"),
    dict(N=77, S=6, L=4, X=4, E=5, mode="ts1", noise=True),
    dict(N=130, S=5, L=5, X=3, E=3, mode="tsinf", ppo=True, env_major=True),
    dict(N=300, S=6, L=4, X=2, E=4, mode="ts1", noise=True, ppo=True, env_major=True),
    dict(N=4800, S=3, L=2, X=4, E=5, mode="mean", hidden=(64, 64)),
]


@pytest.mark.parametrize("kw", CASES)
def test_learned_reward_rollout_lean_equals_generic(dev, kw):
    """Every rollout kernel the 64-wide dispatch can pick matches the restatement; the lean kernel (one tile, two tiles in flight) is
    bit-identical to k_model_rollout64."""
    try:
        _set_rollout_lean(0)
        rg = _rollout_case(dev, AR=1, **kw)
        _set_rollout_lean(3)
        rl = _rollout_case(dev, AR=1, **kw)
        _set_rollout_lean(2)
        rp = _rollout_case(dev, AR=1, **kw)
    finally:
        _set_rollout_lean(-1)
    assert torch.equal(rg, rl)
    assert torch.equal(rg, rp)


@pytest.mark.parametrize("kw", [
    dict(N=100, S=4, L=5, X=4, E=5, mode="mean", AR=2),
    dict(N=100, S=4, L=5, X=4, E=5, mode="ts1", noise=True, AR=2),                 # k_model_rollout64 (the lean kernel takes AR 1 only)
    dict(N=70, S=3, L=4, X=4, E=3, mode="tsinf", AR=1, hidden=(128, 128)),         # k_model_rollout<128>
    dict(N=70, S=3, L=4, X=5, E=3, mode="ts1", noise=True, AR=2, hidden=(128, 128), ppo=True, env_major=True),
])
def test_learned_reward_rollout_other_kernels(dev, kw):
    _rollout_case(dev, **kw)


@pytest.mark.parametrize("mode,noise", [("mean", False), ("ts1", True), ("tsinf", False)])
def test_reward_head_does_not_perturb_the_state_path(dev, mode, noise):
    """A 2X + 2 ensemble under QuadraticReward gives the rows of the same weights with the reward columns cut, bit for bit (lean and
    generic kernels)."""
    X, E, hidden = 4, 5, (64, 64, 64)
    g = torch.Generator().manual_seed(7)
    dims = [X + 1, *hidden, 2 * X + 2]
    dp = _lr_params(dims, E, g)
    cut = lref.reward_head_params(dp, dims, E)
    try:
        for lean in (0, 1):
            _set_rollout_lean(lean)
            kw = dict(N=200, S=5, L=4, AR=1, X=X, E=E, mode=mode, noise=noise, reward="quadratic", check=False)
            a = _rollout_case(dev, dpar=dp, ddims=dims, **kw)
            b = _rollout_case(dev, dpar=cut, ddims=dims[:-1] + [2 * X], **kw)
            assert torch.equal(a, b)
    finally:
        _set_rollout_lean(-1)


# ------------------------------------------------------------------------------------------------------------ 4. System.step
@pytest.mark.parametrize("mode", ["mean", "tsinf"])
def test_system_step_and_learned_reward_call(dev, mode):
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, LearnedReward
    X, U, E, n = 4, 1, 5, 300
    dyn = EnsembleDynamics(X, U, n_members=E, device=dev, learn_reward=True)
    system = EnsembleSystem(dyn, LearnedReward(dyn), mode=mode)
    sp = system.init_params(4)
    g = torch.Generator().manual_seed(2)
    sp.dynamics_params.params.add_(0.05 * torch.randn(sp.dynamics_params.params.numel(), generator=g).to(dev))
    x, u = torch.randn(n, X, generator=g), torch.rand(n, U, generator=g) * 2 - 1
    st = system.step(x.to(dev), u.to(dev), sp)
    dp = sp.dynamics_params.params.cpu()
    ref = lref.LearnedRewardEnsembleSystem(dp, dyn.dims, E, X, U, mode=mode)
    xn, r = ref.step(x, u, env_index=torch.arange(n))
    torch.testing.assert_close(st.x_next.cpu(), xn, atol=2e-4, rtol=2e-4)
    torch.testing.assert_close(st.reward.cpu(), r, atol=2e-4, rtol=2e-4)
    dist, rp = system.reward(x.to(dev), u.to(dev), sp.reward_params)
    assert rp is sp.reward_params
    y = onets.ensemble_forward(dp, dyn.dims, E, torch.cat([x, u], 1))
    torch.testing.assert_close(dist.mean().cpu(), y[..., 2 * X].mean(0), atol=2e-5, rtol=2e-5)
    sig = torch.nn.functional.softplus(y[..., 2 * X + 1]) + MIN_STD
    std = torch.sqrt((sig ** 2).mean(0) + y[..., 2 * X].var(0, unbiased=False))
    torch.testing.assert_close(dist.stddev().cpu(), std, atol=2e-5, rtol=2e-5)
    if mode == "mean":
        torch.testing.assert_close(dist.mean().cpu(), st.reward.cpu(), atol=2e-5, rtol=2e-5)
    # next_state's std reads the state columns only
    nd, _ = dyn.next_state(x.to(dev), u.to(dev), sp.dynamics_params)
    assert nd.stddev().shape == (n, X)


# ------------------------------------------------------------------------------------------------------------------ 5. BPTT
def _lr_bptt_setup(X, U, H, n, E, seed=0):
    cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, _, extra = _setup(X, U, H, n, "ensemble", E, seed)
    g = torch.Generator().manual_seed(seed + 50)
    dd = [X + U, 64, 64, 64, 2 * X + 2]
    dp = _lr_params(dd, E, g)
    P = onets.n_params(dd)
    for e in range(E):
        dp[(e + 1) * P - X - 2:(e + 1) * P - 2] -= 2.0            # raw-std biases of the state: sigma ~ 0.13
    members = torch.randint(0, E, (n, H), generator=g, dtype=torch.int32)
    eps = torch.randn(n, H, X, generator=g)
    return cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, dd, dp, members, eps


def _run_lr_bptt(dev, cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, dd, dp, n, mode, with_noise, members=None, eps=None):
    from mbpo import _hip, ops
    op = ops.BpttActorGrad(x_dim=cfg.x_dim, u_dim=cfg.u_dim, horizon=cfg.horizon, actor_dims=cfg.actor_dims, critic_dims=cfg.critic_dims,
                           n=n, device=dev, init_stddev=cfg.init_stddev, discount=cfg.discount, lambda_=cfg.lambda_, ent_coef=cfg.ent_coef)
    E = dp.numel() // onets.n_params(dd)
    op(actor_params=ap.to(dev), target_critic_params=cp.to(dev), init_states=x0.to(dev), state_mean=s_mean.to(dev), state_std=s_std.to(dev),
       reward_mean_std=r_ms.to(dev), act_noise=noise.to(dev), system_kind=_hip.SYS_ENSEMBLE, reward_kind=_hip.REWARD_LEARNED,
       reward_params=None, dyn_params=dp.to(dev), dyn_spec=ops.MlpSpec(dd, "swish", E), ens_predict_delta=True, ens_mode=MODES[mode],
       ens_sample_noise=with_noise, ens_min_std=MIN_STD, member_idx=None if members is None else members.to(dev).contiguous(),
       model_noise=None if eps is None else eps.to(dev).contiguous())
    torch.cuda.synchronize()
    return op


@pytest.mark.parametrize("X,U,H,n,E,mode,with_noise", [
    (4, 1, 5, 48, 5, "mean", False),           # two member rounds (4 + 1)
    (4, 1, 5, 48, 5, "ts1", True),
    (4, 1, 5, 48, 5, "tsinf", False),
    (4, 2, 6, 17, 3, "ts1", False),            # one round, ragged n, u = 2
    (3, 1, 8, 33, 3, "mean", False),
])
def test_bptt_learned_reward_parity(dev, X, U, H, n, E, mode, with_noise):
    cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, dd, dp, members, eps = _lr_bptt_setup(X, U, H, n, E)
    m = None if mode == "mean" else (members if mode == "ts1" else (torch.arange(n, dtype=torch.int32) % E)[:, None].expand(n, H))
    e = eps if with_noise else None
    sys32 = lref.TorchLearnedRewardSystem(dp, dd, E, X, U, members=m, eps=e)
    g_ref, _, aux = obptt.actor_grads(cfg, sys32, ap, cp, x0, noise, s_mean, s_std, r_ms[0], r_ms[1])
    d = lambda t: t.double()
    sys64 = lref.TorchLearnedRewardSystem(d(dp), dd, E, X, U, members=m, eps=None if e is None else d(e))
    g64, loss64, aux64 = obptt.actor_grads(cfg, sys64, d(ap), d(cp), d(x0), d(noise), d(s_mean), d(s_std), d(r_ms[0]), d(r_ms[1]))
    op = _run_lr_bptt(dev, cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, dd, dp, n, mode, with_noise,
                      members=members if mode == "ts1" else None, eps=eps if with_noise else None)
    _assert_matches_oracle(op, (g_ref, aux, g64, loss64, aux64), X, U, H, n)


@pytest.mark.parametrize("mode", ["mean", "ts1"])
def test_bptt_learned_reward_zstore_equals_recompute(dev, mode):
    import os
    if os.environ.get("MBPO_BPTT_ZSTORE_MAX_MB") is not None:
        pytest.skip("MBPO_BPTT_ZSTORE_MAX_MB caps the z store in this process: the store path may not run")
    X, U, H, n, E = 4, 1, 5, 48, 5
    cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, dd, dp, members, eps = _lr_bptt_setup(X, U, H, n, E, seed=1)
    res = {}
    try:
        for zmode in (-1, 0):
            _set_zstore(zmode)
            op = _run_lr_bptt(dev, cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, dd, dp, n, mode, mode != "mean",
                              members=members if mode == "ts1" else None, eps=eps if mode != "mean" else None)
            res[zmode] = (op.workspace.numel(), op.grads.clone(), op.metrics.clone(), op.transitions.clone(), op.lambda_values.clone())
    finally:
        _set_zstore(-1)
    assert res[-1][0] > res[0][0]
    for a, b in zip(res[-1][1:], res[0][1:]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------ 7. end to end
def test_fit_learns_the_pendulum_reward(dev):
    """EnsembleDynamics(learn_reward=True).fit on true Pendulum transitions: held-out reward MSE below 5 % of the reward variance."""
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, LearnedReward, PendulumSystem
    system = PendulumSystem()
    g = torch.Generator().manual_seed(0)
    n = 6000
    th = (torch.rand(n, generator=g) * 2 - 1) * math.pi
    x = torch.stack([torch.cos(th), torch.sin(th), (torch.rand(n, generator=g) * 2 - 1) * 6], 1).to(dev)
    u = (torch.rand(n, 1, generator=g) * 2 - 1).to(dev)
    sp = system.reset().system_params
    nxt = system.step(x, u, sp)
    rows = torch.cat([x, u, nxt.reward[:, None], torch.ones(n, 1, device=dev), nxt.x_next, torch.zeros(n, 1, device=dev)], 1)
    train, test = rows[:5000], rows[5000:]
    dyn = EnsembleDynamics(3, 1, n_members=5, learn_reward=True)
    lsys = EnsembleSystem(dyn, LearnedReward(dyn))
    lsp = lsys.init_params(1)
    _, losses = dyn.fit(lsp.dynamics_params, train, num_steps=1500, batch_size=256, learning_rate=3e-3, key=7)
    assert bool(torch.isfinite(losses).all())
    pred = lsys.step(test[:, :3], test[:, 3:4], lsp).reward      # the fused kernel, through the bound parameters
    r = test[:, 4]
    mse, var = float(((pred - r) ** 2).mean()), float(r.var())
    assert mse < 0.05 * var, (mse, var)
    dist, _ = dyn.next_state(test[:, :3], test[:, 3:4], lsp.dynamics_params)
    err = float((dist.mean() - test[:, 6:9]).abs().mean())
    base = float((test[:, :3] - test[:, 6:9]).abs().mean())
    assert err < 0.25 * base, (err, base)


# ------------------------------------------------------------------------------------------------------------------- 6. iCEM
@pytest.mark.parametrize("mode,noise", [("mean", False), ("ts1", True), ("tsinf", False)])
def test_icem_learned_reward_batched_equals_single_calls(dev, mode, noise):
    """iCEM on EnsembleSystem(dyn, LearnedReward(dyn)): a batched optimize is bit-identical to single calls, stochastic modes included,
    and the learned reward steers it (a different best value than the same model under a quadratic reward)."""
    from mbpo.optimizers import iCemParams, iCemTO
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, LearnedReward, QuadraticReward
    from test_gpu_icem_batched import _SMALL, _compare_with_single_calls
    X, U, E, H, B = 4, 2, 5, 8, 3
    dyn = EnsembleDynamics(X, U, n_members=E, device=dev, learn_reward=True)
    system = EnsembleSystem(dyn, LearnedReward(dyn), mode=mode, sample_noise=noise)
    opt = iCemTO(horizon=H, action_dim=U, opt_params=iCemParams(**_SMALL), key=5)
    opt.set_system(system)
    g = torch.Generator().manual_seed(3)
    x0 = (torch.randn(B, X, generator=g) * 0.5).to(dev)
    warm = ((torch.rand(B, H, U, generator=g) - 0.5) * 1.5).to(dev)
    new = _compare_with_single_calls(opt, x0, warm)
    assert torch.isfinite(new.best_reward).all()
    qopt = iCemTO(horizon=H, action_dim=U, opt_params=iCemParams(**_SMALL), key=5)
    qopt.set_system(EnsembleSystem(dyn, QuadraticReward(X, U), mode=mode, sample_noise=noise))
    q = qopt.optimize(x0, qopt.init(7, batch_size=B).replace(best_sequence=warm.clone()))
    assert not torch.equal(q.best_reward, new.best_reward)


def test_icem_learned_reward_matches_the_oracle_objective(dev):
    """iCemTO.optimize on EnsembleSystem(dyn, LearnedReward(dyn)) ('mean') vs the numpy loop of tests/test_gpu_icem.py with the
    restated learned-reward system as the objective's step (same Philox candidates)."""
    from mbpo.optimizers import iCemParams, iCemTO
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, LearnedReward
    from mbpo.utils import keys as K
    from oracle import icem as oicem
    X, U, E, H = 4, 1, 5, 8
    params = iCemParams(num_particles=2, num_samples=120, num_elites=12, num_steps=3, exponent=1.0, alpha=0.1, init_std=0.6)
    dyn = EnsembleDynamics(X, U, n_members=E, device=dev, learn_reward=True)
    system = EnsembleSystem(dyn, LearnedReward(dyn))
    opt = iCemTO(horizon=H, action_dim=U, opt_params=params, key=5)
    opt.set_system(system)
    st = opt.init(7)
    g = torch.Generator().manual_seed(4)
    dp = st.system_params.dynamics_params.params
    dp.add_(0.1 * torch.randn(dp.numel(), generator=g).to(dev))          # biases away from zero: a reward that depends on (x, u)
    x0 = (torch.randn(X, generator=g) * 0.5).to(dev)
    new = opt.optimize(x0, st)
    torch.cuda.synchronize()
    osystem = lref.LearnedRewardEnsembleSystem(dp.cpu().double(), dyn.dims, E, X, U, mode="mean")

    def step(x, u):
        xn, r = osystem.step(torch.from_numpy(x), torch.from_numpy(u), env_index=torch.arange(x.shape[0]))
        return xn.numpy(), r.numpy()

    mean = np.zeros((H, U)); std = np.full((H, U), params.init_std)
    best_v, best_s = -np.inf, mean.copy()
    nprev = max(int(params.elite_set_fraction * params.num_elites), 1)
    prev = np.zeros((nprev, H, U))
    carry = K.split(st.key, 2)[0]
    for it in range(params.num_steps):
        sampling_key, _pk = K.split(carry, 2)
        carry = K.split(sampling_key, 2)[0]
        cand = oicem.sample_candidates(mean, std, prev, -1.0, 1.0, params.num_samples, H, U, params.exponent, sampling_key, it)
        vals = oicem.objective(step, x0.cpu().double().numpy(), cand, params.num_particles)
        mean, std, best_v, best_s, prev = oicem.update(vals, cand, mean, std, best_v, best_s, params.num_elites, nprev, params.alpha)
    assert abs(float(new.best_reward) - best_v) <= 2e-3 * max(1.0, abs(best_v))
    np.testing.assert_allclose(new.best_sequence.cpu().numpy(), best_s, atol=5e-3)


def test_rollout_philox_member_draw(dev):
    """'ts1' without member_idx: the kernels draw the member from Philox (the path SAC takes), and the reward follows the drawn member
    — lean and generic kernels against the restatement fed the oracle's Philox draws."""
    from oracle import philox
    N, S, X, E, seed = 200, 4, 4, 5, 9
    m = philox.philox_randint(seed, 0, philox.STREAM_MEMBER, np.arange(S * N, dtype=np.uint64), 0, E)
    midx = torch.from_numpy(m).to(torch.int32).reshape(S, 1, N)
    try:
        rows = []
        for lean in (0, 1):
            _set_rollout_lean(lean)
            rows.append(_rollout_case(dev, N=N, S=S, L=3, AR=1, X=X, E=E, mode="ts1", philox_seed=seed, oracle_members=midx))
    finally:
        _set_rollout_lean(-1)
    assert torch.equal(rows[0], rows[1])


# ---------------------------------------------------------------------------------------------- 5. BPTT: wide path and optimizer
def _lr_system(dev, X, U, E, mode, sample_noise=False):
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, LearnedReward
    dyn = EnsembleDynamics(X, U, n_members=E, device=dev, learn_reward=True)
    return EnsembleSystem(dyn, LearnedReward(dyn), mode=mode, sample_noise=sample_noise)


@pytest.mark.parametrize("mode,noise", [("mean", False), ("ts1", True)])
def test_bptt_wide_path_matches_the_fused_kernel(dev, mode, noise):
    """ops.BpttActorGradGeneric through torch_steps.DifferentiableBuiltin (ops.HipMlp on the device) reads the reward head as the fused
    kernel does; at width 64 both take the same Philox draws, so they agree."""
    from mbpo import ops
    from mbpo.systems.torch_steps import DifferentiableBuiltin
    X, U, H, n, E = 4, 1, 6, 40, 5
    system = _lr_system(dev, X, U, E, mode, noise)
    sp = system.init_params(5)
    spec = system.rollout_spec(sp, dev)
    assert spec["reward_params"] is None
    cfg, ap, cp, x0, _, s_mean, s_std, r_ms, _, _ = _setup(X, U, H, n, "ensemble", E, 4)
    kw = dict(x_dim=X, u_dim=U, horizon=H, actor_dims=cfg.actor_dims, critic_dims=cfg.critic_dims, n=n, device=dev,
              init_stddev=cfg.init_stddev, discount=cfg.discount, lambda_=cfg.lambda_, ent_coef=cfg.ent_coef, seed=77)
    common = dict(actor_params=ap.to(dev), target_critic_params=cp.to(dev), init_states=x0.to(dev), state_mean=s_mean.to(dev),
                  state_std=s_std.to(dev), reward_mean_std=r_ms.to(dev), offset=3, rng_dev=ops.make_rng(dev, seed=0, counter=2))
    fused = ops.BpttActorGrad(**kw)
    fused(**common, system_kind=spec["system_kind"], reward_kind=spec["reward_kind"], reward_params=spec["reward_params"],
          dyn_params=spec["dyn_params"], dyn_spec=spec["dyn_spec"], ens_predict_delta=spec["ens_predict_delta"], ens_mode=spec["ens_mode"],
          ens_sample_noise=spec["ens_sample_noise"], ens_min_std=spec["ens_min_std"])
    wide = ops.BpttActorGradGeneric(**kw)
    wide(**common, system=DifferentiableBuiltin(system, spec), system_params=sp)
    torch.cuda.synchronize()
    torch.testing.assert_close(wide.transitions, fused.transitions, atol=2e-4, rtol=2e-4)
    torch.testing.assert_close(wide.lambda_values, fused.lambda_values, atol=5e-4, rtol=5e-4)
    torch.testing.assert_close(wide.metrics, fused.metrics, atol=2e-5, rtol=1e-4)
    torch.testing.assert_close(wide.grads, fused.grads, atol=5e-6, rtol=2e-3)


@pytest.mark.parametrize("mode,sample_noise", [("mean", False), ("ts1", True)])
def test_bptt_optimizer_train_step_matches_cpu_loop(dev, mode, sample_noise):
    """One whole BPTTOptimizer train step on the learned-reward system vs oracle.bptt.CpuBpttLoop through the restated differentiable
    system (tests/test_gpu_bptt_stochastic.py's checks; the oracle takes the kernel's Philox draws at offset = train-step index)."""
    from mbpo.optimizers import BPTTOptimizer
    from oracle import philox
    from test_gpu_bptt_stochastic import _true_buffer
    X, U, E, n, H, kc = 4, 1, 3, 24, 6, 2
    system = _lr_system(dev, X, U, E, mode, sample_noise)
    sbs = _true_buffer(dev, X, U)
    opt = BPTTOptimizer(action_dim=U, obs_dim=X, horizon=H, num_samples_per_gradient_update=n, train_steps=1, init_stddev=1.5,
                        critic_updates_per_policy_update=kc, sampling_buffer_size=4096)
    opt.set_system(system)
    st0 = opt.init(key=11, true_buffer_state=sbs)
    assert st0.system_params.reward_params is st0.system_params.dynamics_params
    out1 = opt.train(bptt_state=st0)
    tsys = lref.TorchLearnedRewardSystem(st0.system_params.dynamics_params.params.cpu().clone(), system.dynamics.dims, E, X, U,
                                         True, system.min_std)
    act_seed = opt._last_seeds[1]
    cfg = obptt.BpttConfig(x_dim=X, u_dim=U, actor_dims=opt.actor_dims, critic_dims=opt.critic_dims, horizon=H, init_stddev=1.5)
    loop = obptt.CpuBpttLoop(cfg, tsys, st0.actor_params.cpu(), st0.critic_params.cpu(), sbs.data.cpu(), n, kc, opt._last_seeds,
                             buffer_size=4096)
    members = eps = None
    if mode == "ts1":
        step = loop.step_idx
        members = torch.from_numpy(philox.philox_randint(act_seed, step, philox.STREAM_MEMBER, np.arange(n * H, dtype=np.uint64),
                                                         0, E)).reshape(n, H)
        if sample_noise:
            eps = torch.from_numpy(philox.philox_normal(act_seed, step, philox.STREAM_MODEL_NOISE,
                                                        np.arange(n * H * X, dtype=np.uint64))).reshape(n, H, X)
    tsys.set_draws(members, eps)
    r = loop.step()
    assert tsys.t == H
    s1, o1 = out1.bptt_summary, out1.optimizer_state
    assert abs(float(s1.actor_loss[0]) - r["actor_loss"]) <= 2e-5 * max(1.0, abs(r["actor_loss"]))
    assert abs(float(s1.critic_loss[0]) - r["critic_loss"]) <= 1e-4 * max(1.0, abs(r["critic_loss"]))
    assert abs(float(s1.actor_grad_norm[0]) - r["actor_grad_norm"]) <= 2e-3 * r["actor_grad_norm"]
    torch.testing.assert_close(o1.reward_normalizer_state.std.cpu(), loop.r_std, atol=1e-5, rtol=1e-4)
    rel = lambda a, b: float((a.cpu() - b).norm() / b.norm())
    assert rel(o1.actor_params, loop.ap) < 2e-4 and rel(o1.critic_params, loop.cp) < 2e-4


# ------------------------------------------------------------------------------------------ 7b / SAC, PPO and the evaluator
def _lr_trainer_system(dev, mode="mean"):
    X, U, E = 4, 1, 5
    system = _lr_system(dev, X, U, E, mode)
    sp = system.init_params(1)
    g = torch.Generator().manual_seed(6)
    sp.dynamics_params.params.mul_(0.5).add_(0.02 * torch.randn(sp.dynamics_params.params.numel(), generator=g).to(dev))
    osystem = lref.LearnedRewardEnsembleSystem(sp.dynamics_params.params.cpu().clone(), system.dynamics.dims, E, X, U, mode=mode)
    return system, sp, osystem, X, U


@pytest.mark.parametrize("mode", ["mean", "ts1"])
def test_sac_learned_reward_graph_equals_eager_and_oracle(dev, mode):
    """SAC.training_epoch on the learned-reward system through the captured hipGraph (reward_params None inside the captured
    model_rollout) == the same epoch issued eagerly, bit for bit; in 'mean' both agree with CpuSacLoop after the 4 steps ('ts1' draws
    its members from Philox inside the replays)."""
    from mbpo.optimizers.policy_optimizers.sac.sac import SAC
    from mbpo.systems.brax_wrapper import BraxWrapper
    from mbpo.utils import keys as K
    import test_gpu_trainer_parity as tp
    out = []
    for use_graph in (False, True):
        system, sp, osystem, X, U = _lr_trainer_system(dev, mode)
        tb, tbs = tp._true_buffer(dev, X, U, 512)
        env = BraxWrapper(system, sp, tbs, tb)
        N, S = tp.SAC_KW["num_envs"], tp.SAC_KW["num_env_steps_between_updates"]
        tr = SAC(environment=env, num_timesteps=64 + N * S * 4, use_graph=use_graph, **tp.SAC_KW)
        ts, es, bs = tr.init_training_state(7), tr.reset_envs(env, 11, N), tr.replay_buffer.init(13)
        loop = tp._sac_oracle(tr, es, osystem, X, U) if (use_graph and mode == "mean") else None
        ts, es, bs, _ = tr.prefill_replay_buffer(ts, es, bs, 17)
        ts, es, bs, metrics = tr.training_epoch(ts, es, bs, 19)
        torch.cuda.synchronize()
        assert (tr._graph is not None) == use_graph
        out.append(dict(params=tr.updater.params.cpu().clone(), tq=tr.updater.target_q.cpu().clone(), obs=es.obs.cpu().clone(),
                        stats=tr._stats_vec.cpu().clone(), rows=tr._rollout_rows.cpu().clone(), data=bs.data.cpu().clone(),
                        state=bs.state.cpu().tolist(), rng=tr._rng.cpu().tolist(), metrics=metrics))
    a, b = out
    for k in ("params", "tq", "obs", "stats", "rows", "data"):
        assert torch.equal(a[k], b[k]), f"graph replay differs from eager in {k}"
    assert a["state"] == b["state"] and a["rng"] == b["rng"] and a["metrics"] == b["metrics"]
    assert float(b["rows"][:, X + U].abs().max()) > 1e-3                       # the reward column carries the head
    if loop is not None:
        loop.rekey(K.split(17)[0])
        loop.prefill_step()
        loop.rekey(19)
        for _ in range(4):
            loop.training_step()
        torch.testing.assert_close(b["rows"], loop.last_rows, atol=5e-3, rtol=5e-3)
        P = tr.updater.P
        assert tp._rel(b["params"][:P], loop.state.params[:P]) < 5e-3 and tp._rel(b["params"][P:-1], loop.state.params[P:-1]) < 5e-3
        np.testing.assert_allclose(b["stats"].numpy(), loop.stats, rtol=5e-4, atol=5e-5)


def test_ppo_learned_reward_training_step_matches_cpu_oracle(dev):
    """PPO.training_step on the learned-reward system (env_major rows with the PPO extras) against CpuPpoLoop."""
    from mbpo.optimizers.policy_optimizers.ppo.ppo import PPO
    from mbpo.systems.brax_wrapper import BraxWrapper
    from oracle import ppo as oppo, trainer as otr
    import test_gpu_trainer_parity as tp
    system, sp, osystem, X, U = _lr_trainer_system(dev)
    tb, tbs = tp._true_buffer(dev, X, U, 256)
    env = BraxWrapper(system, sp, tbs, tb)
    kw = tp.PPO_KW
    tr = PPO(environment=env, num_timesteps=3 * 16 * 8 * 4, **kw)
    ts = tr.init_training_state(5)
    es = env.reset([101 + i for i in range(kw["num_envs"])])
    cfg = oppo.PpoConfig(X, U, tr.policy_dims, tr.value_dims, entropy_cost=kw["entropy_cost"], discounting=kw["discounting"],
                         gae_lambda=kw["gae_lambda"], clipping_epsilon=kw["clipping_epsilon"], lr=kw["lr"], wd=kw["wd"])
    loop = otr.CpuPpoLoop(cfg, osystem, kw["num_envs"], kw["unroll_length"], kw["episode_length"], kw["batch_size"],
                          kw["num_minibatches"], kw["num_updates_per_batch"], True, init_params=tr.updater.params.cpu().clone(),
                          init_obs=es.obs.cpu().clone())
    tr.rekey(23)
    loop.rekey(23)
    for step in range(2):
        ts, es, _ = tr.training_step(ts, es)
        loop.training_step()
        torch.cuda.synchronize()
        tol = 2e-4 if step == 0 else 3e-3
        torch.testing.assert_close(tr._data.cpu(), loop.last_data, atol=tol, rtol=tol)
        lim = 1e-3 if step == 0 else 1e-2
        assert tp._rel(tr.updater.params, loop.state.params) < lim
    tr.close()


def test_evaluator_on_the_learned_reward(dev):
    """Evaluator (sac/acting.py:82-145) sums the learned reward: episode rewards and lengths against oracle.rollout.evaluate."""
    from mbpo.optimizers.policy_optimizers.sac.sac import Evaluator
    from mbpo.systems.brax_wrapper import BraxWrapper
    from mbpo.utils import keys as K
    import test_gpu_env_adapter as tea
    import test_gpu_trainer_parity as tp
    system, sp, osystem, X, U = _lr_trainer_system(dev)
    tb, tbs = tp._true_buffer(dev, X, U, 128)
    env = BraxWrapper(system, sp, tbs, tb)
    N, L, AR = 50, 12, 3
    pd, ppar = tea._policy(9, X, U)
    g = torch.Generator().manual_seed(2)
    nm, ns = torch.randn(X, generator=g) * 0.1, torch.rand(X, generator=g) + 0.5
    tr = tea._Trainer(dev, pd, True, nm.to(dev), ns.to(dev))
    ev = Evaluator(tr, env, num_eval_envs=N, episode_length=L, action_repeat=AR, key=5)
    m = ev.run_evaluation((None, ppar.to(dev)), {}, unroll_key=31)
    keys = K.split(31, N)
    _, first, _, _ = oro.brax_wrapper_reset(tb.logical_data(tbs).cpu(), tbs.insert_position, tbs.sample_position, keys, X, U)
    er, es = oro.evaluate(osystem, ppar, pd, first, L, AR, "swish", nm, ns, deterministic=True)
    torch.testing.assert_close(ev.last_episode_rewards.cpu(), er, atol=2e-3, rtol=2e-4)
    assert torch.equal(ev.last_episode_steps.cpu(), es)
    assert abs(m["eval/episode_reward"] - float(er.mean())) <= 2e-4 * abs(float(er.mean())) + 1e-3
    assert float(er.abs().max()) > 1e-3
