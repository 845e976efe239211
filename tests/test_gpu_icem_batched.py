"""Batched iCEM (one launch chain for B problems) against B single-problem optimize calls, bit for bit: the analytic Pendulum under
both update kernels and past the 60 KB LDS threshold, the fused EnsembleSystem in 'mean', 'ts1' with model noise and 'tsinf', the
constraint term under pessimism, a NaN problem next to finite ones, the grouped Philox fill against per-problem fills, and batched
MPC on the Pendulum (after the reference's tests/test_icemopt.py) against per-environment single MPC loops."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().contiguous().view(torch.int32)


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """bit equality (NaN == NaN with the same payload, -0 != +0)"""
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _set_icem_update(mode: int) -> None:
    from mbpo import _hip
    lib = _hip.load()
    lib.mbpo_debug_set_icem_update.argtypes = [C.c_int]
    lib.mbpo_debug_set_icem_update.restype = C.c_int
    assert lib.mbpo_debug_set_icem_update(mode) == 0


@pytest.fixture
def icem_update_mode():
    yield _set_icem_update
    _set_icem_update(-1)


def _compare_with_single_calls(opt, x0: torch.Tensor, warm: torch.Tensor, init_key: int = 7):
    """One batched optimize over B problems vs B single optimize calls on (x0[b], warm[b], key[b])."""
    B = x0.shape[0]
    bst = opt.init(init_key, batch_size=B)
    assert bst.best_sequence.shape == (B, opt.horizon, opt.action_dim) and bst.best_reward.shape == (B,)
    assert len(bst.key) == B and len(set(bst.key)) == B
    bst = bst.replace(best_sequence=warm.clone())
    bnew = opt.optimize(x0, bst)
    sst = opt.init(init_key)
    from mbpo.utils import keys as K
    assert bst.key == K.split(sst.key, B)
    for b in range(B):
        one = opt.optimize(x0[b], sst.replace(key=bst.key[b], best_sequence=warm[b].clone()))
        assert _same(bnew.best_sequence[b], one.best_sequence), f"problem {b}: best_sequence"
        assert _same(bnew.best_reward[b], one.best_reward), f"problem {b}: best_reward"
        assert bnew.key[b] == one.key == K.split(bst.key[b], 2)[1], f"problem {b}: key"
    torch.cuda.synchronize()
    return bnew


def _pendulum_case(dev, B, H, params, seed=0, **kw):
    from mbpo.optimizers import iCemTO
    from mbpo.systems import PendulumSystem
    opt = iCemTO(horizon=H, action_dim=1, opt_params=params, key=5, **kw)
    opt.set_system(PendulumSystem())
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(B, 3, generator=g)
    ang = torch.rand(B, generator=g) * 6.28
    x0[:, 0], x0[:, 1] = torch.cos(ang), torch.sin(ang)
    warm = (torch.rand(B, H, 1, generator=g) - 0.5) * 1.5
    return opt, x0.to(dev), warm.to(dev)


_SMALL = dict(num_particles=2, num_samples=126, num_elites=12, num_steps=3, exponent=1.0, alpha=0.1, init_std=0.6)   # NC = 129


@pytest.mark.parametrize("mode", [0, 1])
def test_batched_pendulum_equals_single_calls(dev, icem_update_mode, mode):
    from mbpo.optimizers import iCemParams
    icem_update_mode(mode)
    opt, x0, warm = _pendulum_case(dev, 5, 10, iCemParams(**_SMALL))
    new = _compare_with_single_calls(opt, x0, warm)
    assert torch.isfinite(new.best_reward).all()
    assert len(set(float(v) for v in new.best_reward)) == 5            # five distinct problems


def test_batched_pendulum_past_the_lds_threshold(dev, icem_update_mode):
    """H = 64, 240 elites: 4 (2 NC + NE + NE H U) = 65 KB > 60 KB, so both modes take the global-memory update kernel."""
    from mbpo.optimizers import iCemParams
    params = iCemParams(num_particles=2, num_samples=300, num_elites=240, num_steps=2, exponent=0.5, alpha=0.2, init_std=0.5)
    NC, NE, H = 300 + int(0.3 * 240), 240, 64
    assert 4 * (2 * NC + NE + NE * H) > 60 * 1024
    for mode in (-1, 1):
        icem_update_mode(mode)
        opt, x0, warm = _pendulum_case(dev, 3, H, params, seed=1)
        _compare_with_single_calls(opt, x0, warm)


@pytest.mark.parametrize("mode,noise", [("mean", False), ("ts1", True), ("ts1", False), ("tsinf", True)])
def test_batched_ensemble_equals_single_calls(dev, mode, noise):
    from mbpo.optimizers import iCemParams, iCemTO
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, QuadraticReward
    X, U, E, H, B = 4, 2, 5, 8, 3
    params = iCemParams(**_SMALL)
    assert (params.num_samples + 3) * params.num_particles % E != 0      # 'tsinf': env % E does not line up with the problems
    system = EnsembleSystem(EnsembleDynamics(X, U, n_members=E, device=dev),
                            QuadraticReward(X, U, target=[0.1, 0.0, 0.0, 0.0], q=[1.0, 2.0, 0.5, 0.1], r=[0.3] * U),
                            mode=mode, sample_noise=noise)
    opt = iCemTO(horizon=H, action_dim=U, opt_params=params, key=5)
    opt.set_system(system)
    g = torch.Generator().manual_seed(3)
    x0 = (torch.randn(B, X, generator=g) * 0.5).to(dev)
    warm = ((torch.rand(B, H, U, generator=g) - 0.5) * 1.5).to(dev)
    new = _compare_with_single_calls(opt, x0, warm)
    assert torch.isfinite(new.best_reward).all()


@pytest.mark.parametrize("optimism", [False, True])
def test_batched_cost_fn_with_pessimism_equals_single_calls(dev, optimism):
    from mbpo.optimizers import iCemParams

    def cost_fn(observation, action):
        return torch.clamp(-0.2 - action, min=0.0).sum() + 0.1 * observation[:, 2].abs().mean()

    params = iCemParams(**dict(_SMALL, lambda_constraint=50.0))
    opt, x0, warm = _pendulum_case(dev, 4, 10, params, seed=2, cost_fn=cost_fn, use_pessimism=True, use_optimism=optimism)
    _compare_with_single_calls(opt, x0, warm)


@pytest.mark.parametrize("mode", [0, 1])
def test_batched_nan_problem_is_isolated(dev, icem_update_mode, mode):
    from mbpo.optimizers import iCemParams
    icem_update_mode(mode)
    opt, x0, warm = _pendulum_case(dev, 4, 10, iCemParams(**_SMALL), seed=4)
    x0[1, 2] = float("nan")
    new = _compare_with_single_calls(opt, x0, warm)          # the NaN problem equals its own single call too
    assert torch.isnan(new.best_reward[1]) or torch.isinf(new.best_reward[1])
    assert torch.isfinite(new.best_reward[[0, 2, 3]]).all()
    assert torch.isfinite(new.best_sequence[[0, 2, 3]]).all()
    assert (new.best_sequence.abs() <= 1.0).all()             # whatever was taken is a candidate or the warm start: in [u_min, u_max]


@pytest.mark.parametrize("as_int", [0, 1])
def test_grouped_fill_equals_per_problem_fills(dev, as_int):
    from mbpo import _hip, ops
    lib = _hip.load()
    S, B, G, off = 5, 3, 77, 9
    seeds = [0x1234, (1 << 64) - 5, 42]
    sd = torch.tensor([s - (1 << 64) if s >= 1 << 63 else s for s in seeds], dtype=torch.int64, device=dev)
    out = torch.zeros(S * B * G, device=dev, dtype=torch.int32 if as_int else torch.float32)
    stream = _hip.STREAM_MEMBER if as_int else _hip.STREAM_MODEL_NOISE
    _hip.check(lib.mbpo_philox_fill_grouped(sd.data_ptr(), off, stream, S, B, G, as_int, 0, 7, out.data_ptr(), None),
               "mbpo_philox_fill_grouped")
    got = out.reshape(S, B, G)
    for b, s in enumerate(seeds):
        want = (ops.philox_randint(S * G, 0, 7, seed=s, offset=off, stream=stream) if as_int
                else ops.philox_normal(S * G, seed=s, offset=off, stream=stream)).reshape(S, G)
        assert _same(got[:, b], want)


@pytest.mark.timeout(900)
def test_batched_mpc_solves_pendulum(dev):
    """tests/test_icemopt.py batched: iCEMOptimizer(horizon=20, batch_size=8), default iCemParams, 200 MPC steps from the reset state.
    Every environment's return equals a single-problem MPC loop with that environment's key; the mean return clears -400."""
    from mbpo.optimizers import iCemParams
    from mbpo.optimizers.trajectory_optimizers.icem_optimizer import iCEMOptimizer
    from mbpo.systems import PendulumSystem
    B, steps = 8, 200
    system = PendulumSystem()
    state = system.reset()
    opt = iCEMOptimizer(horizon=20, opt_params=iCemParams(), system=system, key=1, batch_size=B)
    assert opt.can_act_in_batches
    ost = opt.init(2)
    keys0 = list(ost.key)
    x = state.x_next.reshape(1, -1).repeat(B, 1)
    totals = [0.0] * B
    for _ in range(steps):
        u, ost = opt.act(x, ost)
        assert u.shape == (B, 1)
        nxt = system.step(x=x, u=u, system_params=state.system_params)
        r = nxt.reward.reshape(-1).tolist()
        totals = [t + v for t, v in zip(totals, r)]
        x = nxt.x_next
    print("batched icem MPC returns:", [round(t, 2) for t in totals])
    single = iCEMOptimizer(horizon=20, opt_params=iCemParams(), system=system, key=1)
    s0 = single.init(2)
    for b in range(B):
        sst = s0.replace(key=keys0[b])
        xs, tot = state.x_next, 0.0
        for _ in range(steps):
            u, sst = single.act(xs, sst)
            nxt = system.step(x=xs, u=u.reshape(-1), system_params=state.system_params)
            xs, tot = nxt.x_next, tot + float(nxt.reward)
        assert tot == totals[b], f"env {b}: batched {totals[b]} vs single {tot}"
    mean = sum(totals) / B
    print("mean return:", mean)
    assert mean >= -400


def test_icem_optimizer_default_is_not_batched(dev):
    from mbpo.optimizers.trajectory_optimizers.icem_optimizer import iCEMOptimizer
    assert iCEMOptimizer(horizon=20).can_act_in_batches is False
    assert iCEMOptimizer(horizon=20, batch_size=4).can_act_in_batches is True
