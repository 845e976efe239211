"""GPU: SAC on mixed minibatches (SAC(real_ratio=0.05): MBPO's share of real transitions in every SGD minibatch) against
tests/real_ratio_ref.py:MixedCpuSacLoop on identical Philox streams, eagerly and through the captured hipGraph.

Configuration: that of tests/test_gpu_trainer_parity.py (copied, so that neither file depends on the other) — the "ensemble"
system, batch_size 256 x 4 updates per step — with real_ratio = 0.05, i.e. n_real = 12 real rows at the head of each minibatch,
from a 512-row true buffer whose discount column is 0 or 1.  Tolerances are that file's: rollout rows / batch rows 2e-4 on the
first step and 2e-3 later, parameters by relative L2 5e-4 and 5e-3; sampled indices and the real rows are exact (the arithmetic
behind the batch is unchanged, so a miss at these tolerances is a finding).
"""
import numpy as np
import pytest
import torch

import real_ratio_ref as rref
from oracle import replay as oreplay, sac as osac, systems as osys

pytestmark = pytest.mark.gpu

SAC_KW = dict(num_envs=64, batch_size=256, grad_updates_per_step=4, num_env_steps_between_updates=5, episode_length=5,
              normalize_observations=True, max_replay_size=1500, min_replay_size=64, discounting=0.95, lr_policy=3e-4,
              lr_q=3e-4, lr_alpha=3e-4, wd_q=1e-4)
REAL_RATIO, N_REAL, TRUE_ROWS = 0.05, 12, 512
X, U, E = 4, 1, 5


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu().reshape(-1), torch.as_tensor(b).double().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _true_rows():
    g = torch.Generator().manual_seed(0)
    data = torch.randn(TRUE_ROWS, 2 * X + U + 2, generator=g)
    data[:, X + U + 1] = (torch.rand(TRUE_ROWS, generator=g) < 0.8).float()      # discount: 0 or 1
    return data


def _true_buffer(dev, fill=True):
    from mbpo.replay import UniformSamplingQueue
    from mbpo.types import Transition
    dummy = Transition(observation=torch.zeros(X), action=torch.zeros(U), reward=torch.zeros(1), discount=torch.zeros(1),
                       next_observation=torch.zeros(X))
    tb = UniformSamplingQueue(TRUE_ROWS, dummy, 1, device=dev)
    tbs = tb.init(0)
    return tb, (tb.insert_rows(tbs, _true_rows().to(dev)) if fill else tbs)


def _make_system(dev):
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, QuadraticReward
    dyn = EnsembleDynamics(X, U, n_members=E, device=dev)
    rew = QuadraticReward(X, U, target=[0.1, 0, 0, 0], q=[1, 2, 0.5, 0.1], r=[0.3])
    system = EnsembleSystem(dyn, rew)
    sp = system.init_params(1)
    sp.dynamics_params.params.mul_(0.5)
    rp = sp.reward_params
    osystem = osys.EnsembleSystem(sp.dynamics_params.params.cpu().clone(), dyn.dims, E, X, U,
                                  reward_fn=lambda a, b: osys.quadratic_reward(a, b, torch.tensor(rp.target), torch.tensor(rp.q),
                                                                               torch.tensor(rp.r)))
    return system, sp, osystem


def _sac_setup(dev, use_graph, n_steps=4, **extra):
    from mbpo.optimizers.policy_optimizers.sac.sac import SAC
    from mbpo.systems.brax_wrapper import BraxWrapper
    system, sp, osystem = _make_system(dev)
    tb, tbs = _true_buffer(dev)
    env = BraxWrapper(system, sp, tbs, tb)
    N, S = SAC_KW["num_envs"], SAC_KW["num_env_steps_between_updates"]
    tr = SAC(environment=env, num_timesteps=64 + N * S * n_steps, use_graph=use_graph, **SAC_KW, **extra)
    assert tr.num_training_steps_per_epoch == n_steps and tr.num_prefill_actor_steps == 1
    return tr, tr.init_training_state(7), tr.reset_envs(env, 11, N), tr.replay_buffer.init(13), osystem


def _oracle(tr, es, osystem):
    cfg = osac.SacConfig(X, U, tr.policy_dims, tr.q_dims, discounting=SAC_KW["discounting"], lr_policy=3e-4, lr_q=3e-4, lr_alpha=3e-4,
                         wd_q=1e-4)
    rq = oreplay.UniformSamplingQueue(TRUE_ROWS, 2 * X + U + 2, 1)
    rqs = rq.insert(rq.init(), _true_rows().numpy())
    return rref.MixedCpuSacLoop(cfg, osystem, SAC_KW["num_envs"], SAC_KW["num_env_steps_between_updates"], SAC_KW["episode_length"],
                                SAC_KW["batch_size"], SAC_KW["grad_updates_per_step"], SAC_KW["max_replay_size"], True,
                                init_params=tr.updater.params.cpu().clone(), init_obs=es.obs.cpu().clone(), n_real=N_REAL,
                                real_queue=rq, real_qstate=rqs)


def test_mixed_training_step_matches_cpu_oracle(dev):
    """Three eager training steps of SAC(real_ratio=0.05) against MixedCpuSacLoop (prefill included)."""
    from mbpo import ops
    from mbpo.optimizers.policy_optimizers.sac import sac as sac_mod
    from mbpo.utils import keys as K
    tr, ts, es, bs, osystem = _sac_setup(dev, use_graph=False, real_ratio=REAL_RATIO)
    assert tr.n_real == N_REAL and sac_mod.SITE_SAMPLE_REAL == rref.SAC_SITE_SAMPLE_REAL == 3
    loop = _oracle(tr, es, osystem)
    ts, es, bs, _ = tr.prefill_replay_buffer(ts, es, bs, 17)
    loop.rekey(K.split(17)[0])
    loop.prefill_step()
    tr.rekey(19)
    loop.rekey(19)
    B, G = SAC_KW["batch_size"], SAC_KW["grad_updates_per_step"]
    D, RD = 2 * X + U + 3, 2 * X + U + 2
    is_real = (np.arange(B * G) % B) < N_REAL
    real = tr.env.sample_buffer_state
    true_rows = _true_rows().numpy()
    for step in range(3):
        ts, es, bs = tr.training_step(ts, es, bs)
        loop.training_step()
        torch.cuda.synchronize()
        tol = 2e-4 if step == 0 else 2e-3
        torch.testing.assert_close(tr._rollout_rows.cpu(), loop.last_rows, atol=tol, rtol=tol)
        st = bs.state.cpu().tolist()
        assert st[0] == int(loop.qstate["insert_position"]) == bs.insert_position
        assert st[1] == int(loop.qstate["sample_position"]) == bs.sample_position
        # the sampled indices, exactly: the launch of this step issued again with its key spelled out on the host (the device step
        # counter has moved on) reproduces _batch_rows bit for bit, and its indices are the oracle's
        idx = torch.empty(B * G, dtype=torch.int32, device=dev)
        again = ops.replay_sample_mixed(bs.data, bs.state, real.data, real.state, B * G, B, N_REAL, seed=19,
                                        offset=(sac_mod.SITE_SAMPLE << 32) + step, real_offset=(sac_mod.SITE_SAMPLE_REAL << 32) + step,
                                        idx_out=idx)
        assert torch.equal(again, tr._batch_rows)
        assert np.array_equal(idx.cpu().numpy(), loop.last_idx)
        got = tr._batch_rows.cpu().numpy()
        # real rows: bit-equal to the true buffer's rows, truncation column 0; model rows: the oracle's rows at the rollout tolerance
        assert np.array_equal(got[is_real, :RD], true_rows[loop.last_idx[is_real]]) and np.all(got[is_real, RD:] == 0.0)
        assert np.array_equal(got[is_real], loop.last_batch[is_real])
        assert set(np.unique(got[is_real, X + U + 1]).tolist()) <= {0.0, 1.0}
        torch.testing.assert_close(torch.from_numpy(got), torch.from_numpy(loop.last_batch), atol=tol, rtol=tol)
        # the normaliser is fed by the model rollouts only
        sv = tr._stats_vec.cpu().numpy()
        assert sv[0] == loop.stats[0] == 64 * 5 * (step + 2)
        np.testing.assert_allclose(sv[1:], loop.stats[1:], rtol=2e-5 if step == 0 else 2e-4, atol=2e-5)
        lim = 5e-4 if step == 0 else 5e-3
        P, Q2 = tr.updater.P, 2 * tr.updater.Q
        assert _rel(tr.updater.params[:P], loop.state.params[:P]) < lim
        assert _rel(tr.updater.params[P:P + Q2], loop.state.params[P:P + Q2]) < lim
        assert _rel(tr.updater.target_q, loop.state.target_q) < lim
        assert abs(float(tr.updater.params[-1]) - float(loop.state.params[-1])) < 1e-5 * (step + 1)
        assert float(tr.updater.step_count) == loop.state.count == 4 * (step + 1)
        torch.testing.assert_close(es.obs.cpu(), loop.env.obs, atol=tol, rtol=tol)
    # the true buffer was only read
    assert torch.equal(real.data.cpu(), _true_rows()) and real.state.cpu().tolist()[:3] == [TRUE_ROWS, 0, 0]


def _epoch(dev, use_graph, **extra):
    tr, ts, es, bs, osystem = _sac_setup(dev, use_graph=use_graph, **extra)
    ts, es, bs, _ = tr.prefill_replay_buffer(ts, es, bs, 17)
    ts, es, bs, metrics = tr.training_epoch(ts, es, bs, 19)
    torch.cuda.synchronize()
    assert (tr._graph is not None) == use_graph
    st = bs.state.cpu().tolist()
    assert st[0] == bs.insert_position and st[1] == bs.sample_position and st[2] == bs.head
    u = tr.updater
    out = dict(params=u.params.cpu().clone(), tq=u.target_q.cpu().clone(), m=u.adam_m.cpu().clone(), v=u.adam_v.cpu().clone(),
               obs=es.obs.cpu().clone(), stats=tr._stats_vec.cpu().clone(), rows=tr._rollout_rows.cpu().clone(),
               batch=tr._batch_rows.cpu().clone(), data=bs.data.cpu().clone(), state=st, count=float(u.step_count), metrics=metrics,
               rng=tr._rng.cpu().tolist(), env_steps=ts.env_steps)
    tr.close()
    return out


def _assert_same(a, b, what):
    for k in ("params", "tq", "m", "v", "obs", "stats", "rows", "batch", "data"):
        assert torch.equal(a[k], b[k]), f"{what}: differs in {k}"
    for k in ("state", "count", "rng", "env_steps", "metrics"):
        assert a[k] == b[k], f"{what}: differs in {k}"


def test_mixed_graph_epoch_is_bit_identical_to_eager(dev):
    """A 4-step epoch through the captured hipGraph == the same epoch issued eagerly, bit for bit: the mixed sample reads its
    positions (both buffers') and RNG words from device memory like every other launch of the step."""
    eager = _epoch(dev, False, real_ratio=REAL_RATIO)
    graph = _epoch(dev, True, real_ratio=REAL_RATIO)
    _assert_same(eager, graph, "graph replay vs eager")
    assert graph["count"] == 16 and graph["rng"][1] == 4
    pos = torch.arange(graph["batch"].shape[0]) % SAC_KW["batch_size"]
    real = graph["batch"][pos < N_REAL]
    assert bool((real[:, -1] == 0).all()) and bool(((real[:, X + U + 1] == 0) | (real[:, X + U + 1] == 1)).all())
    # and the mixing is live: the same epoch without real rows ends elsewhere
    assert not torch.equal(graph["params"], _epoch(dev, True)["params"])


def test_real_ratio_zero_is_the_trainer_without_the_argument(dev):
    """real_ratio=0.0 issues exactly the plain sample launch: one graph epoch is bit-identical to a trainer built without it."""
    _assert_same(_epoch(dev, True), _epoch(dev, True, real_ratio=0.0), "real_ratio=0.0 vs default")


def test_construction_checks(dev):
    from mbpo.optimizers.policy_optimizers.sac.sac import SAC
    from mbpo.replay import UniformSamplingQueue
    from mbpo.systems.brax_wrapper import BraxWrapper
    from mbpo.types import Transition
    system, sp, _ = _make_system(dev)
    tb, tbs = _true_buffer(dev)
    env = BraxWrapper(system, sp, tbs, tb)
    for r in (-0.1, 1.01):
        with pytest.raises(ValueError, match="real_ratio"):
            SAC(environment=env, num_timesteps=1000, real_ratio=r, **SAC_KW)
    assert SAC(environment=env, num_timesteps=1000, real_ratio=1.0, **SAC_KW).n_real == 256
    assert SAC(environment=env, num_timesteps=1000, real_ratio=0.003, **SAC_KW).n_real == 0
    # a true buffer of another observation size cannot be mixed in (checked at construction, whatever real_ratio is)
    z = lambda k: torch.zeros(k, device=dev)
    other = UniformSamplingQueue(8, Transition(z(X + 1), z(U), z(1), z(1), z(X + 1)), 1, device=dev)
    with pytest.raises(ValueError):
        SAC(environment=BraxWrapper(system, sp, other.init(0), other), num_timesteps=1000, **SAC_KW)
    # an empty true buffer: construction works (BraxOptimizer.set_system builds its dummy trainer on one), run_training refuses
    tb0, tbs0 = _true_buffer(dev, fill=False)
    tr = SAC(environment=BraxWrapper(system, sp, tbs0, tb0), num_timesteps=1000, real_ratio=REAL_RATIO, **SAC_KW)
    with pytest.raises(ValueError, match="true buffer is empty"):
        tr.run_training(key=3)


def test_sac_optimizer_trains_with_real_ratio(dev):
    from mbpo.optimizers import SACOptimizer
    system, sp, _ = _make_system(dev)
    tb, tbs = _true_buffer(dev)
    N, S = SAC_KW["num_envs"], SAC_KW["num_env_steps_between_updates"]
    opt = SACOptimizer(system=system, true_buffer=tb, num_timesteps=64 + N * S * 3, num_evals=1, num_eval_envs=8, real_ratio=REAL_RATIO,
                       **SAC_KW)
    assert opt.dummy_trainer.n_real == N_REAL                              # built on the dummy (empty) true buffer
    out = opt.train(opt.init(key=5, true_buffer_state=tbs))
    norm, pol = out.optimizer_state.policy_params
    assert bool(torch.isfinite(pol).all()) and bool(torch.isfinite(norm.vec).all())
    assert all(np.isfinite(v) for v in out.summary[-1].values())
    with pytest.raises(ValueError, match="true buffer is empty"):
        opt.train(opt.init(key=5))                                         # the dummy true buffer
