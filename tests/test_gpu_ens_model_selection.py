"""GPU: ensemble model selection — mbpo_ens_eval against the restatement (tests/ens_select_ref.py) in fp32 and fp64 and against the
training kernel's own loss, mbpo_ens_keep_best / mbpo_ens_pick_elites bit for bit on poisoned buffers, EnsembleDynamics.fit with a
holdout (defaults unchanged, deterministic stopping, a real fit) and the elites through every rollout consumer.

Tolerance of the metrics: the project's loss tolerance (tests/test_gpu_ensemble_train.py), rtol 2e-5 + atol 2e-5, for both rows and
against both references."""
import math

import numpy as np
import pytest
import torch

from oracle import nets as onets

import ens_select_ref as sref

pytestmark = pytest.mark.gpu

TOL = dict(rtol=2e-5, atol=2e-5)


def _case_data(X, U, E, hidden, reward, seed):
    """Parameters and rows as in test_ens_nll_grads_parity; with `reward` a [2x+2] net and a reward column at X + U."""
    g = torch.Generator().manual_seed(seed)
    dims = [X + U, *hidden, 2 * X + (2 if reward else 0)]
    P = onets.n_params(dims)
    params = torch.cat([onets.init_mlp_flat(dims, g) + 0.02 * torch.randn(P, generator=g) for _ in range(E)])
    R, D = 500, 2 * X + U + 2
    rows = torch.randn(R, D, generator=g)
    rows[:, X + U + 2:] = rows[:, :X] + 0.1 * torch.randn(R, X, generator=g)
    return g, dims, params, rows, R


EVAL_CASES = [
    (4, 1, 5, 256, (64, 64, 64), False),            # baseline fused shape
    (3, 1, 3, 70, (64, 64, 64), False),             # ragged last tile
    (17, 6, 2, 48, (64, 64, 64), False),            # generic output layer
    (4, 1, 4, 2400, (64,), False),                  # more tiles than slots
    (3, 1, 7, 100, (200, 200, 200, 200), False),    # stored at width 256 -> layered
    (3, 1, 2, 40, (96, 32), False),                 # unequal widths -> layered
    (4, 1, 3, 70, (64, 64, 64), True),              # reward head, fused
    (4, 1, 3, 70, (96, 32), True),                  # reward head, layered
]


@pytest.mark.parametrize("X,U,E,n,hidden,reward", EVAL_CASES)
def test_ens_eval_parity(dev, X, U, E, n, hidden, reward):
    from mbpo import ops
    g, dims, params, rows, R = _case_data(X, U, E, hidden, reward, seed=len(hidden) + n)
    if hidden == (200, 200, 200, 200):              # as EnsembleDynamics stores it: zero-padded to the kernel width 256
        kdims = ops.padded_dims(dims, 256)
        kparams = ops.embed_mlp_params(params, dims, 256, E)
    else:
        kdims, kparams = dims, params
    idx = torch.randint(0, R, (n,), generator=g)            # unsorted, with repeats (a small draw may have none: three are forced)
    idx[-3:] = idx[:3]
    assert idx.unique().numel() < n and not bool((idx[1:] >= idx[:-1]).all())
    roff = X + U if reward else None
    ref32 = sref.eval_metrics(params, dims, E, rows, idx, X, U, True, 1e-3, roff)
    ref64 = sref.eval_metrics(params.double(), dims, E, rows.double(), idx, X, U, True, 1e-3, roff)
    op = ops.EnsembleEval(x_dim=X, u_dim=U, spec=ops.MlpSpec(kdims, "swish", E), device=dev)
    got = op(kparams.to(dev), rows.to(dev), idx.to(torch.int32).to(dev), reward_off=roff).cpu()
    assert got.shape == (2, E)
    err = lambda a, b: float(((a.double() - b.double()).abs() / (2e-5 + 2e-5 * b.double().abs())).max())
    print(f"ens_eval {X, U, E, n, hidden, reward}: kernel vs fp64 {err(got, ref64):.3f}, kernel vs fp32 {err(got, ref32):.3f}, "
          f"fp32 restatement vs fp64 {err(ref32, ref64):.3f} (units of the tolerance)")
    np.testing.assert_allclose(got.numpy(), ref32.numpy(), **TOL)
    np.testing.assert_allclose(got.double().numpy(), ref64.numpy(), **TOL)
    assert bool((got[1] >= 0).all())


@pytest.mark.parametrize("hidden", [(64, 64, 64), (96, 32)])       # fused with a ragged last tile; layered
def test_ens_eval_unfitted_reward_head(dev, hidden):
    """reward_off=None on a [x+u] -> [2x+2] ensemble: the reward head's outputs enter neither metric."""
    from mbpo import ops
    X, U, E, n = 4, 1, 3, 70
    g, dims, params, rows, R = _case_data(X, U, E, hidden, True, seed=len(hidden) + n)
    idx = torch.randint(0, R, (n,), generator=g)
    ref32 = sref.eval_metrics(params, dims, E, rows, idx, X, U, True, 1e-3, None)
    ref64 = sref.eval_metrics(params.double(), dims, E, rows.double(), idx, X, U, True, 1e-3, None)
    op = ops.EnsembleEval(x_dim=X, u_dim=U, spec=ops.MlpSpec(dims, "swish", E), device=dev)
    got = op(params.to(dev), rows.to(dev), idx.to(torch.int32).to(dev), reward_off=None).cpu()
    err = lambda a, b: float(((a.double() - b.double()).abs() / (2e-5 + 2e-5 * b.double().abs())).max())
    print(f"ens_eval, unfitted reward head {hidden}: kernel vs fp64 {err(got, ref64):.3f}, kernel vs fp32 {err(got, ref32):.3f}, "
          f"fp32 restatement vs fp64 {err(ref32, ref64):.3f} (units of the tolerance)")
    np.testing.assert_allclose(got.numpy(), ref32.numpy(), **TOL)
    np.testing.assert_allclose(got.double().numpy(), ref64.numpy(), **TOL)


@pytest.mark.parametrize("X,U,E,B,hidden,reward", [
    (4, 1, 5, 256, (64, 64, 64), False),            # fused
    (4, 1, 3, 70, (64, 64, 64), True),              # fused, reward head
    (3, 1, 3, 100, (96, 32), False),                # layered
])
def test_ens_eval_equals_the_training_loss(dev, X, U, E, B, hidden, reward):
    """With every member's minibatch = the shared index list, the NLL row is mbpo_ens_nll_grads's loss."""
    from mbpo import ops
    g, dims, params, rows, R = _case_data(X, U, E, hidden, reward, seed=5)
    idx = torch.randint(0, R, (B,), generator=g).to(torch.int32).to(dev)
    spec = ops.MlpSpec(dims, "swish", E)
    roff = X + U if reward else None
    train = ops.EnsembleNllGrad(x_dim=X, u_dim=U, spec=spec, batch=B, device=dev)
    train(params.to(dev), rows.to(dev), idx[None].expand(E, B).contiguous(), reward_off=roff)
    got = ops.EnsembleEval(x_dim=X, u_dim=U, spec=spec, device=dev)(params.to(dev), rows.to(dev), idx, reward_off=roff)
    np.testing.assert_allclose(got[0].cpu().numpy(), train.metrics.cpu().numpy(), **TOL)


# ------------------------------------------------------------------------------------------------ snapshot and elites
POISON = 12345.0


def _poisoned(values: torch.Tensor, dev, pad=37):
    """`values` inside a larger allocation filled with POISON; returns (whole buffer, view of the values)."""
    buf = torch.full((values.numel() + 2 * pad,), POISON, device=dev)
    view = buf[pad:pad + values.numel()]
    view.copy_(values)
    return buf, view


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def test_keep_best(dev):
    from mbpo import ops
    E, P = 4, 1027                                  # members 1027 floats apart: not a multiple of 4
    g = torch.Generator().manual_seed(0)
    params_h = torch.randn(E * P, generator=g)
    params_h[5] = float("nan")                      # a bit copy carries NaN payloads too
    best_h = torch.randn(E * P, generator=g)
    pbuf, params = _poisoned(params_h, dev)
    bbuf, best = _poisoned(best_h, dev)
    best_score = torch.tensor([float("inf"), 1.0, 1.0, 1.0], device=dev)
    score = torch.tensor([0.7, 0.995, float("nan"), 0.5], device=dev)
    state = torch.zeros(2, device=dev, dtype=torch.int32)
    pbuf0 = pbuf.clone()
    ops.ens_keep_best(params, best, E, score, best_score, 0.01, state)
    torch.cuda.synchronize()
    want_p, want_s, want_st = sref.keep_best(params_h.reshape(E, P), best_h.reshape(E, P), score.cpu(), torch.tensor([float("inf"), 1, 1, 1]),
                                             0.01, [0, 0])
    got = best.cpu().reshape(E, P)
    for e in (0, 3):
        assert torch.equal(_bits(got[e]), _bits(params_h.reshape(E, P)[e])), e
    for e in (1, 2):
        assert torch.equal(_bits(got[e]), _bits(best_h.reshape(E, P)[e])), e
    assert torch.equal(_bits(got), _bits(want_p))
    assert torch.equal(_bits(best_score), _bits(torch.tensor([0.7, 1.0, 1.0, 0.5]))) and torch.equal(best_score.cpu(), want_s)
    assert state.tolist() == [0, 1] == want_st
    assert torch.equal(_bits(pbuf), _bits(pbuf0))                                      # the source and its surroundings
    assert bool((bbuf[:37] == POISON).all()) and bool((bbuf[-37:] == POISON).all())    # the bytes around the destination
    # a second call with score = best_score: nothing improves, nothing is copied
    params.add_(1.0)
    snapshot = bbuf.clone()
    ops.ens_keep_best(params, best, E, best_score.clone(), best_score, 0.01, state)
    torch.cuda.synchronize()
    assert state.tolist() == [1, 2]
    assert torch.equal(_bits(bbuf), _bits(snapshot))
    assert torch.equal(_bits(best_score), _bits(torch.tensor([0.7, 1.0, 1.0, 0.5])))


def test_pick_elites(dev):
    from mbpo import ops
    E, P = 7, 1027
    nan, inf = float("nan"), float("inf")
    g = torch.Generator().manual_seed(1)
    params_h = torch.randn(E * P, generator=g)
    pbuf, params = _poisoned(params_h, dev, pad=3)            # the members start 12 bytes into the allocation
    score_h = torch.tensor([0.3, nan, 0.1, 0.3, inf, 0.1, 0.2])
    score = score_h.to(dev)
    order = sref.ranking(score_h)
    assert order == [2, 5, 6, 0, 3, 4, 1]
    for n_elites in (5, 7, 1):
        ebuf, eparams = _poisoned(torch.zeros(n_elites * P), dev)
        idx = torch.full((n_elites + 2,), -7, device=dev, dtype=torch.int32)
        ops.ens_pick_elites(params, E, score, n_elites, elite_idx=idx[1:1 + n_elites], elite_params=eparams)
        torch.cuda.synchronize()
        assert idx.tolist() == [-7, *order[:n_elites], -7]
        want = params_h.reshape(E, P)[order[:n_elites]]
        assert torch.equal(_bits(eparams.cpu().reshape(n_elites, P)), _bits(want))
        assert bool((ebuf[:37] == POISON).all()) and bool((ebuf[-37:] == POISON).all())
    assert torch.equal(_bits(pbuf[3:-3]), _bits(params_h))
    # allocating form
    idx, ep = ops.ens_pick_elites(params, E, score, 5)
    assert idx.tolist() == [2, 5, 6, 0, 3] and ep.numel() == 5 * P


# ------------------------------------------------------------------------------------------------ EnsembleDynamics.fit
@pytest.fixture(scope="module")
def pendulum_rows(dev):
    """1500 true Pendulum transitions (obs, action, reward, discount, next_obs), as test_ensemble_fit_learns_pendulum_dynamics builds them."""
    from mbpo.systems import PendulumSystem
    system = PendulumSystem()
    g = torch.Generator().manual_seed(0)
    n = 1500
    th = (torch.rand(n, generator=g) * 2 - 1) * math.pi
    x = torch.stack([torch.cos(th), torch.sin(th), (torch.rand(n, generator=g) * 2 - 1) * 6], 1).to(dev)
    u = (torch.rand(n, 1, generator=g) * 2 - 1).to(dev)
    nxt = system.step(x, u, system.reset().system_params)
    return torch.cat([x, u, nxt.reward[:, None], torch.ones(n, 1, device=dev), nxt.x_next], 1).contiguous()


def test_fit_defaults_are_the_parent_fit(dev, pendulum_rows):
    """No new keyword: parameters and losses bit-identical to the fixed-step loop `fit` was before model selection."""
    from mbpo import ops
    from mbpo.systems import EnsembleDynamics
    from mbpo.utils import keys as K
    rows, E, B, steps = pendulum_rows[:600], 5, 64, 5
    dyn = EnsembleDynamics(3, 1, n_members=E, device=dev)
    p0 = dyn.init_params(3)
    mine = p0.replace(params=p0.params.clone())
    got, losses = dyn.fit(mine, rows, num_steps=steps, batch_size=B, learning_rate=3e-3, key=7)
    assert got is mine and got.elite_params is None and got.holdout is None
    # the parent's fit body
    params = p0.params.clone()
    R = rows.shape[0]
    nll = ops.EnsembleNllGrad(x_dim=3, u_dim=1, spec=dyn.spec, batch=B, device=dev, predict_delta=True, min_std=1e-3)
    opt = ops.AdamW(E * dyn.spec.n_params, dev, 3e-3, 0.0, apply_if_finite=True)
    state = torch.tensor([R, 0, 0, R], device=dev, dtype=torch.int32)
    idx = torch.zeros(E * B, device=dev, dtype=torch.int32)
    scratch = torch.zeros(E * B, 1, device=dev, dtype=torch.float32)
    want = torch.zeros(steps, E, device=dev)
    col0 = rows[:, :1].contiguous()
    for it in range(steps):
        ops.replay_sample(col0, state, E * B, seed=K.PRNGKey(7), offset=it, out=scratch, idx_out=idx)
        g = nll(params, rows, idx.view(E, B), next_obs_off=None, reward_off=None)
        opt.step(params, g)
        want[it].copy_(nll.metrics)
    torch.cuda.synchronize()
    assert torch.equal(_bits(got.params), _bits(params)) and torch.equal(_bits(losses), _bits(want))
    assert not torch.equal(params, p0.params)


def test_fit_stopping_logic_is_deterministic(dev, pendulum_rows):
    """Learning rate 0: the first evaluation improves on +inf, the next three do not, and 3 > max_evals_since_improvement = 2."""
    from mbpo.systems import EnsembleDynamics
    from mbpo.utils import keys as K
    rows = pendulum_rows[:600]
    dyn = EnsembleDynamics(3, 1, n_members=4, device=dev)
    p = dyn.init_params(1)
    p0 = p.params.clone()
    got, losses = dyn.fit(p, rows, num_steps=1000, batch_size=96, learning_rate=0.0, weight_decay=0.0, key=11, holdout_ratio=0.2,
                          max_evals_since_improvement=2)
    eval_every = math.ceil(480 / 96)
    assert eval_every == 5
    assert losses.shape == ((1 + 3) * eval_every, 4)
    assert torch.equal(_bits(got.params), _bits(p0))
    hold, train = sref.split(K.PRNGKey(11), 600, 0.2)
    assert hold.numel() == 120 and not set(hold.tolist()) & set(train.tolist())
    assert len(set(hold.tolist()) | set(train.tolist())) == 600
    want = dyn.evaluate(got, rows, hold.to(torch.int32).to(dev))
    assert got.holdout.shape == (2, 4) and torch.equal(_bits(got.holdout), _bits(want))
    # and the holdout the fit used is the restated split's: the restatement's metrics on those rows
    ref = sref.eval_metrics(p0.cpu(), dyn.dims, 4, rows.cpu(), hold, 3, 1)
    np.testing.assert_allclose(got.holdout.cpu().numpy(), ref.numpy(), rtol=2e-5, atol=2e-5)
    with pytest.raises(ValueError):
        dyn.fit(p, rows, num_steps=1, holdout_ratio=0.001)            # an empty holdout


def test_real_fit_with_elites(dev, pendulum_rows):
    from mbpo.systems import EnsembleDynamics
    from mbpo.utils import keys as K
    rows, E = pendulum_rows, 5
    dyn = EnsembleDynamics(3, 1, n_members=E, device=dev)
    p = dyn.init_params(2)
    storage = p.params
    got, losses = dyn.fit(p, rows, num_steps=400, batch_size=256, learning_rate=3e-3, key=5, holdout_ratio=0.2, n_elites=3)
    assert got.params is storage and got.params.data_ptr() == storage.data_ptr()
    assert 0 < losses.shape[0] <= 400 and losses.shape[1] == E
    hold, _ = sref.split(K.PRNGKey(5), 1500, 0.2)
    hidx = hold.to(torch.int32).to(dev)
    again = dyn.evaluate(got, rows, hidx)
    assert torch.equal(_bits(got.holdout[1]), _bits(again[1]))          # the restored parameters are the snapshots that were scored
    mse = got.holdout[1].cpu()
    elites = got.elite_idx.tolist()
    assert len(set(elites)) == 3 and elites == sref.ranking(mse)[:3]
    rest = [e for e in range(E) if e not in elites]
    assert float(mse[elites].max()) <= float(mse[rest].min())
    P = dyn.spec.n_params
    assert torch.equal(_bits(got.elite_params.reshape(3, P)), _bits(got.params.reshape(E, P)[got.elite_idx.long()]))
    # the ensemble mean beats predicting "no change" on the holdout
    h = rows[hidx.long()]
    y = dyn.member_outputs(h[:, :3], h[:, 3:4], got)
    assert y.shape[0] == E                                               # all members, also with elites selected
    pred = h[:, :3] + y[..., :3].mean(0)
    err = float(((pred - h[:, 6:9]) ** 2).sum(1).mean())
    base = float(((h[:, :3] - h[:, 6:9]) ** 2).sum(1).mean())
    assert err < base, (err, base)
    with pytest.raises(ValueError):
        dyn.fit(p, rows, num_steps=1, n_elites=3)                         # elites need a holdout


# ------------------------------------------------------------------------------------------------ elites in every consumer
ELITES = [3, 0, 4]


def _elite_pair(dev, mode, sample_noise=False, learned=False, X=4, U=1, E=5):
    """(system over 5 members with elites [3, 0, 4] selected, its params, a 3-member system of members 3, 0, 4, its params)."""
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, LearnedReward, QuadraticReward
    def make(n):
        dyn = EnsembleDynamics(X, U, n_members=n, device=dev, learn_reward=learned)
        return dyn, EnsembleSystem(dyn, LearnedReward(dyn) if learned else QuadraticReward(X, U), mode=mode, sample_noise=sample_noise)
    dyn5, sys5 = make(E)
    dyn3, sys3 = make(len(ELITES))
    sp5 = sys5.init_params(4)
    g = torch.Generator().manual_seed(2)
    sp5.dynamics_params.params.add_(0.05 * torch.randn(sp5.dynamics_params.params.numel(), generator=g).to(dev))
    score = torch.tensor([1.0, 9.0, 9.0, 0.0, 2.0])
    dp5 = dyn5.select_elites(sp5.dynamics_params, score, 3)
    assert dp5.elite_idx.tolist() == ELITES
    P = dyn5.spec.n_params
    dp3 = dyn3.from_logical_params(dyn5.logical_params(sp5.dynamics_params).reshape(E, -1)[ELITES].reshape(-1))
    assert torch.equal(_bits(dp3.params), _bits(sp5.dynamics_params.params.reshape(E, P)[ELITES].reshape(-1)))
    rp5, rp3 = (dp5, dp3) if learned else (sp5.reward_params, sp5.reward_params)
    sp3 = sp5.replace(dynamics_params=dp3, reward_params=rp3)
    return sys5, sp5.replace(dynamics_params=dp5, reward_params=rp5), sys3, sp3, dyn5, dyn3


def _rollout(dev, system, sp, seed, N=70, S=3):
    from mbpo import ops
    X, U = system.x_dim, system.u_dim
    g = torch.Generator().manual_seed(seed)
    pdims = [X, 64, 64, 2 * U]
    ppar = onets.init_mlp_flat(pdims, g) + 0.02 * torch.randn(onets.n_params(pdims), generator=g)
    obs = torch.randn(N, X, generator=g)
    return ops.model_rollout(policy_params=ppar.to(dev), policy_spec=ops.MlpSpec(pdims, "swish", 1), x_dim=X, u_dim=U, obs=obs.to(dev),
                             first_obs=obs.to(dev), steps=torch.zeros(N, device=dev), done=torch.zeros(N, device=dev), n_steps=S,
                             episode_length=S, seed=seed, **system.rollout_spec(sp, dev))


def test_elites_step_rollouts_and_next_state(dev):
    N = 70
    g = torch.Generator().manual_seed(8)
    x, u = torch.randn(N, 4, generator=g).to(dev), (torch.rand(N, 1, generator=g) * 2 - 1).to(dev)
    sys5, sp5, sys3, sp3, dyn5, dyn3 = _elite_pair(dev, "mean")
    a, b = sys5.step(x, u, sp5), sys3.step(x, u, sp3)
    assert torch.equal(_bits(a.x_next), _bits(b.x_next)) and torch.equal(_bits(a.reward), _bits(b.reward))
    full = sys5.step(x, u, sp5.replace(dynamics_params=sp5.dynamics_params.replace(elite_idx=None, elite_params=None)))
    assert not torch.equal(full.x_next, a.x_next)                          # the five-member mean is another prediction
    da, _ = dyn5.next_state(x, u, sp5.dynamics_params)
    db, _ = dyn3.next_state(x, u, sp3.dynamics_params)
    assert torch.equal(_bits(da.mean()), _bits(db.mean())) and torch.equal(_bits(da.stddev()), _bits(db.stddev()))
    assert dyn5.member_outputs(x, u, sp5.dynamics_params).shape[0] == 5
    for mode in ("ts1", "tsinf"):
        sys5, sp5, sys3, sp3, _, _ = _elite_pair(dev, mode, sample_noise=True)
        ra, rb = _rollout(dev, sys5, sp5, seed=21), _rollout(dev, sys3, sp3, seed=21)
        assert torch.equal(_bits(ra), _bits(rb)), mode
    sys5, sp5, sys3, sp3, dyn5, dyn3 = _elite_pair(dev, "ts1", learned=True)
    ra, rb = _rollout(dev, sys5, sp5, seed=22), _rollout(dev, sys3, sp3, seed=22)
    assert torch.equal(_bits(ra), _bits(rb)) and float(ra[:, 5].abs().max()) > 0
    ra, rb = dyn5.reward(x, u, sp5.dynamics_params), dyn3.reward(x, u, sp3.dynamics_params)
    assert torch.equal(_bits(ra.mean()), _bits(rb.mean()))


def test_elites_icem(dev):
    from mbpo.optimizers import iCemParams, iCemTO
    sys5, sp5, sys3, sp3, _, _ = _elite_pair(dev, "ts1")
    x0 = (torch.randn(4, generator=torch.Generator().manual_seed(3)) * 0.5).to(dev)
    out = []
    for system, sp in ((sys5, sp5), (sys3, sp3)):
        opt = iCemTO(horizon=6, action_dim=1, opt_params=iCemParams(num_particles=3, num_samples=40, num_elites=6, num_steps=2), key=5)
        opt.set_system(system)
        out.append(opt.optimize(x0, opt.init(7).replace(system_params=sp)))
    assert torch.equal(_bits(out[0].best_sequence), _bits(out[1].best_sequence))
    assert torch.equal(_bits(out[0].best_reward), _bits(out[1].best_reward))


def test_elites_bptt_actor_gradients(dev):
    from mbpo import ops
    from test_gpu_bptt import _setup
    X, U, H, n = 4, 1, 4, 32
    sys5, sp5, sys3, sp3, _, _ = _elite_pair(dev, "tsinf", sample_noise=True)
    cfg, ap, cp, x0, _, s_mean, s_std, r_ms, _, _ = _setup(X, U, H, n, "ensemble", 3, 4)
    kw = dict(x_dim=X, u_dim=U, horizon=H, actor_dims=cfg.actor_dims, critic_dims=cfg.critic_dims, n=n, device=dev,
              init_stddev=cfg.init_stddev, discount=cfg.discount, lambda_=cfg.lambda_, ent_coef=cfg.ent_coef, seed=77)
    common = dict(actor_params=ap.to(dev), target_critic_params=cp.to(dev), init_states=x0.to(dev), state_mean=s_mean.to(dev),
                  state_std=s_std.to(dev), reward_mean_std=r_ms.to(dev), offset=3)
    ops_ = []
    for system, sp in ((sys5, sp5), (sys3, sp3)):
        spec = system.rollout_spec(sp, dev)
        op = ops.BpttActorGrad(**kw)
        op(**common, system_kind=spec["system_kind"], reward_kind=spec["reward_kind"], reward_params=spec["reward_params"],
           dyn_params=spec["dyn_params"], dyn_spec=spec["dyn_spec"], ens_predict_delta=spec["ens_predict_delta"], ens_mode=spec["ens_mode"],
           ens_sample_noise=spec["ens_sample_noise"], ens_min_std=spec["ens_min_std"])
        ops_.append(op)
    torch.cuda.synchronize()
    assert float(ops_[0].grads.abs().max()) > 0
    assert torch.equal(_bits(ops_[0].grads), _bits(ops_[1].grads))
    assert torch.equal(_bits(ops_[0].transitions), _bits(ops_[1].transitions))
