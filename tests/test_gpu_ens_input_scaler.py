"""GPU: the ensemble's input scaler — mbpo_ens_scaler_fit / mbpo_ens_scaler_prepare / mbpo_ens_fold_scaler against the restatement
(tests/ens_scaler_ref.py), EnsembleDynamics.fit(normalize_inputs=True) as the composition of those calls with the unchanged fit, and
every consumer of a scaler-bearing EnsembleDynamicsParams against the same consumer on plain folded parameters.

Tolerances.  Statistics: the device accumulates in fp64 and rounds once to fp32 (2^-24 relative); the bound is 4 roundings,
|mean - ref| <= 2^-23 |ref| + 2^-40 max|d| (the second term: the fp64 sums' own error where the mean cancels), std within 2^-21
relative.  Prepare: reward and target are copies or one subtraction (bit-exact); a normalised entry is one subtraction and one
product on the device's own fl(1 / std) (2 ulp).  Fold: W' is one product (2 ulp of fl(W fl(1 / std))); b' is in_dim products and
sums, |b' - ref| <= (in_dim + 1) 2^-24 (|b| + sum |W' mean|).  End to end: 4 x the fp32-vs-fp64 discrepancy the CPU test measures on
set a (ens_scaler_ref.cancellation_case)."""
import importlib.util
import math
from pathlib import Path

import pytest
import torch

from oracle import nets as onets

import ens_scaler_ref as ref

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
POISON = 12345.0


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _poisoned(numel, dev, pad):
    """A view of `numel` floats inside a larger allocation filled with POISON.  pad 36: the view is 16-byte aligned; 37: it is not."""
    buf = torch.full((numel + 2 * pad,), POISON, device=dev)
    return buf, buf[pad:pad + numel]


def _poison_intact(buf, numel, pad):
    return bool((buf[:pad] == POISON).all()) and bool((buf[pad + numel:] == POISON).all())


def _ulps(got: torch.Tensor, want: torch.Tensor) -> float:
    """max |got - want| in units of want's fp32 spacing."""
    want = want.float()
    spacing = torch.nextafter(want.abs(), torch.full_like(want, float("inf"))) - want.abs()
    return float(((got.float().double() - want.double()).abs() / spacing.double()).max())


def _rows(X, U, R, row_len, seed):
    """[R, row_len] rows; input column 1 is constant and input column 2 is 1e4 + N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    rows = torch.randn(R, row_len, generator=g) * (1.0 + torch.arange(row_len) % 5)
    rows[:, 1] = -2.5
    rows[:, 2] = 1e4 + torch.randn(R, generator=g)
    return rows, g


# (X, U, R, row_len, how the rows are selected).  300 rows of 23 inputs already take 4 workgroups (11 rows at a time, 8 passes each);
# 20 000 rows of 4 inputs take 40.
SELECT_CASES = [
    (3, 1, 37, 9, "all"),
    (3, 1, 37, 9, "idx21"),
    (3, 1, 37, 9, "one"),
    (17, 6, 300, 44, "all"),
    (17, 6, 300, 45, "all"),
    (17, 6, 300, 45, "idx21"),
    (3, 1, 20000, 9, "all"),
]


def _selection(how, R, g, dev):
    """(idx on the host or None, n or None)"""
    if how == "all":
        return None, None
    if how == "one":
        return None, 1
    idx = torch.randint(0, R, (21,), generator=g)
    idx[-3:] = idx[:3]                                       # repeats, unsorted
    return idx.to(torch.int32), None


@pytest.mark.parametrize("X,U,R,row_len,how", SELECT_CASES)
def test_scaler_statistics(dev, X, U, R, row_len, how):
    from mbpo import ops
    D = X + U
    rows, g = _rows(X, U, R, row_len, seed=R + row_len)
    idx, n = _selection(how, R, g, dev)
    want = ref.stats64(rows, D, idx=idx, n=n)
    rows_d, idx_d = rows.to(dev), None if idx is None else idx.to(dev)
    got = ops.ens_scaler_fit(rows_d, D, idx=idx_d, n=n)
    again = ops.ens_scaler_fit(rows_d, D, idx=idx_d, n=n)
    torch.cuda.synchronize()
    assert got.shape == (2, D) and torch.equal(_bits(got), _bits(again))
    got = got.cpu().double()
    sel = ref._select(rows, idx, n)[:, :D].double()
    bound = 2.0 ** -23 * want[0].abs() + 2.0 ** -40 * sel.abs().max()
    err_m = (got[0] - want[0]).abs()
    err_s = ((got[1] - want[1]).abs() / want[1]).max()
    print(f"scaler stats {X, U, R, row_len, how}: max mean error / bound {float((err_m / bound).max()):.3f}, "
          f"std relative error {float(err_s):.3e} (bound {2.0 ** -21:.3e})")
    assert bool((err_m <= bound).all())
    assert float(err_s) <= 2.0 ** -21
    assert float(got[1, 1]) == 1.0 and float(got[0, 1]) == -2.5          # the constant column: std exactly 1
    if how == "one":
        assert torch.equal(got[1], torch.ones(D, dtype=torch.float64)) and torch.equal(got[0].float(), rows[0, :D])
    else:
        assert bool((got[1, 2:] != 1.0).all())


@pytest.mark.parametrize("pad", [36, 37])                     # 16-byte stores; dword stores
@pytest.mark.parametrize("delta,reward", [(True, True), (False, False)])
@pytest.mark.parametrize("X,U,R,row_len,how", SELECT_CASES[:6])
def test_scaler_prepare(dev, X, U, R, row_len, how, delta, reward, pad):
    from mbpo import ops
    D = X + U
    rows, g = _rows(X, U, R, row_len, seed=R + row_len)
    idx, n = _selection(how, R, g, dev)
    rows_d, idx_d = rows.to(dev), None if idx is None else idx.to(dev)
    scaler = ops.ens_scaler_fit(rows_d, D, idx=idx_d, n=n)
    n_out = ref._select(rows, idx, n).shape[0]
    L = ops.prepared_row_len(X, U)
    buf, view = _poisoned(n_out * L, dev, pad)
    assert (view.data_ptr() % 16 == 0) == (pad == 36)
    noff, roff = row_len - X, (D if reward else None)         # the target's columns end the row
    out = ops.ens_scaler_prepare(rows_d, scaler, X, U, idx=idx_d, n=n, next_obs_off=noff, reward_off=roff, predict_delta=delta,
                                 out=view.view(n_out, L))
    torch.cuda.synchronize()
    assert _poison_intact(buf, n_out * L, pad)
    want = ref.prepare(rows, scaler.cpu(), X, U, idx=idx, n=n, next_obs_off=noff, reward_off=roff, predict_delta=delta)
    got = out.cpu()
    assert got.shape == want.shape == (n_out, L)
    # rows in idx order, reward and target bit for bit
    assert torch.equal(_bits(got[:, D:]), _bits(want[:, D:]))
    if not reward:
        assert bool((got[:, D] == 0).all())
    cols = [c for c in range(D) if c != 1]                    # (the constant column normalises to exactly 0)
    u = _ulps(got[:, cols], want[:, cols])
    print(f"prepare {X, U, R, row_len, how, delta, reward, pad}: normalised columns within {u:.2f} ulp")
    assert u <= 2.0 and bool((got[:, 1] == 0).all())
    if idx is not None:                                       # gathered, not sorted: row k is rows[idx[k]]
        assert torch.equal(_bits(got[:, D + 1:]), _bits(ref.prepare(rows[idx.long()], scaler.cpu(), X, U, next_obs_off=noff,
                                                                   predict_delta=delta)[:, D + 1:]))


def _fold_case(name, seed=0):
    """(logical dims, stored dims, stored params [E * P], E)"""
    from mbpo import ops
    g = torch.Generator().manual_seed(seed)
    E = 3
    logical, width = {"64x3": ((4, 64, 64, 64, 6), None), "200x4": ((4, 200, 200, 200, 200, 8), 256), "23in": ((23, 64, 64, 34), None),
                      "320": ((4, 320, 6), None)}[name]
    P = onets.n_params(logical)
    params = torch.cat([onets.init_mlp_flat(logical, g) + 0.02 * torch.randn(P, generator=g) for _ in range(E)])
    if width is None:
        return logical, list(logical), params, E
    return logical, ops.padded_dims(logical, width), ops.embed_mlp_params(params, logical, width, E), E


@pytest.mark.parametrize("pad", [36, 37])
@pytest.mark.parametrize("name", ["64x3", "200x4", "23in", "320"])
def test_fold(dev, name, pad):
    from mbpo import ops
    logical, dims, params, E = _fold_case(name)
    d0, d1, P = dims[0], dims[1], onets.n_params(dims)
    g = torch.Generator().manual_seed(5)
    scaler = torch.stack([torch.randn(d0, generator=g) * 5, torch.exp(torch.randn(d0, generator=g) * 2)])
    buf, view = _poisoned(E * P, dev, pad)
    src = params.to(dev)
    src0 = src.clone()
    out = ops.ens_fold_scaler(src, E, d0, d1, scaler.to(dev), out=view)
    torch.cuda.synchronize()
    assert _poison_intact(buf, E * P, pad) and torch.equal(_bits(src), _bits(src0))
    got, par = out.cpu().reshape(E, P), params.reshape(E, P)
    n1 = d0 * d1 + d1
    assert torch.equal(_bits(got[:, n1:]), _bits(par[:, n1:]))                     # every float outside layer one
    inv32 = torch.ones(()) / scaler[1]
    w = par[:, :d0 * d1].reshape(E, d0, d1)
    gw, gb = got[:, :d0 * d1].reshape(E, d0, d1), got[:, d0 * d1:n1]
    nz = w != 0
    u = _ulps(gw[nz], (w * inv32[None, :, None])[nz])
    f64 = ref.fold(params.double(), dims, E, scaler).reshape(E, P)
    terms = (gw.double() * scaler[0].double()[None, :, None]).abs().sum(dim=1)
    bound = (d0 + 1) * 2.0 ** -24 * (par[:, d0 * d1:n1].double().abs() + terms)
    err = (gb.double() - f64[:, d0 * d1:n1]).abs()
    live = bound > 0
    print(f"fold {name} pad {pad}: W' within {u:.2f} ulp, max b' error / bound {float((err[live] / bound[live]).max()):.3f}")
    assert u <= 2.0
    assert bool((err <= bound).all())
    h = logical[1]
    if h < d1:                                                                      # the padding: exactly +0.0
        assert bool((_bits(gw[:, :, h:]) == 0).all()) and bool((_bits(gb[:, h:]) == 0).all())
    with pytest.raises(Exception):
        ops.ens_fold_scaler(src, E, d0, d1, scaler.to(dev), out=src)               # in place is refused


# ------------------------------------------------------------------------------------------------ EnsembleDynamics.fit
@pytest.fixture(scope="module")
def mixed_unit_rows(dev):
    """200 true Pendulum transitions (obs, action, reward, discount, next_obs) with the speed in other units: * 100 + 50."""
    from mbpo.systems import PendulumSystem
    system = PendulumSystem()
    g = torch.Generator().manual_seed(0)
    n = 200
    th = (torch.rand(n, generator=g) * 2 - 1) * math.pi
    x = torch.stack([torch.cos(th), torch.sin(th), (torch.rand(n, generator=g) * 2 - 1) * 6], 1).to(dev)
    u = (torch.rand(n, 1, generator=g) * 2 - 1).to(dev)
    nxt = system.step(x, u, system.reset().system_params)
    rows = torch.cat([x, u, nxt.reward[:, None], torch.ones(n, 1, device=dev), nxt.x_next], 1)
    rows[:, 2] = rows[:, 2] * 100 + 50
    rows[:, 8] = rows[:, 8] * 100 + 50
    return rows.contiguous()


@pytest.mark.parametrize("learn_reward", [False, True])
def test_fit_is_the_composition(dev, mixed_unit_rows, learn_reward):
    from mbpo import ops
    from mbpo.systems import EnsembleDynamics
    X, U, E, B, steps = 3, 1, 3, 32, 20
    rows = mixed_unit_rows
    kw = dict(num_steps=steps, batch_size=B, learning_rate=3e-3, key=7)
    dyn_a = EnsembleDynamics(X, U, n_members=E, device=dev, learn_reward=learn_reward)
    pa = dyn_a.init_params(3)
    p0 = pa.params.clone()
    got, losses = dyn_a.fit(pa, rows, normalize_inputs=True, **kw)
    assert got is pa and got.scaler is not None and got.folded_params is not None and got.elite_params is None
    # the manual chain on a fresh optimizer state
    dyn_b = EnsembleDynamics(X, U, n_members=E, device=dev, learn_reward=learn_reward)
    pb = dyn_b.init_params(3)
    scaler = ops.ens_scaler_fit(rows, X + U)
    prep = ops.ens_scaler_prepare(rows, scaler, X, U, reward_off=X + U if learn_reward else None, predict_delta=True)
    want, want_losses = dyn_b.fit(pb, prep, predict_delta=False, next_obs_off=X + U + 1, **kw)
    torch.cuda.synchronize()
    assert want.scaler is None and want.folded_params is None                       # normalize_inputs=False leaves both unset
    assert torch.equal(_bits(got.scaler), _bits(scaler))
    assert torch.equal(_bits(got.params), _bits(want.params)) and torch.equal(_bits(losses), _bits(want_losses))
    assert not torch.equal(got.params, p0) and bool(torch.isfinite(losses).all())
    assert torch.equal(_bits(got.folded_params), _bits(ops.ens_fold_scaler(got.params, E, dyn_a.dims[0], dyn_a.dims[1], scaler)))
    with pytest.raises(ValueError):
        dyn_a.fit(got, rows, **kw)                                                  # normalised parameters on raw inputs


def test_fit_is_the_composition_with_holdout_and_elites(dev, mixed_unit_rows):
    from mbpo import ops
    from mbpo.systems import EnsembleDynamics
    from mbpo.systems.ensemble_system import FIT_SITE_HOLDOUT
    from mbpo.utils import keys as K
    X, U, E, B, steps, R = 3, 1, 3, 32, 20, 200
    rows = mixed_unit_rows
    kw = dict(num_steps=steps, batch_size=B, learning_rate=3e-3, key=7, holdout_ratio=0.25, n_elites=2, eval_every=5)
    dyn_a = EnsembleDynamics(X, U, n_members=E, device=dev)
    got, losses = dyn_a.fit(dyn_a.init_params(3), rows, normalize_inputs=True, **kw)
    # the manual split at the same Philox site; every row prepared with the TRAINING rows' scaler, then the unchanged fit splits again
    perm = ops.philox_permutation(R, seed=K.PRNGKey(7), offset=FIT_SITE_HOLDOUT << 32)
    n_hold = 50
    scaler = ops.ens_scaler_fit(rows, X + U, idx=perm[n_hold:].contiguous())
    prep = ops.ens_scaler_prepare(rows, scaler, X, U, predict_delta=True)
    dyn_b = EnsembleDynamics(X, U, n_members=E, device=dev)
    want, want_losses = dyn_b.fit(dyn_b.init_params(3), prep, predict_delta=False, next_obs_off=X + U + 1, **kw)
    torch.cuda.synchronize()
    assert torch.equal(_bits(got.scaler), _bits(scaler))
    assert torch.equal(_bits(got.params), _bits(want.params)) and torch.equal(_bits(losses), _bits(want_losses))
    assert torch.equal(_bits(got.holdout), _bits(want.holdout)) and torch.equal(got.elite_idx.cpu(), want.elite_idx.cpu())
    P = dyn_a.spec.n_params
    folded = ops.ens_fold_scaler(got.params, E, dyn_a.dims[0], dyn_a.dims[1], scaler)
    assert torch.equal(_bits(got.folded_params), _bits(folded))
    assert torch.equal(_bits(got.elite_params.reshape(2, P)), _bits(folded.reshape(E, P)[got.elite_idx.long()]))
    assert not torch.equal(_bits(got.elite_params), _bits(want.elite_params))       # (the manual chain's elites are unfolded)
    # evaluate() reports what the fit's holdout reported
    again = dyn_a.evaluate(got, rows, perm[:n_hold].contiguous())
    assert torch.equal(_bits(again[1]), _bits(got.holdout[1]))


def test_fit_at_a_logical_width(dev, mixed_unit_rows):
    """320-wide members (kernel_width None, layer by layer): the same composition, and the fold on the logical layout."""
    from mbpo import ops
    from mbpo.systems import EnsembleDynamics
    X, U, E = 3, 1, 2
    kw = dict(num_steps=3, batch_size=32, learning_rate=1e-3, key=2)
    dyn_a = EnsembleDynamics(X, U, n_members=E, hidden_layer_sizes=(320,), device=dev)
    assert dyn_a.kernel_width is None
    got, losses = dyn_a.fit(dyn_a.init_params(1), mixed_unit_rows, normalize_inputs=True, **kw)
    dyn_b = EnsembleDynamics(X, U, n_members=E, hidden_layer_sizes=(320,), device=dev)
    scaler = ops.ens_scaler_fit(mixed_unit_rows, X + U)
    prep = ops.ens_scaler_prepare(mixed_unit_rows, scaler, X, U)
    want, want_losses = dyn_b.fit(dyn_b.init_params(1), prep, predict_delta=False, next_obs_off=X + U + 1, **kw)
    assert torch.equal(_bits(got.params), _bits(want.params)) and torch.equal(_bits(losses), _bits(want_losses))
    xu = mixed_unit_rows[:16, :X + U]
    y = dyn_a.member_outputs(xu[:, :X], xu[:, X:], got).cpu().double()
    y_ref = ref.normalise_then_net64(got.params.cpu(), dyn_a.dims, E, got.scaler.cpu(), xu.cpu())
    torch.testing.assert_close(y, y_ref, rtol=2e-4, atol=2e-4)                      # (the project's forward tolerance; |mean| / std < 1)


# ------------------------------------------------------------------------------------------------ consumers
def _scaler_pair(dev, mode, learned=False, sample_noise=False, termination=None, X=4, U=1, E=3):
    """(system, SystemParams whose dynamics params bear a scaler, SystemParams with plain params = the folded ones)."""
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, LearnedReward, QuadraticReward
    from mbpo.systems.ensemble_system import EnsembleDynamicsParams
    dyn = EnsembleDynamics(X, U, n_members=E, device=dev, learn_reward=learned)
    system = EnsembleSystem(dyn, LearnedReward(dyn) if learned else QuadraticReward(X, U), mode=mode, sample_noise=sample_noise,
                            termination=termination)
    sp = system.init_params(4)
    g = torch.Generator().manual_seed(2)
    dp = sp.dynamics_params
    dp.params.add_(0.05 * torch.randn(dp.params.numel(), generator=g).to(dev))
    dp.scaler = torch.stack([torch.randn(X + U, generator=g) * 0.5, torch.rand(X + U, generator=g) + 0.5]).to(dev)
    assert dp.folded_params is None
    plain = EnsembleDynamicsParams(params=dyn.fold(dp).folded_params.clone())
    assert not torch.equal(plain.params, dp.params)
    rp_s, rp_p = (dp, plain) if learned else (sp.reward_params, sp.reward_params)
    return system, sp.replace(dynamics_params=dp, reward_params=rp_s), sp.replace(dynamics_params=plain, reward_params=rp_p), dyn


def test_consumers_outputs_step_and_rollout(dev):
    from mbpo import ops
    from mbpo.systems import BoxTermination
    N = 64
    g = torch.Generator().manual_seed(8)
    x, u = torch.randn(N, 4, generator=g).to(dev), (torch.rand(N, 1, generator=g) * 2 - 1).to(dev)
    system, sp_s, sp_p, dyn = _scaler_pair(dev, "mean")
    a, b = dyn.member_outputs(x, u, sp_s.dynamics_params), dyn.member_outputs(x, u, sp_p.dynamics_params)
    assert torch.equal(_bits(a), _bits(b))
    da, _ = dyn.next_state(x, u, sp_s.dynamics_params)
    db, _ = dyn.next_state(x, u, sp_p.dynamics_params)
    assert torch.equal(_bits(da.mean()), _bits(db.mean())) and torch.equal(_bits(da.stddev()), _bits(db.stddev()))
    sa, sb = system.step(x, u, sp_s), system.step(x, u, sp_p)
    assert torch.equal(_bits(sa.x_next), _bits(sb.x_next)) and torch.equal(_bits(sa.reward), _bits(sb.reward))
    # and not what the unfolded parameters would give on raw inputs
    raw = sp_s.dynamics_params.replace(scaler=None, folded_params=None)
    assert not torch.equal(dyn.member_outputs(x, u, raw), a)
    # elites of a scaler-bearing object are copies of the folded members
    picked = dyn.select_elites(sp_s.dynamics_params, torch.tensor([2.0, 0.0, 1.0]), 2)
    P = dyn.spec.n_params
    assert torch.equal(_bits(picked.elite_params.reshape(2, P)), _bits(sp_p.dynamics_params.params.reshape(3, P)[[1, 2]]))
    # learned reward
    system, sp_s, sp_p, dyn = _scaler_pair(dev, "mean", learned=True)
    ra, rb = dyn.reward(x, u, sp_s.dynamics_params), dyn.reward(x, u, sp_p.dynamics_params)
    assert torch.equal(_bits(ra.mean()), _bits(rb.mean()))
    # one fused model rollout, 'ts1', with a termination box
    box = BoxTermination.from_intervals(4, {2: (-1.0, 1.0)})
    system, sp_s, sp_p, dyn = _scaler_pair(dev, "ts1", sample_noise=True, termination=box)
    pdims = [4, 64, 64, 2]
    ppar = (onets.init_mlp_flat(pdims, g) + 0.02 * torch.randn(onets.n_params(pdims), generator=g)).to(dev)
    obs = (torch.randn(N, 4, generator=g) * 0.5).to(dev)
    out = []
    for sp in (sp_s, sp_p):                                   # (the rollout advances obs in place: a fresh copy per call)
        out.append(ops.model_rollout(policy_params=ppar, policy_spec=ops.MlpSpec(pdims, "swish", 1), x_dim=4, u_dim=1, obs=obs.clone(),
                                     first_obs=obs.clone(), steps=torch.zeros(N, device=dev), done=torch.zeros(N, device=dev), n_steps=3,
                                     episode_length=3, seed=21, **system.rollout_spec(sp, dev)))
    assert torch.equal(_bits(out[0]), _bits(out[1])) and bool(torch.isfinite(out[0]).all())


def test_consumers_icem(dev):
    from mbpo.optimizers import iCemParams, iCemTO
    system, sp_s, sp_p, _ = _scaler_pair(dev, "ts1")
    x0 = (torch.randn(4, generator=torch.Generator().manual_seed(3)) * 0.5).to(dev)
    out = []
    for sp in (sp_s, sp_p):
        opt = iCemTO(horizon=6, action_dim=1, opt_params=iCemParams(num_particles=3, num_samples=40, num_elites=6, num_steps=2), key=5)
        opt.set_system(system)
        out.append(opt.optimize(x0, opt.init(7).replace(system_params=sp)))
    assert torch.equal(_bits(out[0].best_sequence), _bits(out[1].best_sequence))
    assert torch.equal(_bits(out[0].best_reward), _bits(out[1].best_reward))


def test_consumers_bptt_actor_gradients(dev):
    from mbpo import ops
    from test_gpu_bptt import _setup
    X, U, H, n = 4, 1, 4, 32
    system, sp_s, sp_p, _ = _scaler_pair(dev, "tsinf", sample_noise=True)
    cfg, ap, cp, x0, _, s_mean, s_std, r_ms, _, _ = _setup(X, U, H, n, "ensemble", 3, 4)
    kw = dict(x_dim=X, u_dim=U, horizon=H, actor_dims=cfg.actor_dims, critic_dims=cfg.critic_dims, n=n, device=dev,
              init_stddev=cfg.init_stddev, discount=cfg.discount, lambda_=cfg.lambda_, ent_coef=cfg.ent_coef, seed=77)
    common = dict(actor_params=ap.to(dev), target_critic_params=cp.to(dev), init_states=x0.to(dev), state_mean=s_mean.to(dev),
                  state_std=s_std.to(dev), reward_mean_std=r_ms.to(dev), offset=3)
    ops_ = []
    for sp in (sp_s, sp_p):
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


def test_member_outputs_match_normalise_then_net(dev):
    """Raw inputs through the device's fold and forward kernel against fp64 "normalise, then the unfolded members", on set a of the
    cancellation measurement (inputs within 3 std of the mean, |mean| <= 3 std); the scaler is the device's fit of those inputs.
    Tolerance: 4 x the CPU figure of set a (fp32 folded restatement vs the same fp64 reference)."""
    from mbpo import ops
    from mbpo.systems import EnsembleDynamics
    from mbpo.systems.ensemble_system import EnsembleDynamicsParams
    params, case_scaler, xu = ref.cancellation_case("a")
    fig_a = ref.fold_discrepancy(params, ref.CANCEL_DIMS, ref.CANCEL_MEMBERS, case_scaler, xu)
    X, U, E = 3, 1, ref.CANCEL_MEMBERS
    dyn = EnsembleDynamics(X, U, n_members=E, device=dev)
    assert tuple(dyn.dims) == ref.CANCEL_DIMS
    xu_d = xu.to(dev)
    scaler = ops.ens_scaler_fit(xu_d, X + U)
    z = ((xu.double() - scaler.cpu().double()[0]) / scaler.cpu().double()[1]).abs().max()
    assert float(z) <= 3.0 and float((scaler[0].abs() / scaler[1]).max()) <= 3.0
    dp = EnsembleDynamicsParams(params=params.to(dev), scaler=scaler)
    got = dyn.member_outputs(xu_d[:, :X], xu_d[:, X:], dp).cpu().double()
    want = ref.normalise_then_net64(params, ref.CANCEL_DIMS, E, scaler.cpu(), xu)
    err = float((got - want).abs().max())
    print(f"member_outputs vs fp64 normalise-then-net: max error {err:.3e}; CPU figure (set a) {fig_a:.3e}, tolerance {4 * fig_a:.3e}")
    assert err <= 4 * fig_a


def test_example_runs_with_normalised_inputs(dev):
    spec = importlib.util.spec_from_file_location("mbpo_pendulum_example", ROOT / "examples" / "mbpo_pendulum.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    hist = mod.run(iters=1, n_true=512, model_steps=50, sac_steps=2000, verbose=False, normalize_inputs=True)
    assert len(hist) == 1 and math.isfinite(hist[0]["model_nll"]) and math.isfinite(hist[0]["true_return"])
