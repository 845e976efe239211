"""GPU: mbpo_ens_calibrate against the restatement (tests/ens_calibrate_ref.py) bit for bit on constructed, near-tie-free fixtures
(tests/test_cpu_ens_calibrate.py checks the fixtures themselves), on non-finite and collapsed rows, on a tie, on reused outputs and
under graph capture; EnsembleDynamics.calibrate / coverage / fit(calibrate=True) through the real member forward; the binding of the
calibration to the hallucinated control's beta; next_state's std.

Every launch-level case poisons its outputs first (0x7f bytes in counts and best_idx, NaN in calibration).  The kernel forms every
product and sum as one rounded fp32 operation, as the restatement does, so equality is demanded in every cell."""
import math

import pytest
import torch

from oracle import nets as onets

import ens_calibrate_ref as ref
import ens_select_ref as sref

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _poisoned_out(b, dev, A=None):
    x, A, P = b["x"], b["alphas"].numel() if A is None else A, b["level_q"].numel()
    counts = torch.full((x, A, P), 0x7f7f7f7f, device=dev, dtype=torch.int32)
    best = torch.full((x,), 0x7f7f7f7f, device=dev, dtype=torch.int32)
    cal = torch.full((x,), float("nan"), device=dev)
    return cal, best, counts


def _launch(b, dev, out=None):
    from mbpo import ops
    d = lambda t: None if t is None else t.to(dev)
    out = _poisoned_out(b, dev) if out is None else out
    got = ops.ens_calibrate(d(b["y"]), d(b["rows"]), b["x"], b["u"], idx=d(b["idx"]), next_obs_off=b["next_obs_off"],
                            predict_delta=b["predict_delta"], alphas=d(b["alphas"]), n_levels=b["level_q"].numel(), scale=d(b["scale"]),
                            out=out)
    assert all(g is o for g, o in zip(got, out))
    return got


def _assert_equals_reference(got, key):
    cal, best, counts = (t.cpu() for t in got)
    want_counts, want_best, want_cal, _ = ref.expected(key)
    bad = int((counts != want_counts).sum())
    assert bad == 0, f"{key}: {bad} of {counts.numel()} cells differ, first at {(counts != want_counts).nonzero()[:3].tolist()}"
    assert torch.equal(best, want_best), key
    assert torch.equal(_bits(cal), _bits(want_cal)), key


# ------------------------------------------------------------------------------------------------ 1. constructed fixtures
@pytest.mark.parametrize("name", list(ref.CASES))
def test_counts_and_picks_equal_the_restatement(dev, name):
    b = ref.case(name)
    assert b["y"].shape[2] == 2 * b["x"] + ref.CASES[name].get("y_extra", 0)
    _assert_equals_reference(_launch(b, dev), name)


def test_levels_on_the_device_are_the_restated_ones(dev):
    from mbpo import ops
    b = ref.case("ragged")
    _launch(b, dev)
    for P in (1, 4, 19):
        assert torch.equal(_bits(ops._cal_cached(("levels", P), lambda: ops.calibration_levels(P), dev)), _bits(ref.levels(P)))


# ------------------------------------------------------------------------------------------------ 2. degenerate and non-finite rows
@pytest.mark.parametrize("kind", ref.DEGENERATE)
def test_degenerate_rows(dev, kind):
    b = ref.degenerate(kind)
    got = _launch(b, dev)
    _assert_equals_reference(got, f"deg:{kind}")
    best = got[1].cpu()
    assert bool(((best >= 0) & (best < b["alphas"].numel())).all())
    if kind == "one_member":                        # v = 0: exactly the rows with d2 = 0, in every cell
        assert set(got[2].cpu().unique().tolist()) == {200}


# ------------------------------------------------------------------------------------------------ 3. ties
def test_a_tie_goes_to_the_lower_index(dev):
    b = ref.tie_case()
    got = _launch(b, dev)
    _assert_equals_reference(got, "tie")
    assert got[1].tolist() == [2, 2, 2] and torch.equal(got[2][:, 2], got[2][:, 3])


# ------------------------------------------------------------------------------------------------ 4. reuse and capture
def test_outputs_are_reused_and_the_call_is_capturable(dev):
    """Two calls into the same outputs with different data (the second must not see the first's counts), then one captured call
    replayed twice on poisoned outputs: bit for bit the eager results."""
    a, b = ref.case("ragged"), ref.degenerate("nan_member")          # both [3][7][4]
    out = _poisoned_out(a, dev)
    _launch(a, dev, out)
    _assert_equals_reference(out, "ragged")
    _launch(b, dev, out)
    _assert_equals_reference(out, "deg:nan_member")
    from mbpo import ops
    d = lambda t: None if t is None else t.to(dev)
    args = (d(a["y"]), d(a["rows"]), a["x"], a["u"])
    kw = dict(idx=d(a["idx"]), next_obs_off=a["next_obs_off"], predict_delta=a["predict_delta"], alphas=d(a["alphas"]),
              n_levels=a["level_q"].numel(), scale=d(a["scale"]), out=out)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.ens_calibrate(*args, **kw)
    for _ in range(2):
        for t, fill in zip(out, (float("nan"), 0x7f7f7f7f, 0x7f7f7f7f)):
            t.fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        _assert_equals_reference(out, "ragged")


# ------------------------------------------------------------------------------------------------ 5. through the forward
def _rows_for(dyn, dp, n, seed, dev, k=(0.5, 1.0, 4.0, 2.0)):
    """Transition rows (obs, action, reward, discount, next_obs) whose next_obs is the members' own mean prediction plus k_c times
    their spread times N(0, 1): a model overconfident by k_c in dimension c."""
    X, U = dyn.x_dim, dyn.u_dim
    g = torch.Generator().manual_seed(seed)
    x, u = torch.randn(n, X, generator=g).to(dev), (torch.rand(n, U, generator=g) * 2 - 1).to(dev)
    mu = dyn.member_outputs(x, u, dp, elites=True)[..., :X]
    kk = torch.tensor(k[:X], device=dev)
    nxt = x + mu.mean(0) + kk * mu.var(dim=0, unbiased=False).sqrt() * torch.randn(n, X, generator=g).to(dev)
    return torch.cat([x, u, torch.zeros(n, 2, device=dev), nxt], dim=1).contiguous()


def _perturbed(dyn, seed, dev):
    dp = dyn.init_params(seed)
    g = torch.Generator().manual_seed(seed)
    dp.params.add_(0.05 * torch.randn(dp.params.numel(), generator=g).to(dev) * (dp.params != 0))       # (padding stays zero)
    return dp


@pytest.mark.parametrize("X,hidden,E,n_elites,scaler", [
    (3, (64, 64, 64), 5, None, False),
    (3, (64, 64, 64), 5, None, True),
    (4, (200,) * 4, 7, 5, False),
    (4, (200,) * 4, 7, 5, True),
])
def test_calibrate_through_the_member_forward(dev, X, hidden, E, n_elites, scaler):
    """Random data has near ties, so equal counts are not demanded: the GPU's pick must be the restated pick of the GPU's OWN counts,
    and its calibration within one grid step of the restatement's on the GPU's own member outputs."""
    from mbpo.systems import EnsembleDynamics
    U, n = 1, 700
    dyn = EnsembleDynamics(X, U, n_members=E, hidden_layer_sizes=hidden, device=dev)
    dp = _perturbed(dyn, 3, dev)
    if scaler:
        g = torch.Generator().manual_seed(9)
        dp.scaler = torch.stack([0.3 * torch.randn(X + U, generator=g), torch.exp(0.3 * torch.randn(X + U, generator=g))]).to(dev)
        dyn.fold(dp)
    if n_elites:
        dp = dyn.select_elites(dp, torch.arange(E, 0, -1).float(), n_elites)
    rows = _rows_for(dyn, dp, n + 50, 4, dev)
    idx = torch.randperm(n + 50, generator=torch.Generator().manual_seed(1))[:n].to(torch.int32).to(dev)
    dp2, best, counts = dyn.calibrate(dp, rows, idx=idx, return_counts=True)
    assert dp2 is dp and dp.calibration.shape == (X,) and dp.calibration.is_cuda
    assert counts.shape == (X, 61, 19)
    h = rows[idx.long()]
    y = dyn.member_outputs(h[:, :X], h[:, X:X + U], dp, elites=True).cpu()
    assert y.shape[0] == (n_elites or E)
    al, q = ref.default_alphas(), ref.levels(19)
    t = ref.targets(rows.cpu(), idx.cpu(), n, X, X + U + 2, True)
    want_counts = ref.counts(y, t, al, q)
    want_best, _ = ref.pick(want_counts, n)
    own_best, _ = ref.pick(counts.cpu(), n)
    assert torch.equal(best.cpu(), own_best)
    assert torch.equal(_bits(dp.calibration), _bits(ref.calibration(al, own_best)))
    moved = int((counts.cpu() != want_counts).sum())
    # |log10(calibration_gpu / calibration_ref)| on the grid's exact values 10^((a - 20) / 20): the index distance over 20
    ratio = (own_best.long() - want_best.long()).abs().double() / 20.0
    print(f"{X, hidden, E, n_elites, scaler}: calibration {[round(float(v), 3) for v in dp.calibration]}, {moved} of {counts.numel()} "
          f"cells differ from the restatement, max |log10 ratio| {float(ratio.max()):.3f}")
    assert float(ratio.max()) <= 0.05


@pytest.mark.parametrize("k", ref.RECOVERY_K)
def test_recovery_on_the_device(dev, k):
    from mbpo import ops
    mu, t = ref.recovery_case(k)
    n, x = t.shape
    rows = torch.cat([torch.zeros(n, x + 1 + 2), t], dim=1).contiguous()          # obs = 0: the target is next_obs itself
    cal, best, counts = ops.ens_calibrate(mu.to(dev), rows.to(dev), x, 1, predict_delta=False)
    print(f"k = {k}: calibration {[round(float(v), 4) for v in cal]}")
    for c in range(x):
        assert abs(math.log10(float(cal[c]) / k)) <= ref.RECOVERY_TOL, (k, c, float(cal[c]))
    assert torch.equal(best.cpu(), ref.pick(counts.cpu(), n)[0])


# ------------------------------------------------------------------------------------------------ 6. fit(calibrate=True)
@pytest.fixture(scope="module")
def pendulum_rows(dev):
    from mbpo.systems import PendulumSystem
    system = PendulumSystem()
    g = torch.Generator().manual_seed(0)
    n = 900
    th = (torch.rand(n, generator=g) * 2 - 1) * math.pi
    x = torch.stack([torch.cos(th), torch.sin(th), (torch.rand(n, generator=g) * 2 - 1) * 6], 1).to(dev)
    u = (torch.rand(n, 1, generator=g) * 2 - 1).to(dev)
    nxt = system.step(x, u, system.reset().system_params)
    return torch.cat([x, u, nxt.reward[:, None], torch.ones(n, 1, device=dev), nxt.x_next], 1).contiguous()


@pytest.mark.parametrize("normalize", [False, True])
def test_fit_calibrates_on_its_holdout_and_changes_nothing_else(dev, pendulum_rows, normalize):
    from mbpo.systems import EnsembleDynamics
    from mbpo.utils import keys as K
    rows, E = pendulum_rows, 5
    dyn, dyn_cal = (EnsembleDynamics(3, 1, n_members=E, device=dev) for _ in range(2))      # (a dynamics keeps its AdamW state across fits)
    p0 = dyn.init_params(2)
    kw = dict(num_steps=40, batch_size=128, learning_rate=3e-3, key=5, holdout_ratio=0.2, n_elites=3, normalize_inputs=normalize)
    plain, l0 = dyn.fit(p0.replace(params=p0.params.clone()), rows, **kw)
    assert plain.calibration is None
    cal, l1 = dyn_cal.fit(p0.replace(params=p0.params.clone()), rows, calibrate=True, **kw)
    assert cal.calibration is not None and cal.calibration.shape == (3,) and bool((cal.calibration > 0).all())
    for name in ("params", "holdout", "elite_idx", "elite_params", "scaler", "folded_params"):
        a, b = getattr(plain, name), getattr(cal, name)
        assert (a is None) == (b is None), name
        if a is not None:
            assert torch.equal(_bits(a.float()), _bits(b.float())), name
    assert torch.equal(_bits(l0), _bits(l1))
    # a separate calibrate call on the same holdout rows: the restated split gives the indices
    hold, _ = sref.split(K.PRNGKey(5), rows.shape[0], 0.2)
    again = dyn.calibrate(plain, rows, idx=hold.to(torch.int32).to(dev))
    assert torch.equal(_bits(again.calibration), _bits(cal.calibration))


# ------------------------------------------------------------------------------------------------ 7. binding
def _optimistic(dev, beta, calibrated, X=3, U=1, E=5):
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, QuadraticReward
    dyn = EnsembleDynamics(X, U, n_members=E, device=dev)
    system = EnsembleSystem(dyn, QuadraticReward(X, U), mode="optimistic", beta=beta, calibrated=calibrated)
    sp = system.init_params(4)
    g = torch.Generator().manual_seed(2)
    sp.dynamics_params.params.add_(0.05 * torch.randn(sp.dynamics_params.params.numel(), generator=g).to(dev))
    return dyn, system, sp


def _policy_rollout(dev, system, sp, seed=21, N=48, S=3):
    from mbpo import ops
    X, A = system.x_dim, system.action_dim
    g = torch.Generator().manual_seed(seed)
    pdims = [X, 64, 64, 2 * A]
    ppar = onets.init_mlp_flat(pdims, g) + 0.02 * torch.randn(onets.n_params(pdims), generator=g)
    obs = torch.randn(N, X, generator=g)
    return ops.model_rollout(policy_params=ppar.to(dev), policy_spec=ops.MlpSpec(pdims, "swish", 1), x_dim=X, u_dim=A, obs=obs.to(dev),
                             first_obs=obs.to(dev), steps=torch.zeros(N, device=dev), done=torch.zeros(N, device=dev), n_steps=S,
                             episode_length=S, seed=seed, **system.rollout_spec(sp, dev))


def test_calibrated_beta_is_beta_times_calibration(dev):
    b = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)
    c = torch.tensor([3.1622777, 0.7079458, 1.0], device=dev)
    dyn, system, sp = _optimistic(dev, b, True)
    with pytest.raises(ValueError, match="calibrate"):
        system.rollout_spec(sp, dev)
    sp.dynamics_params.calibration = c.clone()
    _, plain, _ = _optimistic(dev, b.float() * c.float().cpu(), False)
    spp = sp.replace(dynamics_params=sp.dynamics_params.replace(calibration=None))
    assert torch.equal(system.beta, b.float())                          # the user's value
    g = torch.Generator().manual_seed(4)
    x, a = torch.randn(33, 3, generator=g).to(dev), (torch.rand(33, 4, generator=g) * 2 - 1).to(dev)
    got, want = system.step(x, a, sp), plain.step(x, a, spp)
    assert torch.equal(_bits(got.x_next), _bits(want.x_next)) and torch.equal(_bits(got.reward), _bits(want.reward))
    uncal = _optimistic(dev, b, False)[1].step(x, a, spp)
    assert not torch.equal(got.x_next, uncal.x_next)                    # and the calibration moves the state
    ra, rb = _policy_rollout(dev, system, sp), _policy_rollout(dev, plain, spp)
    assert torch.equal(_bits(ra), _bits(rb))
    # the buffer is the system's own: the same pointer after the calibration is rewritten in place, with the new contents
    spec = system.rollout_spec(sp, dev)
    ptr0 = spec["halluc_beta"].data_ptr()
    assert torch.equal(_bits(spec["halluc_beta"]), _bits(b.float().to(dev) * c))
    rows = _rows_for(dyn, sp.dynamics_params, 600, 6, dev)
    old = sp.dynamics_params.calibration
    dyn.calibrate(sp.dynamics_params, rows)
    assert sp.dynamics_params.calibration is old and not torch.equal(old, c)
    spec = system.rollout_spec(sp, dev)
    assert spec["halluc_beta"].data_ptr() == ptr0
    assert torch.equal(_bits(spec["halluc_beta"]), _bits(b.float().to(dev) * old))
    # another tensor is picked up too
    sp.dynamics_params.calibration = torch.ones(3, device=dev)
    assert torch.equal(_bits(system.rollout_spec(sp, dev)["halluc_beta"]), _bits(b.float().to(dev)))


def test_coverage_is_the_calibrations_own_slice(dev):
    from mbpo.systems import EnsembleDynamics
    dyn = EnsembleDynamics(3, 1, n_members=5, device=dev)
    dp = _perturbed(dyn, 5, dev)
    rows = _rows_for(dyn, dp, 800, 7, dev)
    before = dyn.coverage(dp, rows)                                    # no calibration yet: the raw spread
    assert torch.equal(_bits(before), _bits(dyn.coverage(dp, rows, calibrated=False)))
    dp, best, counts = dyn.calibrate(dp, rows, return_counts=True)
    after = dyn.coverage(dp, rows)
    assert after.shape == (3, 19) and after.dtype == torch.float32
    pick = counts[torch.arange(3, device=dev), best.long()].float() / 800
    assert torch.equal(_bits(after), _bits(pick))
    assert torch.equal(_bits(dyn.coverage(dp, rows, calibrated=False)), _bits(counts[:, ref.ALPHA_ONE].float() / 800))
    # the selection minimises the squared distance to nominal over a grid that holds 1, and these rows are overconfident by (0.5, 1, 4)
    nominal = torch.arange(1, 20, device=dev).float() / 20
    sq = lambda cov: float(((cov - nominal) ** 2).sum())
    print(f"sum (coverage - nominal)^2 before {sq(before):.4f}, after {sq(after):.4f}")
    assert sq(after) < sq(before)


# ------------------------------------------------------------------------------------------------ 8. next_state
def test_next_state_std_with_and_without_a_calibration(dev):
    from mbpo.systems import EnsembleDynamics
    X = 3
    dyn = EnsembleDynamics(X, 1, n_members=5, device=dev)
    dp = _perturbed(dyn, 6, dev)
    g = torch.Generator().manual_seed(3)
    x, u = torch.randn(40, X, generator=g).to(dev), (torch.rand(40, 1, generator=g) * 2 - 1).to(dev)
    y = dyn.member_outputs(x, u, dp, elites=True)
    mu, sig = y[..., :X] + x, torch.nn.functional.softplus(y[..., X:2 * X]) + 1e-3
    plain, _ = dyn.next_state(x, u, dp)
    torch.testing.assert_close(plain.stddev(), torch.sqrt((sig ** 2).mean(0) + mu.var(dim=0, unbiased=False)), rtol=1e-6, atol=0)
    c = torch.tensor([3.0, 0.25, 1.0], device=dev)
    dp.calibration = c
    cal, _ = dyn.next_state(x, u, dp)
    torch.testing.assert_close(cal.stddev(), torch.sqrt((sig ** 2).mean(0) + c ** 2 * mu.var(dim=0, unbiased=False)), rtol=1e-6, atol=0)
    assert torch.equal(_bits(cal.mean()), _bits(plain.mean()))
    assert torch.equal(_bits(cal.stddev()[:, 2]), _bits(plain.stddev()[:, 2])) and bool((cal.stddev()[:, 0] > plain.stddev()[:, 0]).all())


# ------------------------------------------------------------------------------------------------ the example
def test_example_runs_calibrated(dev):
    """examples/mbpo_pendulum.py --calibrate --optimistic: the MBPO loop on an optimistic model whose beta is scaled by the calibration
    picked on the fit's holdout; the report holds the factors and the coverage before and after."""
    import importlib.util
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    spec = importlib.util.spec_from_file_location("mbpo_pendulum_example", root / "examples" / "mbpo_pendulum.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    hist = mod.run(iters=1, n_true=512, model_steps=50, sac_steps=2000, verbose=False, optimistic=1.0, calibrate=True)
    h = hist[0]
    assert len(hist) == 1 and math.isfinite(h["model_nll"]) and math.isfinite(h["true_return"])
    assert len(h["calibration"]) == 3 and all(0.1 - 1e-6 <= v <= 100 + 1e-3 for v in h["calibration"])
    for name in ("holdout", "fresh"):
        for tag in ("before", "after"):
            cov = h[f"coverage_{name}_{tag}"]
            assert len(cov) == 3 and all(len(r) == 2 and 0.0 <= r[0] <= r[1] <= 1.0 for r in cov)
