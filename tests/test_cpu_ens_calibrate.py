"""Calibration of the ensemble's spread without a GPU: the conditions every fixture of tests/test_gpu_ens_calibrate.py meets on the
restatement alone (tests/ens_calibrate_ref.py), recovery of a known overconfidence factor, the integer identity of the selection, the
Python surface's refusals (device="cpu", nothing is launched) and the entry point's argument checks (no launches)."""
import math

import pytest
import torch

import ens_calibrate_ref as ref

ALL_FIXTURES = [*ref.CASES, "tie", *[f"deg:{k}" for k in ref.DEGENERATE]]


def _fixture(key):
    if key == "tie":
        return ref.tie_case()
    return ref.degenerate(key[4:]) if key.startswith("deg:") else ref.case(key)


@pytest.mark.parametrize("key", ALL_FIXTURES)
def test_gpu_fixtures_meet_their_conditions(key):
    """fp32 and fp64 counts agree in every cell; no count moves when every threshold is scaled by 1 +- 1e-3; the counts take more than
    10 distinct values (not an all-0 or all-n table) unless the fixture is degenerate on purpose (v = 0 everywhere, or one cell)."""
    b = _fixture(key)
    c32 = ref.expected(key)[0]
    t = ref.case_targets(b)
    c64 = ref.counts(b["y"], t, b["alphas"], b["level_q"], b["scale"], dtype=torch.float64)
    assert torch.equal(c32, c64), f"{key}: {int((c32 != c64).sum())} cells differ between fp32 and fp64"
    for f in (1 - 1e-3, 1 + 1e-3):
        assert torch.equal(c32, ref.counts(b["y"], t, b["alphas"], b["level_q"], b["scale"], dtype=torch.float64, thr_factor=f)), (key, f)
    distinct = int(c32.unique().numel())
    frac = c32.double() / b["n"]
    print(f"{key}: {distinct} distinct counts, coverage {float(frac.min()):.4f} .. {float(frac.max()):.4f}, kept gaps {b['n_gaps'][:3]}")
    assert c32.shape == (b["x"], b["alphas"].numel(), b["level_q"].numel())
    if key in ref.ONE_CELL:
        assert c32.numel() == 1 and (b["n"] == 1 or 0 < int(c32.reshape(-1)[0]) < b["n"])
    elif key == "deg:one_member":
        assert set(c32.unique().tolist()) == {b["n"] - len(range(0, b["n"], 3))}        # exactly the rows left at d2 = 0
    else:
        assert distinct > 10
    best = ref.expected(key)[1]
    assert bool(((best >= 0) & (best < b["alphas"].numel())).all())


def test_tie_fixture_has_a_real_tie_at_the_minimum():
    cnt, best, _, S = ref.expected("tie")
    assert torch.equal(cnt[:, 2], cnt[:, 3])
    assert best.tolist() == [2, 2, 2] and torch.equal(S[:, 2], S[:, 3]) and bool((S[:, 2] < S[:, 1]).all())


def test_levels_and_default_grid():
    al = ref.default_alphas()
    assert al.numel() == 61 and float(al[ref.ALPHA_ONE]) == 1.0
    assert abs(float(al[0]) - 0.1) < 1e-7 and abs(float(al[-1]) - 100.0) < 1e-4
    q = ref.levels(19)
    assert q.numel() == 19 and bool((q[1:] > q[:-1]).all())
    # 2 erfinv(p)^2 is the squared two-sided Gaussian quantile: p = 0.5 -> 0.6745^2, p = 0.9 -> 1.6449^2
    assert abs(float(q[9]) - 0.67448975 ** 2) < 1e-6 and abs(float(q[17]) - 1.64485363 ** 2) < 1e-5
    from mbpo import ops
    assert torch.equal(ops.calibration_alphas(), al) and torch.equal(ops.calibration_levels(19), q)
    assert torch.equal(ops.calibration_levels(4), ref.levels(4))


@pytest.mark.parametrize("k", ref.RECOVERY_K)
def test_recovery_of_a_known_overconfidence_factor(k):
    """Targets m + k sd N(0, 1): the picked factor is k to within 1.5 grid steps in every dimension (member spreads 0.01, 0.1, 1), and
    the selection's integer identity S[best] <= S[alpha = 1] holds."""
    mu, t = ref.recovery_case(k)
    al, q = ref.default_alphas(), ref.levels(19)
    cnt = ref.counts(mu, t, al, q)
    best, S = ref.pick(cnt, mu.shape[1])
    cal = ref.calibration(al, best)
    print(f"k = {k}: calibration {[round(float(v), 4) for v in cal]}")
    for c in range(3):
        assert abs(math.log10(float(cal[c]) / k)) <= ref.RECOVERY_TOL, (k, c, float(cal[c]))
        assert int(S[c, best[c]]) <= int(S[c, ref.ALPHA_ONE])
        assert int(S[c, best[c]]) == int(S[c].min())


# ------------------------------------------------------------------------------------------------ Python surface
def _dyn(E=3, **kw):
    from mbpo.systems import EnsembleDynamics
    return EnsembleDynamics(3, 1, n_members=E, hidden_layer_sizes=(64, 64), device="cpu", **kw)


def test_params_start_without_a_calibration():
    from mbpo.systems.ensemble_system import EnsembleDynamicsParams
    p = EnsembleDynamicsParams(params=torch.zeros(4))
    assert p.calibration is None
    assert p.replace(calibration=torch.ones(3)).calibration is not None and p.calibration is None
    assert _dyn().init_params(0).calibration is None


def test_fit_refuses_to_calibrate_without_a_holdout():
    dyn = _dyn()
    with pytest.raises(ValueError, match="holdout"):
        dyn.fit(dyn.init_params(0), torch.zeros(50, 9), num_steps=1, calibrate=True)


def test_calibrated_needs_the_optimistic_mode():
    from mbpo.systems import EnsembleSystem, QuadraticReward
    dyn = _dyn()
    for mode in ("mean", "ts1", "tsinf"):
        with pytest.raises(ValueError, match="optimistic"):
            EnsembleSystem(dyn, QuadraticReward(3, 1), mode=mode, calibrated=True)
    s = EnsembleSystem(dyn, QuadraticReward(3, 1), mode="optimistic", beta=[0.5, 1.0, 2.0], calibrated=True)
    assert s.calibrated and torch.equal(s.beta, torch.tensor([0.5, 1.0, 2.0]))          # beta stays the user's value
    assert not EnsembleSystem(dyn, QuadraticReward(3, 1), mode="optimistic").calibrated


def test_rollout_spec_refuses_parameters_without_a_calibration():
    from mbpo.systems import EnsembleSystem, QuadraticReward
    s = EnsembleSystem(_dyn(), QuadraticReward(3, 1), mode="optimistic", calibrated=True)
    sp = s.init_params(0)
    with pytest.raises(ValueError, match="calibrate"):
        s.rollout_spec(sp, torch.device("cpu"))


def test_one_rollout_member_cannot_be_calibrated():
    rows = torch.zeros(20, 9)
    dyn = _dyn(E=1)
    with pytest.raises(ValueError, match="2 rollout members"):
        dyn.calibrate(dyn.init_params(0), rows)
    dyn = _dyn(E=3)                                 # three members, one elite: the rollouts see one
    p = dyn.init_params(0)
    p = p.replace(elite_idx=torch.tensor([1], dtype=torch.int32), elite_params=p.params[:dyn.spec.n_params].clone())
    with pytest.raises(ValueError, match="2 rollout members"):
        dyn.calibrate(p, rows)
    with pytest.raises(ValueError, match="2 rollout members"):
        dyn.coverage(p, rows)


# ------------------------------------------------------------------------------------------------ C-ABI, no device
def test_argument_validation_without_a_device():
    """Every refusal is a negative code with a message, before anything is launched (the pointers are never dereferenced)."""
    from mbpo import _hip
    lib = _hip.load()
    assert hasattr(lib, "mbpo_ens_calibrate")
    ERR_ARG, ERR_UNSUPPORTED = -1, -2
    p = 1 << 20                                     # non-null "device pointers"

    def call(y=p, E=5, n=37, ys=6, rows=p + (1 << 16), n_rows=37, row_len=9, idx=None, x=3, noff=6, delta=1, alphas=p + (2 << 16), A=7,
             lq=p + (3 << 16), P=4, scale=None, counts=p + (4 << 16), best=p + (5 << 16), cal=p + (6 << 16)):
        return lib.mbpo_ens_calibrate(y, E, n, ys, rows, n_rows, row_len, idx, x, noff, delta, alphas, A, lq, P, scale, counts, best, cal,
                                      None)

    for bad in (dict(y=None), dict(rows=None), dict(alphas=None), dict(lq=None), dict(counts=None), dict(best=None), dict(cal=None),
                dict(n=0), dict(n=-3), dict(A=0), dict(P=0), dict(E=0), dict(ys=2), dict(x=0), dict(noff=7), dict(noff=-1), dict(n=38),
                dict(n_rows=0), dict(row_len=0)):
        assert call(**bad) == ERR_ARG, bad
        assert lib.mbpo_last_error(), bad
    # n (P + 1) <= 2^28, so that the int64 selection cannot overflow: refused before any device use, with or without idx
    big = (1 << 28) // 5 + 1
    assert call(n=big, n_rows=big) == ERR_ARG and b"2^28" in lib.mbpo_last_error()
    assert call(n=big, idx=p + (7 << 16)) == ERR_ARG and b"2^28" in lib.mbpo_last_error()
    assert call(ys=2) == ERR_ARG and b"y_stride" in lib.mbpo_last_error()
    assert call(P=128) == ERR_UNSUPPORTED and b"n_levels" in lib.mbpo_last_error()
