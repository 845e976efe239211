"""The many-tile case table (tests/many_tiles_cases.py) checked without a GPU, at the MI355X's 256 compute units:

* every case has more than twice its launch's cap in tiles, a tile count that is not a multiple of the cap, and a ragged last tile;
* no case tensor holds two equal rows (a tile that reads what its predecessor left must read WRONG values);
* the float32 oracle stays within a QUARTER of the tolerance the GPU test uses against the float64 oracle — the reference alone
  does not use up the bound.  The gap check runs on every SAC and PPO case and, for rollout and BPTT (whose oracles are the slow
  ones), on the two largest cases of the family by oracle cost; the ensemble forward has one case.
"""
import pytest
import torch

import many_tiles_cases as mt

CUS = mt.REF_CUS


def _assert_gap(name, got32, ref64, tol):
    ok, ratio = mt.quarter_gap_ok(got32, ref64, **tol)
    print(f"{name}: float32-vs-float64 oracle gap is {ratio * 0.25:.3f} of the tolerance")
    assert ok, f"{name}: the float32 oracle uses {ratio * 0.25:.3f} of the tolerance (limit 0.25)"


@pytest.mark.parametrize("name", list(mt.PPO_CASES))
def test_ppo_case(name):
    case = mt.PPO_CASES[name]
    B, T = mt.ppo_bt(case, CUS)
    assert mt.loops_unevenly(B * T, mt.ppo_cap(case, CUS)) and 5 <= T <= 8
    inputs = mt.ppo_inputs(case, CUS)
    data = inputs[2]
    assert data.shape[:2] == (B, T) and mt.distinct_rows(data)
    g32, _ = mt.ppo_oracle(case, inputs, torch.float32)
    g64, _ = mt.ppo_oracle(case, inputs, torch.float64)
    _assert_gap(name, g32, g64, mt.ppo_tol(case))


@pytest.mark.parametrize("B", mt.SAC_BATCHES)
@pytest.mark.parametrize("name", list(mt.SAC_CASES))
def test_sac_case(name, B):
    case = mt.SAC_CASES[name]
    assert mt.loops_unevenly(B, mt.SAC_BLOCK)
    inputs = mt.sac_inputs(case, B)
    assert mt.distinct_rows(inputs[2])
    g32, _ = mt.sac_oracle(inputs, torch.float32)
    g64, _ = mt.sac_oracle(inputs, torch.float64)
    _assert_gap(f"{name}-{B}", g32, g64, mt.SAC_TOL)


@pytest.mark.parametrize("name", list(mt.RO_CASES))
def test_rollout_case(name):
    case = mt.RO_CASES[name]
    N = mt.ro_n(CUS)
    units, cap = mt.ro_units(case, N), mt.ro_cap(case, CUS)
    assert units > 2 * cap and units % cap != 0 and N % 16 != 0
    inp = mt.ro_inputs(case, N)
    assert mt.distinct_rows(inp["obs0"]) and mt.distinct_rows(inp["pnoise"].permute(1, 0, 2).reshape(N, -1))
    if name in ("wide", "h256"):           # the two largest oracles of the family (10 members at x = 17; four 200-wide layers)
        _, r32 = mt.ro_oracle(case, inp, torch.float32)
        _, r64 = mt.ro_oracle(case, inp, torch.float64)
        _assert_gap(name, r32, r64, mt.RO_TOL)


@pytest.mark.parametrize("name", list(mt.BPTT_CASES))
def test_bptt_case(name):
    case = mt.BPTT_CASES[name]
    n = mt.bptt_n(case, CUS)
    assert mt.loops_unevenly(n, CUS) and mt.tiles_of(n) >= case["min_tiles"]
    s = mt.bptt_inputs(case, n)
    x0, noise = s[3], s[4]
    assert mt.distinct_rows(x0) and mt.distinct_rows(noise.reshape(n, -1))
    if name in ("c2", "c5"):               # the two largest: autograd through 5 and 10 ensemble members
        g32, _, g64, _, _ = mt.bptt_oracle(case, s)
        _assert_gap(name, g32, g64, mt.BPTT_TOL)


def test_ensemble_forward_case():
    N = mt.ens_n(CUS)
    caps = mt.ens_caps(CUS)
    assert mt.loops_unevenly(N, caps["generic"])
    pairs = (mt.tiles_of(N) + 1) // 2
    assert pairs > 2 * caps["lean"] and pairs % caps["lean"] != 0
    params, x = mt.ens_inputs(N)
    assert mt.distinct_rows(x)
    _assert_gap("ensemble forward", mt.ens_oracle(params, x, torch.float32), mt.ens_oracle(params, x, torch.float64), mt.ENS_TOL)
