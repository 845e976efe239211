"""Ensemble model selection without a device: hand-worked cases pin the restatement (tests/ens_select_ref.py) the GPU tests compare
the kernels with, and the three new entry points' ABI (exports, descriptor layout, size query, argument checks) is checked through
calls that launch nothing."""
import ctypes as C
import math
import subprocess
from pathlib import Path

import pytest
import torch

from oracle import nets as onets

import ens_select_ref as sref

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lib():
    from mbpo import _hip
    return _hip.load()


# ------------------------------------------------------------------------------------------------ the restatement, by hand
def test_eval_two_rows_one_dimension_by_hand():
    """X = U = 1, one hidden unit with zero weights: the member's output is its output bias, (mu, raw) = (0.25, 0).
    sigma = softplus(0) + 0.5 = ln 2 + 0.5.  Rows (x, u, r, d, x'): (1, 0, ., ., 1.75) and (-2, 0, ., ., -2.25): delta targets 0.75 and
    -0.25, residuals 0.5 and -0.5.  NLL = 0.5 (0.5 / sigma)^2 + ln sigma for both rows; squared error 0.25 for both.  Absolute
    prediction (predict_delta=False): targets 1.75 and -2.25, residuals 1.5 and -2.5, squared error (2.25 + 6.25) / 2."""
    dims = [2, 1, 2]
    params = torch.zeros(onets.n_params(dims), dtype=torch.float64)
    params[-2] = 0.25                                   # layout: W0 [2, 1], b0 [1], W1 [1, 2], b1 [2] = (mu bias, raw bias)
    rows = torch.tensor([[1.0, 0.0, 9.0, 1.0, 1.75], [-2.0, 0.0, 9.0, 1.0, -2.25]], dtype=torch.float64)
    idx = torch.tensor([0, 1])
    sigma = math.log(2.0) + 0.5
    m = sref.eval_metrics(params, dims, 1, rows, idx, 1, 1, True, 0.5)
    assert m.shape == (2, 1)
    assert abs(float(m[0, 0]) - (0.5 * (0.5 / sigma) ** 2 + math.log(sigma))) < 1e-12
    assert abs(float(m[1, 0]) - 0.25) < 1e-12
    m = sref.eval_metrics(params, dims, 1, rows, idx, 1, 1, False, 0.5)
    assert abs(float(m[1, 0]) - 4.25) < 1e-12
    assert abs(float(m[0, 0]) - (0.5 * (2.25 + 6.25) / 2 / sigma ** 2 + math.log(sigma))) < 1e-12
    # a repeated index counts twice
    m = sref.eval_metrics(params, dims, 1, rows, torch.tensor([1, 1, 0]), 1, 1, False, 0.5)
    assert abs(float(m[1, 0]) - (6.25 + 6.25 + 2.25) / 3) < 1e-12


def test_eval_reward_term_by_hand():
    """The same member with a reward head (mu_r, raw_r) = (-1, 0) and reward targets 0 and 1: residuals 1 and 2 join both sums."""
    dims = [2, 1, 4]
    params = torch.zeros(onets.n_params(dims), dtype=torch.float64)
    params[-4], params[-2] = 0.25, -1.0
    rows = torch.tensor([[1.0, 0.0, 0.0, 1.0, 1.75], [-2.0, 0.0, 1.0, 1.0, -2.25]], dtype=torch.float64)
    sigma = math.log(2.0) + 0.5
    m = sref.eval_metrics(params, dims, 1, rows, torch.tensor([0, 1]), 1, 1, True, 0.5, reward_off=2)
    assert abs(float(m[1, 0]) - (0.25 + (1.0 + 4.0) / 2)) < 1e-12
    want = 0.5 * (0.5 / sigma) ** 2 + math.log(sigma) + 0.5 * (1.0 + 4.0) / 2 / sigma ** 2 + math.log(sigma)
    assert abs(float(m[0, 0]) - want) < 1e-12
    without = sref.eval_metrics(params, dims, 1, rows, torch.tensor([0, 1]), 1, 1, True, 0.5)
    assert abs(float(without[1, 0]) - 0.25) < 1e-12


def test_keep_best_table():
    P = 3
    params = torch.arange(4 * P, dtype=torch.float32).reshape(4, P)
    best = -torch.ones(4, P)
    best_score = torch.tensor([float("inf"), 1.0, 1.0, 1.0])
    score = torch.tensor([0.7, 0.995, float("nan"), 0.5])
    nb, ns, st = sref.keep_best(params, best, score, best_score, 0.01, [4, 7])
    assert torch.equal(nb[0], params[0]) and torch.equal(nb[3], params[3])          # inf -> 0.7, 1.0 -> 0.5
    assert torch.equal(nb[1], best[1]) and torch.equal(nb[2], best[2])              # 0.995 is within the margin; NaN never improves
    assert ns.tolist() == [pytest.approx(0.7), 1.0, 1.0, 0.5] and st == [0, 8]
    nb2, ns2, st2 = sref.keep_best(params + 100, nb, ns, ns, 0.01, st)              # a score equal to the best is no improvement
    assert torch.equal(nb2, nb) and torch.equal(ns2, ns) and st2 == [1, 9]
    # an infinite score does not improve on an infinite best
    _, _, st3 = sref.keep_best(params, best, torch.full((4,), float("inf")), torch.full((4,), float("inf")), 0.01, [0, 0])
    assert st3 == [1, 1]


def test_ranking_with_nan_and_ties():
    nan, inf = float("nan"), float("inf")
    assert sref.ranking(torch.tensor([0.3, nan, 0.1, 0.3, inf, 0.1, 0.2])) == [2, 5, 6, 0, 3, 4, 1]
    assert sref.ranking(torch.tensor([nan, nan, 1.0])) == [2, 0, 1]
    assert sref.ranking(torch.tensor([0.0, -0.0])) == [0, 1]


def test_split_is_a_partition():
    hold, train = sref.split(11, 600, 0.2)
    assert hold.numel() == 120 and train.numel() == 480
    assert sorted(hold.tolist() + train.tolist()) == list(range(600))
    hold, train = sref.split(11, 600, 0.5, max_holdout=50)
    assert hold.numel() == 50 and train.numel() == 550


# ------------------------------------------------------------------------------------------------ the ABI, no device
def test_symbols_and_descriptor_layout(lib, tmp_path):
    from mbpo import _hip
    for name in ("mbpo_ens_eval_workspace_floats", "mbpo_ens_eval", "mbpo_ens_keep_best", "mbpo_ens_pick_elites"):
        assert hasattr(lib, name), name
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "mbpo_hip.h"\nint main(void) { printf("%zu\\n", sizeof(mbpo_ens_eval_desc)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    assert int(out) == C.sizeof(_hip.EnsEvalDesc)


def _eval_desc(hidden, dout, reward_off, n=100, X=4, U=1, E=7):
    from mbpo import _hip
    d = _hip.EnsEvalDesc()
    d.x_dim, d.u_dim, d.n, d.min_std, d.predict_delta = X, U, n, 1e-3, 1
    dims = [X + U, *hidden, dout]
    m = d.dynamics
    m.params, m.n_nets, m.n_layers, m.activation = 16, E, len(dims) - 1, _hip.ACT_IDS["swish"]
    for i, v in enumerate(dims):
        m.dims[i] = v
    m.net_stride = sum(dims[i] * dims[i + 1] + dims[i + 1] for i in range(len(dims) - 1))
    d.row_len, d.next_obs_off, d.reward_off = 2 * X + U + 2, X + U + 2, reward_off
    return d


def test_eval_workspace_query_and_argument_checks(lib):
    X, U, E = 4, 1, 7
    ws = lambda d: int(lib.mbpo_ens_eval_workspace_floats(C.byref(d)))
    fused = ws(_eval_desc((64, 64, 64), 2 * X, -1))
    assert 0 < fused < 100000                                        # two partials per (member, slot), nothing per row
    layered = ws(_eval_desc((256, 256, 256, 256), 2 * X, -1))
    # the layered path stores the shared input and target once, two hidden ping-pong buffers and y for the E members
    assert layered >= 100 * (X + U) + 100 * (X + 1) + 2 * E * 100 * 256 + E * 100 * 2 * X
    assert layered < 100 * (X + U) + 100 * (X + 1) + 2 * E * 100 * 256 + E * 100 * 2 * X + 64
    assert ws(_eval_desc((96, 32), 2 * X + 2, X + U)) > 0
    assert ws(_eval_desc((64, 64, 64), 2 * X + 2, X + U)) > 0
    assert ws(_eval_desc((64, 64, 64), 2 * X, -1, n=0)) < 0 and b"positive" in lib.mbpo_last_error()
    assert ws(_eval_desc((64, 64, 64), 2 * X, X + U)) < 0 and b"reward_off" in lib.mbpo_last_error()
    d = _eval_desc((64, 64, 64), 2 * X, -1)
    d.next_obs_off = X                                               # inside [x, u]
    assert ws(d) < 0 and b"next_obs_off" in lib.mbpo_last_error()
    # the call itself refuses null idx / metrics / workspace before any launch
    d = _eval_desc((64, 64, 64), 2 * X, -1)
    d.rows = 16
    for missing in ("idx", "metrics", "workspace"):
        d.idx, d.metrics, d.workspace = 16, 16, 16
        setattr(d, missing, None)
        assert lib.mbpo_ens_eval(C.byref(d), None) < 0 and b"null pointer" in lib.mbpo_last_error(), missing


def test_keep_best_and_pick_elites_argument_checks(lib):
    p = 16                                                           # a non-null placeholder: the checks run before any launch
    assert lib.mbpo_ens_pick_elites(p, 10, 5, p, 6, p, p, None) < 0 and b"n_elites" in lib.mbpo_last_error()
    assert lib.mbpo_ens_pick_elites(p, 10, 5, p, 0, p, p, None) < 0 and b"n_elites" in lib.mbpo_last_error()
    assert lib.mbpo_ens_pick_elites(p, 10, 0, p, 1, p, p, None) < 0 and b"n_members" in lib.mbpo_last_error()
    assert lib.mbpo_ens_pick_elites(p, 10, -3, p, 1, p, p, None) < 0
    for args in ((None, 10, 5, p, 3, p, p), (p, 10, 5, None, 3, p, p), (p, 10, 5, p, 3, None, p), (p, 10, 5, p, 3, p, None)):
        assert lib.mbpo_ens_pick_elites(*args, None) < 0 and b"null pointer" in lib.mbpo_last_error()
    assert lib.mbpo_ens_keep_best(p, p, 10, 0, p, p, 0.01, p, p, None) < 0 and b"n_members" in lib.mbpo_last_error()
    assert lib.mbpo_ens_keep_best(p, p, 10, -1, p, p, 0.01, p, p, None) < 0
    base = [p, p, 10, 4, p, p, 0.01, p, p]
    for i in (0, 1, 4, 5, 7, 8):
        args = list(base)
        args[i] = None
        assert lib.mbpo_ens_keep_best(*args, None) < 0 and b"null pointer" in lib.mbpo_last_error(), i


def test_host_api_wiring_of_the_elites():
    """EnsembleSystem.rollout_spec hands the kernels the elites as an ensemble of n_elites members (spec cached per n_elites), and the
    new fit keywords are checked before any device work."""
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, QuadraticReward
    from mbpo.systems.ensemble_system import EnsembleDynamicsParams
    X, U, E = 4, 1, 5
    dyn = EnsembleDynamics(X, U, n_members=E, device="cpu")
    system = EnsembleSystem(dyn, QuadraticReward(X, U), mode="ts1")
    sp = system.init_params(0)
    assert sp.dynamics_params.elite_idx is None and sp.dynamics_params.elite_params is None and sp.dynamics_params.holdout is None
    spec = system.rollout_spec(sp, torch.device("cpu"))
    assert spec["dyn_spec"] is dyn.spec and spec["dyn_params"] is sp.dynamics_params.params
    P = dyn.spec.n_params
    ep = torch.zeros(3 * P)
    dp = sp.dynamics_params.replace(elite_idx=torch.tensor([3, 0, 4], dtype=torch.int32), elite_params=ep)
    spec = system.rollout_spec(sp.replace(dynamics_params=dp), torch.device("cpu"))
    assert spec["dyn_params"] is ep and spec["dyn_spec"].n_nets == 3 and list(spec["dyn_spec"].dims) == list(dyn.dims)
    assert system.rollout_spec(sp.replace(dynamics_params=dp), torch.device("cpu"))["dyn_spec"] is spec["dyn_spec"]
    assert EnsembleDynamicsParams(params=ep).elite_params is None
    with pytest.raises(ValueError):
        dyn.fit(sp.dynamics_params, torch.zeros(8, 2 * X + U + 2), 1, n_elites=3)            # elites need a holdout
