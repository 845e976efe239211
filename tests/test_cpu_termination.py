"""BoxTermination and the termination plumbing without a GPU: the host formula on hand cases, the presets' shapes, the rollout spec
(keys, cache key, the consumers that drop it), the descriptor's layout, the argument check that needs no launch, and the oracle
conditions of the GPU cases (tests/termination_cases.py) — which involve no device result."""
import ctypes as C
import math
import re
import subprocess
from pathlib import Path

import pytest
import torch

import termination_cases as tc
import termination_ref as tref

ROOT = Path(__file__).resolve().parent.parent
INF, NAN = math.inf, math.nan


def test_box_termination_hand_cases():
    from mbpo.systems import BoxTermination
    t = BoxTermination([-1.0, -INF, 0.5], [1.0, INF, 2.0])
    x = torch.tensor([
        [0.0, 0.0, 1.0],        # inside
        [1.0, 5.0, 0.5],        # exactly on two bounds: closed, not done
        [-1.0, -1e30, 2.0],     # exactly on the other two
        [1.0000001, 0.0, 1.0],  # one ulp outside
        [0.0, 0.0, 0.4999999],
        [NAN, 0.0, 1.0],        # NaN fails the compares
        [0.0, NAN, 1.0],        # ... in an unbounded dimension too
        [0.0, INF, 1.0],        # +-inf is done whatever the bounds
        [0.0, -INF, 1.0],
        [0.0, 3e38, 1.0],       # large and finite in an unbounded dimension: not done
        [INF, 0.0, 1.0],
    ])
    want = torch.tensor([0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 1], dtype=torch.float32)
    got = t(x)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.equal(t(x[3]), torch.tensor(1.0)) and t(x[0]).shape == ()            # a single state
    assert torch.equal(t(x.reshape(1, 11, 3)), want.reshape(1, 11))                  # leading axes follow
    assert torch.equal(t(x.double()), want.double())
    assert torch.equal(tref.box_done(x, t.low, t.high), want)                        # the tests' own restatement agrees
    with pytest.raises(ValueError):
        t(torch.zeros(4))
    with pytest.raises(ValueError):
        BoxTermination([0.0, 0.0], [1.0])
    with pytest.raises(ValueError):
        BoxTermination([NAN], [1.0])


def test_presets():
    from mbpo.systems import BoxTermination
    ip = BoxTermination.inverted_pendulum()
    assert ip.x_dim == 4
    assert float(ip.low[1]) == pytest.approx(-0.2) and float(ip.high[1]) == pytest.approx(0.2)
    others = [0, 2, 3]
    assert bool((ip.low[others] == -INF).all()) and bool((ip.high[others] == INF).all())
    assert float(ip(torch.tensor([9.0, 0.2, 9.0, 9.0]))) == 0 and float(ip(torch.tensor([0.0, 0.21, 0.0, 0.0]))) == 1
    h = BoxTermination.hopper()
    assert h.x_dim == 11 and h.low[0] == pytest.approx(0.7) and h.high[0] == INF
    assert h.low[1] == pytest.approx(-0.2) and h.high[1] == pytest.approx(0.2)
    assert torch.equal(h.low[2:], torch.full((9,), -100.0)) and torch.equal(h.high[2:], torch.full((9,), 100.0))
    ok = torch.zeros(11)
    ok[0] = 1.0
    assert float(h(ok)) == 0
    for d, v in ((0, 0.69), (1, 0.3), (5, 101.0), (10, -101.0)):
        bad = ok.clone()
        bad[d] = v
        assert float(h(bad)) == 1
    w = BoxTermination.walker2d()
    assert w.x_dim == 17 and (float(w.low[0]), float(w.high[0]), float(w.low[1]), float(w.high[1])) == pytest.approx((0.8, 2.0, -1.0, 1.0))
    assert bool(torch.isinf(w.low[2:]).all()) and bool(torch.isinf(w.high[2:]).all())
    a, hu = BoxTermination.ant(), BoxTermination.humanoid()
    assert a.x_dim == 27 and (float(a.low[0]), float(a.high[0])) == pytest.approx((0.2, 1.0)) and bool(torch.isinf(a.low[1:]).all())
    assert hu.x_dim == 45 and (float(hu.low[0]), float(hu.high[0])) == pytest.approx((1.0, 2.0))
    assert BoxTermination.hopper(x_dim=12).x_dim == 12
    for ctor in ("inverted_pendulum", "hopper", "walker2d", "ant", "humanoid"):
        doc = getattr(BoxTermination, ctor).__doc__
        assert "nverified" in doc and "closed" in doc


def _systems(termination=None):
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, PendulumSystem, QuadraticReward
    dyn = EnsembleDynamics(4, 1, n_members=2, device="cpu")
    return EnsembleSystem(dyn, QuadraticReward(4, 1), termination=termination), PendulumSystem


def test_rollout_spec_keys_and_cache_key():
    from mbpo.systems import BoxTermination, PendulumSystem
    from mbpo.systems.termination import without_termination
    cpu = torch.device("cpu")
    plain, _ = _systems()
    sp = plain.init_params(0)
    spec0 = plain.rollout_spec(sp, cpu)
    assert "term_low" not in spec0 and "term_high" not in spec0
    assert without_termination(spec0) is spec0
    t = BoxTermination.inverted_pendulum()
    system, _ = _systems(t)
    spec = system.rollout_spec(sp, cpu)
    assert torch.equal(spec["term_low"], t.low) and torch.equal(spec["term_high"], t.high)
    assert set(spec) - set(spec0) == {"term_low", "term_high"}
    # the device tensors are cached per device: the same objects on every call (no copy inside a captured graph)
    again = system.rollout_spec(sp, cpu)
    assert again["term_low"] is spec["term_low"] and again["term_high"] is spec["term_high"]
    key = system._rspec_key
    # other bounds: another cache key, other tensors
    system.termination = BoxTermination.from_intervals(4, {1: (-0.3, 0.2)})
    spec2 = system.rollout_spec(sp, cpu)
    assert system._rspec_key != key and float(spec2["term_low"][1]) == pytest.approx(-0.3)
    system.termination = None
    assert "term_low" not in system.rollout_spec(sp, cpu) and system._rspec_key != key
    dropped = without_termination(spec)
    assert "term_low" not in dropped and "term_high" not in dropped and set(dropped) == set(spec0) and "term_low" in spec
    # PendulumSystem
    ps = PendulumSystem()
    psp = ps.init_params(0)
    assert "term_low" not in ps.rollout_spec(psp, cpu)
    k0 = ps._spec_key
    ps.termination = BoxTermination([-INF, -INF, -6.0], [INF, INF, 6.0])
    pspec = ps.rollout_spec(psp, cpu)
    assert ps._spec_key != k0 and float(pspec["term_high"][2]) == 6.0
    ps.termination = BoxTermination([-INF, -INF, -5.0], [INF, INF, 6.0])
    k1 = ps._spec_key
    assert float(ps.rollout_spec(psp, cpu)["term_low"][2]) == -5.0 and ps._spec_key != k1
    # a termination of the wrong length is refused where the system is built
    with pytest.raises(ValueError):
        PendulumSystem(termination=t)
    with pytest.raises(ValueError):
        _systems(BoxTermination([0.0], [1.0]))


def test_rollout_desc_layout_and_the_one_null_check(tmp_path):
    """term_low / term_high close mbpo_rollout_desc in the header and in the ctypes mirror, the sizes agree, a zero-initialised
    descriptor carries none, and exactly one NULL is MBPO_ERR_ARG before anything is launched."""
    from mbpo import _hip
    header = (ROOT / "include" / "mbpo_hip.h").read_text()
    body = re.search(r"typedef struct mbpo_rollout_desc \{(.*?)\} mbpo_rollout_desc;", header, re.S).group(1)
    assert re.search(r"const float \*term_low, \*term_high;\s*$", body), "term_low / term_high must be the last fields"
    assert [f[0] for f in _hip.RolloutDesc._fields_[-2:]] == ["term_low", "term_high"]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mbpo_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu\\n", sizeof(mbpo_rollout_desc), offsetof(mbpo_rollout_desc, term_low), '
                   'offsetof(mbpo_rollout_desc, term_high));\n  return 0;\n}\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    size, off_lo, off_hi = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert size == C.sizeof(_hip.RolloutDesc)
    assert off_lo == _hip.RolloutDesc.term_low.offset and off_hi == _hip.RolloutDesc.term_high.offset
    lib = _hip.load()
    d = _hip.RolloutDesc()
    assert d.term_low is None and d.term_high is None
    d.x_dim, d.u_dim, d.n_envs, d.n_steps, d.episode_length, d.action_repeat = 3, 1, 0, 0, 5, 1      # (empty: nothing to launch)
    d.term_low = 64
    assert lib.mbpo_model_rollout(C.byref(d), None) < 0 and b"term_low and term_high" in lib.mbpo_last_error()
    d.term_low, d.term_high = None, 64
    assert lib.mbpo_model_rollout(C.byref(d), None) < 0 and b"term_low and term_high" in lib.mbpo_last_error()


@pytest.mark.parametrize("name", list(tc.CASES))
def test_gpu_cases_meet_the_oracle_conditions(name):
    """What tests/test_gpu_termination.py compares against: on the oracle run alone, at most 10 % of the envs come within 2e-3 of a
    bound, at least 10 % terminate by sys_done, a truncation occurs (asserted inside tc.oracle) — and terminations that are not
    truncations are among the kept rows."""
    ref = tc.oracle(name)
    c = tc.CASES[name]
    rows = tc.env_rows(ref["rows"], name)[ref["keep"]]
    disc = c["X"] + c["U"] + 1
    assert int(((rows[..., disc] == 0) & (rows[..., -1] == 0)).sum()) >= 1
    assert ref["n_excluded"] <= 0.1 * c["N"] <= ref["n_terminating"] and ref["n_truncations"] >= 1
    # the wrapper's done is BoxTermination's
    from mbpo.systems import BoxTermination
    b = tc.build(name)
    x = torch.randn(64, c["X"], generator=torch.Generator().manual_seed(1)) * 2
    assert torch.equal(BoxTermination(b["low"], b["high"])(x), tref.box_done(x, b["low"], b["high"]))
