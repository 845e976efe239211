"""GPU: every kernel instantiation behind mbpo_model_rollout, launched once each (tests/rollout_matrix_cases.py), identified by the
test hook mbpo_debug_last_rollout_kernel and compared — every row, every column, the final obs, first_obs, steps and done — with the
composed fp32 and fp64 reference runs at the owning modules' tolerance (2e-4; 5e-4 for the x = 9 cases).  The lean and open-loop
kernels' bit-for-bit contracts are checked in every instantiation."""
import contextlib
import ctypes as C

import pytest
import torch

import rollout_matrix_cases as mc

pytestmark = pytest.mark.gpu

NAMES = list(mc.CASES)
LEAN_NAMES = [n for n in NAMES if mc.CASES[n]["kernel"]["family"] in (mc.FLEAN, mc.FOPEN)]


@contextlib.contextmanager
def lean_mode(mode: int):
    """mbpo_debug_set_rollout_lean(mode) for the block; the default afterwards, whatever happened."""
    from mbpo import _hip
    lib = _hip.load()
    lib.mbpo_debug_set_rollout_lean.argtypes = [C.c_int]
    lib.mbpo_debug_set_rollout_lean.restype = C.c_int
    try:
        assert lib.mbpo_debug_set_rollout_lean(mode) == 0
        yield
    finally:
        lib.mbpo_debug_set_rollout_lean(-1)


def _run(name, dev, knob):
    """(device results, the hook's answer) of the case under mbpo_debug_set_rollout_lean(knob)."""
    with lean_mode(knob):
        out = mc.run_device(name, dev)
        return out, mc.last_kernel()


def _same_bits(a, b, what):
    for x, y, part in zip(a, b, ("rows", "obs", "first_obs", "steps", "done")):
        assert torch.equal(x, y), f"{what}: {part} differ in {int((x != y).sum())} elements"


@pytest.mark.parametrize("name", NAMES)
def test_kernel_is_the_declared_one_and_matches_the_composed_reference(name, dev):
    b = mc.build(name)
    t = mc.tol(name)
    (rows, obs, first, steps, done), hook = _run(name, dev, mc.lean_knob(name))
    assert hook == mc.expected_hook(name), f"launched {dict(zip(mc.FIELDS, hook))}"
    cols = mc.integer_columns(b)
    refs = {dt: mc.reference(name, dt) for dt in (torch.float32, torch.float64)}
    got = dict(rows=rows, state=mc.oro.EnvState(obs, first, steps, done))
    print(f"MATRIX {name} family={mc.FAMILY_NAME[hook[0]]} tol={t:g} gap32={mc.run_gap(got, refs[torch.float32], t):.4f} "
          f"gap64={mc.run_gap(got, refs[torch.float64], t):.4f} ref_gap={mc.run_gap(refs[torch.float32], refs[torch.float64], t):.4f}")
    assert bool(torch.isfinite(rows).all())
    for dt, r in refs.items():
        st = r["state"]
        kw = dict(atol=t, rtol=t, check_dtype=False)
        torch.testing.assert_close(rows, r["rows"], msg=lambda m: f"rows vs {dt}: {m}", **kw)
        torch.testing.assert_close(obs, st.obs, msg=lambda m: f"obs vs {dt}: {m}", **kw)
        torch.testing.assert_close(first, st.first_obs, msg=lambda m: f"first_obs vs {dt}: {m}", **kw)
        # the integer-valued columns and counters: exactly
        assert torch.equal(rows[:, cols].double(), r["rows"][:, cols].double()), f"discount / truncation vs {dt}"
        assert torch.equal(steps.double(), st.steps.double()), f"steps vs {dt}"
        assert torch.equal(done.double(), st.done.double()), f"done vs {dt}"
        # first_obs holds start states, copied not computed: with a start buffer the drawn rows, without one what the caller set
        assert torch.equal(first.double(), st.first_obs.double()), f"first_obs vs {dt}"
    if not b["SB"]:
        assert torch.equal(first, b["first"])


@pytest.mark.parametrize("name", LEAN_NAMES)
def test_lean_and_openloop_contracts_hold_in_every_instantiation(name, dev):
    """k_rollout_lean equals the generic kernel bit for bit, PIPE on equals PIPE off, k_openloop_pendulum<START> equals the tile kernel."""
    k = mc.CASES[name]["kernel"]
    b = mc.build(name)
    fi = mc.FIELDS.index
    got, hook = _run(name, dev, mc.lean_knob(name))
    assert hook == mc.expected_hook(name)
    generic, ghook = _run(name, dev, 0)
    assert ghook == mc.dispatch(b, 0) and ghook[fi("family")] == mc.F64
    assert (ghook[fi("LR")], ghook[fi("TM")], ghook[fi("SB")]) == (b["LR"], int(b["TM"]), int(b["SB"]))
    _same_bits(got, generic, f"{mc.FAMILY_NAME[k['family']]} against k_model_rollout64")
    if k["family"] == mc.FLEAN and b["E"] > 0:
        other, ohook = _run(name, dev, 3 if k["PIPE"] else 2)
        assert ohook[fi("family")] == mc.FLEAN and ohook[fi("PIPE")] == 1 - k["PIPE"]
        assert ohook[:fi("PIPE")] + ohook[fi("PIPE") + 1:] == hook[:fi("PIPE")] + hook[fi("PIPE") + 1:]
        _same_bits(got, other, "PIPE on against PIPE off")
