"""CPU: the case table of tests/rollout_matrix_cases.py — one case per kernel instantiation behind mbpo_model_rollout — checked without
a device: the table is the enumeration, every case's inputs make the dispatch pick its kernel, the run-time options meet every switch
value, every seed is the first that passes the conditions on the reference runs, and every switch that is on does something."""
import collections

import pytest

import rollout_matrix_cases as mc

NAMES = list(mc.CASES)


def test_enumeration_counts_the_launch_nests():
    ks = mc.kernels()
    per = collections.Counter(k["family"] for k in ks)
    assert (per[mc.F64], per[mc.FWIDE], per[mc.FLEAN], per[mc.FOPEN]) == (60, 36, 56, 2)
    names = [mc.kernel_name(k) for k in ks]
    assert len(set(names)) == len(names) == 154
    assert len({tuple(k[f] for f in mc.FIELDS) for k in ks}) == 154
    # the combinations the nests leave out
    for k in ks:
        assert not (k["TA"] and k["HL"])
        assert not (k["family"] == mc.F64 and k["TA"] and k["W"])
        assert not (k["family"] == mc.FLEAN and k["PEND"] and k["LR"])
    assert len(mc.NO_INSTANTIATION) == 4


def test_table_declares_exactly_the_reachable_kernels():
    want = {mc.kernel_name(k) for k in mc.kernels()} - set(mc.UNREACHABLE)
    assert set(mc.UNREACHABLE) <= {mc.kernel_name(k) for k in mc.kernels()}
    assert all(reason for reason in mc.UNREACHABLE.values())
    # a case is declared by its seed: a kernel without one, or a seed without a kernel, fails here
    assert set(mc.SEEDS) == want == set(mc.CASES)
    assert all(isinstance(s, int) and 0 <= s < 64 for s in mc.SEEDS.values())


@pytest.mark.parametrize("name", NAMES)
def test_inputs_pick_the_declared_kernel(name):
    c = mc.CASES[name]
    b = mc.build(name)
    k = c["kernel"]
    assert mc.dispatch(b, mc.lean_knob(name)) == mc.expected_hook(name)
    # the options are the rule's, and each is one the host accepts for this kernel
    assert c["opt"] == mc.options(k)
    assert all(c["opt"][o] in mc.option_values(k)[o] for o in mc.OPTIONS)
    # the shapes the edges need: a ragged last tile, resets inside the launch, more than 16 columns where W is on
    assert mc.N == 40 and mc.L == 3 and b["S"] in (4, 5) and b["steps0"].tolist() == [float(i % 3) for i in range(40)]
    assert 1 <= int(b["done0"].sum()) < mc.N
    if k["family"] == mc.F64:
        assert b["E"] == 5 and (b["ddims"][-1] > 16) == bool(k["W"]) and (not (k["W"] and k["HL"]) or b["A"] == 10)
    if k["family"] == mc.FWIDE:
        assert b["E"] == {128: 3, 256: 2}[k["H"]]
    if k["family"] == mc.FLEAN:
        assert b["X"] in (2, 3, 4) and b["A"] == 1
        # the contracts' twins: the generic kernel under knob 0, the other PIPE under the other knob
        assert mc.dispatch(b, 0)[0] == mc.F64
        if b["E"] > 0:
            other = mc.dispatch(b, 3 if k["PIPE"] else 2)
            assert other[0] == mc.FLEAN and other[mc.FIELDS.index("PIPE")] == 1 - k["PIPE"]
    if k["family"] == mc.FOPEN:
        assert mc.dispatch(b, 0)[0] == mc.F64


def test_every_option_value_meets_every_switch_value():
    """Wherever the host accepts the pair: (switch = value) x (option = value) is needed when some kernel with that switch value accepts
    that option value, and some case of the table must then have both."""
    need, have = set(), set()
    for k in mc.kernels():
        for f in mc.FIELDS:
            for o, values in mc.option_values(k).items():
                need |= {(f, k[f], o, v) for v in values}
    for c in mc.CASES.values():
        for f in mc.FIELDS:
            have |= {(f, c["kernel"][f], o, v) for o, v in c["opt"].items()}
    assert not (need - have), sorted(need - have)
    # and the option values are really all there
    for o, n in (("mode", 4), ("noise", 2), ("AR", 2), ("ppo", 2), ("norm", 2), ("philox", 2), ("box", 2)):
        assert len({c["opt"][o] for c in mc.CASES.values()}) == n


@pytest.mark.parametrize("name", NAMES)
def test_seed_is_the_first_that_passes_and_every_switch_is_at_work(name):
    b = mc.build(name)
    assert mc.first_seed(name) == mc.SEEDS[name]
    e = mc.examine(name)
    t = mc.tol(name)
    print(f"MATRIX-REF {name} ref_gap={e['ref_gap']:.4f} of tol {t:g}")
    assert e["ok"], [k for k, v in e["cond"].items() if not v]
    assert e["near"] == 0 and e["excluded"] == 0.0 and e["ints_agree"]
    assert e["ref_gap"] <= 0.25                      # fp32 and fp64 within a quarter of the tolerance: three quarters are the kernel's
    if b["TM"]:
        assert e["terminated"] >= 4
    if b["SB"]:
        assert e["draws"] >= 1 and e["first_changed"]
    if b["HL"]:
        assert e["hal_mean"] > 100 * t
    if b["TA"]:
        assert e["holds"] == [1, 2, 3] and e["int_dist"] >= 2e-3
    if b["LR"] != mc.LR_FORMULA:
        assert e["reward_effect"] > 100 * t
    for fl in mc.flips(name):
        assert e["flip_" + fl[0]] > 100 * t
    assert {f[0] for f in mc.flips(name)} >= {"TM", "SB"}


def test_a_changed_case_is_noticed():
    """What the table's tests rest on: other inputs pick another kernel, and the conditions can fail."""
    name = "lean_x3_pend0_pipe1_lr0_tm1_sb0"
    b = dict(mc.build(name))
    assert mc.dispatch(dict(b, AR=2), mc.lean_knob(name))[0] == mc.F64
    assert mc.dispatch(dict(b, TM=False), mc.lean_knob(name)) != mc.expected_hook(name)
    assert mc.dispatch(b, 3) != mc.expected_hook(name)
    assert any(not mc.examine(n, s)["ok"] for n, first in mc.SEEDS.items() for s in range(first))
