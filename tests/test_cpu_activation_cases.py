"""The cases of tests/activation_cases.py, on the host alone: every case that differentiates a relu network is clear of relu's kink at its
committed seed; every case tells its activations from all-swish and from the networks' activations exchanged by at least 100 x its
tolerance (a kernel that ignored `act`, or gave one network another's, cannot pass); the oracle's own fp32-fp64 gap stays below half of
each owning tolerance (so none had to be set from a measured gap); and the shapes reach the dispatch arms the table names."""
import pytest
import torch

import activation_cases as ac
import many_tiles_cases as mt

RELU_BACKWARD = [n for n in ac.CASES if ac.has_relu_backward(n)]


def test_every_relu_backward_case_has_a_recorded_seed():
    assert sorted(ac.KINK) == sorted(RELU_BACKWARD)
    assert all(0 <= ac.KINK[n][0] < 64 for n in ac.KINK)
    # where several networks meet in one launch, they do not share an activation
    for name, c in ac.ALL.items():
        if len(c["acts"]) > 1:
            assert len(set(c["acts"])) == len(c["acts"]), name
        assert set(c["acts"]) - {"swish"}, name


@pytest.mark.parametrize("name", RELU_BACKWARD)
def test_relu_backward_case_is_clear_of_the_kink(name):
    """|z64| >= 10 G on every relu pre-activation, no sign differs between the fp32 and the fp64 oracle, and the recorded G and
    min |z| are reproduced within 2 x (they depend on the host's summation order only in their last digits)."""
    seed, G, minz = ac.KINK[name]
    k = ac.kink(name)
    print(f"{name}: seed {seed}, G {k['G']:.3g} (recorded {G:.3g}), min |z| {k['minz']:.3g} (recorded {minz:.3g}), {k['units']} relu units")
    assert k["units"] > 0 and k["flips"] == 0
    assert k["minz"] >= ac.KINK_FACTOR * k["G"]
    assert G / 2 <= k["G"] <= 2 * G and minz / 2 <= k["minz"] <= 2 * minz
    assert minz >= ac.KINK_FACTOR * G


@pytest.mark.parametrize("name", [n for n in ac.KINK if ac.KINK[n][0] > 0])
def test_the_recorded_seed_is_the_first_that_qualifies(name):
    """(the cases whose seed is not 0: every earlier seed fails the condition)"""
    seed = ac.KINK[name][0]
    assert seed > 0 and not any(ac.kink(name, s)["ok"] for s in range(seed))


def test_padded_network_relu_seed_is_clear_of_the_kink():
    """test_gpu_sac.test_sac_layered_path_equals_fused_path_on_a_padded_network under relu: its seed is the first that qualifies."""
    from test_gpu_sac import PADDED_NETWORK_CASES, padded_network_inputs
    seed = dict(PADDED_NETWORK_CASES)["relu"]
    for s in range(seed + 1):
        inp = padded_network_inputs("relu", s)
        k = ac.kink_of(lambda dtype: mt.sac_oracle(inp, dtype))
        assert k["ok"] == (s == seed), (s, k)
    assert 1.14e-6 / 2 <= k["G"] <= 2 * 1.14e-6 and 1.15e-5 / 2 <= k["minz"] <= 2 * 1.15e-5


@pytest.mark.parametrize("name", list(ac.ALL))
def test_case_discriminates_its_activations(name):
    c = ac.ALL[name]
    want = 100 * ac.REL_TOL[c["family"]]
    ref = ac.oracle(name, torch.float64)["main"].reshape(-1)
    swish = ac.oracle(name, torch.float64, acts=("swish",) * len(c["acts"]))["main"].reshape(-1)
    for gname, sl in ac.groups(name).items():
        d_swish = ac.rel_l2(swish[sl], ref[sl])
        print(f"{name} {gname}: all-swish differs by {d_swish:.3g} (needed {want:.3g})")
        assert d_swish >= want, (name, gname)
        for acts in ac.swapped(c["acts"]):      # three networks: every pairwise swap, so that crossing any two of them shows
            other = ac.oracle(name, torch.float64, acts=acts)["main"].reshape(-1)
            d_other = ac.rel_l2(other[sl], ref[sl])
            print(f"{name} {gname}: under {acts} differs by {d_other:.3g}")
            assert d_other >= want, (name, gname, acts)


@pytest.mark.parametrize("name", list(ac.ROLLOUT_CASES))
def test_rollout_case_discriminates_its_activations(name):
    """The oracle's rows of a rollout case against the same inputs under all-swish and with policy and members exchanged: apart by at
    least 100 x test_gpu_rollout's row tolerance (relative L2 over the rows)."""
    from test_gpu_rollout import _run_rollout_case
    kw = dict(ac.ROLLOUT_CASES[name])
    pa, ma = kw.pop("policy_act"), kw.pop("member_act", None)
    run = lambda p, m: _run_rollout_case(None, **kw, policy_act=p, **({} if ma is None else dict(member_act=m)))
    ref = run(pa, ma)
    want = 100 * mt.RO_TOL["rtol"]
    d_swish = ac.rel_l2(run("swish", "swish"), ref)
    d_other = ac.rel_l2(run(ma, pa) if ma is not None else run("tanh", None), ref)      # (the Pendulum has no members: the other activation)
    print(f"{name}: all-swish differs by {d_swish:.3g}, exchanged by {d_other:.3g} (needed {want:.3g})")
    assert d_swish >= want and d_other >= want


@pytest.mark.parametrize("name", list(ac.ALL))
def test_oracle_gap_is_below_half_of_the_owning_tolerance(name):
    """No tolerance of tests/test_gpu_activations.py had to be set from a measured gap: the fp32 oracle stays within half of the
    owning module's fp64 tolerance of the fp64 oracle, elementwise (or in relative L2 where the module states it so)."""
    c = ac.ALL[name]
    fam = c["family"]
    o32, o64 = ac.oracle(name, torch.float32)["main"].double(), ac.oracle(name, torch.float64)["main"]
    assert o64.dtype == torch.float64
    if fam == "tv":
        import terminal_value_cases as tvc
        tol = dict(atol=tvc.TOL64, rtol=tvc.TOL64)
    elif fam == "mlp":
        t = ac.TOL[fam]["dw"]
        tol = dict(atol=t["atol"] * max(float(o64.abs().max()), 1.0), rtol=t["rtol"])
    else:
        tol = ac.TOL[fam].get("tol64")
    if tol is None:
        gap = ac.rel_l2(o32, o64)
        print(f"{name}: relative L2 gap {gap:.3g} of {ac.TOL[fam]['rel64']:.3g}")
        assert gap < ac.TOL[fam]["rel64"] / 2
    else:
        ratio = float(((o32 - o64).abs() / (tol["atol"] + tol["rtol"] * o64.abs())).max())
        print(f"{name}: fp32-fp64 gap {ratio:.3g} of the tolerance")
        assert ratio < 0.5


# ------------------------------------------------------------------------------------------------------------------ dispatch
def test_shapes_agree_with_the_tables_dispatch_notes():
    """NOT a check of the dispatch (no query names the variant; the table's comments give the host lines each case rests on, and the
    only host evidence is the workspace count of the two-per-CU case below): the shapes are what those notes reason from — two tiles
    or more with a ragged last one, uniform kernel widths where a fused kernel is meant, wide ends exactly where a case is called
    wide, and the row counts at PPO's two thresholds."""
    for name, c in ac.CASES.items():
        fam = c["family"]
        if fam == "sac":
            assert c["B"] > 16 and c["B"] % 16, name
            assert len(set(c["hidden"])) == 1 and c["hidden"][0] in (64, 128), name
            wide = c["X"] + c["U"] > 16 or 2 * c["U"] > 16
            assert wide == ("wide" in name), name
        if fam == "ppo":
            rows = c["B"] * c["T"]
            assert rows > 16 and rows % 16, name
            layered = c["v_hidden"] is not None
            assert layered == ("layered" in name), name
            if not layered:
                assert len(set(c["hidden"])) == 1 and c["hidden"][0] in (64, 128), name
            assert (c["X"] > 16 or 2 * c["U"] > 16) == ("wide" in name), name
        if fam in ("bptt", "bptt_ts"):
            assert c["n"] >= 16 and c["E"] == 2 and len(set(c["acts"])) == 3, name
    assert ac.CASES["ppo_t1030_rt"]["T"] > 1023                               # past the fused values + GAE launch's LDS arrays
    sp2 = ac.CASES["ppo_sp2_rt"]
    assert (sp2["B"], sp2["T"]) == ac.ppo_sp2_shape(mt.REF_CUS)
    for cus in (80, 304):       # sized from another device's CU count: the same 7 trajectories, so the same kink record
        B = ac.ppo_sp2_shape(cus)[0]
        d = ac.inputs("ppo_sp2_rt", cus=cus)[2]
        assert d.shape[0] == B and mt.tiles_of(B * sp2["T"]) == cus + 1 and torch.equal(d[:7], ac.inputs("ppo_sp2_rt")[2][:7])
    assert mt.tiles_of(sp2["B"] * sp2["T"]) == mt.REF_CUS + 1 and mt.tiles_of((sp2["B"] - 1) * sp2["T"]) == mt.REF_CUS
    data = ac.inputs("ppo_sp2_rt")[2]
    assert data.shape[0] == sp2["B"] and torch.equal(data[:sp2["base"]], data[sp2["base"]:2 * sp2["base"]])
    assert (sp2["base"] * sp2["T"]) % 16 != 0                                 # the copies do not line up with the tiles


def test_ppo_workspace_query_accepts_every_ppo_case():
    """mbpo_ppo_workspace_floats (pure host arithmetic, tests/ppo_plan_cases.py) takes every PPO shape under its activations."""
    import ppo_plan_cases as pc
    from mbpo import _hip
    lib = _hip.load()
    lib.mbpo_ppo_workspace_floats.restype = __import__("ctypes").c_int64
    for name, c in ac.CASES.items():
        if c["family"] != "ppo":
            continue
        d = pc.desc(c["X"], c["U"], c["hidden"], c["v_hidden"] or c["hidden"], c["B"], c["T"],
                    policy_activation=_hip.ACT_IDS[c["acts"][0]], value_activation=_hip.ACT_IDS[c["acts"][1]])
        n, text = pc.query(lib, d)
        assert n > 0, (name, text)
        # the activation moves the layout only by the kernel it selects: under swish the 64 x 2, u = 1 shapes go to k_ppo_lean (one slab
        # per CU); past one tile per CU the generic path is the two-per-CU launch with twice the slabs, everywhere else the count is equal
        n_swish = pc.query(lib, pc.desc(c["X"], c["U"], c["hidden"], c["v_hidden"] or c["hidden"], c["B"], c["T"]))[0]
        assert (n > n_swish) if name == "ppo_sp2_rt" else (n == n_swish), (name, n, n_swish)


def test_oracle_tap_sees_every_pre_activation_and_changes_nothing():
    from oracle import nets as onets
    g = torch.Generator().manual_seed(0)
    dims = [3, 8, 8, 2]
    p, x = onets.init_mlp_flat(dims, g), torch.randn(5, 3, generator=g)
    seen = []
    with onets.tap(lambda z, act: seen.append((tuple(z.shape), act))):
        y = onets.mlp_forward(p, dims, x, "relu")
    assert seen == [((5, 8), "relu"), ((5, 8), "relu")]
    assert torch.equal(y, onets.mlp_forward(p, dims, x, "relu")) and onets._TAP is None
