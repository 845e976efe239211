"""The streaming-kernel case table (tests/stream_cases.py) checked without a GPU:

* every case reaches the branch it is there for, by the arithmetic of the launch it restates: more items than the capped grid
  holds, not a multiple of the cap, a ragged last workgroup; the kernel `launch_scan` picks; the 16-byte or the dword path;
* the float32 oracle stays within a quarter of each tolerance the GPU module uses against the float64 oracle, and every widened
  tolerance is 4 x its recorded gap rounded up to one digit, recorded from a gap that is still current and was needed;
* the inputs of the bit-exact (replay) cases are distinct rows of the stated form, so a wrong source row cannot compare equal.
"""
import numpy as np
import pytest
import torch

import stream_cases as sc
from oracle import replay as orep


def _check_tol(tag, g, module_tol, widened, key):
    """The rule under "Tolerances" in stream_cases.py, on the references alone."""
    print(f"{tag}: float32-vs-float64 oracle gap {g:.3g} = {g / module_tol:.2f} of the module's tolerance {module_tol:g}")
    if key in widened:
        rec, tol = widened[key]
        assert rec > module_tol / 4, f"{tag}: recorded gap {rec:g} did not need a widened tolerance"
        assert tol == pytest.approx(sc.round_up_1sig(4 * rec), rel=1e-9), f"{tag}: {tol:g} is not 4 x {rec:g} rounded up to one digit"
        assert 0.5 * rec <= g <= rec, f"{tag}: the recorded gap {rec:g} is out of date (measured {g:.3g})"
    else:
        tol = module_tol
    assert g <= tol / 4, f"{tag}: the float32 oracle uses {g / tol:.3f} of the tolerance {tol:g} (limit 0.25)"


# ------------------------------------------------------------------------------------------------------------------ scans
@pytest.mark.parametrize("name", list(sc.SCAN_CASES))
def test_scan_case(name):
    c = sc.SCAN_CASES[name]
    T, B = c["T"], c["B"]
    k = sc.scan_kernel(T, sc.scan_aligned(c), c.get("tm", False))
    groups = sc.scan_groups(B, k)
    if c.get("trip"):
        assert groups > k["waves"] and groups % k["waves"] != 0 and groups % 4 != 0
        assert k["kernel"] == {"tm_2x1048869": "tm", "v4_132x20483": "v4", "bm64_65x16387": "bm"}[name]
        assert name != "bm64_65x16387" or (k["tp"], k["chunks"]) == (64, 2)
        assert name != "v4_132x20483" or (k["tl"], k["rpw"], k["idle"]) == (33, 1, 31)
    else:
        assert groups <= k["waves"]
    if name.startswith("edge_"):
        want = {4: ("bm", 16), 12: ("v4", 21), 68: ("v4", 3), 252: ("v4", 1), 256: ("v4", 1), 260: ("bm", 1)}[T]
        assert (k["kernel"], k["rpw"]) == want
        if k["kernel"] == "v4":
            assert (k["tl"], k["idle"]) == {12: (3, 1), 68: (17, 13), 252: (63, 1), 256: (64, 0)}[T]
        else:
            assert (k["tp"], k["chunks"]) == {4: (4, 1), 260: (64, 5)}[T] and (T != 260 or T - 4 * 64 == 4)
    if name.startswith("fb_"):
        assert sc.scan_kernel(T, True)["kernel"] == "v4" and (k["kernel"], k["tp"]) == ("bm", 64)
        assert k["chunks"] == {40: 1, 64: 1, 128: 2, 192: 3}[T] and groups % 4 != 0
    if name.startswith("mask_"):
        i = sc.scan_inputs(name)
        assert (i["trunc"] == (c["mask"] == "trunc")).all() and (i["term"] == (c["mask"] == "term")).all()
        assert k["kernel"] == "v4" and k["tl"] == 64
    for mode in sc.scan_modes(name):
        o32, o64 = sc.scan_oracle32(name, mode), sc.scan_oracle64(name, mode)
        assert o64[0].shape == (T, B) and o64[0].dtype == np.float64 and o32[0].dtype == np.float32
        g = max(sc.gap(a, b) for a, b in zip(o32, o64))
        _check_tol(f"{name}/{mode}", g, sc.SCAN_TOL, sc.SCAN_WIDENED, (name, mode))
    assert not [key for key in sc.SCAN_WIDENED if key[0] == name and key[1] not in sc.scan_modes(name)]


def test_scan_edges_cover_every_b():
    for T in (4, 12, 68, 252, 256, 260):
        rpw = sc.scan_kernel(T, True)["rpw"]
        bs = sorted(c["B"] for n, c in sc.SCAN_CASES.items() if n.startswith("edge_") and c["T"] == T)
        assert bs[0] == 1 and (rpw == 1 or rpw - 1 in bs)
        ragged = bs[-1]
        assert -(-ragged // rpw) % 4 != 0 and (rpw == 1 or ragged % rpw != 0) and ragged > 4 * rpw
    assert not set(sc.SCAN_WIDENED) - {(n, m) for n in sc.SCAN_CASES for m in sc.SCAN_MODES}


def test_td_target_is_the_oracle_at_lambda_zero():
    name = "edge_256x5"
    for mode, disc in (("gae", False), ("gae_disc", True)):
        vs, _ = sc._scan_oracle(name, mode, np.float64, lam=0.0)
        np.testing.assert_allclose(vs, sc.td_target(name, disc), rtol=1e-13, atol=1e-13)


# ----------------------------------------------------------------------------------------------------------------- replay
def test_rows_are_distinct_and_exact():
    r = sc.rows(330_000, 12, 1000.0)
    assert r.dtype == np.float32 and (np.diff(r[:, 0]) == 16).all() and (np.diff(r, axis=1) == 1).all()
    assert r[7, 3] == 1000.0 + 16 * 7 + 3 and sc.rows(5, 3, -9000.0, first=10)[2, 1] == -9000.0 + 16 * 12 + 1
    for ring, D, base in ((sc.GATHER_RING, 4, 1000.0), (sc.MIXED_RINGS["real"], 3, -9000.0)):
        allr = np.concatenate(sc.ring_chunks(ring, D, base))
        assert np.unique(allr, axis=0).shape[0] == allr.shape[0] == sum(ring["chunks"])


@pytest.mark.parametrize("name", list(sc.INSERT_CASES))
def test_insert_case(name):
    c = sc.INSERT_CASES[name]
    plans = sc.insert_plans(c)
    assert len(plans) == len(c["batches"])
    wraps = [0 < p["n1"] < p["total"] // c["D"] for p, _, _ in plans]
    vecs = [v for _, v, _ in plans]
    trips = [t for _, _, t in plans]
    if name == "big_d12":
        assert vecs == [True] and wraps == [True] and trips == [2] and (plans[0][0]["total"] // 4) % 256 != 0
    if name == "big_d11":
        assert vecs == [False] and wraps == [True] and trips == [2] and plans[0][0]["total"] % 256 != 0
        # with 150 000 held rows: no wrap, 16-byte path, one trip — not the branch this case is for
        p = sc.insert_plan(c["max"], c["D"], 150_000, 0, 50_000)
        assert sc.insert_takes_vec(p, c["D"]) and p["n1"] == 50_000 and sc.insert_trips(p, True) == 1
    if name.startswith("small_"):
        assert c["D"] % 4 != 0 and all(vecs)
        assert any(w for w in wraps) and any(not w for w in wraps)
    if name.endswith("_off_d12"):
        assert c["D"] % 4 == 0 and not any(vecs) and any(wraps)
        assert all(v for _, v, _ in sc.insert_plans(dict(c, data_k=0, rows_k=0)))          # alignment alone decides
    # the oracle's state follows the restated plan (insert_position and the head it implies)
    q = orep.UniformSamplingQueue(c["max"], c["D"], 1)
    st, pos, head = q.init(), 0, 0
    for n in ([c["held"]] if c["held"] else []) + list(c["batches"])[:3]:
        p = sc.insert_plan(c["max"], c["D"], pos, head, n)
        pos, head = p["pos"], p["head"]
        st = q.insert(st, np.zeros((n, c["D"]), np.float32))
        assert int(st["insert_position"]) == pos


@pytest.mark.parametrize("name", list(sc.GATHER_CASES))
def test_gather_case(name):
    c = sc.GATHER_CASES[name]
    rb = sc.gather_rows_per_block(c["D"])
    vec = sc.gather_takes_vec(c["D"], out_k=c["out_k"])
    if name.endswith("second_trip"):
        assert rb == 256 and sc.gather_trips(c["n"], c["D"]) == 2 and c["n"] % (sc.GATHER_BLOCKS * rb) != 0 and c["n"] % rb != 0
        assert vec == (c["D"] == 4)
    else:
        assert c["D"] % 4 == 0 and not vec and sc.gather_takes_vec(c["D"]) and c["n"] > rb and c["n"] % rb != 0
    q, st = sc.oracle_ring(sc.GATHER_RING, c["D"], 1000.0)
    assert int(st["insert_position"]) == sc.GATHER_RING["max"] and int(st["sample_position"]) > 0
    assert sum(sc.GATHER_RING["chunks"]) > sc.GATHER_RING["max"]                             # wrapped: head != 0


@pytest.mark.parametrize("name", list(sc.MIXED_CASES))
def test_mixed_case(name):
    c = sc.MIXED_CASES[name]
    D, RD, mb, n = c["D"], c["RD"], c["mb"], c["mb"] * c["G"]
    rb = sc.gather_rows_per_block(D)
    vec_out = sc.gather_takes_vec(D, out_k=c.get("out_k", 0))
    vec_real = RD % 4 == 0 and c.get("real_k", 0) == 0
    want = {"12_8": (True, True), "12_8_real_off": (True, False), "12_11_out_off": (False, False), "4_3_full_grid": (True, False),
            "4_3_second_trip": (True, False)}[name]
    assert (vec_out, vec_real) == want and RD < D and 0 < c["n_real"] < mb
    assert name != "12_8" or D - RD >= 4                                  # a whole 16-byte piece of a real row is padding
    trips = sc.gather_trips(n, D)
    if name == "4_3_full_grid":
        assert n == sc.GATHER_BLOCKS * rb - 1 == 1_048_575 and trips == 1
    elif name == "4_3_second_trip":
        cap = sc.GATHER_BLOCKS * rb
        assert trips == 2 and n % rb != 0
        inside = [b for b in range(mb, n, mb) if b >= cap]
        assert inside and all(b % rb != 0 for b in inside) and inside[0] - cap < rb       # real rows in workgroup 0's second iteration
    else:
        assert n > rb and n % rb != 0 and any(b % rb != 0 for b in range(mb, n, mb))
    for ring in sc.MIXED_RINGS.values():
        assert sum(ring["chunks"]) > ring["max"] and ring["sample_position"] > 0


# ----------------------------------------------------------------------------------------------------- running statistics
@pytest.mark.parametrize("name", list(sc.STATS_CASES))
def test_stats_case(name):
    c = sc.STATS_CASES[name]
    per_trip = sc.stats_rows_per_trip(c["X"])
    rpp = 256 // c["X"]
    assert c["n"] > per_trip and c["n"] % per_trip != 0 and c["off"] + c["X"] <= c["D"]
    assert (rpp, 256 - rpp * c["X"]) == {"x4": (64, 0), "x128": (2, 0), "x100": (2, 56), "x17": (15, 1)}[name]
    stats, g = orep.stats_init(c["X"]), 0.0
    for it in range(3):
        ref64 = sc.stats_ref64(name, stats, it)
        b = sc.stats_batches(name)[it][:, c["off"]:c["off"] + c["X"]]
        stats = orep.stats_update(stats, b, dtype=np.float32)
        assert stats[0] == ref64[0] == (it + 1) * c["n"]
        g = max(g, sc.gap(stats, ref64))
    _check_tol(name, g, sc.STATS_TOL, sc.STATS_WIDENED, name)


# ------------------------------------------------------------------------------------- AdamW, Polyak, fills, policy_act
def test_optimizer_and_fill_sizes():
    a = sc.ADAMW_CASES
    n = a["grad_stats_trip"]["n"]
    assert sc.second_trip(n, sc.GRAD_STATS_ELEMS) and n < sc.ADAMW_THREADS and n % 4 == 3
    n = a["body_trip"]["n"]
    assert sc.second_trip(sc.adamw_quads(a["body_trip"]), sc.ADAMW_THREADS) is False          # 256 quads: a whole workgroup
    assert sc.adamw_quads(a["body_trip"]) == sc.ADAMW_THREADS + 256 and n % 4 == 2 and sc.second_trip(n, sc.GRAD_STATS_ELEMS)
    n = a["target_off"]["n"]
    assert sc.adamw_quads(a["target_off"]) == 0 and sc.second_trip(n, sc.ADAMW_THREADS)
    assert sc.second_trip(sc.SOFT_UPDATE_N, sc.SOFT_UPDATE_THREADS)
    assert sc.second_trip(sc.FILL_N, sc.FILL_THREADS)
    b = sc.FILL_BASES
    assert 0 < 2 ** 32 - b["wrap_in_first_trip"] < sc.FILL_THREADS < 2 ** 32 - b["wrap_in_second_trip"] < sc.FILL_N
    g = sc.GROUPED
    assert sc.second_trip(g["S"] * g["B"] * g["G"], sc.FILL_THREADS) and len(g["seeds"]) == g["B"] and len(set(g["seeds"])) == g["B"]
    assert sc.second_trip(sc.ACT["n"] * sc.ACT["X"], sc.NORMALIZE_THREADS)


def test_policy_act_case():
    o32, o64 = sc.act_oracle(torch.float32), sc.act_oracle64()
    for what in ("mode", "raw", "action", "log_prob"):
        module = sc.ACT_LP_TOL if what == "log_prob" else sc.ACT_TOL
        _check_tol(f"policy_act/{what}", sc.gap(o32[what].numpy(), o64[what].numpy()), module, sc.ACT_WIDENED, what)


def test_misaligned_helper():
    t = torch.arange(10, dtype=torch.float32).reshape(2, 5)
    for k in (1, 2, 3):
        v = sc.misaligned(t, k)
        assert v.is_contiguous() and torch.equal(v, t) and v.data_ptr() % 16 == 4 * k and sc.slack_untouched(v)
        whole = torch.empty(0).set_(v.untyped_storage())
        whole[v.storage_offset() - 1] = 0.0
        assert not sc.slack_untouched(v)
    i = sc.guarded(7, "cpu", k=0, fill=-7, dtype=torch.int32)
    assert sc.aligned16(i) and (i == -7).all() and sc.slack_untouched(i, -7)
    whole = torch.empty(0, dtype=torch.int32).set_(i.untyped_storage())
    whole[i.storage_offset() + 7] = 3
    assert not sc.slack_untouched(i, -7)
