"""GPU parity of the small streaming kernels past their grid caps, off 16-byte alignment and at the scan's lane-packing edges, against
the float64 (or bit-exact integer) oracles.  Cases, caps, predicates and tolerances: tests/stream_cases.py; that every case reaches
its branch is asserted without a GPU in tests/test_cpu_stream_cases.py.

Outputs are NaN-filled (integers: a sentinel outside the range) before the call and carry guard bands that must stay untouched, so a
loop that drops its stride (second-trip elements never written), a carry read from the wrong lane, or a padding piece zeroed in the
wrong place shows as a wrong or NaN element.  Where a Python wrapper allocates its output itself (the scans, the Philox fills,
soft_update) the case calls the C entry point the wrapper calls, with such an output, and one test per family pins the wrapper to it.

kernel: branch -> case id
  k_scan_time_major: second trip ............................. test_scan_parity[tm_2x1048869-*]
  k_scan_batch_major_v4: second trip, TL = 33 (31 idle lanes)  test_scan_parity[v4_132x20483-*]
      TL = 3 / 17 / 63 / 64, B = 1, B = RPW - 1, ragged ..... test_scan_parity[edge_12x* | edge_68x* | edge_252x* | edge_256x*]
      every step truncated / terminated, lambda = 0 .......... test_scan_parity[mask_*], test_scan_lambda_zero_is_the_td_target
  k_scan_batch_major<64>: second trip, 2 chunks .............. test_scan_parity[bm64_65x16387-*]
      5 chunks, the last of 4 steps .......................... test_scan_parity[edge_260x*]
      1 / 2 / 3 chunks at T = 40, 64 / 128 / 192 behind launch_scan's alignment test (all arrays off; only vs off)
                                                               test_scan_parity[fb_all1_* | fb_vs2_*] (also against k_scan_time_major)
  k_scan_batch_major<4> ...................................... test_scan_parity[edge_4x*]
  k_replay_insert: 16-byte path, wrap, second trip ........... test_replay_insert[big_d12]
      dword path, wrap, second trip .......................... test_replay_insert[big_d11]
      16-byte path at D % 4 != 0, with / without a wrap ...... test_replay_insert[small_d10 | small_d6]
      dword path at D % 4 == 0 (rows / data off alignment) ... test_replay_insert[rows_off_d12 | data_off_d12]
  k_replay_gather<false|true>: second trip, 16-byte / dword .. test_replay_gather_and_sample[d4_second_trip | d3_second_trip]
      dword path at D % 4 == 0 (out off alignment) ........... test_replay_gather_and_sample[d12_out_off]
  k_replay_sample_mixed: vec_real, a zero-filled piece ....... test_replay_sample_mixed[12_8]
      vec_out with real_data off alignment ................... test_replay_sample_mixed[12_8_real_off]
      dword path (out off alignment) ......................... test_replay_sample_mixed[12_11_out_off]
      full grid, ragged last workgroup; second trip .......... test_replay_sample_mixed[4_3_full_grid | 4_3_second_trip]
  k_stats_partial<0|1>, k_stats_pass1_fused: second trip ..... test_running_stats[x4 | x128 | x100 | x17]
  k_grad_stats: second trip, non-finite verdict there ........ test_adamw[grad_stats_trip], test_grad_stats_sees_a_nan_in_a_second_trip_chunk
  k_adamw_step: 16-byte body second trip, scalar tail ........ test_adamw[body_trip]
      scalar path (target off alignment), second trip ........ test_adamw[target_off]
  k_soft_update: second trip ................................. test_soft_update
  k_philox_normal_fill, k_philox_randint_fill: second trip, element index across 2^32  test_philox_fills[*]
  k_philox_fill_grouped<false|true>: second trip ............. test_philox_fill_grouped[*]
  k_normalize_rows: second trip .............................. test_policy_act
"""
import math

import numpy as np
import pytest
import torch

import real_ratio_ref as rref
import stream_cases as sc
from oracle import bptt as obptt
from oracle import philox
from oracle import replay as orep

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1


def _assert_within(tag, got, ref, tol):
    ok, worst = sc.within(got, ref, tol)
    print(f"{tag}: worst |got - ref| / (tol + tol |ref|) = {worst:.3f} at tol {tol:g}")
    assert ok, f"{tag}: {worst:.3f} of the tolerance {tol:g} (or a non-finite element)"


# ------------------------------------------------------------------------------------------------------------------ scans
def _scan(dev, name, mode, lam=sc.LAM, time_major=None, plain=False):
    """One scan through the C entry point ops.gae_scan / ops.lambda_return_scan call, inputs and NaN-filled outputs placed as the
    case says (plain: everything 16-byte aligned).  Returns the outputs time-major [T, B] as numpy."""
    from mbpo import _hip
    lib = _hip.load()
    c = sc.SCAN_CASES[name]
    T, B = c["T"], c["B"]
    tm = c.get("tm", False) if time_major is None else time_major
    mis = None if plain else c.get("mis")
    in_k = 1 if mis == "all1" else 0
    out_k = ({"all1": 1, "vs2": 2}.get(mis, 0), 1 if mis == "all1" else 0)
    i = sc.scan_inputs(name)
    put = lambda key: sc.misaligned(torch.tensor(i[key] if tm else np.ascontiguousarray(i[key].T)).to(dev), in_k)
    shape = (T, B) if tm else (B, T)
    st = _hip.current_stream_ptr()
    if mode == "lambda":
        ins = [put("rew"), put("val")]
        outs = [sc.guarded(shape, dev, out_k[0])]
        _hip.check(lib.mbpo_lambda_return_scan(ins[0].data_ptr(), ins[1].data_ptr(), outs[0].data_ptr(), B, T, sc.GAMMA, lam, int(tm), st),
                   "mbpo_lambda_return_scan")
    else:
        ins = [put("trunc"), put("term"), put("rew"), put("val"), sc.misaligned(torch.tensor(i["boot"]).to(dev), in_k)]
        outs = [sc.guarded(shape, dev, out_k[0]), sc.guarded(shape, dev, out_k[1])]
        if mode == "gae_disc":
            ins.append(put("disc"))
            _hip.check(lib.mbpo_gae_scan_discounts(*[t.data_ptr() for t in ins], outs[0].data_ptr(), outs[1].data_ptr(), B, T, lam, int(tm),
                                                   st), "mbpo_gae_scan_discounts")
        else:
            _hip.check(lib.mbpo_gae_scan(*[t.data_ptr() for t in ins], outs[0].data_ptr(), outs[1].data_ptr(), B, T, sc.GAMMA, lam, int(tm),
                                         st), "mbpo_gae_scan")
    torch.cuda.synchronize()
    if mis == "all1":
        assert all((t.data_ptr() % 16) == 4 for t in ins + outs)
    elif mis == "vs2":
        assert outs[0].data_ptr() % 16 == 8 and all(sc.aligned16(t) for t in ins + outs[1:])
    else:
        assert all(sc.aligned16(t) for t in ins + outs)
    assert all(sc.slack_untouched(t) for t in ins + outs), f"{name}/{mode}: a guard band was written"
    return [o.cpu().numpy() if tm else o.cpu().numpy().T for o in outs]


# (the mask cases have no lambda-return form: it takes no masks)
@pytest.mark.parametrize("name,mode", [(n, m) for n in sc.SCAN_CASES for m in sc.scan_modes(n)], ids=lambda v: str(v))
def test_scan_parity(dev, name, mode):
    got = _scan(dev, name, mode)
    ref = sc.scan_oracle64(name, mode)
    for k, (g, r) in enumerate(zip(got, ref)):
        _assert_within(f"{name}/{mode}/out{k}", g, r, sc.scan_tol(name, mode))
    if name.startswith("fb_"):
        # the fallback against the time-major kernel on the transposed inputs, at the module's batch-major-vs-time-major tolerance
        for k, (g, t) in enumerate(zip(got, _scan(dev, name, mode, time_major=True, plain=True))):
            _assert_within(f"{name}/{mode}/out{k} vs time-major", g, t, sc.SCAN_TOL)


@pytest.mark.parametrize("mode", ["gae", "gae_disc"])
def test_scan_lambda_zero_is_the_td_target(dev, mode):
    """T = 256 (one row on all 64 lanes) at lambda = 0: vs = (r + g (1 - term) V_{t+1} - V)(1 - trunc) + V in closed form."""
    name = "edge_256x5"
    vs, adv = _scan(dev, name, mode, lam=0.0)
    _assert_within(f"{name}/{mode}/td", vs, sc.td_target(name, mode == "gae_disc"), sc.SCAN_TOL)
    ref = sc._scan_oracle(name, mode, np.float64, lam=0.0)
    _assert_within(f"{name}/{mode}/adv", adv, ref[1], sc.SCAN_TOL)


def test_scan_wrappers_call_the_same_entry_points(dev):
    from mbpo import ops
    name = "edge_68x16"
    i = sc.scan_inputs(name)
    bm = lambda key: torch.tensor(np.ascontiguousarray(i[key].T)).to(dev)
    boot = torch.tensor(i["boot"]).to(dev)
    for mode, gamma in (("gae", sc.GAMMA), ("gae_disc", bm("disc"))):
        vs, adv = ops.gae_scan(bm("trunc"), bm("term"), bm("rew"), bm("val"), boot, gamma, sc.LAM, False)
        raw = _scan(dev, name, mode)
        assert np.array_equal(vs.cpu().numpy().T, raw[0]) and np.array_equal(adv.cpu().numpy().T, raw[1])
    out = ops.lambda_return_scan(bm("rew"), bm("val"), sc.GAMMA, sc.LAM, False)
    assert np.array_equal(out.cpu().numpy().T, _scan(dev, name, "lambda")[0])


# ----------------------------------------------------------------------------------------------------------------- replay
def _logical(data, state):
    """logical row i = physical row (i + head) % max."""
    mx = data.shape[0]
    return data.cpu()[(torch.arange(mx) + int(state[2])) % mx].numpy()


def _device_ring(dev, ring, D, base, data_k=0):
    """The ring's inserts into a guarded device buffer (mbpo_replay_insert) and into the oracle; sample_position written into both."""
    from mbpo import ops
    data = sc.misaligned(torch.zeros(ring["max"], D, device=dev), data_k)
    state = torch.zeros(4, dtype=torch.int32, device=dev)
    for c in sc.ring_chunks(ring, D, base):
        ops.replay_insert(data, state, torch.from_numpy(c).to(dev))
    state[1] = ring["sample_position"]
    q, st = sc.oracle_ring(ring, D, base)
    s = state.cpu()
    assert int(s[0]) == int(st["insert_position"]) and int(s[2]) != 0 and np.array_equal(_logical(data, s), st["data"])
    return data, state, q, st


@pytest.mark.parametrize("name", list(sc.INSERT_CASES))
def test_replay_insert(dev, name):
    from mbpo import ops
    c = sc.INSERT_CASES[name]
    mx, D = c["max"], c["D"]
    data = sc.misaligned(torch.zeros(mx, D, device=dev), c.get("data_k", 0))
    state = torch.zeros(4, dtype=torch.int32, device=dev)
    q = orep.UniformSamplingQueue(mx, D, 1)
    st, first, pos, head = q.init(), 0, 0, 0
    rng = np.random.default_rng(3)
    for j, n in enumerate(([c["held"]] if c["held"] else []) + list(c["batches"])):
        r = sc.rows(n, D, 1000.0, first)
        first += n
        under_test = j > 0 or not c["held"]
        rows_d = sc.misaligned(torch.from_numpy(r).to(dev), c.get("rows_k", 0) if under_test else 0)
        ops.replay_insert(data, state, rows_d)
        st = q.insert(st, r)
        plan = sc.insert_plan(mx, D, pos, head, n)
        pos, head = plan["pos"], plan["head"]
        s = state.cpu()
        assert (int(s[0]), int(s[1]), int(s[2]), int(s[3])) == (int(st["insert_position"]), int(st["sample_position"]), head, first), (name, j)
        assert np.array_equal(_logical(data, s), st["data"]), (name, j)                    # bit-exact logical contents
        assert sc.slack_untouched(data) and sc.slack_untouched(rows_d), (name, j)
        assert torch.equal(rows_d.cpu(), torch.from_numpy(r)), (name, j)
        idx = rng.integers(-3 * mx, 3 * mx, size=37).astype(np.int32)
        got = ops.replay_gather(data, state, torch.from_numpy(idx).to(dev)).cpu().numpy()
        assert np.array_equal(got, q.gather(st, idx)), (name, j)
    assert (data.data_ptr() % 16) == 4 * c.get("data_k", 0)


@pytest.mark.parametrize("name", list(sc.GATHER_CASES))
def test_replay_gather_and_sample(dev, name):
    from mbpo import ops
    c = sc.GATHER_CASES[name]
    D, n, mx = c["D"], c["n"], sc.GATHER_RING["max"]
    data, state, q, st = _device_ring(dev, sc.GATHER_RING, D, 1000.0)
    idx = np.random.default_rng(4).integers(-3 * mx, 3 * mx, size=n).astype(np.int32)
    out = sc.guarded((n, D), dev, c["out_k"])
    ret = ops.replay_gather(data, state, torch.from_numpy(idx).to(dev), out=out)
    assert ret.data_ptr() == out.data_ptr() and out.data_ptr() % 16 == 4 * c["out_k"]
    assert np.array_equal(out.cpu().numpy(), q.gather(st, idx))
    assert sc.slack_untouched(out) and sc.slack_untouched(data)
    out2 = sc.guarded((n, D), dev, c["out_k"])
    idx_out = sc.guarded(n, dev, 0, fill=-7, dtype=torch.int32)
    ops.replay_sample(data, state, n, sc.SEED, sc.OFF, out=out2, idx_out=idx_out)
    idx_ref, ref = q.sample(st, sc.SEED, sc.OFF, n)
    assert np.array_equal(idx_out.cpu().numpy(), idx_ref)
    assert np.array_equal(out2.cpu().numpy(), ref)
    assert idx_ref.min() >= sc.GATHER_RING["sample_position"] and idx_ref.max() < mx
    assert sc.slack_untouched(out2) and sc.slack_untouched(idx_out, -7) and sc.slack_untouched(data)


@pytest.mark.parametrize("name", list(sc.MIXED_CASES))
def test_replay_sample_mixed(dev, name):
    from mbpo import ops
    c = sc.MIXED_CASES[name]
    D, RD, mb, n_real = c["D"], c["RD"], c["mb"], c["n_real"]
    n = mb * c["G"]
    data, state, q, qs = _device_ring(dev, sc.MIXED_RINGS["model"], D, 1000.0)
    rdata, rstate, rq, rqs = _device_ring(dev, sc.MIXED_RINGS["real"], RD, -9000.0, data_k=c.get("real_k", 0))
    out = sc.guarded((n, D), dev, c.get("out_k", 0))
    idx = sc.guarded(n, dev, 0, fill=-7, dtype=torch.int32)
    ret = ops.replay_sample_mixed(data, state, rdata, rstate, n, mb, n_real, seed=sc.SEED, offset=sc.OFF, real_offset=sc.ROFF, out=out,
                                  idx_out=idx)
    assert ret.data_ptr() == out.data_ptr() and out.data_ptr() % 16 == 4 * c.get("out_k", 0) and rdata.data_ptr() % 16 == 4 * c.get("real_k", 0)
    got, gidx = out.cpu().numpy(), idx.cpu().numpy()
    ref_idx, ref = rref.mixed_rows(q, qs, rq, rqs, sc.SEED, sc.OFF, sc.ROFF, n, mb, n_real)
    assert np.array_equal(gidx, ref_idx)
    assert np.array_equal(got, ref)                                        # (no NaN left inside: array_equal would fail on one)
    is_real = (np.arange(n) % mb) < n_real
    # padded columns of the real rows are exactly 0.0 (sign included); real rows are negative, model rows positive
    assert np.array_equal(got[is_real, RD:].view(np.uint32), np.zeros((int(is_real.sum()), D - RD), np.uint32))
    assert (got[is_real, 0] < 0).all() and (got[~is_real, 0] > 0).all()
    assert sc.slack_untouched(out) and sc.slack_untouched(idx, -7) and sc.slack_untouched(data) and sc.slack_untouched(rdata)


# ----------------------------------------------------------------------------------------------------- running statistics
@pytest.mark.parametrize("name", list(sc.STATS_CASES))
def test_running_stats(dev, name):
    """Three chained updates through the fused launch chain and through the split one (what a process group runs): the same bits in
    both, an exact count, and the float64 oracle within the case's tolerance.  Workspaces start as NaN: a partial that is read
    without having been written shows."""
    from mbpo import ops
    c = sc.STATS_CASES[name]
    X, off = c["X"], c["off"]
    a = torch.from_numpy(orep.stats_init(X)).to(dev)
    b = a.clone()
    sums_a, sums_b = torch.zeros(1 + 2 * X, device=dev), torch.zeros(1 + 2 * X, device=dev)
    ws_a, ws_b = (sc.guarded(ops.stats_workspace_floats(X), dev) for _ in range(2))
    stats = orep.stats_init(X)
    for it in range(3):
        rows = sc.misaligned(torch.tensor(sc.stats_batches(name)[it]).to(dev), 0)
        ref64 = sc.stats_ref64(name, stats, it)
        ops.running_stats_update(rows, off, X, a, sums=sums_a, workspace=ws_a)                                   # fused
        ops.running_stats_update(rows, off, X, b, all_reduce=lambda t: None, sums=sums_b, workspace=ws_b)        # split
        assert torch.equal(a, b) and torch.equal(sums_a, sums_b), (name, it)
        got = a.cpu().numpy()
        assert got[0] == ref64[0] == (it + 1) * c["n"]
        _assert_within(f"{name}/update {it}", got, ref64, sc.stats_tol(name))
        assert sc.slack_untouched(rows) and sc.slack_untouched(ws_a) and sc.slack_untouched(ws_b)
        stats = got.copy()


# -------------------------------------------------------------------------------------------------------- AdamW / Polyak
@pytest.mark.parametrize("name", list(sc.ADAMW_CASES))
def test_adamw(dev, name):
    """tests/test_gpu_bptt.py::test_adamw_step_parity's scheme and per-element tolerances at the sizes of the case table: five
    chained apply_if_finite(adamw) steps with a Polyak target; the third gradient holds a NaN in its last chunk (index n - 2)."""
    from mbpo import ops
    c = sc.ADAMW_CASES[name]
    n, lr, wd, tau = c["n"], sc.ADAMW_LR, sc.ADAMW_WD, sc.ADAMW_TAU
    g = torch.Generator().manual_seed(n)
    p = torch.randn(n, generator=g)
    tgt = p.clone()
    m, v, cnt = torch.zeros(n), torch.zeros(n), 0
    opt = ops.AdamW(n, dev, lr=lr, weight_decay=wd, apply_if_finite=True)
    dp, dt = p.to(dev), sc.misaligned(tgt.to(dev), c.get("target_k", 0))
    assert dt.data_ptr() % 16 == 4 * c.get("target_k", 0) and all(sc.aligned16(t) for t in (dp, opt.m, opt.v))
    for it in range(5):
        gr = torch.randn(n, generator=g) * (10.0 ** (it - 2))
        if it == 2:
            gr[n - 2] = float("nan")
        p, m, v, cnt2 = obptt.apply_if_finite_adamw(p, gr, m, v, cnt, lr, wd)
        if cnt2 != cnt:
            tgt = (1 - tau) * tgt + tau * p
        cnt = cnt2
        dg = gr.to(dev)
        assert sc.aligned16(dg)
        opt.step(dp, dg, target=dt, tau=tau)
        torch.cuda.synchronize()
        if it == 2:
            assert math.isnan(float(opt.grad_norm))
        else:
            norm = float(gr.double().norm())
            assert abs(float(opt.grad_norm) - norm) <= 1e-5 * norm, (it, float(opt.grad_norm), norm)
        assert float(opt.count) == cnt
        torch.testing.assert_close(opt.m.cpu(), m, atol=2e-7 * float(m.abs().max()), rtol=2e-6)
        torch.testing.assert_close(opt.v.cpu(), v, atol=2e-7 * float(v.abs().max()), rtol=2e-6)
        torch.testing.assert_close(dp.cpu(), p, atol=3e-7, rtol=1e-6)
        torch.testing.assert_close(dt.cpu(), tgt, atol=3e-7, rtol=1e-6)
    assert cnt == 4 and sc.slack_untouched(dt)


def test_grad_stats_sees_a_nan_in_a_second_trip_chunk(dev):
    """n = 263 147: chunks 1024 .. 1027 are summed on the second trip of workgroups 0 .. 3 only.  A NaN there (and in the last chunk)
    must give grad_norm = NaN and skip the whole update; the finite norm of the same vector must include those chunks."""
    from mbpo import ops
    n = sc.ADAMW_CASES["grad_stats_trip"]["n"]
    g = torch.Generator().manual_seed(1)
    p0, gr = torch.randn(n, generator=g), torch.randn(n, generator=g)
    for where in (sc.GRAD_STATS_ELEMS + 5, n - 2):
        opt = ops.AdamW(n, dev, lr=1e-3, weight_decay=0.0, apply_if_finite=True)
        dp = p0.to(dev)
        big = gr.clone()
        big[where] = 3.0e4                                   # the norm is this element: dropped, the norm would be ~ sqrt(n)
        opt.step(dp, big.to(dev))
        torch.cuda.synchronize()
        norm = float(big.double().norm())
        assert abs(float(opt.grad_norm) - norm) <= 1e-5 * norm and norm > 3.0e4 and float(opt.count) == 1.0
        before = (dp.clone(), opt.m.clone(), opt.v.clone())
        bad = gr.clone()
        bad[where] = float("nan")
        opt.step(dp, bad.to(dev))
        torch.cuda.synchronize()
        assert math.isnan(float(opt.grad_norm)) and float(opt.count) == 1.0, where
        assert torch.equal(dp, before[0]) and torch.equal(opt.m, before[1]) and torch.equal(opt.v, before[2]), where


def test_soft_update(dev):
    """k_soft_update past its grid cap, bit for bit: every element equals (1 - tau)_f32 t + tau o evaluated in float32 without
    contraction, or with either product contracted into a fused multiply-add."""
    from mbpo import _hip
    from mbpo.utils.optimizer_utils import soft_update
    n, tau = sc.SOFT_UPDATE_N, 0.05
    g = torch.Generator().manual_seed(6)
    t, o = torch.randn(n, generator=g), torch.randn(n, generator=g)
    dt, do = sc.misaligned(t.to(dev), 0), sc.misaligned(o.to(dev), 0)
    out = sc.guarded(n, dev)
    _hip.check(_hip.load().mbpo_soft_update(dt.data_ptr(), do.data_ptr(), out.data_ptr(), n, tau, _hip.current_stream_ptr()), "mbpo_soft_update")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    omt, tau32 = np.float32(1.0 - tau), np.float32(tau)          # (1 - tau) formed in double on the host, then float32
    tn, on = t.numpy(), o.numpy()
    pt, po = omt * tn, tau32 * on                                # float32 products
    unfused = pt + po
    # a float32 product is exact in float64; the sum is rounded to float64 and then to float32
    fma_t = (omt.astype(np.float64) * tn.astype(np.float64) + po.astype(np.float64)).astype(np.float32)
    fma_o = (tau32.astype(np.float64) * on.astype(np.float64) + pt.astype(np.float64)).astype(np.float32)
    ok = (got == unfused) | (got == fma_t) | (got == fma_o)
    assert ok.all(), f"{int((~ok).sum())} of {n} elements match no float32 evaluation; first at {int(np.argmax(~ok))}"
    assert sc.slack_untouched(out) and sc.slack_untouched(dt) and sc.slack_untouched(do)
    assert torch.equal(soft_update(dt, do, tau), out)            # the Python entry point: the same launch


# ------------------------------------------------------------------------------------------------------------ Philox fills
@pytest.mark.parametrize("base", list(sc.FILL_BASES))
def test_philox_fills(dev, base):
    from mbpo import _hip, ops
    lib = _hip.load()
    n, eb = sc.FILL_N, sc.FILL_BASES[base]
    seed, off = 2 ** 40 + 17, (5 << 32) + 3
    elems = np.arange(n, dtype=np.uint64) + np.uint64(eb)
    assert int(elems[0]) < 2 ** 32 <= int(elems[-1])
    out = sc.guarded(n, dev)
    _hip.check(lib.mbpo_philox_normal_fill(seed & U64, off & U64, None, philox.STREAM_POLICY_NOISE, eb, n, out.data_ptr(),
                                           _hip.current_stream_ptr()), "mbpo_philox_normal_fill")
    torch.cuda.synchronize()
    np.testing.assert_allclose(out.cpu().numpy(), philox.philox_normal(seed, off, philox.STREAM_POLICY_NOISE, elems),
                               rtol=sc.NORMAL_TOL, atol=sc.NORMAL_TOL)
    assert sc.slack_untouched(out)
    assert torch.equal(ops.philox_normal(n, seed, off, stream=philox.STREAM_POLICY_NOISE, elem_base=eb), out)
    lo, hi = -3, 1000
    iout = sc.guarded(n, dev, 0, fill=-777, dtype=torch.int32)
    _hip.check(lib.mbpo_philox_randint_fill(seed & U64, off & U64, None, philox.STREAM_MEMBER, eb, n, lo, hi, iout.data_ptr(),
                                            _hip.current_stream_ptr()), "mbpo_philox_randint_fill")
    torch.cuda.synchronize()
    assert np.array_equal(iout.cpu().numpy(), philox.philox_randint(seed, off, philox.STREAM_MEMBER, elems, lo, hi))
    assert sc.slack_untouched(iout, -777)
    assert torch.equal(ops.philox_randint(n, lo, hi, seed, off, stream=philox.STREAM_MEMBER, elem_base=eb), iout)


@pytest.mark.parametrize("as_int", [0, 1])
def test_philox_fill_grouped(dev, as_int):
    """out[(s B + b) G + j] = draw(seeds[b], s G + j) at n = S B G past the grid cap: every problem equals its own single fill, and the
    oracle's stream."""
    from mbpo import _hip, ops
    lib = _hip.load()
    S, B, G, seeds = sc.GROUPED["S"], sc.GROUPED["B"], sc.GROUPED["G"], sc.GROUPED["seeds"]
    off, lo, hi = 9, 0, 7
    sd = torch.tensor([s - (1 << 64) if s >= 1 << 63 else s for s in seeds], dtype=torch.int64, device=dev)
    out = sc.guarded(S * B * G, dev, 0, fill=-777, dtype=torch.int32) if as_int else sc.guarded(S * B * G, dev)
    stream = _hip.STREAM_MEMBER if as_int else _hip.STREAM_MODEL_NOISE
    _hip.check(lib.mbpo_philox_fill_grouped(sd.data_ptr(), off, stream, S, B, G, as_int, lo, hi, out.data_ptr(), None),
               "mbpo_philox_fill_grouped")
    torch.cuda.synchronize()
    assert sc.slack_untouched(out, -777 if as_int else sc.NAN)
    got = out.reshape(S, B, G)
    elems = np.arange(S * G, dtype=np.uint64)
    for b, s in enumerate(seeds):
        if as_int:
            want = ops.philox_randint(S * G, lo, hi, seed=s, offset=off, stream=stream).reshape(S, G)
            assert np.array_equal(got[:, b].cpu().numpy().reshape(-1), philox.philox_randint(s, off, stream, elems, lo, hi)), b
        else:
            want = ops.philox_normal(S * G, seed=s, offset=off, stream=stream).reshape(S, G)
            np.testing.assert_allclose(got[:, b].cpu().numpy().reshape(-1), philox.philox_normal(s, off, stream, elems), rtol=sc.NORMAL_TOL,
                                       atol=sc.NORMAL_TOL)
        assert torch.equal(got[:, b], want), b


# -------------------------------------------------------------------------------------------------------------- policy_act
def test_policy_act(dev):
    """n x = 525 488 elements through k_normalize_rows (cap 524 288): the last 300 rows are normalised on a second trip.  The
    workspace starts as NaN, so a row that is not normalised gives NaN actions."""
    from mbpo import ops
    i, o64 = sc.act_inputs(), sc.act_oracle64()
    n, X, U = sc.ACT["n"], sc.ACT["X"], sc.ACT["U"]
    spec = ops.MlpSpec(sc.ACT["dims"])
    d = {k: v.to(dev) for k, v in i.items()}
    ws = sc.guarded(n * (X + 2 * U), dev)
    act, raw, lp = ops.policy_act(d["ppar"], spec, d["obs"], d["nm"], d["ns"], noise=d["noise"], want_extras=True, workspace=ws)
    torch.cuda.synchronize()
    assert sc.slack_untouched(ws)
    _assert_within("policy_act/raw", raw.cpu().numpy(), o64["raw"].numpy(), sc.act_tol("raw"))
    _assert_within("policy_act/action", act.cpu().numpy(), o64["action"].numpy(), sc.act_tol("action"))
    _assert_within("policy_act/log_prob", lp.cpu().numpy(), o64["log_prob"].numpy(), sc.act_tol("log_prob"))
    ws2 = sc.guarded(n * (X + 2 * U), dev)
    mode = ops.policy_act(d["ppar"], spec, d["obs"], d["nm"], d["ns"], deterministic=True, workspace=ws2)
    torch.cuda.synchronize()
    assert sc.slack_untouched(ws2)
    _assert_within("policy_act/mode", mode.cpu().numpy(), o64["mode"].numpy(), sc.act_tol("mode"))
