"""The scratch contract of include/mbpo_hip.h, entry point by entry point (tests/scratch_contract_cases.py holds the table): whatever a
caller leaves in a `workspace`, and whatever an `out` buffer held before, every result is bit for bit what the same call gives on
zeroed memory, and nothing is written outside the sizes the header states.

There is no tolerance in this file.  The only oracle is the library's own run on zeroed workspace and zeroed outputs (the control);
the parity modules (test_gpu_ppo.py, test_gpu_bptt.py, ...) tie that run to the float64 oracles.  Per case:
  control        two zero-memory runs agree bit for bit (otherwise nothing below means anything);
  dirty scratch  the workspace pre-filled with quiet-NaN bits and with 3.0e38 (finite: it survives a `cond ? x : 0` select but wrecks
                 any sum it enters); integer workspaces with -1 and 0x7FFFFFFF;
  second hand    case B on the buffer case A of the same entry point just used, untouched in between;
  guard bands    [64 elements | exactly the stated size | 256 elements] around the workspace and around every `out` buffer (and the
                 `inout` ones), the guards filled with a sentinel that must survive (64 floats in front keep the payload
                 256-byte aligned);
  poisoned out   every `out` buffer pre-filled with NaN bits, `inout` ones at their proper initial state.
Elements of an `out` buffer that a kernel legitimately never writes would be excluded by the explicit index lists of the case table
(Case.unwritten, from the header) and never by a mask computed from a result; every list is empty today, and the check below keeps
any future list under 1 % of its buffer.

Out of scope: the SAC entry points (the header states their zero requirement; the control block is state) and the mbpo_p2p_* regions.
Every pointer stays valid and aligned; nothing is read or written outside the test's own allocations.
"""
import contextlib
import ctypes as C

import pytest
import torch

import scratch_contract_cases as scc

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000
SENTINEL = 0x5EA7BEEF
FRONT, BACK = 64, 256                       # guard elements (4 bytes each): 256 B in front, 1 KiB behind
FLOAT_FILLS = {"nan": NAN_BITS, "3e38": None}
INT_FILLS = {"minus1": -1, "int_max": 0x7FFFFFFF}

_DT = {"float32": torch.float32, "int32": torch.int32}


def _raw(n, dev, bits=0):
    """n 4-byte elements holding the int32 pattern `bits`."""
    return torch.full((max(int(n), 1),), bits, dtype=torch.int32, device=dev)


def _typed(raw, dtype):
    return raw if dtype == torch.int32 else raw.view(dtype)


def _fill_value(t, name):
    if name == "3e38":
        t.view(torch.float32).fill_(3.0e38)
    else:
        t.fill_({**FLOAT_FILLS, **INT_FILLS}[name])


class Mem:
    """Where a case's `out` / `inout` buffers come from.  mode: zero | poison | guard."""

    def __init__(self, dev, mode="zero"):
        self.dev, self.mode, self.guarded, self.outs = dev, mode, [], {}

    def out(self, name, n, dtype=torch.float32):
        n = int(n)
        if self.mode == "guard":
            full = _raw(FRONT + n + BACK, self.dev, SENTINEL)
            full[FRONT:FRONT + n] = 0
            self.guarded.append((name, full, n))
            t = full[FRONT:FRONT + n]
        else:
            t = _raw(n, self.dev, NAN_BITS if self.mode == "poison" else 0)[:n]
        self.outs[name] = n
        return _typed(t, dtype)

    def inout(self, name, initial):
        """A private copy of the initial state; between guard bands too in guard mode (state is not to be overrun either)."""
        initial = initial.detach().contiguous()
        if self.mode != "guard":
            return initial.clone()
        n = initial.numel()
        full = _raw(FRONT + n + BACK, self.dev, SENTINEL)
        t = _typed(full[FRONT:FRONT + n], initial.dtype).view(initial.shape)
        t.copy_(initial)
        self.guarded.append((name, full, n))
        return t

    def check_guards(self, what):
        for name, full, n in self.guarded:
            assert bool((full[:FRONT] == SENTINEL).all()), f"{what}: write in front of `{name}`"
            assert bool((full[FRONT + n:] == SENTINEL).all()), f"{what}: write past the {n} stated elements of `{name}`"


@contextlib.contextmanager
def _knob(case):
    if case.knob is None:
        yield
        return
    from mbpo import _hip
    fn = getattr(_hip.load(), case.knob[0])
    fn.argtypes, fn.restype = [C.c_int], C.c_int
    try:
        assert fn(case.knob[1]) == 0
        yield
    finally:
        assert fn(-1) == 0


def _host(res):
    """Every out / inout tensor on the host, as int32 bit patterns."""
    return {k: v.detach().contiguous().view(-1).view(torch.int32).cpu().clone() for k, v in res.items()}


def _run(case, dev, ws_fill=None, mem_mode="zero", guard_ws=False, ws=None):
    """One run of `case`: the workspace zeroed, pre-filled (ws_fill), guarded, or handed in (`ws`, raw int32: second-hand)."""
    with _knob(case):
        need = case.need()
        mem = Mem(dev, mem_mode)
        full = None
        if case.ws_dtype is None:
            view = None
        elif ws is not None:
            assert ws.numel() >= need
            view = _typed(ws, _DT[case.ws_dtype])
        elif guard_ws:
            full = _raw(FRONT + need + BACK, dev, SENTINEL)
            full[FRONT:FRONT + need] = 0
            view = _typed(full[FRONT:FRONT + max(need, 1)], _DT[case.ws_dtype])
        else:
            raw = _raw(need, dev, 0)
            if ws_fill is not None:
                _fill_value(raw, ws_fill)
            view = _typed(raw, _DT[case.ws_dtype])
        res = case.run(dev, view, mem)
        torch.cuda.synchronize()
        if full is not None:
            assert bool((full[:FRONT] == SENTINEL).all()), f"{case.id}: write in front of the workspace"
            assert bool((full[FRONT + need:] == SENTINEL).all()), f"{case.id}: write past the {need} elements the size query states"
        mem.check_guards(case.id)
        return _host(res), mem


_CONTROL = {}


def _control(case, dev):
    """The zero-memory result, computed once per case and shared (never modified)."""
    if case.id not in _CONTROL:
        _CONTROL[case.id] = _run(case, dev)[0]
    return _CONTROL[case.id]


def _assert_same(got, ref, what, skip=None):
    assert got.keys() == ref.keys()
    for k in ref:
        a, b = got[k], ref[k]
        assert a.shape == b.shape, f"{what}: `{k}` changed size"
        if skip and skip.get(k):
            keep = torch.ones(a.numel(), dtype=torch.bool)
            keep[torch.tensor(skip[k], dtype=torch.long)] = False
            a, b = a[keep], b[keep]
        if not torch.equal(a, b):
            bad = (a != b).nonzero().flatten()
            raise AssertionError(f"{what}: `{k}` differs from the zero-memory run in {bad.numel()} of {a.numel()} elements, first at {bad[:8].tolist()}")


IDS = sorted(scc.CASES)
WS_IDS = [i for i in IDS if scc.CASES[i].ws_dtype is not None]


@pytest.mark.parametrize("cid", IDS)
def test_control_is_deterministic(dev, cid):
    case = scc.CASES[cid]
    first = _control(case, dev)
    again = _run(case, dev)[0]
    _assert_same(again, first, f"{cid}: second zero-memory run")
    assert all(v.numel() > 0 for v in first.values())


@pytest.mark.parametrize("fill", [0, 1], ids=["nan_or_minus1", "3e38_or_int_max"])
@pytest.mark.parametrize("cid", WS_IDS)
def test_dirty_scratch(dev, cid, fill):
    case = scc.CASES[cid]
    name = list(FLOAT_FILLS if case.ws_dtype == "float32" else INT_FILLS)[fill]
    got = _run(case, dev, ws_fill=name)[0]
    _assert_same(got, _control(case, dev), f"{cid}: workspace pre-filled with {name}")


@pytest.mark.parametrize("a,b", scc.SECOND_HAND, ids=[f"{a}->{b}" for a, b in scc.SECOND_HAND])
def test_second_hand_scratch(dev, a, b):
    ca, cb = scc.CASES[a], scc.CASES[b]
    assert ca.ws_dtype == cb.ws_dtype and ca.ws_dtype is not None
    with _knob(ca):
        na = ca.need()
    with _knob(cb):
        nb = cb.need()
    ws = _raw(max(na, nb), dev, 0)
    first = _run(ca, dev, ws=ws)[0]
    _assert_same(first, _control(ca, dev), f"{a}: on the oversized buffer")
    got = _run(cb, dev, ws=ws)[0]
    _assert_same(got, _control(cb, dev), f"{b}: on the buffer {a} left behind")


@pytest.mark.parametrize("cid", IDS)
def test_guard_bands(dev, cid):
    case = scc.CASES[cid]
    got, mem = _run(case, dev, mem_mode="guard", guard_ws=True)
    assert mem.guarded, "the case handed out no buffer"
    _assert_same(got, _control(case, dev), f"{cid}: guarded buffers")


@pytest.mark.parametrize("cid", IDS)
def test_poisoned_outputs(dev, cid):
    case = scc.CASES[cid]
    got, mem = _run(case, dev, mem_mode="poison")
    skip = case.unwritten or {}
    for k, idxs in skip.items():
        # an explicit list from the header, never a mask computed from the result; below 1 % of the buffer
        assert k in mem.outs and len(set(idxs)) == len(idxs) and 100 * len(idxs) < mem.outs[k]
    _assert_same(got, _control(case, dev), f"{cid}: outputs pre-filled with NaN bits", skip=skip)


# ---------------------------------------------------------------------------------------------------------------- the trainers' reuse
def test_ensemble_eval_object_reused_across_shapes(dev):
    """ops.EnsembleEval keeps the larger workspace across shapes on purpose (_ws_key): layered then fused rows through ONE object, each
    call equal to a fresh object's."""
    for big in ("ens_eval_fused_many_tiles", "ens_eval_layered_unfitted"):
        c = scc._ENS[big]
        params, rows, idx = (t.to(dev) for t in scc.ens_inputs(big))
        shared = scc.ens_op(c, dev)
        shared(params, rows, idx, reward_off=c["X"] + c["U"] if c.get("fit_reward") else None)
        kept = shared.workspace
        # fewer rows (a ragged last tile), the reward term switched the other way: another workspace key, a smaller need
        few, roff = idx[:37].contiguous(), None if c.get("fit_reward") else c["X"] + c["U"]
        got = shared(params, rows, few, reward_off=roff).clone()
        assert shared.workspace is kept, "the object was expected to keep its larger workspace"
        fresh = scc.ens_op(c, dev)(params, rows, few, reward_off=roff)
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), fresh.view(torch.int32)), big


def test_bptt_object_reused_across_modes(dev):
    """ops.BpttActorGrad keeps its first workspace for life: trajectory sampling with noise first (the largest layout), then the
    ensemble mean and 'tsinf' through the same object, each equal to a fresh object's call."""
    first = scc._BPTT["bptt_ts1_noise_zstore"]
    inputs = scc._bptt_inputs("bptt_ts1_noise_zstore")
    shared = scc.bptt_op(first, inputs[0], dev)
    scc.bptt_call(shared, first, inputs, dev)
    kept = shared.workspace
    for later in (dict(first, mode="mean", noise=False), dict(first, mode="tsinf", noise=False), dict(first, given=False)):
        scc.bptt_call(shared, later, inputs, dev)
        assert shared.workspace is kept
        fresh = scc.bptt_op(later, inputs[0], dev)
        scc.bptt_call(fresh, later, inputs, dev)
        assert fresh.workspace.numel() <= kept.numel()
        for name in ("grads", "metrics", "transitions", "lambda_values"):
            a, b = getattr(shared, name), getattr(fresh, name)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{later.get('mode')}: `{name}` after a reused workspace"
