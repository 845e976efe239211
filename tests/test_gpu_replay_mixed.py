"""GPU: mbpo_replay_sample_mixed (MBPO's mixed minibatches in one launch) bit for bit against numpy — indices from
oracle.philox.philox_randint, rows from oracle.replay's gather on the logical data (tests/real_ratio_ref.py:mixed_rows) — and
against mbpo_replay_sample at the model positions.

Shapes: a model ring of 37 rows filled with 50 distinct rows in two inserts (wrapped: head != 0; sample_position set to 4); a real ring
of 23 rows holding 15 (insert_position < max) or 30 inserted (wrapped, sample_position 2); row lengths 12/11 (16-byte output, dword real source),
10/9 (all dwords) and 8/8 (a true buffer with truncation: 16 bytes on both sides, nothing padded); minibatches of 10 x 3 with
n_real in {0, 1, 3, 10} and of 200 x 3 with n_real = 7 (600 rows: more than one 256-row workgroup iteration, a ragged last one,
a minibatch boundary inside an iteration).
"""
import functools

import numpy as np
import pytest
import torch

import real_ratio_ref as rref
from oracle import replay as oreplay

pytestmark = pytest.mark.gpu

SEED, OFF, ROFF = 2 ** 40 + 7, (2 << 32) + 5, (3 << 32) + 5
LAYOUTS = {"12_11": (4, 1, False), "10_9": (3, 1, False), "8_8": (2, 1, True)}      # x, u, real rows carry truncation
CASES = [(10, 3, 0), (10, 3, 1), (10, 3, 3), (10, 3, 10), (200, 3, 7)]              # minibatch, G, n_real


def _rows(n, D, base):
    """n distinct rows: row r, column c holds base + 16 r + c (exact in float32)."""
    return (base + 16.0 * np.arange(n, dtype=np.float32)[:, None] + np.arange(D, dtype=np.float32)[None, :]).astype(np.float32)


def _fill(dev, max_size, D, chunks, sample_position=0):
    """The same inserts into a device ring (mbpo_replay_insert) and into the oracle's logical array.  Inserts alone leave
    sample_position at 0 (max(0, 0 + roll)): a positive one is written into both states afterwards, so that the draws' lower end
    is exercised."""
    from mbpo import ops
    data = torch.zeros(max_size, D, device=dev)
    state = torch.zeros(4, dtype=torch.int32, device=dev)
    q = oreplay.UniformSamplingQueue(max_size, D, 1)
    qs = q.init()
    for c in chunks:
        ops.replay_insert(data, state, torch.from_numpy(c).to(dev))
        qs = q.insert(qs, c)
    if sample_position:
        state[1] = sample_position
        qs = dict(qs, sample_position=np.int32(sample_position))
    return data, state, q, qs


@functools.lru_cache(maxsize=None)
def _buffers(layout, real_wrapped):
    dev = torch.device("cuda:0")
    x, u, trunc = LAYOUTS[layout]
    D, RD = 2 * x + u + 3, 2 * x + u + 2 + int(trunc)
    m = _rows(50, D, 1000.0)
    model = _fill(dev, 37, D, [m[:25], m[25:]], sample_position=4)
    r = _rows(30, RD, -9000.0)
    real = _fill(dev, 23, RD, [r[:15], r[15:]], sample_position=2) if real_wrapped else _fill(dev, 23, RD, [r[:15]])
    st, rst = model[1].cpu().tolist(), real[1].cpu().tolist()
    assert st[:2] == [37, 4] and st[2] != 0                               # the model ring wrapped
    assert (rst[:2] == [23, 2] and rst[2] != 0) if real_wrapped else rst[:3] == [15, 0, 0]
    return model, real, D, RD


@functools.lru_cache(maxsize=None)
def _plain_sample(layout, n):
    """mbpo_replay_sample of the model ring at the same (seed, offset): computed once per n, shared, never written again."""
    from mbpo import ops
    (data, state, _, _), _, _, _ = _buffers(layout, False)
    out, idx = ops.replay_sample(data, state, n, SEED, OFF, return_idx=True)
    return out.cpu().numpy(), idx.cpu().numpy()


@pytest.mark.parametrize("real_wrapped", [False, True], ids=["real_partial", "real_wrapped"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_mixed_sample_bit_exact(dev, layout, real_wrapped):
    from mbpo import ops
    (data, state, q, qs), (rdata, rstate, rq, rqs), D, RD = _buffers(layout, real_wrapped)
    for mb, G, n_real in CASES:
        n = mb * G
        out = torch.full((n + 5, D), float("nan"), device=dev)              # 5 rows more than asked for: they must stay NaN
        idx = torch.full((n,), -7, dtype=torch.int32, device=dev)
        ret = ops.replay_sample_mixed(data, state, rdata, rstate, n, mb, n_real, seed=SEED, offset=OFF, real_offset=ROFF, out=out,
                                      idx_out=idx)
        assert ret.data_ptr() == out.data_ptr()
        got, gidx = out.cpu().numpy(), idx.cpu().numpy()
        ref_idx, ref = rref.mixed_rows(q, qs, rq, rqs, SEED, OFF, ROFF, n, mb, n_real)
        tag = (layout, real_wrapped, mb, n_real)
        assert np.array_equal(gidx, ref_idx), tag
        assert np.array_equal(got[:n], ref), tag                           # (no NaN left inside: array_equal would fail on one)
        assert np.isnan(got[n:]).all(), tag
        pos = np.arange(n) % mb
        is_real = pos < n_real
        # padded columns of the real rows are exactly 0.0 (sign included), the real columns are the real ring's rows
        assert np.array_equal(got[:n][is_real, RD:].view(np.uint32), np.zeros((int(is_real.sum()), D - RD), np.uint32)), tag
        assert (got[:n][is_real, 0] < 0).all() and (got[:n][~is_real, 0] > 0).all(), tag
        # model positions: mbpo_replay_sample's index and row at the same j, whatever n_real is
        p_out, p_idx = _plain_sample(layout, n)
        assert np.array_equal(gidx[~is_real], p_idx[~is_real]) and np.array_equal(got[:n][~is_real], p_out[~is_real]), tag
        if n_real == 0:
            assert np.array_equal(got[:n], p_out) and np.array_equal(gidx, p_idx), tag
        else:
            lo, hi = int(rqs["sample_position"]), int(rqs["insert_position"])
            assert ((gidx[is_real] >= lo) & (gidx[is_real] < hi)).all(), tag


def test_mixed_sample_without_out_or_idx(dev):
    from mbpo import ops
    (data, state, q, qs), (rdata, rstate, rq, rqs), D, RD = _buffers("12_11", False)
    got = ops.replay_sample_mixed(data, state, rdata, rstate, 600, 200, 7, seed=SEED, offset=OFF, real_offset=ROFF)
    assert got.shape == (600, D)
    assert np.array_equal(got.cpu().numpy(), rref.mixed_rows(q, qs, rq, rqs, SEED, OFF, ROFF, 600, 200, 7)[1])


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_device_rng_words_are_added_to_both_offsets(dev, layout):
    from mbpo import ops
    (data, state, _, _), (rdata, rstate, _, _), D, RD = _buffers(layout, True)
    s, c = 2 ** 33 + 11, 9
    rng = ops.make_rng(dev, seed=s, counter=c)
    kw = dict(n=600, minibatch=200, n_real=7)
    ia, ib = (torch.empty(600, dtype=torch.int32, device=dev) for _ in range(2))
    a = ops.replay_sample_mixed(data, state, rdata, rstate, seed=0, offset=OFF, real_offset=ROFF, rng_dev=rng, idx_out=ia, **kw)
    b = ops.replay_sample_mixed(data, state, rdata, rstate, seed=s, offset=OFF + c, real_offset=ROFF + c, idx_out=ib, **kw)
    assert torch.equal(a, b) and torch.equal(ia, ib)
    assert rng.cpu().tolist() == [s, c]                                    # read only
    other = ops.replay_sample_mixed(data, state, rdata, rstate, seed=s, offset=OFF + c, real_offset=ROFF + c + 1, **kw)
    pos = torch.arange(600, device=dev) % 200
    assert torch.equal(other[pos >= 7], b[pos >= 7]) and not torch.equal(other[pos < 7], b[pos < 7])


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_empty_real_buffer_gives_zero_rows_at_sample_position(dev, layout):
    """randint over an empty range returns its lower end (span 0): the never-inserted, all-zero logical row sample_position."""
    from mbpo import ops
    (data, state, _, _), _, D, RD = _buffers(layout, False)
    rdata = torch.zeros(23, RD, device=dev)
    rstate = torch.tensor([5, 5, 0, 0], dtype=torch.int32, device=dev)      # insert_position == sample_position == 5
    n, mb, n_real = 30, 10, 2
    out = torch.full((n, D), float("nan"), device=dev)
    idx = torch.full((n,), -7, dtype=torch.int32, device=dev)
    ops.replay_sample_mixed(data, state, rdata, rstate, n, mb, n_real, seed=SEED, offset=OFF, real_offset=ROFF, out=out, idx_out=idx)
    torch.cuda.synchronize()
    got, gidx = out.cpu().numpy(), idx.cpu().numpy()
    is_real = (np.arange(n) % mb) < n_real
    assert (got[is_real] == 0.0).all() and (gidx[is_real] == 5).all()
    p_out, p_idx = _plain_sample(layout, n)
    assert np.array_equal(got[~is_real], p_out[~is_real]) and np.array_equal(gidx[~is_real], p_idx[~is_real])


def test_python_layers_validate(dev):
    from mbpo import _hip, ops
    from mbpo.replay import UniformSamplingQueue
    from mbpo.types import Transition
    (data, state, _, _), (rdata, rstate, _, _), D, RD = _buffers("12_11", False)
    with pytest.raises(_hip.MbpoHipError, match="minibatch"):
        ops.replay_sample_mixed(data, state, rdata, rstate, 25, 10, 3, seed=1, offset=0, real_offset=1)
    with pytest.raises(_hip.MbpoHipError, match="n_real"):
        ops.replay_sample_mixed(data, state, rdata, rstate, 30, 10, 11, seed=1, offset=0, real_offset=1)
    with pytest.raises(_hip.MbpoHipError, match="real_row_len"):
        ops.replay_sample_mixed(rdata, rstate, data, state, 30, 10, 3, seed=1, offset=0, real_offset=1)
    with pytest.raises(ValueError):
        ops.replay_sample_mixed(data, state, rdata, rstate, 30, 10, 3, seed=1, offset=0, real_offset=1, out=torch.empty(29, D, device=dev))
    z = lambda k: torch.zeros(k, device=dev)

    def queue(x, u, trunc=False, ppo=False, size=16):
        ex = {}
        if trunc:
            ex["state_extras"] = {"truncation": z(1)}
        if ppo:
            ex["policy_extras"] = {"log_prob": z(1), "raw_action": z(u)}
        return UniformSamplingQueue(size, Transition(z(x), z(u), z(1), z(1), z(x), extras=ex), 30, device=dev)

    model, real = queue(4, 1, trunc=True), queue(4, 1)
    for bad in (queue(3, 1), queue(4, 2), queue(4, 1, ppo=True)):
        with pytest.raises(ValueError):
            model.check_mixable(bad)
    with pytest.raises(ValueError):
        real.check_mixable(model)                                          # a real row longer than the model row
    # sample_rows_mixed: key split and sample_count as sample_rows; the real state object untouched; the rows are the op's
    bs = model.insert_rows(model.init(3), torch.from_numpy(_rows(12, 12, 1000.0)).to(dev))
    rbs = real.insert_rows(real.init(4), torch.from_numpy(_rows(9, 11, -9000.0)).to(dev))
    before = (rbs.key, rbs.sample_count, rbs.insert_position, rbs.sample_position, rbs.head, rbs.state.cpu().tolist())
    bs2, plain = model.sample_rows(bs)
    bs3, mixed = model.sample_rows_mixed(bs, real, rbs, n_real=3, minibatch=10, real_offset=1 << 32)
    assert (bs3.key, bs3.sample_count) == (bs2.key, bs2.sample_count) == (bs2.key, 1)
    assert before == (rbs.key, rbs.sample_count, rbs.insert_position, rbs.sample_position, rbs.head, rbs.state.cpu().tolist())
    pos = torch.arange(30, device=dev) % 10
    assert torch.equal(mixed[pos >= 3], plain[pos >= 3]) and bool((mixed[pos < 3, 0] < 0).all()) and bool((mixed[pos < 3, 11] == 0).all())
    with pytest.raises(ValueError, match="empty"):
        model.sample_rows_mixed(bs, real, real.init(5), n_real=3, minibatch=10)
