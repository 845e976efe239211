"""SAC on mixed minibatches (MBPO's real_ratio) without a GPU: the CPU reference loop (tests/real_ratio_ref.py) against the plain
CpuSacLoop, and mbpo_replay_sample_mixed's argument validation / header declaration (no launches)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import real_ratio_ref as rref
from oracle import philox, replay as oreplay, sac as osac, systems as osys, trainer as otr

ROOT = Path(__file__).resolve().parent.parent
X, U, B, G = 3, 1, 16, 2
D, RD = 2 * X + U + 3, 2 * X + U + 2


def _loop(cls, **kw):
    cfg = osac.SacConfig(X, U, [X, 16, 16, 2 * U], [X + U, 16, 16, 1], discounting=0.95, lr_policy=3e-4, lr_q=3e-4, lr_alpha=3e-4)
    g = torch.Generator().manual_seed(3)
    params = osac.init_state(cfg, g).params
    obs = torch.randn(8, X, generator=g)
    return cls(cfg, osys.PendulumSystem(), 8, 4, 6, B, G, 100, True, seed=19, init_params=params, init_obs=obs, **kw)


def _real_queue(rows=21, max_size=30):
    q = oreplay.UniformSamplingQueue(max_size, RD, 1)
    data = np.random.default_rng(5).standard_normal((rows, RD)).astype(np.float32)
    return q, q.insert(q.init(), data)


def test_n_real_zero_equals_the_plain_loop_exactly():
    q, qs = _real_queue()
    plain, mixed = _loop(otr.CpuSacLoop), _loop(rref.MixedCpuSacLoop, n_real=0, real_queue=q, real_qstate=qs)
    for _ in range(2):
        plain.training_step()
        mixed.training_step()
        assert np.array_equal(plain.last_idx, mixed.last_idx)
        assert torch.equal(plain.last_rows, mixed.last_rows)
        for name in ("params", "target_q"):
            assert torch.equal(getattr(plain.state, name), getattr(mixed.state, name)), name
        assert plain.state.count == mixed.state.count
        assert np.array_equal(plain.stats, mixed.stats)
    assert mixed.model_indices_drawn == 2 * B * G


def test_mixed_minibatches_put_padded_real_rows_first():
    q, qs = _real_queue()
    n_real = 5
    plain, mixed = _loop(otr.CpuSacLoop), _loop(rref.MixedCpuSacLoop, n_real=n_real, real_queue=q, real_qstate=qs)
    plain.training_step()
    mixed.training_step()
    pos = np.arange(B * G) % B
    # model positions: the plain step's indices and rows at the same j (the rollouts of the first step are identical)
    assert np.array_equal(mixed.last_idx[pos >= n_real], plain.last_idx[pos >= n_real])
    ref_model = plain.queue.gather(plain.qstate, plain.last_idx)
    assert np.array_equal(mixed.last_batch[pos >= n_real], ref_model[pos >= n_real])
    # real positions: SITE_SAMPLE_REAL's draw at the same element indices, on the real queue's positions; truncation column 0
    j = np.arange(B * G, dtype=np.uint64)[pos < n_real]
    ridx = philox.philox_randint(19, rref.SAC_SITE_SAMPLE_REAL << 32, philox.STREAM_REPLAY, j, 0, 21)
    assert np.array_equal(mixed.last_idx[pos < n_real], ridx)
    assert np.array_equal(mixed.last_batch[pos < n_real, :RD], qs["data"][ridx])
    assert np.all(mixed.last_batch[pos < n_real, RD:] == 0.0)
    assert mixed.model_indices_drawn == (B - n_real) * G
    assert not torch.equal(plain.state.params, mixed.state.params)


def test_all_real_minibatches_consume_no_model_index(monkeypatch):
    q, qs = _real_queue()
    mixed = _loop(rref.MixedCpuSacLoop, n_real=B, real_queue=q, real_qstate=qs)

    def no_model_draw(*a, **k):
        raise AssertionError("a model index was drawn")

    monkeypatch.setattr(mixed.queue, "sample_indices", no_model_draw)
    monkeypatch.setattr(mixed.queue, "sample", no_model_draw)
    monkeypatch.setattr(mixed.queue, "gather", no_model_draw)
    mixed.training_step()
    assert mixed.model_indices_drawn == 0
    ridx = philox.philox_randint(19, rref.SAC_SITE_SAMPLE_REAL << 32, philox.STREAM_REPLAY, np.arange(B * G, dtype=np.uint64), 0, 21)
    assert np.array_equal(mixed.last_idx, ridx)
    assert np.array_equal(mixed.last_batch[:, :RD], qs["data"][ridx]) and np.all(mixed.last_batch[:, RD:] == 0.0)


def test_site_ids_agree_with_the_trainer():
    src = (ROOT / "model-based-policy-optimizers_amd" / "mbpo" / "optimizers" / "policy_optimizers" / "sac" / "sac.py").read_text()
    m = re.search(r"^SITE_ROLLOUT, SITE_SAMPLE, SITE_SAMPLE_REAL, SITE_SGD = (\d+), (\d+), (\d+), (\d+)$", src, re.M)
    assert m and [int(v) for v in m.groups()] == [otr.SAC_SITE_ROLLOUT, otr.SAC_SITE_SAMPLE, rref.SAC_SITE_SAMPLE_REAL, otr.SAC_SITE_SGD]


@pytest.fixture(scope="module")
def lib():
    from mbpo import _hip
    return _hip.load()


def test_header_declares_the_entry_point_and_the_library_exports_it(lib):
    """The existing export test (tests/test_cpu_abi.py) reads every declared name from the header: the new one is among them."""
    import test_cpu_abi
    assert "mbpo_replay_sample_mixed" in test_cpu_abi._declared()
    assert hasattr(lib, "mbpo_replay_sample_mixed")
    assert lib.mbpo_replay_sample_mixed.argtypes is not None and len(lib.mbpo_replay_sample_mixed.argtypes) == 18


def test_validation_without_a_device(lib):
    """Every bad argument returns MBPO_ERR_ARG with a message before anything is launched or dereferenced (the pointers are
    fake non-null host addresses: a launch would be an error of its own)."""
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    good = dict(data=p, max_size=37, row_len=12, state=p, real_data=p, real_max_size=23, real_row_len=11, real_state=p, seed=1,
                offset=2, real_offset=3, rng_dev=None, n=30, minibatch=10, n_real=3, idx_out=None, out=p, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.mbpo_replay_sample_mixed(*[a[k] for k in good])

    bad = [dict(data=None), dict(state=None), dict(real_data=None), dict(real_state=None), dict(out=None),
           dict(minibatch=0), dict(minibatch=-4), dict(n=25), dict(n=-10), dict(n_real=-1), dict(n_real=11),
           dict(real_row_len=0), dict(real_row_len=13), dict(row_len=0, real_row_len=0), dict(max_size=0), dict(max_size=1 << 31),
           dict(real_max_size=0), dict(real_max_size=-1), dict(real_max_size=1 << 31)]
    for kw in bad:
        assert call(**kw) == -1, kw                       # MBPO_ERR_ARG
        assert b"replay_sample_mixed" in lib.mbpo_last_error(), kw
    # n == 0: OK, nothing launched (out may then be NULL); n_real at both ends of its range passes validation with n == 0
    assert call(n=0) == 0 and call(n=0, out=None) == 0
    assert call(n=0, n_real=0) == 0 and call(n=0, n_real=10) == 0 and call(n=0, real_row_len=12) == 0


def test_sac_rejects_a_real_ratio_outside_0_1():
    """The range check comes before anything touches a device or the environment."""
    from mbpo.optimizers.policy_optimizers.sac.sac import SAC
    for r in (-0.01, 1.5, float("nan")):
        with pytest.raises(ValueError, match="real_ratio"):
            SAC(environment=None, num_timesteps=1000, episode_length=10, real_ratio=r)
