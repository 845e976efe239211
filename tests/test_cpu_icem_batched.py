"""Batched iCEM without a device: K.split_many equals K.split element for element, the three batched entry points are declared in
include/mbpo_hip.h and exported, and their argument checks refuse bad problem counts, NULL seeds and bad elite counts with a
message before any HIP call."""
import ctypes as C
import random
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "mbpo_hip.h"
NEW = ("mbpo_icem_sample_batched", "mbpo_icem_update_batched", "mbpo_philox_fill_grouped")
P = 4096      # a non-NULL pointer the checks never dereference: every call below is refused before it would be used


@pytest.fixture(scope="module")
def lib():
    from mbpo import _hip
    return _hip.load()


def test_split_many_equals_split():
    from mbpo.utils import keys as K
    rnd = random.Random(11)
    keys = [0, 1, (1 << 64) - 1, (1 << 63), 0x9E3779B97F4A7C15] + [rnd.getrandbits(64) for _ in range(200)]
    for num in (1, 2, 3, 7):
        got = K.split_many(keys, num)
        assert got.dtype == np.uint64 and got.shape == (len(keys), num)
        for k, row in zip(keys, got):
            assert [int(v) for v in row] == K.split(k, num)
    # numpy input (the batched optimizer chains its own outputs) and chaining
    arr = K.split_many(keys, 2)[:, 0]
    again = K.split_many(arr, 2)
    for k, row in zip(arr, again):
        assert [int(v) for v in row] == K.split(int(k), 2)
    assert K.split_many([], 2).shape == (0, 2)


def test_batched_symbols_declared_and_exported(lib):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    declared = set(re.findall(r"\b(mbpo_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name


def _sample(lib, n_problems=2, seeds=P, n_prev=3, prev=P):
    return lib.mbpo_icem_sample_batched(P, P, prev, P, P, 50, n_prev, 10, 1, 2, 0.0, n_problems, seeds, 0, P, P, None)


def _update(lib, n_problems=2, n_elites=5, n_prev=2, NC=40, prev=P):
    return lib.mbpo_icem_update_batched(P, 10, 4, n_problems, NC, 2, 10, 1, P, n_elites, n_prev, 0.1, 0, None, 1.0, 0, P, P, P, P, prev,
                                        P, P, None)


def _fill(lib, n_problems=2, seeds=P, as_int=1, lo=0, hi=5, stream=3):
    return lib.mbpo_philox_fill_grouped(seeds, 0, stream, 4, n_problems, 100, as_int, lo, hi, P, None)


def _refused(rc, lib, *words):
    assert rc < 0
    msg = lib.mbpo_last_error()
    assert all(w in msg for w in words), msg


def test_icem_sample_batched_checks(lib):
    _refused(_sample(lib, n_problems=0), lib, b"icem_sample_batched", b"n_problems")
    _refused(_sample(lib, n_problems=-3), lib, b"icem_sample_batched", b"n_problems")
    _refused(_sample(lib, n_problems=1 << 20), lib, b"n_problems")
    _refused(_sample(lib, seeds=None), lib, b"icem_sample_batched", b"seeds")
    _refused(_sample(lib, prev=None), lib, b"prev_elites")


def test_icem_update_batched_checks(lib):
    _refused(_update(lib, n_problems=0), lib, b"icem_update_batched", b"n_problems")
    _refused(_update(lib, n_problems=-1), lib, b"n_problems")
    _refused(_update(lib, n_elites=0), lib, b"icem_update_batched", b"elite counts")
    _refused(_update(lib, n_elites=41), lib, b"elite counts")          # more elites than candidates
    _refused(_update(lib, n_prev=6), lib, b"elite counts")             # more carried elites than elites
    _refused(_update(lib, prev=None), lib, b"prev_elites")
    _refused(_update(lib, n_problems=1 << 20, NC=1 << 12), lib, b"overflows")


def test_philox_fill_grouped_checks(lib):
    _refused(_fill(lib, n_problems=0), lib, b"philox_fill_grouped", b"n_problems")
    _refused(_fill(lib, seeds=None), lib, b"philox_fill_grouped", b"seeds")
    _refused(_fill(lib, lo=3, hi=3), lib, b"empty range")
    _refused(_fill(lib, stream=0), lib, b"stream")
