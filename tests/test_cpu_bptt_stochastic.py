"""BPTT through a trajectory-sampling ensemble, without a device: the workspace of mbpo_bptt_actor_grads grows by exactly the
checkpoints of the TS modes (member per trajectory and step; with model noise eps and the selected member's raw std), the mean and
pendulum sizes do not move, bptt_plan refuses what the kernel cannot run, and the Philox integer fill is exported."""
import ctypes as C
import os

import pytest

X, U, H, N, E = 4, 1, 5, 48, 5


def up4(v):
    return (v + 3) & ~3


@pytest.fixture(scope="module")
def lib():
    from mbpo import _hip
    return _hip.load()


def _desc(system="ensemble", dyn_out=2 * X, x=X, u=U):
    from mbpo import _hip
    d = _hip.BpttDesc()
    d.x_dim, d.u_dim, d.horizon, d.n = x, u, H, N
    d.actor_layers = d.critic_layers = 4
    for i, (a, c) in enumerate(zip([x, 64, 64, 64, 2 * u], [x, 64, 64, 64, 1])):
        d.actor_dims[i], d.critic_dims[i] = a, c
    d.actor_activation = d.critic_activation = _hip.ACT_IDS["swish"]
    if system == "pendulum":
        d.system_kind, d.reward_kind = _hip.SYS_PENDULUM, _hip.REWARD_PENDULUM
        d.sys_params = 16
        return d
    d.system_kind, d.reward_kind = _hip.SYS_ENSEMBLE, _hip.REWARD_QUADRATIC
    m = d.dynamics
    m.params, m.n_nets, m.n_layers, m.activation = 16, E, 4, _hip.ACT_IDS["swish"]      # (a size query never reads the parameters)
    for i, v in enumerate([x + u, 64, 64, 64, dyn_out]):
        m.dims[i] = v
    m.net_stride = sum(m.dims[i] * m.dims[i + 1] + m.dims[i + 1] for i in range(4))
    return d


def _ws(lib, d):
    return lib.mbpo_bptt_workspace_floats(C.byref(d))


def _expected_mean_ensemble(with_store=True):
    """mbpo_bptt_workspace_floats for the mean ensemble at (X, U, H, N, E), restated from bptt_plan (as on main)."""
    tiles = (N + 15) // 16
    slabs = min(tiles, 256)                      # no device: the CU count falls back to 256
    P = sum(a * b + b for a, b in zip([X, 64, 64, 64], [64, 64, 64, 2 * U]))
    total = up4(N * (H + 1) * X) + 2 * up4(N * H * U) + 3 * up4(N * H)
    if with_store and os.environ.get("MBPO_BPTT_ZSTORE_MAX_MB") is None:
        total += tiles * H * E * 3 * 1024
    return total + up4(slabs * P) + up4(slabs * 2)


def test_mean_and_pendulum_workspace_unchanged(lib):
    from mbpo import _hip
    d = _desc()
    assert _ws(lib, d) == _expected_mean_ensemble()
    d.ens_sample_noise, d.ens_min_std = 1, 0.01             # no effect in 'mean' mode
    assert _ws(lib, d) == _expected_mean_ensemble()
    p = _desc("pendulum", x=3)
    tiles = (N + 15) // 16
    P = sum(a * b + b for a, b in zip([3, 64, 64, 64], [64, 64, 64, 2]))
    assert _ws(lib, p) == up4(N * (H + 1) * 3) + 2 * up4(N * H) + 3 * up4(N * H) + up4(tiles * P) + up4(tiles * 2)
    assert p.ens_mode == _hip.ENS_MEAN


@pytest.mark.parametrize("mode", ["ts1", "tsinf"])
def test_ts_workspace_adds_exactly_the_checkpoints(lib, mode):
    from mbpo import _hip
    d = _desc()
    mean = _ws(lib, d)
    d.ens_mode = _hip.ENS_TS1 if mode == "ts1" else _hip.ENS_TSINF
    assert _ws(lib, d) == mean + up4(N * H)                                     # member per (trajectory, step)
    d.ens_sample_noise = 1
    assert _ws(lib, d) == mean + up4(N * H) + up4(N * H * X) + up4(N * H * X)   # + eps and raw_m per (trajectory, step, state)
    # the z store is untouched by the checkpoints: recompute removes exactly the same amount in both modes
    lib.mbpo_debug_set_bptt_zstore.argtypes = [C.c_int]
    lib.mbpo_debug_set_bptt_zstore.restype = C.c_int
    try:
        assert lib.mbpo_debug_set_bptt_zstore(0) == 0
        recompute_ts = _ws(lib, d)
        d.ens_mode, d.ens_sample_noise = _hip.ENS_MEAN, 0
        recompute_mean = _ws(lib, d)
    finally:
        assert lib.mbpo_debug_set_bptt_zstore(-1) == 0
    assert recompute_ts - recompute_mean == up4(N * H) + 2 * up4(N * H * X)
    assert recompute_mean == _expected_mean_ensemble(with_store=False)


def test_plan_refuses_what_the_kernel_cannot_run(lib):
    from mbpo import _hip
    d = _desc()
    d.ens_mode = 3
    assert _ws(lib, d) < 0 and b"ens_mode" in lib.mbpo_last_error()
    d.ens_mode = -1
    assert _ws(lib, d) < 0 and b"ens_mode" in lib.mbpo_last_error()
    p = _desc("pendulum", x=3)
    p.ens_mode = _hip.ENS_TS1
    assert _ws(lib, p) < 0 and b"ENSEMBLE" in lib.mbpo_last_error()
    p.ens_mode = _hip.ENS_TSINF
    assert _ws(lib, p) < 0
    q = _desc(dyn_out=X)                         # a model without the raw-std half
    q.ens_mode = _hip.ENS_TS1
    assert _ws(lib, q) > 0                       # members without noise need only mu
    q.ens_sample_noise = 1
    assert _ws(lib, q) < 0 and b"noise" in lib.mbpo_last_error()
    q.ens_mode = _hip.ENS_MEAN                   # 'mean' ignores the noise flag
    assert _ws(lib, q) > 0


def test_philox_randint_fill_is_exported_and_validates(lib):
    assert hasattr(lib, "mbpo_philox_randint_fill")
    out = (C.c_int32 * 4)()
    assert lib.mbpo_philox_randint_fill(1, 0, None, 3, 0, 0, 0, 5, C.cast(out, C.c_void_p), None) < 0       # n <= 0
    assert lib.mbpo_philox_randint_fill(1, 0, None, 11, 0, 4, 0, 5, C.cast(out, C.c_void_p), None) < 0      # unknown stream
    assert b"stream" in lib.mbpo_last_error()
    assert lib.mbpo_philox_randint_fill(1, 0, None, 3, 0, 4, 5, 5, C.cast(out, C.c_void_p), None) < 0       # empty range
    assert b"range" in lib.mbpo_last_error()

