"""The drop-in boundary without a GPU: libmbpo_hip.so loads, exports every entry point include/mbpo_hip.h declares, the ctypes
mirror of the descriptor structs has the C layout, and size queries / argument validation (no launches) behave."""
import ctypes as C
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "model-based-policy-optimizers_amd"))
HEADER = ROOT / "include" / "mbpo_hip.h"


def _declared():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(mbpo_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    from mbpo import _hip
    return _hip.load()


def test_library_exports_every_declared_symbol(lib):
    names = _declared()
    assert len(names) >= 40
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, f"declared in include/mbpo_hip.h but not exported: {missing}"
    assert lib.mbpo_version() >= 100


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof of every descriptor struct as gcc sees the header == sizeof of its ctypes mirror."""
    from mbpo import _hip
    pairs = {"mbpo_mlp_desc": _hip.MlpDesc, "mbpo_sac_desc": _hip.SacDesc, "mbpo_ppo_desc": _hip.PpoDesc,
             "mbpo_bptt_desc": _hip.BpttDesc, "mbpo_ens_train_desc": _hip.EnsTrainDesc, "mbpo_p2p_desc": _hip.P2pDesc}
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "mbpo_hip.h"\nint main(void) {\n' +
                   "".join(f'  printf("{n} %zu\\n", sizeof({n}));\n' for n in pairs) + "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    sizes = dict(line.split() for line in out.strip().splitlines())
    for name, cls in pairs.items():
        assert int(sizes[name]) == C.sizeof(cls), f"{name}: C {sizes[name]} bytes, ctypes {C.sizeof(cls)}"


def test_size_queries_and_validation_without_a_device(lib):
    from mbpo import _hip
    # size queries are pure host arithmetic
    assert lib.mbpo_running_stats_workspace_floats(4) > 0
    assert lib.mbpo_running_stats_workspace_floats(0) < 0          # MBPO_ERR_ARG
    assert lib.mbpo_p2p_region_bytes(2, 1000) > 0
    assert lib.mbpo_p2p_region_bytes(0, 1000) < 0
    d = _hip.SacDesc()
    d.x_dim, d.u_dim, d.batch_size, d.row_len = 4, 1, 256, 12
    d.policy_layers = d.q_layers = 4
    for i, v in enumerate([4, 64, 64, 64, 2]):
        d.policy_dims[i] = v
    for i, v in enumerate([5, 64, 64, 64, 1]):
        d.q_dims[i] = v
    n = lib.mbpo_sac_workspace_floats(C.byref(d))
    assert n >= 16 * (9026 + 2 * 8641)                             # 16 tiles of gradient slabs at least
    # error convention: negative code + message, nothing launched
    d.row_len = 11
    assert lib.mbpo_sac_workspace_floats(C.byref(d)) < 0
    assert b"row_len" in lib.mbpo_last_error()
    d.row_len = 12
    d.policy_dims[1] = 96                                          # not a fused-kernel width: the layered path (one tile of slabs + its buffers)
    n96 = lib.mbpo_sac_workspace_floats(C.byref(d))
    assert n96 > 0
    d.policy_dims[4] = 3                                           # a policy must end in 2 * u_dim outputs
    assert lib.mbpo_sac_workspace_floats(C.byref(d)) < 0
    assert b"policy" in lib.mbpo_last_error()
    # PPO: fused shapes and the reference's experiments/train_inverted_pendulum/exp_ppo.py shapes (policy (32,)*4 padded, critic (256,)*5)
    p = _hip.PpoDesc()
    p.x_dim, p.u_dim, p.batch_size, p.unroll_length, p.row_len = 3, 1, 512, 40, 12
    p.policy_layers, p.value_layers = 3, 3
    for i, v in enumerate([3, 64, 64, 2]):
        p.policy_dims[i] = v
    for i, v in enumerate([3, 64, 64, 1]):
        p.value_dims[i] = v
    n_fused = lib.mbpo_ppo_workspace_floats(C.byref(p))
    assert n_fused > 0
    p.value_layers = 6
    for i, v in enumerate([3, 256, 256, 256, 256, 256, 1]):
        p.value_dims[i] = v
    n_layered = lib.mbpo_ppo_workspace_floats(C.byref(p))
    assert n_layered > (512 * 40 + 512) * 256 * 2 * 5              # stored z and h of five 256-wide layers for every row
    p.value_dims[6] = 2                                            # a value net ends in one output
    assert lib.mbpo_ppo_workspace_floats(C.byref(p)) < 0


def test_test_hooks_without_a_device(lib):
    """The kernel-selection hooks and the fast-math helper hook the GPU tests use are exported but not declared (not part of the API),
    reject unknown modes or helpers, and mbpo_debug_set_bptt_zstore(0) removes exactly the z store from the BPTT workspace: 1024
    floats per (trajectory tile, step, member, hidden layer)."""
    from mbpo import _hip
    for name in ("mbpo_debug_set_icem_update", "mbpo_debug_set_bptt_zstore"):
        assert hasattr(lib, name) and name not in _declared()
        getattr(lib, name).argtypes = [C.c_int]
        getattr(lib, name).restype = C.c_int
    assert lib.mbpo_debug_set_icem_update(2) < 0 and b"mode" in lib.mbpo_last_error()
    assert lib.mbpo_debug_set_bptt_zstore(1) < 0 and b"mode" in lib.mbpo_last_error()
    # the fast-math helper hook (tests/test_gpu_fastmath.py): an unknown helper is refused before anything is launched
    assert hasattr(lib, "mbpo_debug_eval_fastmath") and "mbpo_debug_eval_fastmath" not in _declared()
    lib.mbpo_debug_eval_fastmath.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.mbpo_debug_eval_fastmath.restype = C.c_int
    for fn in (-1, 10, 1 << 20):
        assert lib.mbpo_debug_eval_fastmath(fn, None, None, 4, None) < 0 and b"unknown helper" in lib.mbpo_last_error()
    assert lib.mbpo_debug_eval_fastmath(2, None, None, -1, None) < 0 and b"n=-1" in lib.mbpo_last_error()
    assert lib.mbpo_debug_eval_fastmath(2, None, None, 4, None) < 0 and b"null" in lib.mbpo_last_error()
    # which rollout kernel ran last (tests/test_gpu_rollout_matrix.py): read-only, eleven ints, family 0 before any launch
    assert hasattr(lib, "mbpo_debug_last_rollout_kernel") and "mbpo_debug_last_rollout_kernel" not in _declared()
    lib.mbpo_debug_last_rollout_kernel.argtypes = [C.c_void_p, C.c_int32]
    lib.mbpo_debug_last_rollout_kernel.restype = C.c_int
    ids = (C.c_int32 * 11)(*([7] * 11))
    assert lib.mbpo_debug_last_rollout_kernel(ids, 10) < 0 and b"11 ints" in lib.mbpo_last_error()
    assert lib.mbpo_debug_last_rollout_kernel(None, 11) < 0
    assert lib.mbpo_debug_last_rollout_kernel(ids, 11) == 0 and 0 <= ids[0] <= 4 and (ids[0] != 0 or list(ids) == [0] * 11)
    X, U, H, n, E = 4, 1, 5, 48, 5
    d = _hip.BpttDesc()
    d.x_dim, d.u_dim, d.horizon, d.n = X, U, H, n
    d.actor_layers = d.critic_layers = 4
    for i, (a, c) in enumerate(zip([X, 64, 64, 64, 2 * U], [X, 64, 64, 64, 1])):
        d.actor_dims[i], d.critic_dims[i] = a, c
    d.actor_activation = d.critic_activation = _hip.ACT_IDS["swish"]
    d.system_kind, d.reward_kind = _hip.SYS_ENSEMBLE, _hip.REWARD_QUADRATIC
    m = d.dynamics
    m.params, m.n_nets, m.n_layers, m.activation = 16, E, 4, _hip.ACT_IDS["swish"]      # (a size query never reads the parameters)
    for i, v in enumerate([X + U, 64, 64, 64, 2 * X]):
        m.dims[i] = v
    m.net_stride = sum(m.dims[i] * m.dims[i + 1] + m.dims[i + 1] for i in range(4))
    try:
        with_store = lib.mbpo_bptt_workspace_floats(C.byref(d))
        assert lib.mbpo_debug_set_bptt_zstore(0) == 0
        recompute = lib.mbpo_bptt_workspace_floats(C.byref(d))
    finally:
        assert lib.mbpo_debug_set_bptt_zstore(-1) == 0
    if os.environ.get("MBPO_BPTT_ZSTORE_MAX_MB") is None:      # (a cap in the environment may switch the store off already)
        assert recompute > 0 and with_store - recompute == (n + 15) // 16 * H * E * 3 * 1024
    assert lib.mbpo_bptt_workspace_floats(C.byref(d)) == with_store


def test_environment_switches_live_in_one_table():
    """csrc/knobs.hpp is the only list of MBPO_* switches: api.hip holds the library's single getenv, and INTEGRATION.md
    documents every environment name of the table."""
    csrc = ROOT / "model-based-policy-optimizers_amd" / "csrc"
    users = {p.name: p.read_text().count("getenv(") for p in sorted(csrc.iterdir()) if p.is_file()}
    assert {n: c for n, c in users.items() if c} == {"api.hip": 1}
    table = (csrc / "knobs.hpp").read_text()
    rows = re.findall(r'^\s*X\((\w+),\s*(?:"(MBPO_[A-Z0-9_]+)"|nullptr),\s*(-?\d+),\s*(true|false),\s*"', table, re.M)
    names = [env for _, env, _, _ in rows if env]
    assert len(rows) >= 18 and len(names) >= 16 and len(set(names)) == len(names)
    assert [env for _, env, _, reread in rows if reread == "true"] == ["MBPO_SAC_THIN"]
    doc = (ROOT / "INTEGRATION.md").read_text()
    assert [n for n in names if f"`{n}`" not in doc] == []


def test_product_path_refuses_cpu_tensors():
    """No CPU fallback: a host tensor is an error, not a slow path."""
    import torch
    from mbpo import _hip, ops
    with pytest.raises((_hip.MbpoHipError, ValueError, TypeError)):
        ops.gae_scan(torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4), 0.99, 0.95)
