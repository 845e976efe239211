"""The descriptor table of tests/test_cpu_ppo_plan.py, and the recorder of its golden file.

mbpo_ppo_workspace_floats is pure host arithmetic (csrc/ppo.hip ppo_plan + ppo_variant: 256 compute units when no device is visible,
the MI355X's count), and the workspace layout is what the GPU tests poison and guard.  The golden file holds, per (x, u, hidden) block of
the sweep, a SHA-256 over the block's float counts (or negative statuses) and error texts in sweep order, and the bad descriptors'
statuses and texts in clear.  It is recorded from the
library of the commit BEFORE a change to the PPO host, and the test then holds the changed library to it:

    MBPO_HIP_LIB=/path/to/the/earlier/libmbpo_hip.so python tests/ppo_plan_cases.py --record
"""
import ctypes as C
import hashlib
import itertools
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "model-based-policy-optimizers_amd"))
GOLDEN = Path(__file__).resolve().parent / "golden" / "ppo_workspace_floats.json"

XS = (2, 3, 4, 6, 17)
US = (1, 2, 6)
# (policy hidden, value hidden): lean 64 x 2 / 64 x 3, 128 wide, layered by unequal widths, layered because the policy's layers differ
HIDDEN = (((64, 64), (64, 64)), ((64, 64, 64), (64, 64, 64)), ((128, 128), (128, 128)), ((48, 80), (200, 72, 40)), ((64, 128), (64, 64)))
BS = (1, 20, 128, 1040, 5000)
TS = (1, 5, 40, 1024)
BLOCK = len(BS) * len(TS) * 2 * 2


def desc(X, U, hidden, v_hidden, B, T, neq=False, clip=False, **over):
    from mbpo import _hip
    d = _hip.PpoDesc()
    d.x_dim, d.u_dim, d.batch_size, d.unroll_length, d.row_len = X, U, B, T, 2 * X + 2 * U + 4
    pd, vd = [X, *hidden, 2 * U], [X, *v_hidden, 1]
    d.policy_layers, d.value_layers = len(pd) - 1, len(vd) - 1
    for i, v in enumerate(pd):
        d.policy_dims[i] = v
    for i, v in enumerate(vd):
        d.value_dims[i] = v
    d.policy_activation = d.value_activation = _hip.ACT_IDS["swish"]
    d.normalize_advantage = 1
    d.max_grad_norm = 0.5 if clip else 0.0
    d.non_equidistant_time, d.env_dt, d.max_time_between_switches = int(neq), 0.1 if neq else 0.0, 1.0
    for k, v in over.items():
        if k in ("policy_out", "value_out"):
            (d.policy_dims if k == "policy_out" else d.value_dims)[d.policy_layers if k == "policy_out" else d.value_layers] = v
        else:
            setattr(d, k, v)
    return d


def sweep():
    """The descriptors of the sweep, in the order of the golden list."""
    for X, U, (hid, vhid), B, T, neq, clip in itertools.product(XS, US, HIDDEN, BS, TS, (False, True), (False, True)):
        yield desc(X, U, hid, vhid, B, T, neq, clip)


# one refusal per check of ppo_plan that a size query reaches, in the checks' order; the first two rows are test_ppo_bad_args's
_OK = dict(X=3, U=1, hidden=(64, 64), v_hidden=(64, 64), B=8, T=4)
BAD = {
    "value_net_two_outputs": dict(_OK, value_out=2),
    "unequal_hidden_is_layered": dict(_OK, hidden=(64, 128)),
    "null_descriptor": None,
    "zero_batch": dict(_OK, B=0),
    "zero_unroll": dict(_OK, T=0),
    "row_len": dict(_OK, row_len=11),
    "no_hidden_layer": dict(_OK, hidden=()),
    "policy_three_outputs": dict(_OK, policy_out=3),
    "neq_without_env_dt": dict(_OK, non_equidistant_time=1),
}


def query(lib, d):
    """(float count or negative status, error text of a refusal or None)"""
    n = int(lib.mbpo_ppo_workspace_floats(None if d is None else C.byref(d)))
    return n, (lib.mbpo_last_error().decode() if n < 0 else None)


def observe(lib):
    lib.mbpo_ppo_workspace_floats.restype = C.c_int64
    lib.mbpo_debug_set_ppo_lean(-1)
    results = [query(lib, d) for d in sweep()]
    # one block per (x, u, hidden): its BLOCK = |B| |T| 2 2 results in sweep order, as a SHA-256 of their JSON (6000 numbers would make
    # a golden file nobody reads), with the block's smallest and largest count in clear
    blocks = {}
    for k, (X, U, hid) in enumerate(itertools.product(XS, US, HIDDEN)):
        part = results[k * BLOCK:(k + 1) * BLOCK]
        blocks[f"x={X} u={U} hidden={hid}"] = dict(sha256=hashlib.sha256(json.dumps(part).encode()).hexdigest(),
                                                    min=min(n for n, _ in part), max=max(n for n, _ in part))
    refusals = sorted({text for _, text in results if text is not None})
    bad = {name: list(query(lib, None if kw is None else desc(**kw))) for name, kw in BAD.items()}
    return dict(axes=dict(x=XS, u=US, hidden=HIDDEN, B=BS, T=TS, neq=(False, True), clip=(False, True)), descriptors=len(results),
                blocks=blocks, refusals=refusals, bad=bad)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    from mbpo import _hip
    g = observe(_hip.load())
    one_per_line = lambda d: "{\n" + ",\n".join(f'  "{k}": {json.dumps(v)}' for k, v in d.items()) + "\n }"      # noqa: E731
    GOLDEN.write_text("{\n" + ",\n".join(f' "{k}": {one_per_line(v) if k in ("blocks", "bad") else json.dumps(v)}' for k, v in g.items()) + "\n}\n")
    print(GOLDEN)
