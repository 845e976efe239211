"""SHA-256 of the PPO train state after three chained minibatch updates on seeded inputs, for every dispatch path of the PPO host
(csrc/ppo.hip: ppo_variant) and both step flavours: a record to compare two builds of the library bit for bit (run once per library,
MBPO_HIP_LIB choosing it), not a test of either.

    MBPO_HIP_LIB=/path/to/libmbpo_hip.so python scripts/ppo_digests.py --out digests.json [--summary per_path.json]

Paths, each at the smallest shape that reaches it (JOBS below; the CU count comes from the device): k_ppo_vg_lean + k_ppo_lean at x = 3
and x = 4 (two-stage reduce) and at 64 x 2; the generic kernels on the same shape (mbpo_debug_set_ppo_lean(0)); k_ppo_values_gae with
1, 2, 3 and 4 value chains (u = 2); hidden width 128; WIDE (x = 17, u = 6); more tiles than two per CU (the 512-thread launch, and the
1024-thread one with MBPO_PPO_SP2=0); fewer than 64 slabs (one-stage reduce); trajectories too long for the values + GAE launch with
two-pass and with fused moments; MBPO_PPO_VALUES_GAE=0 at both widths; layered by widths and by MBPO_PPO_LAYERED=1.  Each crossed
with: mbpo_ppo_step or mbpo_ppo_grads + mbpo_ppo_apply; max_grad_norm off or so small that every step clips; non_equidistant_time off
/ on; normalize_advantage off / on; Philox or given entropy noise.  A combination the library refuses is recorded as refused, with
its message.

The knobs are read once per process, so every knob value gets one fresh child process: one at a time, each under a time limit, and the
parent stops at the first one that fails (the pattern of scripts/sac_digests.py).  The parent itself never opens the GPU.
"""
import argparse
import hashlib
import itertools
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "tests", ROOT / "model-based-policy-optimizers_amd"):
    sys.path.insert(0, str(p))

CHILD_TIMEOUT_S = 420
H64x2, H64x3 = (64, 64), (64, 64, 64)
_REF = dict(X=3, U=1, hidden=H64x2, B=128, T=40)
_H128 = dict(X=4, U=2, hidden=(128, 128), B=24, T=7)
_FEW = dict(X=3, U=1, hidden=H64x2, B=20, T=7)
_MANY = dict(X=4, U=2, hidden=H64x3, many_tiles="sp2_neq")       # B, T of tests/many_tiles_cases.py for this device's CU count
# {knob setting of the child process: [(path name, shape)]}
JOBS = {
    "": [("lean_x3", dict(X=3, U=1, hidden=H64x3, B=128, T=40)),
         ("lean_x4", dict(X=4, U=1, hidden=H64x3, B=128, T=40)),
         ("lean_64x2", _REF),
         ("generic_x3", dict(X=3, U=1, hidden=H64x3, B=128, T=40, lean=0)),
         *[(f"u2_nc{nc}", dict(X=4, U=2, hidden=H64x2, B=24, T=T)) for nc, T in ((1, 5), (2, 20), (3, 40), (4, 50))],
         ("h128", _H128),
         ("wide_x17", dict(X=17, U=6, hidden=H64x2, B=8, T=3)),
         ("sp2", _MANY),
         ("one_stage_reduce", _FEW),
         ("long_two_pass", dict(X=3, U=1, hidden=H64x2, B=65, T=1024)),
         ("long_fused", dict(X=3, U=1, hidden=H64x2, B=8, T=1024)),
         ("layered", dict(X=4, U=2, hidden=(48, 80), v_hidden=(200, 72, 40), B=20, T=7))],
    "MBPO_PPO_SP2=0": [("sp2_off", _MANY)],
    "MBPO_PPO_VALUES_GAE=0": [("vg_off_64", _REF), ("vg_off_128", _H128)],
    "MBPO_PPO_LAYERED=1": [("layered_knob_64", _FEW)],
}
FLAVOURS = ("step", "grads_apply")
CLIPS = {"noclip": None, "clip": 1e-6}
NEQ_KW = dict(non_equidistant_time=True, continuous_discounting=0.5, min_time_between_switches=0.0, max_time_between_switches=1.0, env_dt=0.1)
N_UPDATES = 3
STATE = ("params", "adam_m", "adam_v", "grads", "metrics", "metrics_accum", "step_count")


def run_path(dev, shape):
    """{flavour_clip_neq_normadv_noise: digests} of one shape through whatever kernels this process's knobs select."""
    import torch
    from mbpo import _hip, ops
    lib = _hip.load()
    X, U, hid = shape["X"], shape["U"], shape["hidden"]
    vhid = shape.get("v_hidden", hid)
    if "many_tiles" in shape:
        import many_tiles_cases as mt
        B, T = mt.ppo_bt(mt.PPO_CASES[shape["many_tiles"]], torch.cuda.get_device_properties(dev).multi_processor_count)
    else:
        B, T = shape["B"], shape["T"]
    D = 2 * X + 2 * U + 4
    g = torch.Generator().manual_seed(17 * X + U + B + T)
    NPV = ops.MlpSpec([X, *hid, 2 * U]).n_params + ops.MlpSpec([X, *vhid, 1]).n_params
    inputs = dict(params=(torch.randn(NPV, generator=g) * 0.1).to(dev), batches=[], noise=[],
                  mean=(torch.randn(X, generator=g) * 0.1).to(dev), std=(torch.rand(X, generator=g) + 0.5).to(dev))
    for _ in range(N_UPDATES):
        data = torch.randn(B, T, D, generator=g)
        data[..., X + U + 1] = (torch.rand(B, T, generator=g) > 0.1).float()           # discount
        data[..., D - 1] = (torch.rand(B, T, generator=g) < 0.15).float()              # truncation
        inputs["batches"].append(data.to(dev))
        inputs["noise"].append(torch.randn(B, T, U, generator=g).to(dev))
    lib.mbpo_debug_set_ppo_lean(shape.get("lean", -1))
    out = {"B": B, "T": T}
    for flavour, clip, neq, norm_adv, noise_kind in itertools.product(FLAVOURS, CLIPS, (0, 1), (0, 1), ("philox", "given")):
        name = f"{flavour}_{clip}_neq{neq}_normadv{norm_adv}_{noise_kind}"
        try:
            up = ops.PpoUpdater(x_dim=X, u_dim=U, policy_dims=[X, *hid, 2 * U], value_dims=[X, *vhid, 1], batch_size=B, unroll_length=T,
                                device=dev, entropy_cost=1e-2, discounting=0.99, reward_scaling=0.5, gae_lambda=0.95, clipping_epsilon=0.3,
                                normalize_advantage=bool(norm_adv), lr=3e-3, wd=0.01, seed=5, max_grad_norm=CLIPS[clip],
                                **(NEQ_KW if neq else {}))
            up.fused_step = flavour == "step"
            up.load_state(inputs["params"])
            for k in range(N_UPDATES):
                up.minibatch_step(inputs["batches"][k], inputs["mean"], inputs["std"],
                                  inputs["noise"][k] if noise_kind == "given" else None, offset=4 * k)
            torch.cuda.synchronize()
        except _hip.MbpoHipError as e:
            out[name] = {"refused": str(e)}
            continue
        out[name] = {n: hashlib.sha256(getattr(up, n).detach().cpu().contiguous().numpy().tobytes()).hexdigest() for n in STATE}
    lib.mbpo_debug_set_ppo_lean(-1)
    return out


def child(knob, out_path):
    import torch
    dev = torch.device("cuda:0")
    out = {}
    for name, shape in JOBS[knob]:
        out[name] = run_path(dev, shape)
        print(f"ppo_digests[{knob or 'default'}]: {name} B={out[name]['B']} T={out[name]['T']}", flush=True)
    Path(out_path).write_text(json.dumps(out))


def summary(digests):
    """{path: B, T, runs, refused, one SHA-256 over the path's digests in key order}: the record small enough to keep; the full one
    says which run and which tensor moved when two summaries differ."""
    return {name: dict(B=p["B"], T=p["T"], runs=len(p) - 2, refused=sum("refused" in r for r in p.values() if isinstance(r, dict)),
                       sha256=hashlib.sha256(json.dumps(p, sort_keys=True).encode()).hexdigest()) for name, p in sorted(digests.items())}


def write_summary(digests, path):
    Path(path).write_text("{\n" + ",\n".join(f' "{k}": {json.dumps(v)}' for k, v in summary(digests).items()) + "\n}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="the full record: every run's seven digests")
    ap.add_argument("--summary", default=None, help="also write one line per path: a SHA-256 over that path's part of the full record")
    ap.add_argument("--from", dest="full", default=None, help="no run: summarise this full record (with --summary)")
    ap.add_argument("--child", default=None, help="(internal) the knob setting whose paths this process runs")
    ap.add_argument("--child-out", default=None)
    args = ap.parse_args()
    if args.child is not None:
        return child(args.child, args.child_out)
    if args.full is not None:
        return write_summary(json.loads(Path(args.full).read_text())["digests"], args.summary)
    out_dir = Path(args.out).parent if args.out else Path(".")
    out_dir.mkdir(parents=True, exist_ok=True)
    digests = {}
    for knob in JOBS:
        env = dict(os.environ)
        if knob:
            k, v = knob.split("=")
            env[k] = v
        part = out_dir / f".ppo_digests_{knob or 'default'}.json"
        try:      # (a child that times out raises here: nothing further is started either, and its part file does not stay behind)
            r = subprocess.run([sys.executable, __file__, "--child", knob, "--child-out", str(part)], env=env, timeout=CHILD_TIMEOUT_S)
            if r.returncode != 0:
                sys.exit(f"ppo_digests: the child for '{knob or 'default knobs'}' ended with status {r.returncode}; nothing further is started")
            digests.update(json.loads(part.read_text()))
        finally:
            part.unlink(missing_ok=True)
    txt = json.dumps(dict(digests=digests), indent=1, sort_keys=True)
    if args.summary:
        write_summary(digests, args.summary)
    if args.out:
        Path(args.out).write_text(txt + "\n")
        print(f"ppo_digests: {sum(len(v) - 2 for v in digests.values())} runs of {len(digests)} paths -> {args.out}")
    else:
        print(txt)


if __name__ == "__main__":
    main()
