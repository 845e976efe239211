"""SHA-256 of the SAC train state after three chained updates on seeded inputs, for every single-process dispatch path of the SAC host
(csrc/sac.hip: sac_variant, SacReduceKind) and every step flavour: a record to compare two builds of the library bit for bit (run once per
library, MBPO_HIP_LIB choosing it), not a test of either.

    MBPO_HIP_LIB=/path/to/libmbpo_hip.so python scripts/sac_digests.py --out digests.json

Paths: k_sac_lean at x = 3 and x = 4; the generic thin kernel (mbpo_debug_set_sac_lean(0)); MBPO_SAC_THIN=0; u = 2 (no forward-mode
actor); MBPO_SAC_JVP=0; MBPO_SAC_SPLIT=0 at hidden width 64 and 128; WIDE (x = 17); 128 x 2 with the default three workgroups per tile;
layered (policy (48, 80), critics (200, 72, 40)).  Flavours: mbpo_sac_step x 3 + mbpo_sac_finalize; mbpo_sac_grads + mbpo_sac_apply;
mbpo_sac_grads_phase 1 then 2 + mbpo_sac_grad_norms + mbpo_sac_apply — each with max_grad_norm 1e5 and with one so small that every
step clips, with Philox noise and with given noise.  B = 40 (two and a half tiles; 104 at 128 wide).  The p2p entry points need two ranks:
tests/test_gpu_distributed.py.

The knobs are read once per process, so every knob value gets one fresh child process: one at a time, each under a time limit, and the
parent stops at the first one that fails (the pattern of tests/test_gpu_knob_variants.py).  The parent itself never opens the GPU.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "model-based-policy-optimizers_amd"))

CHILD_TIMEOUT_S = 300
H64 = (64, 64, 64)
# {knob setting of the child process: [(path name, shape)]}
JOBS = {
    "": [("lean_x3", dict(X=3, U=1, hidden=H64, B=40)),
         ("lean_x4", dict(X=4, U=1, hidden=H64, B=40)),
         ("generic_thin_x4", dict(X=4, U=1, hidden=H64, B=40, lean=0)),
         ("u2_no_jvp", dict(X=4, U=2, hidden=H64, B=40)),
         ("wide_x17", dict(X=17, U=1, hidden=H64, B=40)),
         ("h128x2_split", dict(X=3, U=1, hidden=(128, 128), B=104)),
         ("layered", dict(X=4, U=2, hidden=(48, 80), q_hidden=(200, 72, 40), B=40))],
    "MBPO_SAC_THIN=0": [("thin_off_x4", dict(X=4, U=1, hidden=H64, B=40))],
    "MBPO_SAC_JVP=0": [("jvp_off_x4", dict(X=4, U=1, hidden=H64, B=40))],
    "MBPO_SAC_SPLIT=0": [("split_off_64", dict(X=4, U=1, hidden=H64, B=40)),
                         ("split_off_128", dict(X=3, U=1, hidden=(128, 128), B=104))],
}
FLAVOURS = ("step_finalize", "grads_apply", "phases_norms_apply")
CLIPS = {"noclip": 1e5, "clip": 1e-6}
N_UPDATES = 3


def run_path(dev, shape):
    """{flavour_clip_noise: digests} of one shape through whatever kernels this process's knobs select."""
    import torch
    from mbpo import _hip, ops
    lib = _hip.load()
    X, U, B, hid = shape["X"], shape["U"], shape["B"], shape["hidden"]
    qhid = shape.get("q_hidden", hid)
    g = torch.Generator().manual_seed(17 * X + U + B)
    lib.mbpo_debug_set_sac_lean(shape.get("lean", -1))
    out = {}
    for clip_name, max_norm in CLIPS.items():
        for noise_kind in ("philox", "given"):
            up0 = None
            for flavour in FLAVOURS:
                up = ops.SacUpdater(x_dim=X, u_dim=U, policy_dims=[X, *hid, 2 * U], q_dims=[X + U, *qhid, 1], batch_size=B, device=dev,
                                    max_grad_norm=max_norm, lr_policy=3e-3, lr_q=3e-3, lr_alpha=3e-3, wd_q=0.01, seed=5)
                if up0 is None:       # the same seeded inputs for the three flavours
                    up0 = dict(params=(torch.randn(up.NP, generator=g) * 0.1).to(dev),
                               batches=[torch.randn(B, 2 * X + U + 3, generator=g).to(dev) for _ in range(N_UPDATES)],
                               mean=(torch.randn(X, generator=g) * 0.1).to(dev), std=(torch.rand(X, generator=g) + 0.5).to(dev),
                               noise=[[torch.randn(B, U, generator=g).to(dev) for _ in range(3)] for _ in range(N_UPDATES)])
                up.load_state(up0["params"])
                d, st = up.desc, torch.cuda.current_stream().cuda_stream
                d.norm_mean, d.norm_std = up0["mean"].data_ptr(), up0["std"].data_ptr()
                call = lambda fn, *a: _hip.check(fn(C.byref(d), *a, st), fn.__name__)       # noqa: E731
                for k in range(N_UPDATES):
                    d.batch, d.offset = up0["batches"][k].data_ptr(), 4 * k
                    na, nc, nt = up0["noise"][k] if noise_kind == "given" else (None, None, None)
                    d.noise_alpha, d.noise_critic, d.noise_actor = ops.ptr(na), ops.ptr(nc), ops.ptr(nt)
                    if flavour == "step_finalize":
                        call(lib.mbpo_sac_step)
                    elif flavour == "grads_apply":
                        call(lib.mbpo_sac_grads)
                        call(lib.mbpo_sac_apply)
                    else:
                        call(lib.mbpo_sac_grads_phase, 1)
                        call(lib.mbpo_sac_grads_phase, 2)
                        call(lib.mbpo_sac_grad_norms)
                        call(lib.mbpo_sac_apply)
                if flavour == "step_finalize":
                    call(lib.mbpo_sac_finalize)
                torch.cuda.synchronize()
                res = {n: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
                       for n, t in (("params", up.params), ("target_q", up.target_q), ("adam_m", up.adam_m), ("adam_v", up.adam_v),
                                    ("grads", up.grads), ("metrics", up.metrics), ("metrics_accum", up.metrics_accum),
                                    ("control", up._control))}
                res["clip_events"] = int(up._control[13])
                out[f"{flavour}_{clip_name}_{noise_kind}"] = res
    lib.mbpo_debug_set_sac_lean(-1)
    return out


def child(knob, out_path):
    import torch
    dev = torch.device("cuda:0")
    Path(out_path).write_text(json.dumps({name: run_path(dev, shape) for name, shape in JOBS[knob]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help="(internal) the knob setting whose paths this process runs")
    ap.add_argument("--child-out", default=None)
    args = ap.parse_args()
    if args.child is not None:
        return child(args.child, args.child_out)
    out_dir = Path(args.out).parent if args.out else Path(".")
    out_dir.mkdir(parents=True, exist_ok=True)
    digests = {}
    for knob in JOBS:
        env = dict(os.environ)
        if knob:
            k, v = knob.split("=")
            env[k] = v
        part = out_dir / f".sac_digests_{knob or 'default'}.json"
        try:      # (a child that times out raises here: nothing further is started either, and its part file does not stay behind)
            r = subprocess.run([sys.executable, __file__, "--child", knob, "--child-out", str(part)], env=env, timeout=CHILD_TIMEOUT_S)
            if r.returncode != 0:
                sys.exit(f"sac_digests: the child for '{knob or 'default knobs'}' ended with status {r.returncode}; nothing further is started")
            digests.update(json.loads(part.read_text()))
        finally:
            part.unlink(missing_ok=True)
    txt = json.dumps(dict(digests=digests), indent=1, sort_keys=True)
    if args.out:
        Path(args.out).write_text(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
