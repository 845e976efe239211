"""Per-kernel register / spill / code-size table from the output of `build.py --save-temps`: the -Rpass-analysis=kernel-resource-usage dump
(<build>/resource_usage.txt) and the kernels' code length from the gfx950 assembly beside it (<build>/*-gfx950.s).

    python scripts/resource_table.py [--build DIR] [--against DIR] [substring ...]

--build    the build directory to tabulate (default: model-based-policy-optimizers_amd/build)
--against  another tree's build directory: every row then ends in "same", or in the other tree's figures where they differ, and kernels
           that exist on one side only are listed; the exit status is 1 unless every row is "same"
"""
import re
import subprocess
import sys
from pathlib import Path

DEFAULT = Path(__file__).resolve().parent.parent / "model-based-policy-optimizers_amd" / "build"
KEYS = ["k_sac_fwd_bwd", "k_sac_lean", "k_sac_reduce", "k_sac_apply", "k_sac_gather", "k_sac_sumsq", "k_sac_finalize", "k_ppo_", "k_moments", "k_bptt_actor", "k_model_rollout", "k_rollout_lean",
        "k_critic_fwd", "k_ensemble_forward", "k_openloop_pendulum", "k_hold_steps", "k_reward_eval", "k_mlp_vjp", "k_ens_nll"]
COLS = ("VGPR", "vspill", "scratch", "SGPR", "sspill", "LDS", "occ", "code")


def figures(build: Path) -> dict:
    """{demangled kernel: (VGPR, spilled VGPRs, scratch B/lane, SGPR, spilled SGPRs, LDS B/block, waves/SIMD, code bytes)}"""
    txt = (build / "resource_usage.txt").read_text()
    blocks = re.findall(r"Function Name: (\S+).*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)"
                        r".*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+).*?LDS Size \[bytes/block\]: (\d+)", txt, re.S)
    code = {}
    for s in build.glob("*-gfx950.s"):
        code.update(re.findall(r"^\t\.size\t(\S+), \.Lfunc_end\d+-\S+\n(?:.*\n){0,40}?; codeLenInByte = (\d+)", s.read_text(), re.M))
    names = subprocess.run(["c++filt"], input="\n".join(b[0] for b in blocks), capture_output=True, text=True).stdout.splitlines()
    out = {}
    for dem, (sym, sg, vg, scr, occ, ssp, vsp, lds) in zip(names, blocks):
        dem = re.sub(r"\(.*\)$", "", dem.replace("void ", ""))
        out[dem] = tuple(int(v) for v in (vg, vsp, scr, sg, ssp, lds, occ, code.get(sym, -1)))
    return out


def main(argv):
    build, against = DEFAULT, None
    while argv and argv[0] in ("--build", "--against"):
        if argv[0] == "--build":
            build = Path(argv[1])
        else:
            against = Path(argv[1])
        argv = argv[2:]
    keys = argv or KEYS
    mine = {k: v for k, v in figures(build).items() if any(s in k for s in keys)}
    theirs = {k: v for k, v in figures(against).items() if any(s in k for s in keys)} if against else None
    print(f"{'kernel':72s} " + " ".join(f"{c:>7}" for c in COLS) + ("  against" if theirs is not None else ""))
    differ = 0
    for k in sorted(mine):
        line = f"{k[:72]:72s} " + " ".join(f"{v:>7}" for v in mine[k])
        if theirs is not None:
            if k not in theirs:
                line, differ = line + "  (not there)", differ + 1
            elif theirs[k] == mine[k]:
                line += "  same"
            else:
                line, differ = line + "  " + " ".join(str(v) for v in theirs[k]), differ + 1
        print(line)
    if theirs is not None:
        for k in sorted(set(theirs) - set(mine)):
            print(f"{k[:72]:72s} (only in {against})")
            differ += 1
        fams = sorted({re.sub(r"<.*", "", k) for k in list(mine) + list(theirs)})
        print("\ninstantiations (this tree / the other): " +
              ", ".join(f"{f} {sum(re.sub(r'<.*', '', k) == f for k in mine)} / {sum(re.sub(r'<.*', '', k) == f for k in theirs)}" for f in fams))
        print(f"{len(mine) - differ} of {len(mine)} rows same" + (f", {differ} differ" if differ else ""))
        return 1 if differ else 0
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
