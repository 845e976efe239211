"""One case per kernel instantiation behind mbpo_model_rollout, shared by tests/test_cpu_rollout_matrix.py and
tests/test_gpu_rollout_matrix.py: the enumeration of the four kernel families from the rules of their launch nests, the case table, the
composed reference run and the device run.

THIS TABLE IS WHERE A NEW SWITCH OR INSTANTIATION IS ENTERED: add the template argument to FIELDS and `kernels()`, the inputs that make
the dispatch pick it to `build`, its reference to `reference`, and the seed of each new case to SEEDS (tests/test_cpu_rollout_matrix.py
fails until the table and the enumeration agree again).

A kernel is the tuple of FIELDS, which is also what the test hook mbpo_debug_last_rollout_kernel reports (csrc/rollout_shared.hpp,
RolloutKernelId): family, H, X, PEND, PIPE, LR, W, TM, SB, HL, TA; a field a family does not have is 0.
    k_model_rollout64   (csrc/rollout64.hip)            LR x W x TM x SB x HL x TA, no TA with HL or W        3 * 2 * 2 * 5 = 60
    k_model_rollout     (csrc/rollout_wide_kernel.hpp)  H x LR x SB x HL x TA, no TA with HL                  2 * 3 * 2 * 3 = 36
                        (the box is a run-time flag there: the hook reports it in TM, the table rotates it as the option `box`)
    k_rollout_lean      (csrc/rollout_lean.hip)         (X, PEND) x PIPE x LR x TM x SB, no LR with PEND      32 + 24       = 56
    k_openloop_pendulum (csrc/rollout.hip)              SB (the box is a run-time test, rotated as `box`)                      2
NO_INSTANTIATION lists the combinations the nests leave out, UNREACHABLE the instantiations no valid descriptor reaches (none today).

Shapes: N = 40 envs (three 16-row tiles, the last ragged), S = 4 or 5, episode_length 3, initial steps = env % 3, a few envs entering
done; E = 5 at 64-wide, 3 at 128, 2 at 256; x = 5, u = 1 for the tile kernels, x = 9 for W (18 member outputs; with HL 10 action
columns and 20 policy outputs); x = 2, 3, 4 with u = 1 for the lean kernel.  Members and policy are lecun-initialised with small non-zero
biases, so that members disagree.  Every case owns a box (on x_0; the Pendulum's on thetadot), a true buffer and a term table, used when
its switch — or a flipped copy of the case — asks for them.

The run-time options (OPTIONS) are dealt over the table by a fixed rule, kernel after kernel in enumeration order: of the values the
host accepts for that kernel (`option_values`), option o takes the one that meets the most (switch, value) pairs of the kernel it has not
met in the cases before; equals are broken by starting the values at crc32(name + "/" + o) % len(values).

Tolerance: atol = rtol = 2e-4 (tests/test_gpu_rollout.py, S <= 5), 5e-4 for the x = 9 cases (tests/termination_cases.py "d").

The seed of a case is the first in 0 .. 63 at which `examine` passes: no env of the fp64 run within 10 * TOL of the box, no hold decision
within 2e-3 of an integer, fp32 and fp64 runs within TOL / 4 of each other on every row (none is left out), every switch that is on
visibly at work, and every valid single-switch flip of the case more than 100 * TOL away.  It stands in SEEDS as a literal.
"""
from __future__ import annotations

import functools
import math
import zlib

import numpy as np
import torch

from oracle import nets as onets
from oracle import philox
from oracle import replay as oreplay
from oracle import rollout as oro
from oracle import systems as osys

import fresh_start_ref as fref
import halluc_ref as href
import learned_reward_ref as lref
import term_reward_ref as trref
import termination_ref as tref
import time_adaptive_ref as taref

N, L = 40, 3
F64, FWIDE, FLEAN, FOPEN = 1, 2, 3, 4                  # RO_FAMILY_* (csrc/rollout_shared.hpp)
FAMILY_NAME = {F64: "k_model_rollout64", FWIDE: "k_model_rollout", FLEAN: "k_rollout_lean", FOPEN: "k_openloop_pendulum"}
LR_FORMULA, LR_LEARNED, LR_TERMS = 0, 1, 2             # RO_LR_* (csrc/rollout_tile.hpp)
FIELDS = ("family", "H", "X", "PEND", "PIPE", "LR", "W", "TM", "SB", "HL", "TA")
SEED, OFFSET = 2468, (3 << 32) + 11                    # Philox key of the start-buffer draws and of the Philox-drawn noise (+ the case seed)
DT, HOLD_K, HOLD_CD, HOLD_COST = 0.05, 3, 0.5, 0.05
INT_MARGIN = 2e-3
MIN_TERMINATIONS = 4
EFFECT = 100.0                                         # a switch's effect, in units of the tolerance
BUF_MAX, BUF_INSERTS, BUF_SAMPLE_POSITION = 37, (20, 20, 10), 5      # tests/fresh_start_cases.py's ring: wrapped, head != 0
INF = float("inf")

NO_INSTANTIATION = {
    "k_model_rollout64<TA, HL>": "the host refuses hold_max_steps with halluc_beta; the nest's guard creates no such kernel",
    "k_model_rollout64<TA, W>": "no time-adaptive kernel for 64-wide networks with more than 16 inputs or outputs: the launch refuses it",
    "k_model_rollout<TA, HL>": "the host refuses hold_max_steps with halluc_beta",
    "k_rollout_lean<PEND, LR>": "the learned reward needs an ensemble and the Pendulum reward is a formula",
}
UNREACHABLE: dict = {}      # kernel name -> reason: an instantiation that exists and that no valid descriptor reaches


def _kernel(**kw) -> dict:
    return dict(dict.fromkeys(FIELDS, 0), **kw)


def kernels() -> list:
    """Every instantiation of the four families, from the rules of the launch nests."""
    out = []
    for lr in (0, 1, 2):
        for w in (0, 1):
            for tm in (0, 1):
                for sb in (0, 1):
                    for hl in (0, 1):
                        for ta in (0, 1):
                            if ta and (hl or w):
                                continue
                            out.append(_kernel(family=F64, H=64, LR=lr, W=w, TM=tm, SB=sb, HL=hl, TA=ta))
    for lr in (0, 1, 2):
        for h in (128, 256):
            for sb in (0, 1):
                for hl in (0, 1):
                    for ta in (0, 1):
                        if ta and hl:
                            continue
                        out.append(_kernel(family=FWIDE, H=h, LR=lr, SB=sb, HL=hl, TA=ta))
    for lr in (0, 1):
        for x, pend in ((2, 0), (3, 0), (3, 1), (4, 0)):
            if lr and pend:
                continue
            for pipe in (0, 1):
                for tm in (0, 1):
                    for sb in (0, 1):
                        out.append(_kernel(family=FLEAN, H=64, X=x, PEND=pend, PIPE=pipe, LR=lr, TM=tm, SB=sb))
    for sb in (0, 1):
        out.append(_kernel(family=FOPEN, X=3, PEND=1, SB=sb))
    return out


def kernel_name(k: dict) -> str:
    f = k["family"]
    if f == F64:
        return "k64_lr{LR}_w{W}_tm{TM}_sb{SB}_hl{HL}_ta{TA}".format(**k)
    if f == FWIDE:
        return "wide{H}_lr{LR}_sb{SB}_hl{HL}_ta{TA}".format(**k)
    if f == FLEAN:
        return "lean_x{X}_pend{PEND}_pipe{PIPE}_lr{LR}_tm{TM}_sb{SB}".format(**k)
    return "openloop_sb{SB}".format(**k)


def pendulum_system(k: dict) -> bool:
    """The analytic Pendulum system: the open-loop kernel, and the lean PEND kernels that are not pipelined (PIPE needs members: its
    PEND kernels run an ensemble under the Pendulum reward)."""
    return k["family"] == FOPEN or (k["family"] == FLEAN and bool(k["PEND"]) and not k["PIPE"])


OPTIONS = ("mode", "noise", "AR", "ppo", "norm", "philox", "box")


def option_values(k: dict, mode=None) -> dict:
    """What the host accepts for kernel k, per run-time option (and what keeps the dispatch on k: the lean kernel takes action_repeat 1).
    noise: ens_sample_noise, dealt only where something reads it: in the 'ts1' / 'tsinf' modes (mode: the one already dealt).
    ppo: ppo_extras with env_major.  box: the termination box where it is a run-time flag; elsewhere it is the switch TM."""
    lean, openloop = k["family"] == FLEAN, k["family"] == FOPEN
    pend = pendulum_system(k)
    return dict(mode=("none",) if pend else (("mean",) if k["HL"] else ("mean", "ts1", "tsinf")),
                noise=(0,) if (pend or k["HL"] or mode == "mean") else (0, 1),
                AR=(1,) if (k["TA"] or lean) else (1, 2),
                ppo=(0,) if openloop else (0, 1), norm=(0,) if openloop else (0, 1), philox=(0,) if openloop else (0, 1),
                box=(0, 1) if k["family"] in (FWIDE, FOPEN) else (k["TM"],))


@functools.lru_cache(maxsize=None)
def _deal() -> dict:
    """name -> options: the rule of the module docstring, over the kernels in enumeration order."""
    met, out = set(), {}
    for k in kernels():
        name, opt = kernel_name(k), {}
        for o in OPTIONS:
            values = option_values(k, opt.get("mode"))[o]
            r = zlib.crc32(f"{name}/{o}".encode()) % len(values)
            order = values[r:] + values[:r]
            v = max(order, key=lambda v: sum((f, k[f], o, v) not in met for f in FIELDS))      # (max keeps the first of equals)
            opt[o] = v
            met |= {(f, k[f], o, v) for f in FIELDS}
        out[name] = opt
    return out


def options(k: dict) -> dict:
    return dict(_deal()[kernel_name(k)])


# name -> the first passing seed (tests/test_cpu_rollout_matrix.py re-derives each)
SEEDS: dict = {
    "k64_lr0_w0_tm0_sb0_hl0_ta0": 0, "k64_lr0_w0_tm0_sb0_hl0_ta1": 2, "k64_lr0_w0_tm0_sb0_hl1_ta0": 0,
    "k64_lr0_w0_tm0_sb1_hl0_ta0": 0, "k64_lr0_w0_tm0_sb1_hl0_ta1": 3, "k64_lr0_w0_tm0_sb1_hl1_ta0": 0,
    "k64_lr0_w0_tm1_sb0_hl0_ta0": 0, "k64_lr0_w0_tm1_sb0_hl0_ta1": 4, "k64_lr0_w0_tm1_sb0_hl1_ta0": 0,
    "k64_lr0_w0_tm1_sb1_hl0_ta0": 0, "k64_lr0_w0_tm1_sb1_hl0_ta1": 0, "k64_lr0_w0_tm1_sb1_hl1_ta0": 0,
    "k64_lr0_w1_tm0_sb0_hl0_ta0": 0, "k64_lr0_w1_tm0_sb0_hl1_ta0": 0, "k64_lr0_w1_tm0_sb1_hl0_ta0": 0,
    "k64_lr0_w1_tm0_sb1_hl1_ta0": 0, "k64_lr0_w1_tm1_sb0_hl0_ta0": 1, "k64_lr0_w1_tm1_sb0_hl1_ta0": 0,
    "k64_lr0_w1_tm1_sb1_hl0_ta0": 0, "k64_lr0_w1_tm1_sb1_hl1_ta0": 7, "k64_lr1_w0_tm0_sb0_hl0_ta0": 0,
    "k64_lr1_w0_tm0_sb0_hl0_ta1": 1, "k64_lr1_w0_tm0_sb0_hl1_ta0": 0, "k64_lr1_w0_tm0_sb1_hl0_ta0": 0,
    "k64_lr1_w0_tm0_sb1_hl0_ta1": 2, "k64_lr1_w0_tm0_sb1_hl1_ta0": 0, "k64_lr1_w0_tm1_sb0_hl0_ta0": 3,
    "k64_lr1_w0_tm1_sb0_hl0_ta1": 0, "k64_lr1_w0_tm1_sb0_hl1_ta0": 1, "k64_lr1_w0_tm1_sb1_hl0_ta0": 0,
    "k64_lr1_w0_tm1_sb1_hl0_ta1": 2, "k64_lr1_w0_tm1_sb1_hl1_ta0": 1, "k64_lr1_w1_tm0_sb0_hl0_ta0": 0,
    "k64_lr1_w1_tm0_sb0_hl1_ta0": 0, "k64_lr1_w1_tm0_sb1_hl0_ta0": 0, "k64_lr1_w1_tm0_sb1_hl1_ta0": 0,
    "k64_lr1_w1_tm1_sb0_hl0_ta0": 0, "k64_lr1_w1_tm1_sb0_hl1_ta0": 5, "k64_lr1_w1_tm1_sb1_hl0_ta0": 0,
    "k64_lr1_w1_tm1_sb1_hl1_ta0": 0, "k64_lr2_w0_tm0_sb0_hl0_ta0": 0, "k64_lr2_w0_tm0_sb0_hl0_ta1": 1,
    "k64_lr2_w0_tm0_sb0_hl1_ta0": 0, "k64_lr2_w0_tm0_sb1_hl0_ta0": 0, "k64_lr2_w0_tm0_sb1_hl0_ta1": 0,
    "k64_lr2_w0_tm0_sb1_hl1_ta0": 0, "k64_lr2_w0_tm1_sb0_hl0_ta0": 4, "k64_lr2_w0_tm1_sb0_hl0_ta1": 4,
    "k64_lr2_w0_tm1_sb0_hl1_ta0": 0, "k64_lr2_w0_tm1_sb1_hl0_ta0": 0, "k64_lr2_w0_tm1_sb1_hl0_ta1": 0,
    "k64_lr2_w0_tm1_sb1_hl1_ta0": 0, "k64_lr2_w1_tm0_sb0_hl0_ta0": 0, "k64_lr2_w1_tm0_sb0_hl1_ta0": 0,
    "k64_lr2_w1_tm0_sb1_hl0_ta0": 0, "k64_lr2_w1_tm0_sb1_hl1_ta0": 0, "k64_lr2_w1_tm1_sb0_hl0_ta0": 0,
    "k64_lr2_w1_tm1_sb0_hl1_ta0": 1, "k64_lr2_w1_tm1_sb1_hl0_ta0": 1, "k64_lr2_w1_tm1_sb1_hl1_ta0": 1,
    "wide128_lr0_sb0_hl0_ta0": 0, "wide128_lr0_sb0_hl0_ta1": 0, "wide128_lr0_sb0_hl1_ta0": 0,
    "wide128_lr0_sb1_hl0_ta0": 0, "wide128_lr0_sb1_hl0_ta1": 4, "wide128_lr0_sb1_hl1_ta0": 1,
    "wide256_lr0_sb0_hl0_ta0": 0, "wide256_lr0_sb0_hl0_ta1": 0, "wide256_lr0_sb0_hl1_ta0": 0,
    "wide256_lr0_sb1_hl0_ta0": 0, "wide256_lr0_sb1_hl0_ta1": 0, "wide256_lr0_sb1_hl1_ta0": 0,
    "wide128_lr1_sb0_hl0_ta0": 0, "wide128_lr1_sb0_hl0_ta1": 1, "wide128_lr1_sb0_hl1_ta0": 0,
    "wide128_lr1_sb1_hl0_ta0": 1, "wide128_lr1_sb1_hl0_ta1": 4, "wide128_lr1_sb1_hl1_ta0": 0,
    "wide256_lr1_sb0_hl0_ta0": 0, "wide256_lr1_sb0_hl0_ta1": 6, "wide256_lr1_sb0_hl1_ta0": 0,
    "wide256_lr1_sb1_hl0_ta0": 0, "wide256_lr1_sb1_hl0_ta1": 0, "wide256_lr1_sb1_hl1_ta0": 0,
    "wide128_lr2_sb0_hl0_ta0": 0, "wide128_lr2_sb0_hl0_ta1": 2, "wide128_lr2_sb0_hl1_ta0": 0,
    "wide128_lr2_sb1_hl0_ta0": 0, "wide128_lr2_sb1_hl0_ta1": 3, "wide128_lr2_sb1_hl1_ta0": 0,
    "wide256_lr2_sb0_hl0_ta0": 1, "wide256_lr2_sb0_hl0_ta1": 0, "wide256_lr2_sb0_hl1_ta0": 0,
    "wide256_lr2_sb1_hl0_ta0": 0, "wide256_lr2_sb1_hl0_ta1": 1, "wide256_lr2_sb1_hl1_ta0": 0,
    "lean_x2_pend0_pipe0_lr0_tm0_sb0": 0, "lean_x2_pend0_pipe0_lr0_tm0_sb1": 0, "lean_x2_pend0_pipe0_lr0_tm1_sb0": 1,
    "lean_x2_pend0_pipe0_lr0_tm1_sb1": 0, "lean_x2_pend0_pipe1_lr0_tm0_sb0": 0, "lean_x2_pend0_pipe1_lr0_tm0_sb1": 0,
    "lean_x2_pend0_pipe1_lr0_tm1_sb0": 1, "lean_x2_pend0_pipe1_lr0_tm1_sb1": 0, "lean_x3_pend0_pipe0_lr0_tm0_sb0": 0,
    "lean_x3_pend0_pipe0_lr0_tm0_sb1": 0, "lean_x3_pend0_pipe0_lr0_tm1_sb0": 0, "lean_x3_pend0_pipe0_lr0_tm1_sb1": 0,
    "lean_x3_pend0_pipe1_lr0_tm0_sb0": 0, "lean_x3_pend0_pipe1_lr0_tm0_sb1": 0, "lean_x3_pend0_pipe1_lr0_tm1_sb0": 0,
    "lean_x3_pend0_pipe1_lr0_tm1_sb1": 1, "lean_x3_pend1_pipe0_lr0_tm0_sb0": 0, "lean_x3_pend1_pipe0_lr0_tm0_sb1": 0,
    "lean_x3_pend1_pipe0_lr0_tm1_sb0": 1, "lean_x3_pend1_pipe0_lr0_tm1_sb1": 0, "lean_x3_pend1_pipe1_lr0_tm0_sb0": 0,
    "lean_x3_pend1_pipe1_lr0_tm0_sb1": 0, "lean_x3_pend1_pipe1_lr0_tm1_sb0": 1, "lean_x3_pend1_pipe1_lr0_tm1_sb1": 1,
    "lean_x4_pend0_pipe0_lr0_tm0_sb0": 0, "lean_x4_pend0_pipe0_lr0_tm0_sb1": 0, "lean_x4_pend0_pipe0_lr0_tm1_sb0": 0,
    "lean_x4_pend0_pipe0_lr0_tm1_sb1": 1, "lean_x4_pend0_pipe1_lr0_tm0_sb0": 0, "lean_x4_pend0_pipe1_lr0_tm0_sb1": 0,
    "lean_x4_pend0_pipe1_lr0_tm1_sb0": 1, "lean_x4_pend0_pipe1_lr0_tm1_sb1": 0, "lean_x2_pend0_pipe0_lr1_tm0_sb0": 0,
    "lean_x2_pend0_pipe0_lr1_tm0_sb1": 0, "lean_x2_pend0_pipe0_lr1_tm1_sb0": 0, "lean_x2_pend0_pipe0_lr1_tm1_sb1": 0,
    "lean_x2_pend0_pipe1_lr1_tm0_sb0": 0, "lean_x2_pend0_pipe1_lr1_tm0_sb1": 0, "lean_x2_pend0_pipe1_lr1_tm1_sb0": 0,
    "lean_x2_pend0_pipe1_lr1_tm1_sb1": 0, "lean_x3_pend0_pipe0_lr1_tm0_sb0": 0, "lean_x3_pend0_pipe0_lr1_tm0_sb1": 0,
    "lean_x3_pend0_pipe0_lr1_tm1_sb0": 0, "lean_x3_pend0_pipe0_lr1_tm1_sb1": 1, "lean_x3_pend0_pipe1_lr1_tm0_sb0": 0,
    "lean_x3_pend0_pipe1_lr1_tm0_sb1": 0, "lean_x3_pend0_pipe1_lr1_tm1_sb0": 0, "lean_x3_pend0_pipe1_lr1_tm1_sb1": 0,
    "lean_x4_pend0_pipe0_lr1_tm0_sb0": 0, "lean_x4_pend0_pipe0_lr1_tm0_sb1": 0, "lean_x4_pend0_pipe0_lr1_tm1_sb0": 0,
    "lean_x4_pend0_pipe0_lr1_tm1_sb1": 2, "lean_x4_pend0_pipe1_lr1_tm0_sb0": 0, "lean_x4_pend0_pipe1_lr1_tm0_sb1": 0,
    "lean_x4_pend0_pipe1_lr1_tm1_sb0": 0, "lean_x4_pend0_pipe1_lr1_tm1_sb1": 0, "openloop_sb0": 0,
    "openloop_sb1": 1,
}


def _case(index: int, k: dict) -> dict:
    name = kernel_name(k)
    return dict(name=name, index=index, kernel=k, opt=options(k), seed=SEEDS.get(name))


CASES = {kernel_name(k): _case(i, k) for i, k in enumerate(kernels()) if kernel_name(k) not in UNREACHABLE}


def expected_hook(name: str) -> tuple:
    """What mbpo_debug_last_rollout_kernel reports after the case ran."""
    c = CASES[name]
    k = dict(c["kernel"])
    if k["family"] in (FWIDE, FOPEN):
        k["TM"] = c["opt"]["box"]
    if k["family"] == FOPEN:
        k["H"] = 0
    return tuple(k[f] for f in FIELDS)


def tol(name: str) -> float:
    return 5e-4 if CASES[name]["kernel"]["W"] else 2e-4


def lean_knob(name: str) -> int:
    """mbpo_debug_set_rollout_lean of the case: 2 / 3 force PIPE on / off in the lean family, -1 (the default) elsewhere."""
    k = CASES[name]["kernel"]
    return (2 if k["PIPE"] else 3) if k["family"] == FLEAN else -1


def term_table(X: int, UE: int):
    """The case's term table (tests/term_reward_cases.py's layout and its mix of functions and links), by rule from the widths."""
    return (X, UE, 0.3, [
        (0.5, "identity", [("x_next", X - 1, "identity", 0.8, 0.1)]),
        (-0.1, "identity", [("u", d, "square", 1.0 - 0.25 * d, 0.0) for d in range(UE)]),
        (-0.4, "sqrt", [("x", 0, "square", 1.0, 0.2), ("x", 1, "square", 1.0, -0.3)]),
        (1.0, "exp", [("x_next", 0, "square", -1.5, 0.1), ("x_next", 1, "square", -1.2, 0.0)]),
        (0.25, "identity", [("x", X // 2, "cos", 1.0, 0.0), ("x_next", X - 2, "sin", 0.7, 0.5), ("x", X - 1, "abs", -0.5, 0.2)]),
        (0.2, "tanh", [("u", 0, "identity", 1.5, 0.0), ("x", X - 1, "identity", -1.0, 0.0)]),
    ])


def _pendulum_obs(n, gen, speed):
    th = (torch.rand(n, generator=gen) * 2 - 1) * math.pi
    thd = (torch.rand(n, generator=gen) * 2 - 1) * speed
    return torch.stack([torch.cos(th), torch.sin(th), thd], dim=1)


def _member_params(dims, E, g) -> torch.Tensor:
    return torch.cat([onets.init_mlp_flat(dims, g) + 0.05 * torch.randn(onets.n_params(dims), generator=g) for _ in range(E)])


def hold() -> taref.Hold:
    from mbpo.systems import TimeAdaptive
    ks = TimeAdaptive(DT, (HOLD_K + 0.999) * DT, DT, switch_cost=HOLD_COST, continuous_discounting=HOLD_CD).kernel_spec()
    assert ks["hold_max_steps"] == HOLD_K
    return taref.Hold(ks["hold_min_time"], ks["hold_max_time"], ks["hold_dt"], ks["hold_max_steps"], ks["hold_gamma"], ks["hold_switch_cost"])


@functools.lru_cache(maxsize=512)
def build(name: str, seed: int | None = None) -> dict:
    """The inputs of case `name` at `seed` (None: the table's)."""
    c = CASES[name]
    k, o = c["kernel"], c["opt"]
    seed = c["seed"] if seed is None else seed
    assert seed is not None, f"{name}: no seed in SEEDS"
    fam = k["family"]
    pend = pendulum_system(k)
    if fam == F64:
        X, hidden, E = (9 if k["W"] else 5), (64, 64, 64), 5
    elif fam == FWIDE:
        X, hidden, E = 5, (k["H"], k["H"]), (3 if k["H"] == 128 else 2)
    else:
        X, hidden, E = k["X"], (64, 64, 64), (0 if pend else 5)
    UE = 1
    A = UE + X if k["HL"] else (UE + 1 if k["TA"] else UE)
    S = 4 + zlib.crc32(f"{name}/S".encode()) % 2
    AR = o["AR"]
    KI = HOLD_K if k["TA"] else AR                      # inner steps per decision: the stride of the model-noise / member indices
    mode, noise = o["mode"], bool(o["noise"])
    reward = "pendulum" if (fam in (FLEAN, FOPEN) and k["PEND"]) else "quadratic"
    g = torch.Generator().manual_seed(64 * zlib.crc32(name.encode()) + seed)      # (by name: a new kernel moves no other case's inputs)
    offset = OFFSET + seed
    b = dict(name=name, kernel=k, opt=o, X=X, UE=UE, A=A, E=E, S=S, AR=AR, KI=KI, hidden=hidden, mode=mode, noise=noise, reward=reward,
             pend=pend, openloop=fam == FOPEN, ppo=bool(o["ppo"]), env_major=bool(o["ppo"]), offset=offset,
             TM=bool(o["box"]), SB=bool(k["SB"]), LR=k["LR"], HL=bool(k["HL"]), TA=bool(k["TA"]))
    b["pdims"] = [X, *hidden, 2 * A]
    b["ppar"] = onets.init_mlp_flat(b["pdims"], g) + 0.02 * torch.randn(onets.n_params(b["pdims"]), generator=g)
    if not pend:
        b["ddims"] = [X + UE, *hidden, 2 * X + (2 if k["LR"] == LR_LEARNED else 0)]
        b["dpar"] = _member_params(b["ddims"], E, g)
    b["beta"] = torch.rand(X, generator=g) * 1.5 + 0.5
    b["rparams"] = torch.cat([torch.randn(X, generator=g), torch.rand(X, generator=g), torch.rand(UE, generator=g) * 0.1])
    if X == 3 and reward == "pendulum":
        b["obs0"], b["first"] = _pendulum_obs(N, g, 2.4), _pendulum_obs(N, g, 2.4)
        lo, hi = [-INF, -INF, -2.5], [INF, INF, 2.5]
    else:
        b["obs0"], b["first"] = torch.randn(N, X, generator=g), torch.randn(N, X, generator=g)
        lo, hi = [-1.15] + [-INF] * (X - 1), [1.15] + [INF] * (X - 1)
    b["low"], b["high"] = torch.tensor(lo), torch.tensor(hi)
    b["steps0"] = (torch.arange(N) % L).float()
    b["done0"] = (torch.rand(N, generator=g) < 0.15).float()
    b["nm"] = torch.randn(X, generator=g) * 0.3 if o["norm"] else None
    b["ns"] = torch.rand(X, generator=g) + 0.5 if o["norm"] else None
    b["actions"] = (torch.rand(S, N, A, generator=g) * 2 - 1) if b["openloop"] else None
    if o["philox"]:      # the draws the kernels make themselves (csrc: element (s N + env) U + d, ((s K + j) N + env) [X + c])
        f = lambda stream, n: torch.from_numpy(np.asarray(philox.philox_normal(SEED, offset, stream, np.arange(n, dtype=np.uint64)))).float()
        b["pnoise"] = f(philox.STREAM_POLICY_NOISE, S * N * A).reshape(S, N, A)
        b["mnoise"] = f(philox.STREAM_MODEL_NOISE, S * KI * N * X).reshape(S, KI, N, X) if noise else None
        b["midx"] = None
        if mode == "ts1":
            m = philox.philox_randint(SEED, offset, philox.STREAM_MEMBER, np.arange(S * KI * N, dtype=np.uint64), 0, E)
            b["midx"] = torch.from_numpy(np.asarray(m).astype(np.int32)).reshape(S, KI, N)
    else:
        b["pnoise"] = None if b["openloop"] else torch.randn(S, N, A, generator=g)
        b["mnoise"] = torch.randn(S, KI, N, X, generator=g) if noise else None
        b["midx"] = torch.randint(0, max(E, 1), (S, KI, N), generator=g, dtype=torch.int32) if mode == "ts1" else None
    # the true buffer: 50 rows [obs | action | reward | discount | next_obs] in three inserts
    rows = torch.randn(sum(BUF_INSERTS), 2 * X + UE + 2, generator=g)
    rows[:, :X] = _pendulum_obs(rows.shape[0], g, 2.4) if reward == "pendulum" else 0.5 * torch.randn(rows.shape[0], X, generator=g)
    b["buffer"] = rows
    b["table"] = term_table(X, UE) if X >= 5 else None
    return b


def dispatch(b: dict, knob: int, n_cus: int = 256) -> tuple:
    """The kernel mbpo_model_rollout picks for the inputs `b` under mbpo_debug_set_rollout_lean(knob), as FIELDS: a restatement of
    rollout_plan / rollout_dispatch (csrc/rollout.hip), rollout_lean_supports and rollout_lean_launch (csrc/rollout_lean.hip)."""
    X, A, E, hidden = b["X"], b["A"], b["E"], tuple(b["hidden"])
    has_policy = not b["openloop"]
    lr, tm, sb, hl, ta = b["LR"], int(b["TM"]), int(b["SB"]), int(b["HL"]), int(b["TA"])
    if not ta and not has_policy and b["pend"] and b["reward"] == "pendulum" and not b["ppo"] and knob != 0:
        return tuple(_kernel(family=FOPEN, X=3, PEND=1, TM=tm, SB=sb)[f] for f in FIELDS)
    H = hidden[0] if (has_policy or not b["pend"]) else 64
    if H != 64:
        return tuple(_kernel(family=FWIDE, H=H, LR=lr, TM=tm, SB=sb, HL=hl, TA=ta)[f] for f in FIELDS)
    dyn_out = None if b["pend"] else b["ddims"][-1]
    lean = (knob != 0 and not ta and has_policy and lr != LR_TERMS and A == 1 and 2 <= X <= 4 and b["AR"] == 1 and
            hidden in ((64, 64, 64), (64, 64)) and oro.row_len(X, A, b["ppo"]) <= 16 and
            ((b["pend"] and X == 3) or (not b["pend"] and 1 <= E <= 5 and dyn_out in (X, 2 * X, 2 * X + 2))))
    if lean:
        n_tiles = (N + 15) // 16
        pipe = E > 0 and (knob == 2 or (knob != 3 and n_tiles >= 2 * n_cus))
        pend = b["pend"] or b["reward"] == "pendulum"
        return tuple(_kernel(family=FLEAN, H=64, X=X, PEND=int(pend), PIPE=int(pipe), LR=lr, TM=tm, SB=sb)[f] for f in FIELDS)
    wide = (has_policy and (X > 16 or 2 * A > 16)) or (not b["pend"] and (b["ddims"][0] > 16 or dyn_out > 16))
    return tuple(_kernel(family=F64, H=64, LR=lr, W=int(wide), TM=tm, SB=sb, HL=hl, TA=ta)[f] for f in FIELDS)


def oracle_buffer(b: dict):
    """(queue, state) of oracle.replay.UniformSamplingQueue after the inserts, sample_position moved to BUF_SAMPLE_POSITION."""
    rows = b["buffer"].numpy()
    q = oreplay.UniformSamplingQueue(BUF_MAX, rows.shape[1], 1)
    st, at = q.init(), 0
    for n in BUF_INSERTS:
        st = q.insert(st, rows[at:at + n])
        at += n
    st["sample_position"] = np.int32(BUF_SAMPLE_POSITION)
    return q, st


class _Gather64:
    """oracle.replay.UniformSamplingQueue whose gathered rows are float64 (the same values)."""

    def __init__(self, queue):
        self.queue = queue

    def gather(self, qstate, idx):
        return self.queue.gather(qstate, idx).astype("float64")


def flips(name: str) -> list:
    """The single-switch flips of the case whose descriptor is valid: the box and the start buffer either way, the reward selector to
    the formula (from the formula: to the term table, where there is an ensemble and a table).  Flipping HL or TA leaves an action width
    the dynamics' input no longer matches, and W follows from the shapes: neither is a descriptor of its own."""
    b_k = CASES[name]["kernel"]
    out = [("TM", None), ("SB", None)]
    if b_k["LR"] != LR_FORMULA:
        out.append(("LR", LR_FORMULA))
    elif not pendulum_system(b_k) and b_k["family"] != FLEAN:
        out.append(("LR", LR_TERMS))
    return out


def _system(b: dict, dtype, lr: int):
    X, UE, E = b["X"], b["UE"], b["E"]
    if b["pend"]:
        return osys.PendulumSystem()
    dpar = b["dpar"].to(dtype)
    if b["reward"] == "pendulum":
        rfn = lambda x, u: osys.pendulum_reward(x, u, osys.PendulumParams())
    else:
        tgt, q, r = b["rparams"][:X], b["rparams"][X:2 * X], b["rparams"][2 * X:]
        rfn = lambda x, u: osys.quadratic_reward(x, u, tgt.to(x.dtype), q.to(x.dtype), r.to(x.dtype))
    if b["HL"]:
        if lr == LR_TERMS:
            return trref.TermHallucinatedSystem(b["table"], dpar, b["ddims"], E, b["beta"].to(dtype))
        return href.HallucinatedEnsembleSystem(dpar, b["ddims"], E, X, UE, b["beta"].to(dtype), learned_reward=lr == LR_LEARNED, reward_fn=rfn)
    kw = dict(mode=b["mode"], sample_noise=b["noise"], min_std=1e-3)
    if lr == LR_TERMS:
        return trref.TermEnsembleSystem(b["table"], dpar, b["ddims"], E, **kw)
    if lr == LR_LEARNED:
        return lref.LearnedRewardEnsembleSystem(dpar, b["ddims"], E, X, UE, **kw)
    return osys.EnsembleSystem(dpar, b["ddims"], E, X, UE, reward_fn=rfn, **kw)


def _openloop(run, st, actions, episode_length, action_repeat):
    rows = []
    for s in range(actions.shape[0]):
        nst, reward, trunc = oro.env_step(run, st, actions[s], episode_length, action_repeat, 0, None, None)
        rows.append(torch.cat([st.obs, actions[s], reward[:, None], (1 - nst.done)[:, None], nst.obs, trunc[:, None]], dim=1))
        st = nst
    return st, torch.cat(rows)


@functools.lru_cache(maxsize=1024)
def reference(name: str, dtype=torch.float64, seed: int | None = None, flip=None) -> dict:
    """The composed reference run of the case (flip: one of `flips(name)`, the same inputs with that switch changed): rows [S*N, D],
    the final EnvState, and what the conditions read — near [N] (ever within 10 * TOL of the box), terminated (envs the box ended),
    draws (start-buffer draws), hal_mean (mean |beta sd eta|), k [S, N] and int_dist (the holds)."""
    b = build(name, seed)
    TM, SB, lr = b["TM"], b["SB"], b["LR"]
    if flip is not None:
        TM, SB, lr = (not TM if flip[0] == "TM" else TM), (not SB if flip[0] == "SB" else SB), (flip[1] if flip[0] == "LR" else lr)
    X, UE, S, AR = b["X"], b["UE"], b["S"], b["AR"]
    c = lambda t: None if t is None else t.to(dtype)
    system = _system(b, dtype, lr)
    hal_terms = []
    if b["HL"]:
        inner = system.step

        def recording_step(x, a, **kw):
            _, sd, _ = system.spread(x, a[:, :UE])
            hal_terms.append((system.beta.to(x.dtype) * sd * a[:, UE:]).abs())
            return inner(x, a, **kw)

        system.step = recording_step
    st0 = oro.EnvState(c(b["obs0"]), c(b["first"]), c(b["steps0"]), c(b["done0"]))
    queue = qstate = None
    if SB:
        queue, qstate = oracle_buffer(b)
        if dtype == torch.float64:
            queue = _Gather64(queue)
    margin = 10 * tol(name)
    out = dict(near=torch.zeros(N, dtype=torch.bool), terminated=0, draws=0, hal_mean=None, k=None, int_dist=None)
    if b["TA"]:
        h = hold()
        r = taref.rollout(system, UE, h, c(b["ppar"]), b["pdims"], st0, S, L, box=(b["low"], b["high"]) if TM else None, norm_mean=c(b["nm"]),
                          norm_std=c(b["ns"]), policy_noise=c(b["pnoise"]), model_noise=c(b["mnoise"]), member_idx=b["midx"],
                          ppo_extras=b["ppo"], env_major=b["env_major"],
                          start=dict(queue=queue, qstate=qstate, seed=SEED, offset=b["offset"]) if SB else None)
        rows, st = r["rows"], r["state"]
        if TM:
            out.update(near=~(r["box_dist"] >= margin).all(dim=0), terminated=int((r["term_at"] >= 0).any(dim=0).sum()))
        if SB:
            out.update(draws=int(r["reset"].sum()))
        rr = rows.reshape(N, S, -1).permute(1, 0, 2) if b["env_major"] else rows.reshape(S, N, -1)
        out.update(k=r["k"], int_dist=taref.integer_distance(rr[:, :, X:X + b["A"]], UE, h))
    else:
        run = tref.TerminatingSystem(system, b["low"], b["high"]) if TM else system
        kw = dict(action_repeat=AR, policy_noise=c(b["pnoise"]), model_noise=c(b["mnoise"]), member_idx=b["midx"], ppo_extras=b["ppo"],
                  env_major=b["env_major"], norm_mean=c(b["nm"]), norm_std=c(b["ns"]))
        if SB:
            st, rows, draws = fref.rollout(run, c(b["ppar"]), b["pdims"], st0, S, L, queue=queue, qstate=qstate, seed=SEED, offset=b["offset"],
                                           actions=c(b["actions"]), **kw)
            out.update(draws=len(draws))
        elif b["openloop"]:
            st, rows = _openloop(run, st0, c(b["actions"]), L, AR)
        else:
            st, rows = oro.rollout(run, c(b["ppar"]), b["pdims"], st0, S, L, **kw)
        if TM:
            out.update(near=run.near_mask(margin), terminated=int(run.terminated_mask(last_of=AR).sum()))
    if hal_terms:
        out.update(hal_mean=float(torch.cat(hal_terms).mean()))
    out.update(rows=rows, state=st)
    return out


def integer_columns(b: dict) -> list:
    """The row columns that hold integers: discount and truncation."""
    D = oro.row_len(b["X"], b["A"], b["ppo"])
    return [b["X"] + b["A"] + 1, D - 1]


def gap(a: torch.Tensor, ref: torch.Tensor, t: float) -> float:
    """max |a - ref| / (t + t |ref|): the distance in units of the tolerance (atol = rtol = t); inf where a is not finite."""
    if a.numel() == 0:
        return 0.0
    a, ref = a.double(), ref.double()
    if not bool(torch.isfinite(a).all()):
        return INF
    return float(((a - ref).abs() / (t + t * ref.abs())).max())


def run_gap(ra, rb, t: float) -> float:
    """The largest `gap` over the rows and the final obs / first_obs of two runs."""
    return max(gap(ra["rows"], rb["rows"], t), gap(ra["state"].obs, rb["state"].obs, t), gap(ra["state"].first_obs, rb["state"].first_obs, t))


def run_distance(ra, rb) -> float:
    """max |difference| over the rows and the final obs / first_obs of two fp64 runs."""
    f = lambda x, y: float((x - y).abs().max())
    return max(f(ra["rows"], rb["rows"]), f(ra["state"].obs, rb["state"].obs), f(ra["state"].first_obs, rb["state"].first_obs))


@functools.lru_cache(maxsize=None)
def examine(name: str, seed: int | None = None) -> dict:
    """Every condition on the case's inputs at `seed`, from the reference runs alone.  `ok`: all hold.  The flips are only run once
    everything else holds."""
    b = build(name, seed)
    t = tol(name)
    r64, r32 = reference(name, torch.float64, seed), reference(name, torch.float32, seed)
    cols = integer_columns(b)
    res = dict(near=int(r64["near"].sum()), ref_gap=run_gap(r32, r64, t),
               ints_agree=bool(torch.equal(r32["rows"][:, cols].double(), r64["rows"][:, cols]) and
                               torch.equal(r32["state"].steps.double(), r64["state"].steps) and
                               torch.equal(r32["state"].done.double(), r64["state"].done) and
                               (not b["SB"] or torch.equal(r32["state"].first_obs.double(), r64["state"].first_obs))),
               excluded=0.0)
    cond = dict(near=res["near"] == 0, ref_gap=res["ref_gap"] <= 0.25, ints_agree=res["ints_agree"],
                finite=bool(torch.isfinite(r64["rows"]).all()))
    if b["TM"]:
        res["terminated"] = r64["terminated"]
        cond["terminated"] = r64["terminated"] >= MIN_TERMINATIONS
    if b["SB"]:
        res["draws"] = r64["draws"]
        res["first_changed"] = not torch.equal(r64["state"].first_obs, b["first"].double())
        cond["draws"] = r64["draws"] >= 1 and res["first_changed"]
    if b["HL"]:
        res["hal_mean"] = r64["hal_mean"]
        cond["hal_mean"] = r64["hal_mean"] > EFFECT * t
    if b["TA"]:
        res["int_dist"] = float(r64["int_dist"].min())
        res["holds"] = sorted(set(r64["k"].reshape(-1).tolist()))
        cond["int_dist"] = res["int_dist"] >= INT_MARGIN and bool(torch.equal(r32["k"], r64["k"]))
        cond["holds"] = res["holds"] == list(range(1, HOLD_K + 1))
    if all(cond.values()):
        for fl in flips(name):
            d = run_distance(r64, reference(name, torch.float64, seed, fl))
            key = "flip_" + fl[0]
            res[key] = d
            cond[key] = d > EFFECT * t
            if fl[0] == "LR" and b["LR"] != LR_FORMULA:      # the reward column against the formula reward's
                col = b["X"] + b["A"]
                res["reward_effect"] = float((r64["rows"][:, col] - reference(name, torch.float64, seed, fl)["rows"][:, col]).abs().max())
                cond["reward_effect"] = res["reward_effect"] > EFFECT * t
    res.update(cond=cond, ok=all(cond.values()))
    return res


def first_seed(name: str):
    """The first seed in 0 .. 63 at which every condition holds (None: there is none)."""
    for s in range(64):
        if examine(name, s)["ok"]:
            return s
    return None


# ------------------------------------------------------------------------------------------------ the device side
def device_buffer(b: dict, dev):
    """(data, state) of the case's true buffer on the device, through mbpo_replay_insert (head != 0)."""
    from mbpo import ops
    rows = b["buffer"].to(dev)
    data = torch.zeros(BUF_MAX, rows.shape[1], device=dev)
    state = torch.zeros(4, dtype=torch.int32, device=dev)
    at = 0
    for n in BUF_INSERTS:
        ops.replay_insert(data, state, rows[at:at + n].contiguous())
        at += n
    state[1] = BUF_SAMPLE_POSITION
    return data, state


def device_table(b: dict, dev):
    from mbpo.systems import Group, Term, TermReward
    X, U, bias, groups = b["table"]
    rew = TermReward(X, U, bias=bias, groups=[Group([Term(*t) for t in terms], weight=w, link=link) for w, link, terms in groups])
    return rew.kernel_spec(rew.init_params(0), dev)[1]


def run_device(name: str, dev):
    """Case `name` through ops.model_rollout (the caller sets the lean knob).  Returns (rows, obs, first_obs, steps, done) on the host."""
    from mbpo import _hip, ops
    b = build(name)
    d = lambda t: None if t is None else t.contiguous().to(dev)
    obs, first, steps, done = d(b["obs0"]).clone(), d(b["first"]).clone(), d(b["steps0"]).clone(), d(b["done0"]).clone()
    px = bool(b["opt"]["philox"])
    kw = dict(x_dim=b["X"], u_dim=b["A"], obs=obs, first_obs=first, steps=steps, done=done, n_steps=b["S"], episode_length=L,
              action_repeat=b["AR"], ppo_extras=b["ppo"], env_major=b["env_major"], seed=SEED, offset=b["offset"])
    if b["openloop"]:
        kw.update(actions=d(b["actions"]))
    else:
        kw.update(policy_params=d(b["ppar"]), policy_spec=ops.MlpSpec(b["pdims"], "swish", 1), norm_mean=d(b["nm"]), norm_std=d(b["ns"]),
                  policy_noise=None if px else d(b["pnoise"]))
    if b["pend"]:
        p = osys.PendulumParams()
        kw.update(system_kind=_hip.SYS_PENDULUM, sys_params=torch.tensor(p.sys_vector(), device=dev), reward_kind=_hip.REWARD_PENDULUM,
                  reward_params=torch.tensor(p.reward_vector(), device=dev))
    else:
        kw.update(system_kind=_hip.SYS_ENSEMBLE, dyn_params=d(b["dpar"]), dyn_spec=ops.MlpSpec(b["ddims"], "swish", b["E"]),
                  ens_mode={"mean": _hip.ENS_MEAN, "ts1": _hip.ENS_TS1, "tsinf": _hip.ENS_TSINF}[b["mode"]], ens_predict_delta=True,
                  ens_sample_noise=b["noise"], ens_min_std=1e-3, model_noise=None if px else d(b["mnoise"]),
                  member_idx=None if px else d(b["midx"]))
        if b["LR"] == LR_LEARNED:
            kw.update(reward_kind=_hip.REWARD_LEARNED, reward_params=None)
        elif b["LR"] == LR_TERMS:
            kw.update(reward_kind=_hip.REWARD_TERMS, reward_params=device_table(b, dev))
        elif b["reward"] == "pendulum":
            kw.update(reward_kind=_hip.REWARD_PENDULUM, reward_params=torch.tensor(osys.PendulumParams().reward_vector(), device=dev))
        else:
            kw.update(reward_kind=_hip.REWARD_QUADRATIC, reward_params=d(b["rparams"]))
    if b["TM"]:
        kw.update(term_low=d(b["low"]), term_high=d(b["high"]))
    if b["SB"]:
        data, state = device_buffer(b, dev)
        kw.update(start_rows=data, start_state=state)
    if b["HL"]:
        kw.update(halluc_beta=d(b["beta"]))
    if b["TA"]:
        h = hold()
        kw.update(hold_max_steps=h.K, hold_min_time=h.t_lo, hold_max_time=h.t_hi, hold_dt=h.dt, hold_gamma=h.gamma, hold_switch_cost=h.switch_cost)
    rows = ops.model_rollout(**kw)
    torch.cuda.synchronize()
    return rows.cpu(), obs.cpu(), first.cpu(), steps.cpu(), done.cpu()


def last_kernel() -> tuple:
    """mbpo_debug_last_rollout_kernel: the FIELDS of the kernel mbpo_model_rollout launched last."""
    import ctypes as C
    from mbpo import _hip
    lib = _hip.load()
    buf = (C.c_int32 * len(FIELDS))()
    lib.mbpo_debug_last_rollout_kernel.argtypes = [C.c_void_p, C.c_int32]
    lib.mbpo_debug_last_rollout_kernel.restype = C.c_int
    assert lib.mbpo_debug_last_rollout_kernel(buf, len(FIELDS)) == 0
    return tuple(buf)
