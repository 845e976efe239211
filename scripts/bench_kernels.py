"""Per-kernel rooflines for every row of SURVEY §8a (the secondary measurements of SURVEY §8d).

    python scripts/bench_kernels.py [--out profiles/r02_kernel_rooflines.json]

Each entry: the C-ABI entry point, the configuration, average launch time from HIP events on the launch stream, the
ALGORITHMIC work per unit (SURVEY §8d's figures, restated next to each case), achieved GB/s or TFLOP/s and the fraction of the
bounding roof (HBM 8 TB/s, fp32 MFMA 157.3 TFLOP/s; MI355X_MICROARCH.md).  Small cases are the BASELINE.json configurations
(launch-latency-bound: their time is the ~4.5 us kernel floor); the "large" case of every HBM-bound kernel is sized so the
launch floor is negligible and shows what the kernel reaches against the roof.
Inputs are synthetic (seeded); nothing under oracle/ or /root/reference is touched.
"""
import argparse
import json
import math
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "model-based-policy-optimizers_amd"))

import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0
LAST_EAGER = None     # eager (Python + launch API) time per call of the case measured last
MFMA_F32_PEAK_TF = 157.3


def mlp_macs(dims):
    return sum(a * b for a, b in zip(dims[:-1], dims[1:]))


def lecun_flat(dims, g, n_nets=1):
    parts = []
    for _ in range(n_nets):
        for i, o in zip(dims[:-1], dims[1:]):
            lim = math.sqrt(3.0 / i)
            parts += [((torch.rand(i, o, generator=g) * 2 - 1) * lim).reshape(-1), torch.zeros(o)]
    return torch.cat(parts)


def timed(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    st = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        fn()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def timed_graph(fn, inner=20, reps=10):
    """Device-side time per call: `inner` calls captured into one hipGraph and replayed (no Python / launch-API time between
    kernels).  Returns None when the op cannot be captured."""
    try:
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(inner):
                fn()
        graph.replay()
        torch.cuda.synchronize()
        st = torch.cuda.current_stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(reps):
            graph.replay()
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / (reps * inner)
    except Exception as e:      # noqa: BLE001
        print(f"  (graph capture failed: {type(e).__name__}: {str(e)[:120]})", file=sys.stderr)
        torch.cuda.synchronize()
        return None


def both(fn, reps, warm=5, inner=20):
    """(device time per call under graph replay if capturable else eager, eager time per call)"""
    global LAST_EAGER
    te = timed(fn, reps, warm)
    LAST_EAGER = te
    tg = timed_graph(fn, inner=inner, reps=max(2, reps // inner))
    return (tg if tg is not None else te), te


def hbm_entry(name, entry, cfg, t, nbytes, unit_note):
    gbs = nbytes / t / 1e9
    return {"kernel": name, "entry": entry, "config": cfg, "device_us": t * 1e6, "eager_us": LAST_EAGER * 1e6, "bound": "hbm", "algorithmic_bytes": nbytes,
            "per_unit": unit_note, "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS}


def mfma_entry(name, entry, cfg, t, flop, unit_note, extra=None):
    tf = flop / t / 1e12
    e = {"kernel": name, "entry": entry, "config": cfg, "device_us": t * 1e6, "eager_us": LAST_EAGER * 1e6, "bound": "mfma", "algorithmic_flop": flop,
         "per_unit": unit_note, "achieved": tf, "peak": MFMA_F32_PEAK_TF, "unit": "TFLOP/s", "frac": tf / MFMA_F32_PEAK_TF}
    if extra:
        e.update(extra)
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="run only the cases whose function name contains this (rollout, ens_fwd, sac, ppo, bptt, icem, ...)")
    args = ap.parse_args()
    want = lambda name: args.only is None or args.only in name
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: the HIP path has no CPU fallback")
    from mbpo import _hip, ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    out = []

    def log(s):
        print(s, file=sys.stderr, flush=True)

    # ---------------------------------------------------------------- P4: GAE scan (24 B / element)
    for (B, T, reps) in [(16384, 5, 200), (16384, 40, 200), (1 << 20, 40, 20)]:
        f = lambda: torch.rand(B, T, generator=g).to(dev)
        trunc, term = (f() < 0.05).float(), (f() < 0.02).float()
        rew, val, boot = f(), f(), torch.rand(B, generator=g).to(dev)
        t, te = both(lambda: ops.gae_scan(trunc, term, rew, val, boot, 0.99, 0.95), reps)
        out.append(hbm_entry("k_gae_scan", "mbpo_gae_scan", {"B": B, "T": T}, t, 24 * B * T, "24 B per element (4 reads + 2 writes)"))
        out[-1]["elements_per_s"] = B * T / t
        log(f"gae {B}x{T}: {t * 1e6:.1f} us (eager {te * 1e6:.1f})")
        del trunc, term, rew, val, boot
    # ---------------------------------------------------------------- B2: lambda-return scan (12 B / element)
    for (B, T, reps) in [(4096, 32, 200), (1 << 20, 32, 20)]:
        rew, nv = torch.rand(B, T, generator=g).to(dev), torch.rand(B, T, generator=g).to(dev)
        t, te = both(lambda: ops.lambda_return_scan(rew, nv, 0.99, 0.97), reps)
        out.append(hbm_entry("k_lambda_return_scan", "mbpo_lambda_return_scan", {"B": B, "T": T}, t, 12 * B * T,
                             "12 B per element (2 reads + 1 write)"))
        log(f"lambda {B}x{T}: {t * 1e6:.1f} us")
        del rew, nv
    # ---------------------------------------------------------------- R6/S1: replay insert / sample (48 B rows)
    D = 12
    for (mx, n, reps) in [(1 << 20, 20480, 200), (1 << 22, 1 << 20, 20)]:
        data = torch.zeros(mx, D, device=dev)
        state = torch.zeros(4, dtype=torch.int32, device=dev)
        rows = torch.rand(n, D, generator=g).to(dev)
        t, te = both(lambda: ops.replay_insert(data, state, rows), reps)
        out.append(hbm_entry("k_replay_insert", "mbpo_replay_insert", {"max_replay": mx, "rows": n, "D": D}, t, 2 * 48 * n,
                             "48 B read + 48 B write per row (SURVEY counts the 48 B write only)"))
        log(f"insert {n}: {t * 1e6:.1f} us")
        # (256 x 64 = 16384 rows: the sampling launch of the benchmark's training step, plain and with MBPO's real_ratio)
        for (ns, r2) in ([(256, 200), (256 * 64, 200)] if n == 20480 else [(1 << 20, 20)]):
            buf = torch.empty(ns, D, device=dev)
            t, te = both(lambda: ops.replay_sample(data, state, ns, 1, 0, out=buf), r2)
            out.append(hbm_entry("k_replay_sample", "mbpo_replay_sample", {"max_replay": mx, "rows": ns, "D": D}, t, 2 * 48 * ns,
                                 "48 B read + 48 B write per sampled row (random rows: 64 B sectors)"))
            log(f"sample {ns}: {t * 1e6:.1f} us")
            if ns == 256 * 64:
                mb, n_real, rmx, RD = 256, 12, 100_000, 11
                rdata = torch.rand(rmx, RD, generator=g).to(dev)
                rstate = torch.tensor([rmx, 0, 0, rmx], dtype=torch.int32, device=dev)          # a full real ring
                t, te = both(lambda: ops.replay_sample_mixed(data, state, rdata, rstate, ns, mb, n_real, 1, 0, 1 << 32, out=buf), r2)
                nb = 48 * ns + (ns // mb) * (n_real * 4 * RD + (mb - n_real) * 48)
                out.append(hbm_entry("k_replay_sample_mixed", "mbpo_replay_sample_mixed",
                                     {"max_replay": mx, "real_replay": rmx, "rows": ns, "minibatch": mb, "n_real": n_real, "D": D, "real_D": RD},
                                     t, nb, "48 B write per row + 48 B (model) or 44 B (real) read"))
                log(f"sample_mixed {ns} ({n_real} real of every {mb}): {t * 1e6:.1f} us")
                del rdata
        del data, rows
    # ---------------------------------------------------------------- R8: running statistics (2 passes over x columns)
    for (n, reps) in [(20480, 200), (1 << 22, 10)]:
        X = 4
        rows = torch.rand(n, D, generator=g).to(dev)
        stats = torch.cat([torch.zeros(1 + 2 * X), torch.ones(X)]).to(dev)
        sums = torch.zeros(1 + 2 * X, device=dev)
        ws = torch.empty(ops.stats_workspace_floats(X), device=dev)
        t, te = both(lambda: ops.running_stats_update(rows, 0, X, stats, sums=sums, workspace=ws), reps)
        out.append(hbm_entry("k_running_stats (2 reduce passes + apply)", "mbpo_running_stats_reduce x2 + _apply",
                             {"rows": n, "x": X, "row_len": D}, t, 2 * 4 * X * n,
                             "2 passes x 4x B per row (the obs columns; rows are 48 B apart, so sectors fetch 3x that)"))
        log(f"stats {n}: {t * 1e6:.1f} us (3 launches)")
        del rows
    # ---------------------------------------------------------------- S8/B4: AdamW (+ Polyak)  28 / 36 B per parameter
    for (n, reps) in [(26309, 200), (1 << 24, 20)]:
        opt = ops.AdamW(n, dev, lr=3e-4, weight_decay=0.0)
        p, gr, tgt = torch.randn(n, generator=g).to(dev), torch.randn(n, generator=g).to(dev), torch.zeros(n, device=dev)
        t, te = both(lambda: opt.step(p, gr, target=tgt, tau=0.005), reps)
        out.append(hbm_entry("k_adamw_step (+Polyak)", "mbpo_adamw_step", {"params": n}, t, 36 * n,
                             "36 B per parameter (read g,p,m,v,target; write p,m,v,target)"))
        log(f"adamw {n}: {t * 1e6:.1f} us")
        del p, gr, tgt, opt

    # ---------------------------------------------------------------- R1-R7: fused model rollout
    def rollout_case(N, X, U, E, S, hid_pi, hid_dyn, reps, learned_reward=False, terminate=False, start_buffer=False):
        # start_buffer: a full 100 000-row true buffer (mbpo_rollout_desc.start_*): every reset — each env's last step of every launch,
        # the horizon being S — is followed by a fresh draw into first_obs (the trainers' resample_starts)
        # terminate: a termination box |x0| <= 1 (mbpo_rollout_desc.term_low / term_high; envs that leave it restart from first_obs)
        # learned_reward: the members carry the reward head (2X + 2 outputs) and the rollout reads it (MBPO_REWARD_LEARNED)
        pd, dd = [X, *hid_pi, 2 * U], [X + U, *hid_dyn, 2 * X + (2 if learned_reward else 0)]
        pp = lecun_flat(pd, g).to(dev)
        dp = lecun_flat(dd, g, E).to(dev)
        pd_k, dd_k = pd, dd
        w = ops.common_width(hid_pi, hid_dyn, supported=ops.ROLLOUT_WIDTHS)
        if any(h != w for h in (*hid_pi, *hid_dyn)):
            # the fused kernel walks policy and members at ONE hidden width in {64, 128, 256}: the host zero-pads the narrower nets
            # (as the trainers and EnsembleDynamics do, INTEGRATION.md "Network shapes"); FLOP are counted on the logical shapes
            pp, dp = ops.embed_mlp_params(pp, pd, w), ops.embed_mlp_params(dp, dd, w, E)
            pd_k, dd_k = ops.padded_dims(pd, w), ops.padded_dims(dd, w)
        obs = torch.randn(N, X, generator=g).to(dev)
        first = obs.clone()
        steps, done = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
        rp = None if learned_reward else torch.cat([torch.zeros(X), torch.ones(X), torch.ones(U) * 0.1]).to(dev)
        rk = _hip.REWARD_LEARNED if learned_reward else _hip.REWARD_QUADRATIC
        rows = torch.empty(S * N, 2 * X + U + 3, device=dev)
        term = {}
        if terminate:
            lo, hi = torch.full((X,), float("-inf")), torch.full((X,), float("inf"))
            lo[0], hi[0] = -1.0, 1.0
            term = dict(term_low=lo.to(dev), term_high=hi.to(dev))
        if start_buffer:
            smx = 100_000
            term.update(start_rows=torch.randn(smx, 2 * X + U + 2, generator=g).to(dev),
                        start_state=torch.tensor([smx, 0, 0, smx], dtype=torch.int32, device=dev))

        def run():
            ops.model_rollout(policy_params=pp, policy_spec=ops.MlpSpec(pd_k), x_dim=X, u_dim=U, obs=obs, first_obs=first, steps=steps,
                              done=done, n_steps=S, episode_length=S, system_kind=_hip.SYS_ENSEMBLE, dyn_params=dp,
                              dyn_spec=ops.MlpSpec(dd_k, "swish", E), reward_kind=rk, reward_params=rp, seed=1,
                              offset=0, out=rows, **term)
        t, te = both(run, reps)
        flop = N * S * (2 * E * mlp_macs(dd) + 2 * mlp_macs(pd))
        e = mfma_entry("k_model_rollout", "mbpo_model_rollout",
                       {"N": N, "x": X, "u": U, "E": E, "S": S, "policy": list(hid_pi), "member": list(hid_dyn),
                        "reward": "learned" if learned_reward else "quadratic", **({"termination": "|x0| <= 1"} if terminate else {}),
                        **({"start_buffer_rows": 100_000} if start_buffer else {})}, t, flop,
                       "2*E*M + 2*P FLOP per transition", {"transitions_per_s": N * S / t})
        out.append(e)
        log(f"rollout N={N} x={X} E={E} {hid_dyn}{' learned reward' if learned_reward else ''}{' termination' if terminate else ''}{' start buffer' if start_buffer else ''}: {t * 1e6:.1f} us  "
            f"{N * S / t / 1e6:.1f} M transitions/s")

    def attempt(fn, *a):
        try:
            fn(*a)
        except Exception as e:      # noqa: BLE001 — a configuration the kernels reject is reported, not hidden
            out.append({"kernel": fn.__name__, "config": [list(x) if isinstance(x, tuple) else x for x in a], "error": str(e)[:300]})
            log(f"{fn.__name__}{a}: {e}")

    if want("rollout_case"): rollout_case(4096, 4, 1, 5, 5, (64, 64, 64), (64, 64, 64), 50)       # C2
    if want("rollout_case"): rollout_case(4096, 4, 1, 5, 5, (64, 64, 64), (64, 64, 64), 50, learned_reward=True)   # C2, learned reward
    if want("rollout_case"): rollout_case(4096, 4, 1, 5, 5, (64, 64, 64), (64, 64, 64), 50, terminate=True)        # C2, termination box
    if want("rollout_case"): rollout_case(4096, 4, 1, 5, 5, (64, 64, 64), (64, 64, 64), 50, start_buffer=True)     # C2, fresh starts
    if want("rollout_case"): rollout_case(32768, 4, 1, 5, 5, (64, 64, 64), (64, 64, 64), 20)      # C4's global env count on one GPU
    if want("rollout_case"): attempt(rollout_case, 4096, 4, 1, 5, 5, (64, 64, 64), (256, 256), 20)   # "also report 256x2" members
    if want("rollout_case"): attempt(rollout_case, 4096, 4, 1, 5, 5, (256, 256), (256, 256), 20)
    if want("rollout_case"): attempt(rollout_case, 4096, 17, 6, 10, 5, (64, 64, 64), (64, 64, 64), 20)     # C5 shape through the rollout kernel
    if want("rollout_case"): attempt(rollout_case, 4096, 4, 1, 7, 5, (64, 64, 64), (200, 200, 200, 200), 20)   # MBPO's model, stored at 256

    # hallucinated control (mbpo_rollout_desc.halluc_beta; EnsembleSystem(mode="optimistic")) next to the plain 'mean' rollout of the
    # same shape on the same kernel: k_model_rollout64 (mbpo_debug_set_rollout_lean(0): the optimistic action width u + x keeps the
    # rollout off k_rollout_lean, so the like-for-like baseline is the tile kernel, not the benchmark's default path)
    def rollout_optimistic_case(N, X, UE, E, S, hid, reps):
        lib = _hip.load()
        dd = [X + UE, *hid, 2 * X]
        dp = lecun_flat(dd, g, E).to(dev)
        obs = torch.randn(N, X, generator=g).to(dev)
        first = obs.clone()
        steps, done = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
        rp = torch.cat([torch.zeros(X), torch.ones(X), torch.ones(UE) * 0.1]).to(dev)
        beta = torch.ones(X, device=dev)
        lib.mbpo_debug_set_rollout_lean(0)
        try:
            for mode, U, extra in (("mean", UE, {}), ("optimistic", UE + X, dict(halluc_beta=beta))):
                pd = [X, *hid, 2 * U]
                pp = lecun_flat(pd, g).to(dev)
                rows = torch.empty(S * N, 2 * X + U + 3, device=dev)

                def run():
                    ops.model_rollout(policy_params=pp, policy_spec=ops.MlpSpec(pd), x_dim=X, u_dim=U, obs=obs, first_obs=first, steps=steps,
                                      done=done, n_steps=S, episode_length=S, system_kind=_hip.SYS_ENSEMBLE, dyn_params=dp,
                                      dyn_spec=ops.MlpSpec(dd, "swish", E), reward_kind=_hip.REWARD_QUADRATIC, reward_params=rp, seed=1,
                                      offset=0, out=rows, **extra)
                t, te = both(run, reps)
                flop = N * S * (2 * E * mlp_macs(dd) + 2 * mlp_macs(pd))
                out.append(mfma_entry("k_model_rollout64", "mbpo_model_rollout",
                                      {"N": N, "x": X, "u_env": UE, "action_width": U, "E": E, "S": S, "policy": list(hid), "member": list(hid),
                                       "reward": "quadratic", "mode": mode, "rollout_lean": 0}, t, flop,
                                      "2*E*M + 2*P FLOP per transition", {"transitions_per_s": N * S / t}))
                log(f"rollout ({mode}, k_model_rollout64) N={N} x={X} u_env={UE} E={E} {hid}: {t * 1e6:.1f} us  {N * S / t / 1e6:.1f} M transitions/s")
        finally:
            lib.mbpo_debug_set_rollout_lean(-1)

    if want("rollout_optimistic_case"): rollout_optimistic_case(4096, 4, 1, 5, 5, (64, 64, 64), 50)      # C2's shape, 'mean' and 'optimistic'

    # time-adaptive rollouts (mbpo_rollout_desc.hold_*; TimeAdaptive) at C2's shape with action width A = 2, next to the plain C2 row of
    # the same session: the plain rollout at u_dim = 2 (its dynamics read both columns), the hold at t_lo = t_hi = env_dt (every k = 1:
    # the cost of the flag alone) and at t_hi = 4 env_dt (tau is sampled: k in 1 .. 4, a tile runs to its largest k).  All three on
    # k_model_rollout64 (u_dim = 2 keeps the rollout off k_rollout_lean).  A record, no target.
    def rollout_time_adaptive_case(N, X, UE, E, S, hid, reps):
        from mbpo.systems import TimeAdaptive
        A, dt = UE + 1, 0.05
        obs = torch.randn(N, X, generator=g).to(dev)
        first = obs.clone()
        steps, done = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
        pd = [X, *hid, 2 * A]
        pp = lecun_flat(pd, g).to(dev)
        rows = torch.empty(S * N, 2 * X + A + 3, device=dev)
        for label, ue, hold in (("off", A, None), ("k=1", UE, TimeAdaptive(dt, dt, dt)), ("k<=4", UE, TimeAdaptive(dt, 4 * dt, dt))):
            dd = [X + ue, *hid, 2 * X]
            dp = lecun_flat(dd, g, E).to(dev)
            rp = torch.cat([torch.zeros(X), torch.ones(X), torch.ones(ue) * 0.1]).to(dev)
            extra = {} if hold is None else hold.kernel_spec()

            def run():
                ops.model_rollout(policy_params=pp, policy_spec=ops.MlpSpec(pd), x_dim=X, u_dim=A, obs=obs, first_obs=first, steps=steps,
                                  done=done, n_steps=S, episode_length=S, system_kind=_hip.SYS_ENSEMBLE, dyn_params=dp,
                                  dyn_spec=ops.MlpSpec(dd, "swish", E), reward_kind=_hip.REWARD_QUADRATIC, reward_params=rp, seed=1,
                                  offset=0, out=rows, **extra)
            t, te = both(run, reps)
            torch.cuda.synchronize()
            mean_k = 1.0
            if hold is not None:
                mean_k = float(ops.hold_steps(rows[:, X:X + A].contiguous(), dt, hold.max_time_between_switches, dt, hold.max_steps).float().mean())
            flop = N * S * (2 * E * mlp_macs(dd) * mean_k + 2 * mlp_macs(pd))
            out.append(mfma_entry("k_model_rollout64", "mbpo_model_rollout",
                                  {"N": N, "x": X, "u_env": ue, "action_width": A, "E": E, "S": S, "policy": list(hid), "member": list(hid),
                                   "reward": "quadratic", "time_adaptive": label, "hold_max_steps": 0 if hold is None else hold.max_steps,
                                   "mean_hold": mean_k}, t, flop, "2*E*M*mean_hold + 2*P FLOP per decision",
                                  {"decisions_per_s": N * S / t, "model_steps_per_s": N * S * mean_k / t}))
            log(f"rollout (time-adaptive {label}, k_model_rollout64) N={N} x={X} A={A} E={E} {hid}: {t * 1e6:.1f} us  mean hold {mean_k:.2f}  "
                f"{N * S * mean_k / t / 1e6:.1f} M model steps/s")

    if args.only is not None and want("rollout_time_adaptive_case"):      # the plain C2 row in the same session (a full run has it above)
        rollout_case(4096, 4, 1, 5, 5, (64, 64, 64), (64, 64, 64), 50)
    if want("rollout_time_adaptive_case"): rollout_time_adaptive_case(4096, 4, 1, 5, 5, (64, 64, 64), 50)

    # term rewards (MBPO_REWARD_TERMS; mbpo.systems.TermReward) at C2's shape on k_model_rollout64 (mbpo_debug_set_rollout_lean(0):
    # k_rollout_lean never takes the kind, so the like-for-like baseline is the tile kernel): the quadratic kind, the same function as a
    # table (TermReward.from_quadratic: 5 square terms in 2 groups), and a 12-term table holding cos, exp and sqrt, two of its terms on
    # the next state.  One session.  A record, no target.
    def rollout_term_reward_case(N, X, U, E, S, hid, reps):
        from mbpo.systems import Group, Term, TermReward
        lib = _hip.load()
        pd, dd = [X, *hid, 2 * U], [X + U, *hid, 2 * X]
        pp, dp = lecun_flat(pd, g).to(dev), lecun_flat(dd, g, E).to(dev)
        obs = torch.randn(N, X, generator=g).to(dev)
        first = obs.clone()
        steps, done = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
        rows = torch.empty(S * N, 2 * X + U + 3, device=dev)
        tgt, q, r = [0.0] * X, [1.0] * X, [0.1] * U
        twelve = TermReward(X, U, bias=0.5, groups=[
            Group([Term("x", c, "square", 1.0) for c in range(X)], weight=-1.0),
            Group([Term("u", 0, "square", 0.1)], weight=-1.0),
            Group([Term("x", 0, "square", 1.0, 0.5), Term("x", 1, "square", 1.0, -0.5)], weight=-0.5, link="sqrt"),
            Group([Term("x_next", 0, "square", -4.0), Term("x_next", 1, "square", -4.0)], weight=1.0, link="exp"),
            Group([Term("x", 2, "cos", 1.0), Term("x", 3, "sin", 0.5), Term("u", 0, "abs", -0.1)], weight=0.3),
        ])
        assert sum(len(gr.terms) for gr in twelve.init_params(0).groups) == 12
        quad_tab = TermReward.from_quadratic(tgt, q, r)
        cases = (("quadratic", _hip.REWARD_QUADRATIC, torch.tensor(tgt + q + r).to(dev)),
                 ("terms: from_quadratic", _hip.REWARD_TERMS, quad_tab.kernel_spec(quad_tab.init_params(0), dev)[1]),
                 ("terms: 12 terms (cos, exp, sqrt)", _hip.REWARD_TERMS, twelve.kernel_spec(twelve.init_params(0), dev)[1]))
        lib.mbpo_debug_set_rollout_lean(0)
        try:
            for label, rk, rp in cases:
                def run():
                    ops.model_rollout(policy_params=pp, policy_spec=ops.MlpSpec(pd), x_dim=X, u_dim=U, obs=obs, first_obs=first, steps=steps,
                                      done=done, n_steps=S, episode_length=S, system_kind=_hip.SYS_ENSEMBLE, dyn_params=dp,
                                      dyn_spec=ops.MlpSpec(dd, "swish", E), reward_kind=rk, reward_params=rp, seed=1, offset=0, out=rows)
                t, te = both(run, reps)
                flop = N * S * (2 * E * mlp_macs(dd) + 2 * mlp_macs(pd))
                out.append(mfma_entry("k_model_rollout64", "mbpo_model_rollout",
                                      {"N": N, "x": X, "u": U, "E": E, "S": S, "policy": list(hid), "member": list(hid), "reward": label,
                                       "rollout_lean": 0}, t, flop, "2*E*M + 2*P FLOP per transition", {"transitions_per_s": N * S / t}))
                log(f"rollout ({label}, k_model_rollout64) N={N} x={X} E={E} {hid}: {t * 1e6:.1f} us  {N * S / t / 1e6:.1f} M transitions/s")
        finally:
            lib.mbpo_debug_set_rollout_lean(-1)

    if want("rollout_term_reward_case"): rollout_term_reward_case(4096, 4, 1, 5, 5, (64, 64, 64), 50)      # C2's shape, three rewards

    # ---------------------------------------------------------------- R2: vmapped ensemble forward (System.step outside the fused rollout)
    def ens_fwd_case(N, X, U, E, hid, reps):
        dd = [X + U, *hid, 2 * X]
        spec = ops.MlpSpec(dd, "swish", E)
        dp = lecun_flat(dd, g, E).to(dev)
        xu = torch.randn(N, X + U, generator=g).to(dev)
        t, te = both(lambda: ops.ensemble_mlp_forward(dp, spec, xu), reps)
        out.append(mfma_entry("k_ensemble_forward", "mbpo_ensemble_mlp_forward", {"N": N, "x": X, "u": U, "E": E, "member": list(hid)}, t,
                              N * 2 * E * mlp_macs(dd), "2*E*M FLOP per row (shared input)", {"rows_per_s": N / t}))
        log(f"ensemble forward N={N} E={E} {hid}: {t * 1e6:.1f} us")

    if want("ens_fwd_case"): attempt(ens_fwd_case, 4096, 4, 1, 5, (64, 64, 64), 100)
    if want("ens_fwd_case"): attempt(ens_fwd_case, 32768, 4, 1, 5, (64, 64, 64), 50)

    # ---------------------------------------------------------------- S3-S8: SAC sgd_step
    def sac_case(X, U, hidden, B, reps):
        pd, qd = [X, *hidden, 2 * U], [X + U, *hidden, 1]
        up = ops.SacUpdater(x_dim=X, u_dim=U, policy_dims=pd, q_dims=qd, batch_size=B, device=dev)
        params = torch.cat([lecun_flat(pd, g), lecun_flat(qd, g, 2), torch.zeros(1)]).to(dev)
        up.load_state(params)
        batch = torch.randn(B, 2 * X + U + 3, generator=g)
        batch[:, X + U + 1] = 1.0
        batch[:, -1] = 0.0
        batch = batch.to(dev)
        # as the trainer issues it: each step's clip check is resolved by the next step's first launch (a scan of sgd_steps ends
        # in ONE mbpo_sac_finalize, not timed here)
        t, te = both(lambda: up.sgd_step(batch, defer_clip_check=True), reps)
        up.finalize()
        flop = B * 2 * (5 * mlp_macs(pd) + 12 * mlp_macs(qd))
        layered = not (len(set(hidden)) == 1 and hidden[0] in (64, 128))
        out.append(mfma_entry("k_layered_gemm x ~46 + heads + k_sac_reduce + k_sac_apply (layered path)" if layered
                              else "k_sac_fwd_bwd + k_sac_reduce_apply", "mbpo_sac_step",
                              {"x": X, "u": U, "hidden": list(hidden), "B": B}, t, flop, "2*(5P + 12Q) FLOP per sample",
                              {"updates_per_s": 1.0 / t}))
        log(f"sac sgd_step x={X} {hidden} B={B}: {t * 1e6:.1f} us")

    if want("sac_case"): sac_case(4, 1, (64, 64, 64), 256, 200)
    if want("sac_case"): sac_case(3, 1, (128, 128, 128), 256, 200)      # the reference tests' width (tests/test_sac.py)
    if want("sac_case"): attempt(sac_case, 4, 1, (64, 64, 64), 2048, 100)        # C4's global batch on one GPU
    if want("sac_case"): attempt(sac_case, 17, 6, (64, 64, 64), 256, 200)
    if want("sac_case"): attempt(sac_case, 4, 1, (256, 256, 256), 256, 50)        # wider than the fused kernels take: one GEMM launch per Dense layer
    if want("sac_case"): attempt(sac_case, 4, 1, (256, 256, 256), 4096, 20)

    # ---------------------------------------------------------------- P3-P6: PPO minibatch_step (C3)
    def ppo_case(X, U, hidden, B, T, reps, opts=None):
        pd, vd = [X, *hidden, 2 * U], [X, *hidden, 1]
        up = ops.PpoUpdater(x_dim=X, u_dim=U, policy_dims=pd, value_dims=vd, batch_size=B, unroll_length=T, device=dev, **(opts or {}))
        up.load_state(torch.cat([lecun_flat(pd, g), lecun_flat(vd, g)]).to(dev))
        Dp = ops.transition_row_len(X, U, True)
        data = torch.randn(B, T, Dp, generator=g) * 0.5
        data[..., X + U + 1] = 1.0                       # discount
        data[..., -1] = 0.0                              # truncation
        data = data.to(dev)
        t, te = both(lambda: up.minibatch_step(data), reps)
        flop = B * T * 2 * 3 * (mlp_macs(pd) + mlp_macs(vd)) + B * 2 * mlp_macs(vd)
        out.append(mfma_entry("k_ppo_values + k_ppo_fwd_bwd + reduce/apply", "mbpo_ppo_grads + mbpo_ppo_apply",
                              {"x": X, "u": U, "hidden": list(hidden), "B": B, "T": T, **({"options": opts} if opts else {})}, t, flop,
                              "3*2*(P+V) FLOP per (sample, step) + bootstrap value; includes the in-kernel GAE",
                              {"gae_elements_per_s": B * T / t}))
        log(f"ppo minibatch_step B={B} T={T}{' ' + str(opts) if opts else ''}: {t * 1e6:.1f} us")

    if want("ppo_case"): ppo_case(4, 1, (64, 64, 64), 512, 5, 100)
    if want("ppo_case"): attempt(ppo_case, 4, 1, (64, 64, 64), 512, 40, 50)
    if want("ppo_case"): attempt(ppo_case, 3, 1, (64, 64), 128, 40, 100)        # the reference's own PPO test shape (tests/test_ppo.py:30-56)
    # ppo_brax_env.py's options at C3: clip_by_global_norm (one more launch per minibatch_step; max_grad_norm small enough to clip),
    # and the per-sample discount of non_equidistant_time
    if want("ppo_case"): attempt(ppo_case, 4, 1, (64, 64, 64), 512, 40, 50, {"max_grad_norm": 1e-3})
    if want("ppo_case"): attempt(ppo_case, 4, 1, (64, 64, 64), 512, 40, 50, {"non_equidistant_time": True, "continuous_discounting": 0.5,
                                                                            "max_time_between_switches": 0.5, "env_dt": 0.05})

    # ---------------------------------------------------------------- B1-B5: BPTT actor gradient (C5)
    def bptt_case(X, U, E, H, n, reps):
        hidden = (64, 64, 64)
        ad, cd, dd = [X, *hidden, 2 * U], [X, *hidden, 1], [X + U, *hidden, 2 * X]
        op = ops.BpttActorGrad(x_dim=X, u_dim=U, horizon=H, actor_dims=ad, critic_dims=cd, n=n, device=dev, seed=3)
        apar, cpar = lecun_flat(ad, g).to(dev), lecun_flat(cd, g, 2).to(dev)
        dpar = (lecun_flat(dd, g, E) * 0.5).to(dev)
        x0 = torch.randn(n, X, generator=g).to(dev)
        kw = dict(actor_params=apar, target_critic_params=cpar, init_states=x0, state_mean=torch.zeros(X, device=dev),
                  state_std=torch.ones(X, device=dev), reward_mean_std=torch.tensor([0.0, 1.0], device=dev),
                  system_kind=_hip.SYS_ENSEMBLE, reward_kind=_hip.REWARD_QUADRATIC,
                  reward_params=torch.cat([torch.zeros(X), torch.ones(X), torch.ones(U) * 0.1]).to(dev), dyn_params=dpar,
                  dyn_spec=ops.MlpSpec(dd, "swish", E))
        t, te = both(lambda: op(**kw), reps, warm=2, inner=2)
        P_, M_, V_ = mlp_macs(ad), mlp_macs(dd), mlp_macs(cd)
        flop = n * H * (3 * 2 * P_ + 2 * 2 * E * M_ + 2 * 2 * 2 * V_)
        out.append(mfma_entry("k_bptt_actor + reduce", "mbpo_bptt_actor_grads", {"x": X, "u": U, "E": E, "H": H, "n": n}, t, flop,
                              "3*(2P) + 2*(2*E*M) + 2*(2*2V) FLOP per (state, step), fwd+bwd",
                              {"state_steps_per_s": n * H / t, "grads_finite": bool(torch.isfinite(op.grads).all())}))
        log(f"bptt x={X} u={U} E={E} H={H} n={n}: {t * 1e3:.2f} ms  {n * H / t / 1e6:.2f} M state-steps/s")

    if want("bptt_case"): attempt(bptt_case, 17, 6, 10, 32, 4096, 5)          # C5, one GPU's share
    if want("bptt_case"): bptt_case(4, 1, 5, 5, 4096, 20)            # north-star shape

    # ---------------------------------------------------------------- N3: ensemble NLL fwd+bwd
    X, U, E, Bn = 4, 1, 5, 256
    dd = [X + U, 64, 64, 64, 2 * X]
    spec = ops.MlpSpec(dd, "swish", E)
    nll = ops.EnsembleNllGrad(x_dim=X, u_dim=U, spec=spec, batch=Bn, device=dev)
    dpar = lecun_flat(dd, g, E).to(dev)
    rows = torch.randn(8192, 2 * X + U + 2, generator=g).to(dev)
    idx = torch.randint(0, 8192, (E, Bn), generator=g, dtype=torch.int32).to(dev)
    t, te = both(lambda: nll(dpar, rows, idx), 100)
    out.append(mfma_entry("k_ens_nll_fwd_bwd + k_ens_reduce", "mbpo_ens_nll_grads", {"x": X, "u": U, "E": E, "B": Bn}, t,
                          E * Bn * 3 * 2 * mlp_macs(dd), "3*(2M) FLOP per (member, sample)"))
    log(f"ensemble nll: {t * 1e6:.1f} us")

    # one EnsembleDynamics.fit step on MBPO's model (7 x 4 x 200, stored zero-padded at 256): Philox minibatch draw, the layered NLL path
    # (gather, one GEMM launch per Dense layer forward, NLL head, the backward's GEMM levels) and AdamW, as fit issues them
    def fit_case(X, U, E, hid, B, reps):
        from mbpo.systems import EnsembleDynamics
        dyn = EnsembleDynamics(X, U, n_members=E, hidden_layer_sizes=hid, device=dev)
        p = dyn.init_params(0)
        rows = torch.randn(8192, 2 * X + U + 2, generator=g).to(dev)
        dyn.fit(p, rows, num_steps=1, batch_size=B)          # builds the fit state (descriptor, workspace, optimizer)
        col0 = rows[:, :1].contiguous()

        def step():
            ops.replay_sample(col0, dyn._fit_state, E * B, seed=1, offset=0, out=dyn._fit_scratch, idx_out=dyn._fit_idx)
            dyn._opt.step(p.params, dyn._nll(p.params, rows, dyn._fit_idx.view(E, B)))
        t, te = both(step, reps)
        out.append(mfma_entry("k_replay_sample + layered NLL path + AdamW", "mbpo_ens_nll_grads", {"x": X, "u": U, "E": E, "B": B,
                              "member": list(hid), "stored": dyn.dims[1:-1]}, t, E * B * 3 * 2 * mlp_macs(dyn.dims_logical),
                              "3*(2M) FLOP per (member, sample), logical shapes"))
        log(f"ensemble fit step E={E} {hid} B={B}: {t * 1e6:.1f} us (eager {te * 1e6:.1f} us)")

    if want("fit_case"): attempt(fit_case, 4, 1, 7, (200, 200, 200, 200), 256, 50)

    # held-out loss of every member (mbpo_ens_eval, forward only) on n shared rows, next to mbpo_ensemble_mlp_forward on the same
    # [E, n] rows in the same run: the eval drops the y write and adds the row gather and the loss head.  The forward row's roof.
    def ens_eval_case(X, U, E, hid, n, reps):
        from mbpo.systems import EnsembleDynamics
        dyn = EnsembleDynamics(X, U, n_members=E, hidden_layer_sizes=hid, device=dev)
        p = dyn.init_params(0)
        rows = torch.randn(8192, 2 * X + U + 2, generator=g).to(dev)
        idx = torch.randperm(8192, generator=g)[:n].to(torch.int32).to(dev)
        ev = ops.EnsembleEval(x_dim=X, u_dim=U, spec=dyn.spec, device=dev)
        xu = rows[idx.long(), :X + U].contiguous()
        t, te = both(lambda: ev(p.params, rows, idx), reps)
        tf, _ = both(lambda: ops.ensemble_mlp_forward(p.params, dyn.spec, xu), reps)
        out.append(mfma_entry("k_ens_eval + k_ens_eval_reduce" if dyn.dims[1:-1] == [64] * len(hid) else "k_ens_gather + layered forward + k_ens_head<false>",
                              "mbpo_ens_eval", {"n": n, "x": X, "u": U, "E": E, "member": list(hid), "stored": dyn.dims[1:-1]}, t,
                              n * 2 * E * mlp_macs(dyn.dims_logical), "2*E*M FLOP per row (shared rows), logical shapes",
                              {"eager_us": te * 1e6, "forward_device_us": tf * 1e6, "eval_over_forward": t / tf}))
        log(f"ensemble eval n={n} E={E} {hid}: {t * 1e6:.1f} us (eager {te * 1e6:.1f} us); forward of the same rows {tf * 1e6:.1f} us; ratio {t / tf:.2f}")

    if want("ens_eval_case"): attempt(ens_eval_case, 4, 1, 7, (64, 64, 64), 5000, 100)
    if want("ens_eval_case"): attempt(ens_eval_case, 4, 1, 7, (200, 200, 200, 200), 5000, 50)

    # ---------------------------------------------------------------- N3c: the ensemble's input scaler (three one-shot calls per fit)
    # Statistics and prepare on 100 000 true-buffer rows of 12 floats, next to mbpo_replay_gather of the same rows (the launch
    # prepare replaces in fit); the fold of 7 members next to mbpo_ens_pick_elites copying the same 7 members.  All HBM / latency bound.
    def ens_scaler_case(n, reps):
        X, U, D = 4, 1, 12
        rows = torch.randn(n, D, generator=g).to(dev)
        perm = torch.randperm(n, generator=g).to(torch.int32).to(dev)
        state = torch.tensor([n, 0, 0, n], device=dev, dtype=torch.int32)
        scaler = torch.empty(2, X + U, device=dev)
        L = ops.prepared_row_len(X, U)
        prep, gath = torch.empty(n, L, device=dev), torch.empty(n, D, device=dev)
        for tag, idx in (("rows in order", None), ("permuted rows", perm)):
            cfg = {"rows": n, "row_len": D, "x": X, "u": U, "selection": tag, "group": "ens_scaler"}
            t, te = both(lambda: ops.ens_scaler_fit(rows, X + U, idx=idx, out=scaler), reps)
            out.append(hbm_entry("k_ens_scaler_partial<0> + <1> + k_ens_scaler_finish", "mbpo_ens_scaler_fit", cfg, t, 2 * 4 * (X + U) * n,
                                 "2 passes x 4(x+u) B per row (rows are 48 B apart: sectors fetch more)"))
            log(f"scaler fit {n} ({tag}): {t * 1e6:.1f} us (eager {te * 1e6:.1f} us; 3 launches)")
            t, te = both(lambda: ops.ens_scaler_prepare(rows, scaler, X, U, idx=idx, next_obs_off=X + U + 2, predict_delta=True, out=prep), reps)
            out.append(hbm_entry("k_ens_scaler_prepare", "mbpo_ens_scaler_prepare", cfg, t, (4 * D + 4 * L) * n,
                                 f"{4 * D} B row read + {4 * L} B written per row"))
            log(f"scaler prepare {n} ({tag}): {t * 1e6:.1f} us (eager {te * 1e6:.1f} us)")
        t, te = both(lambda: ops.replay_gather(rows, state, perm, out=gath), reps)
        out.append(hbm_entry("k_replay_gather", "mbpo_replay_gather", {"rows": n, "row_len": D, "selection": "permuted rows", "group": "ens_scaler"},
                             t, 2 * 4 * D * n, "48 B read + 48 B write per row (the comparison for prepare)"))
        log(f"replay_gather {n} (permuted rows): {t * 1e6:.1f} us")

    def ens_fold_case(E, hid, reps):
        from mbpo.systems import EnsembleDynamics
        X, U = 4, 1
        dyn = EnsembleDynamics(X, U, n_members=E, hidden_layer_sizes=hid, device=dev)
        p = dyn.init_params(0)
        scaler = torch.stack([torch.randn(X + U, generator=g), torch.rand(X + U, generator=g) + 0.5]).to(dev)
        folded, copy = torch.empty_like(p.params), torch.empty_like(p.params)
        score, eidx = torch.rand(E, generator=g).to(dev), torch.empty(E, device=dev, dtype=torch.int32)
        cfg = {"E": E, "member": list(hid), "stored": dyn.dims[1:-1], "params_per_member": dyn.spec.n_params, "group": "ens_scaler"}
        t, te = both(lambda: ops.ens_fold_scaler(p.params, E, dyn.dims[0], dyn.dims[1], scaler, out=folded), reps)
        out.append(hbm_entry("k_ens_fold_scaler", "mbpo_ens_fold_scaler", cfg, t, 8 * p.params.numel(), "4 B read + 4 B written per parameter"))
        t2, _ = both(lambda: ops.ens_pick_elites(p.params, E, score, E, elite_idx=eidx, elite_params=copy), reps)
        out.append(hbm_entry("k_ens_rank + k_ens_member_copy", "mbpo_ens_pick_elites", dict(cfg, n_elites=E), t2, 8 * p.params.numel(),
                             "4 B read + 4 B written per parameter (the comparison for the fold; two launches)"))
        log(f"fold E={E} {hid}: {t * 1e6:.1f} us (eager {te * 1e6:.1f} us); pick_elites copying the same members {t2 * 1e6:.1f} us")

    # Evidence, not a test: Pendulum transitions with the speed in other units (* 1000 + 500, state and next state alike), 4000
    # training and 1000 held-out rows, 5 members, 500 steps, same seeds; held-out squared error of the ensemble-mean prediction in
    # target units, with and without normalize_inputs.
    def ens_scaler_mse_case(steps):
        from mbpo.systems import EnsembleDynamics, PendulumSystem
        system = PendulumSystem()
        n = 5000
        th = (torch.rand(n, generator=g) * 2 - 1) * math.pi
        x = torch.stack([torch.cos(th), torch.sin(th), (torch.rand(n, generator=g) * 2 - 1) * 8], 1).to(dev)
        u = (torch.rand(n, 1, generator=g) * 2 - 1).to(dev)
        nxt = system.step(x, u, system.reset().system_params)
        rows = torch.cat([x, u, nxt.reward[:, None], torch.ones(n, 1, device=dev), nxt.x_next], 1)
        rows[:, 2] = rows[:, 2] * 1000 + 500
        rows[:, 8] = rows[:, 8] * 1000 + 500
        train, held = rows[:4000].contiguous(), rows[4000:].contiguous()
        res = {}
        for norm in (False, True):
            dyn = EnsembleDynamics(3, 1, n_members=5, device=dev)
            p, losses = dyn.fit(dyn.init_params(1), train, num_steps=steps, batch_size=256, learning_rate=3e-3, key=3, normalize_inputs=norm)
            y = dyn.member_outputs(held[:, :3], held[:, 3:4], p)
            err = (held[:, :3] + y[..., :3].mean(0) - held[:, 6:9]) ** 2
            res["normalize_inputs" if norm else "raw_inputs"] = {
                "heldout_mse_sum_over_dims": float(err.sum(1).mean()), "heldout_mse_per_dim": [float(v) for v in err.mean(0)],
                "final_train_nll": float(losses[-20:].mean())}
            log(f"scaler evidence, normalize_inputs={norm}: {res['normalize_inputs' if norm else 'raw_inputs']}")
        out.append({"kernel": "EnsembleDynamics.fit with / without normalize_inputs (evidence, unasserted)", "entry": "mbpo_ens_scaler_*",
                    "config": {"rows_train": 4000, "rows_heldout": 1000, "E": 5, "steps": steps, "batch": 256, "lr": 3e-3,
                               "data": "Pendulum, speed column * 1000 + 500", "group": "ens_scaler"}, **res})

    if want("ens_scaler_case"): attempt(ens_scaler_case, 100_000, 100)
    if want("ens_scaler_case"): attempt(ens_fold_case, 7, (64, 64, 64), 100)
    if want("ens_scaler_case"): attempt(ens_fold_case, 7, (200, 200, 200, 200), 100)
    if want("ens_scaler_case"): attempt(ens_scaler_mse_case, 500)

    # ---------------------------------------------------------------- N3d: calibration of the ensemble's spread (once per fit)
    # mbpo_ens_calibrate (memset + count + pick) on n held-out rows at the default grid, next to the member forward that produces its
    # input and to mbpo_ens_eval on the same rows and members.  Reported, not tuned.
    def ens_calibrate_case(n, X, U, E, hid, reps):
        from mbpo.systems import EnsembleDynamics
        dyn = EnsembleDynamics(X, U, n_members=E, hidden_layer_sizes=hid, device=dev)
        p = dyn.init_params(0)
        rows = torch.randn(8192, 2 * X + U + 2, generator=g).to(dev)
        idx = torch.randperm(8192, generator=g)[:n].to(torch.int32).to(dev)
        xu = rows[idx.long(), :X + U].contiguous()
        y = ops.ensemble_mlp_forward(p.params, dyn.spec, xu)
        A, P = ops.CAL_N_ALPHAS, 19
        outs = (torch.empty(X, device=dev), torch.empty(X, device=dev, dtype=torch.int32), torch.empty(X, A, P, device=dev, dtype=torch.int32))
        ev = ops.EnsembleEval(x_dim=X, u_dim=U, spec=dyn.spec, device=dev)
        t, te = both(lambda: ops.ens_calibrate(y, rows, X, U, idx=idx, out=outs), reps)
        tf, _ = both(lambda: ops.ensemble_mlp_forward(p.params, dyn.spec, xu), reps)
        tv, _ = both(lambda: ev(p.params, rows, idx), reps)
        out.append({"kernel": "memset + k_ens_cal_count + k_ens_cal_pick", "entry": "mbpo_ens_calibrate",
                    "config": {"n": n, "x": X, "u": U, "E": E, "A": A, "P": P, "member": list(hid), "group": "ens_calibrate"},
                    "device_us": t * 1e6, "eager_us": te * 1e6, "forward_device_us": tf * 1e6, "ens_eval_device_us": tv * 1e6,
                    "calibrate_over_forward_plus_eval": t / (tf + tv), "comparisons": n * X * A * P,
                    "comparisons_per_s": n * X * A * P / t, "global_atomics_at_most": -(-n // 512) * X * A * P})
        log(f"ens_calibrate n={n} x={X} E={E} A={A} P={P}: {t * 1e6:.1f} us (eager {te * 1e6:.1f} us); forward {tf * 1e6:.1f} us; "
            f"ens_eval {tv * 1e6:.1f} us")

    # Evidence, not a test: Pendulum, 7 members, 5 elites, 4000 true transitions with a 20 % holdout; coverage of the intervals at the
    # 0.5 and 0.9 levels on 2000 FRESH transitions, raw spread and calibrated.
    def ens_calibrate_coverage_case(steps, seed):
        from mbpo.systems import EnsembleDynamics, PendulumSystem
        system = PendulumSystem()
        gg = torch.Generator().manual_seed(seed)

        def draw(n):
            th = (torch.rand(n, generator=gg) * 2 - 1) * math.pi
            x = torch.stack([torch.cos(th), torch.sin(th), (torch.rand(n, generator=gg) * 2 - 1) * 8], 1).to(dev)
            u = (torch.rand(n, 1, generator=gg) * 2 - 1).to(dev)
            nxt = system.step(x, u, system.reset().system_params)
            return torch.cat([x, u, nxt.reward[:, None], torch.ones(n, 1, device=dev), nxt.x_next], 1).contiguous()

        train, fresh = draw(4000), draw(2000)
        dyn = EnsembleDynamics(3, 1, n_members=7, device=dev)
        p, losses = dyn.fit(dyn.init_params(seed + 1), train, num_steps=steps, batch_size=256, learning_rate=3e-3, key=seed, holdout_ratio=0.2,
                            n_elites=5, calibrate=True)
        lv = [9, 17]
        res = {"calibration": [float(v) for v in p.calibration], "steps_run": int(losses.shape[0]), "levels": [0.5, 0.9],
               "coverage_fresh_before": dyn.coverage(p, fresh, calibrated=False)[:, lv].tolist(),
               "coverage_fresh_after": dyn.coverage(p, fresh, calibrated=True)[:, lv].tolist()}
        log(f"calibration evidence (seed {seed}): {res}")
        out.append({"kernel": "EnsembleDynamics.fit(calibrate=True) + coverage on fresh rows (evidence, unasserted)", "entry": "mbpo_ens_calibrate",
                    "config": {"rows": 4000, "holdout_ratio": 0.2, "rows_fresh": 2000, "E": 7, "n_elites": 5, "steps": steps, "batch": 256,
                               "lr": 3e-3, "seed": seed, "data": "Pendulum, uniform states and actions", "group": "ens_calibrate"}, **res})

    if want("ens_calibrate_case"): attempt(ens_calibrate_case, 5000, 17, 6, 7, (64, 64, 64), 100)
    if want("ens_calibrate_case"): attempt(ens_calibrate_case, 5000, 3, 1, 7, (64, 64, 64), 100)
    if want("ens_calibrate_case"): attempt(ens_calibrate_coverage_case, 1500, 0)

    # ---------------------------------------------------------------- N4: iCEM planner at the reference's defaults (icem_optimizer.py:25-50)
    def icem_case(H, reps):
        from mbpo.optimizers.trajectory_optimizers.icem_optimizer import iCemParams, iCemTO
        from mbpo.systems import PendulumSystem
        from mbpo.utils import keys as K
        p = iCemParams()
        system = PendulumSystem()
        X, U = system.x_dim, system.u_dim
        opt = iCemTO(horizon=H, action_dim=U, opt_params=p, system=system)
        st0 = opt.init(K.PRNGKey(0))
        b = opt._buffers(dev)
        spec = system.rollout_spec(st0.system_params, dev)
        lib, stp = _hip.load(), _hip.current_stream_ptr
        b["std"].fill_(p.init_std)
        x0 = torch.tensor([-1.0, 0.0, 0.0], device=dev)
        NC, N, D = b["NC"], b["N"], b["rows"].shape[1]

        def sample():
            _hip.check(lib.mbpo_icem_sample(b["mean"].data_ptr(), b["std"].data_ptr(), b["prev"].data_ptr(), b["u_min"].data_ptr(),
                                            b["u_max"].data_ptr(), p.num_samples, opt.num_prev, H, U, p.num_particles, float(p.exponent),
                                            11, 0, None, b["actions"].data_ptr(), b["cand"].data_ptr(), stp()), "mbpo_icem_sample")

        def rollout():
            b["obs"].copy_(x0.expand(N, X)); b["first"].copy_(b["obs"]); b["steps"].zero_(); b["done"].zero_()
            ops.model_rollout(x_dim=X, u_dim=U, actions=b["actions"], obs=b["obs"], first_obs=b["first"], steps=b["steps"], done=b["done"],
                              n_steps=H, episode_length=2 ** 30, seed=5, offset=0, out=b["rows"], **spec)

        def update():
            b["best_value"].fill_(float("-inf"))
            _hip.check(lib.mbpo_icem_update_constrained(
                b["rows"].data_ptr(), D, X + U, NC, p.num_particles, H, U, b["cand"].data_ptr(), p.num_elites, opt.num_prev, float(p.alpha),
                0, None, float(p.lambda_constraint), 0, b["mean"].data_ptr(), b["std"].data_ptr(), b["best_value"].data_ptr(),
                b["best_seq"].data_ptr(), b["prev"].data_ptr(), b["values"].data_ptr(), b["rank"].data_ptr(), stp()), "mbpo_icem_update")

        cfg = {"num_samples": p.num_samples, "num_particles": p.num_particles, "num_elites": p.num_elites, "horizon": H, "x": X, "u": U,
               "system": "Pendulum"}
        sample(); rollout(); update()
        t, te = both(sample, reps)
        out.append(hbm_entry("k_icem_sample", "mbpo_icem_sample", cfg, t, 4 * (NC * H * U + H * N * U),
                             "4 B per candidate element written once + once per particle (actions [H][N][u])"))
        log(f"icem sample: {t * 1e6:.1f} us")
        t, te = both(rollout, reps)
        out.append(hbm_entry("k_model_rollout (open loop, Pendulum)", "mbpo_model_rollout", cfg, t, 4 * H * N * (U + D),
                             "4 B per action read + one transition row written per (step, trajectory)",))
        out[-1]["transitions_per_s"] = H * N / t
        log(f"icem open-loop rollout: {t * 1e6:.1f} us  {H * N / t / 1e6:.1f} M transitions/s")
        t, te = both(update, reps)
        out.append(hbm_entry("k_icem_update", "mbpo_icem_update_constrained", cfg, t, 4 * H * N * 1 + 4 * NC * H * U,
                             "4 B per reward element of the rows + the candidates read once"))
        log(f"icem update: {t * 1e6:.1f} us")
        ost = st0
        t, te = both(lambda: opt.optimize(x0, ost), max(reps // 10, 3), warm=1, inner=1)
        out.append({"kernel": "iCemTO.optimize (one MPC step)", "entry": "mbpo_icem_sample + mbpo_model_rollout + mbpo_icem_update x num_steps",
                    "config": dict(cfg, num_steps=p.num_steps), "device_us": t * 1e6, "eager_us": te * 1e6, "bound": "launch",
                    "note": "num_steps iterations of sample -> open-loop rollout -> update, host loop as icem_optimizer.py:135-252"})
        log(f"icem optimize: {t * 1e6:.1f} us (eager {te * 1e6:.1f})")

    if want("icem_case"): attempt(icem_case, 20, 100)

    # ---------------------------------------------------------------- batched MPC: one optimize for B problems vs B single calls
    def icem_batched_case(H):
        from mbpo.optimizers.trajectory_optimizers.icem_optimizer import iCemParams, iCemTO
        from mbpo.systems import PendulumSystem
        p = iCemParams()
        system = PendulumSystem()
        X, U = system.x_dim, system.u_dim
        opt = iCemTO(horizon=H, action_dim=U, opt_params=p, system=system)
        cfg = {"num_samples": p.num_samples, "num_particles": p.num_particles, "num_elites": p.num_elites, "num_steps": p.num_steps,
               "horizon": H, "x": X, "u": U, "system": "Pendulum"}
        single = {}
        st1 = opt.init(0)
        x1 = torch.tensor([-1.0, 0.0, 0.0], device=dev)
        for B in (8, 64):      # B sequential single-problem calls (the Python loop this replaces), same session
            t = timed(lambda: [opt.optimize(x1, st1) for _ in range(B)], 3, warm=1)
            single[B] = t
            log(f"icem {B} sequential optimize: {t * 1e3:.2f} ms")
        opt._bufs = None
        for B in (1, 8, 64, 256):
            st = opt.init(0, batch_size=B)
            x0 = x1.expand(B, X).contiguous()
            t = timed(lambda: opt.optimize(x0, st), 10 if B <= 64 else 3, warm=2)
            row = {"kernel": "iCemTO.optimize batched (B problems, one launch chain)",
                   "entry": "mbpo_icem_sample_batched + mbpo_model_rollout + mbpo_icem_update_batched x num_steps",
                   "config": dict(cfg, B=B), "eager_us": t * 1e6, "bound": "launch" if B <= 8 else "rollout",
                   "note": "HIP-event time of one eager optimize call (host key chain, one seed upload, 3 launches per iteration)"}
            if B in single:
                row["sequential_single_us"] = single[B] * 1e6
                row["speedup_vs_sequential"] = single[B] / t
            out.append(row)
            log(f"icem batched optimize B={B}: {t * 1e3:.3f} ms" + (f"  ({single[B] / t:.1f}x {B} single calls)" if B in single else ""))
            opt._bbufs = None

    if want("icem_batched_case"): attempt(icem_batched_case, 20)

    # ---------------------------------------------------------------- constrained iCEM: the cost as a term table (one launch) vs a torch callable (vmap)
    def icem_term_cost_case(H):
        """One Pendulum `optimize` at the reference's defaults, single and at batch_size 64, in three forms in one session — no cost, the
        speed constraint max_t(|theta_dot_t| - 5) as a TermCost (mbpo_traj_cost_eval), the same constraint as a torch callable (vmap) —
        timed in alternating rounds (median, min and max of the rounds), and mbpo_traj_cost_eval alone at the two sizes."""
        from mbpo.optimizers.trajectory_optimizers.icem_optimizer import iCemParams, iCemTO
        from mbpo.systems import Group, PendulumSystem, Term, TermCost
        p = iCemParams()
        system = PendulumSystem()
        X, U = system.x_dim, system.u_dim
        table = TermCost(X, U, bias=-5.0, groups=[Group([Term("x", 2, "abs")])], reduce="max")
        forms = {"no_cost": None, "term_cost": table, "callable": lambda o, a: o[:, 2].abs().max() - 5.0}
        opts = {k: iCemTO(horizon=H, action_dim=U, opt_params=p, system=system, cost_fn=cf) for k, cf in forms.items()}
        cfg = {"num_samples": p.num_samples, "num_particles": p.num_particles, "num_elites": p.num_elites, "num_steps": p.num_steps,
               "horizon": H, "x": X, "u": U, "system": "Pendulum", "constraint": "max_t(|theta_dot_t| - 5)"}
        x1 = torch.tensor([math.cos(2.5), math.sin(2.5), 4.5], device=dev)      # falling, close to the limit: the constraint binds
        ROUNDS = 5
        for B, reps in ((None, 20), (64, 5)):
            calls = {}
            for k, opt in opts.items():
                st = opt.init(0, batch_size=B)
                x0 = x1 if B is None else x1.expand(B, X).contiguous()
                calls[k] = (lambda opt=opt, x0=x0, st=st: opt.optimize(x0, st))
                timed(calls[k], 2, warm=2)
            times = {k: [] for k in calls}
            for _ in range(ROUNDS):
                for k, fn in calls.items():
                    times[k].append(timed(fn, reps, warm=0))
            med = {k: sorted(v)[ROUNDS // 2] for k, v in times.items()}
            for k, v in times.items():
                out.append({"kernel": f"iCemTO.optimize, cost_fn: {k}", "entry": "mbpo_icem_sample + mbpo_model_rollout"
                            + (" + mbpo_traj_cost_eval" if k == "term_cost" else " + torch.func.vmap(cost_fn)" if k == "callable" else "")
                            + " + mbpo_icem_update x num_steps", "config": dict(cfg, B=1 if B is None else B, batched=B is not None),
                            "eager_us": med[k] * 1e6, "eager_us_min": min(v) * 1e6, "eager_us_max": max(v) * 1e6, "rounds": ROUNDS,
                            "calls_per_round": reps, "bound": "launch" if B is None else "rollout",
                            "over_no_cost_us": (med[k] - med["no_cost"]) * 1e6,
                            "note": "HIP-event time of one eager optimize call; the three forms alternate round by round in one session"})
                log(f"icem optimize B={B or 1} cost_fn={k}: {med[k] * 1e6:.1f} us (min {min(v) * 1e6:.1f}, max {max(v) * 1e6:.1f}; "
                    f"{(med[k] - med['no_cost']) * 1e6:+.1f} us over no cost)")
            # the kernel alone, on the rows the last rollout left
            b = opts["term_cost"]._bufs if B is None else opts["term_cost"]._bbufs
            n, rows, buf = (b["N"] if B is None else b["NT"]), b["rows"], b["term_cost"]
            t, te = both(lambda: table.trajectory_cost(rows, H, n, out=buf), 200)
            out.append(hbm_entry("k_traj_cost", "mbpo_traj_cost_eval", dict(cfg, n_traj=n, row_len=rows.shape[1], reduce="max", terms=1), t,
                                 4 * H * n * rows.shape[1] + 4 * n, "the rows' 64 B sectors once (40 B rows: every sector is touched) + 4 B per cost"))
            log(f"traj_cost_eval n_traj={n}: {t * 1e6:.1f} us (eager {te * 1e6:.1f})")
            # the same launch with one thread per trajectory forced (what the dispatch picks once the tiles fill the device)
            lib = _hip.load()
            lib.mbpo_debug_set_traj_cost_slots(1)
            try:
                t1, _ = both(lambda: table.trajectory_cost(rows, H, n, out=buf), 200)
            finally:
                lib.mbpo_debug_set_traj_cost_slots(-1)
            out.append(hbm_entry("k_traj_cost (slots forced to 1)", "mbpo_traj_cost_eval", dict(cfg, n_traj=n, row_len=rows.shape[1], reduce="max",
                                                                                             terms=1, slots=1), t1,
                                 4 * H * n * rows.shape[1] + 4 * n, "as above"))
            log(f"traj_cost_eval n_traj={n}, one thread per trajectory: {t1 * 1e6:.1f} us")
            for opt in opts.values():
                opt._bufs = opt._bbufs = None

    if want("icem_term_cost_case"): icem_term_cost_case(20)

    # ---------------------------------------------------------------- iCEM plan rewards: parameters per problem and per step (one launch per iteration)
    def icem_plan_reward_case(H):
        """One Pendulum `optimize` at the reference's defaults, single and at batch_size 64, without and with a [B, H] Pendulum plan
        reward, timed in alternating rounds (median, min and max of the rounds); and mbpo_plan_reward_eval alone on the rows the last
        rollout left — the Pendulum kind [B, 1], the quadratic kind [B, H], a 12-term table [B, H], dense (as iCEM issues it) and in place — next
        to mbpo_traj_cost_eval on the same rows in the same session."""
        from mbpo.optimizers.trajectory_optimizers.icem_optimizer import iCemParams, iCemTO
        from mbpo.systems import Group, PendulumSystem, PlanRewardParams, QuadraticReward, Term, TermCost, TermReward, TermRewardParams
        from mbpo.systems.rewards.pendulum_reward import PendulumRewardParams, QuadraticRewardParams
        p = iCemParams()
        system = PendulumSystem()
        X, U = system.x_dim, system.u_dim
        opt = iCemTO(horizon=H, action_dim=U, opt_params=p, system=system)
        cfg = {"num_samples": p.num_samples, "num_particles": p.num_particles, "num_elites": p.num_elites, "num_steps": p.num_steps,
               "horizon": H, "x": X, "u": U, "system": "Pendulum"}
        x1 = torch.tensor([math.cos(2.5), math.sin(2.5), 4.5], device=dev)
        ROUNDS = 5

        def term12(b, t):
            c, s = math.cos(0.1 * b + 0.02 * t), math.sin(0.1 * b + 0.02 * t)
            return TermRewardParams(X, U, 0.0, (
                Group((Term("x", 0, "square", 1.0, c), Term("x", 1, "square", 1.0, s)), weight=-1.0, link="sqrt"),
                Group((Term("x_next", 0, "square", -4.0, c), Term("x_next", 1, "square", -4.0, s)), weight=1.0, link="exp"),
                Group((Term("x", 2, "square", -0.1, 0.0), Term("u", 0, "square", -0.02, 0.0), Term("x", 0, "cos", 0.05, 0.0),
                       Term("x", 1, "sin", 0.05, 0.0), Term("x", 2, "abs", -0.01, 0.0), Term("x", 2, "relu", -0.01, 5.0),
                       Term("u", 0, "abs", -0.01, 0.0), Term("x", 0, "identity", 0.1, 0.0)))))

        for B, reps in ((None, 20), (64, 5)):
            nb = 1 if B is None else B
            plan = PlanRewardParams.stack(system.reward, [[PendulumRewardParams(target_angle=0.1 * b + 0.02 * t) for t in range(H)]
                                                          for b in range(nb)], dev)
            x0 = x1 if B is None else x1.expand(B, X).contiguous()
            st = opt.init(0, batch_size=B)
            stp = st.replace(system_params=st.system_params.replace(reward_params=plan))
            calls = {"plain": lambda st=st, x0=x0: opt.optimize(x0, st), "plan_reward": lambda stp=stp, x0=x0: opt.optimize(x0, stp)}
            for fn in calls.values():
                timed(fn, 2, warm=2)
            times = {k: [] for k in calls}
            for _ in range(ROUNDS):
                for k, fn in calls.items():
                    times[k].append(timed(fn, reps, warm=0))
            med = {k: sorted(v)[ROUNDS // 2] for k, v in times.items()}
            for k, v in times.items():
                out.append({"kernel": f"iCemTO.optimize, reward: {k}", "entry": "mbpo_icem_sample + mbpo_model_rollout"
                            + (" + mbpo_plan_reward_eval" if k == "plan_reward" else "") + " + mbpo_icem_update x num_steps",
                            "config": dict(cfg, B=nb, batched=B is not None, table=[nb, H, 3] if k == "plan_reward" else None),
                            "eager_us": med[k] * 1e6, "eager_us_min": min(v) * 1e6, "eager_us_max": max(v) * 1e6, "rounds": ROUNDS,
                            "calls_per_round": reps, "bound": "launch" if B is None else "rollout", "over_plain_us": (med[k] - med["plain"]) * 1e6,
                            "note": "HIP-event time of one eager optimize call; the two forms alternate round by round in one session"})
                log(f"icem optimize B={nb} reward={k}: {med[k] * 1e6:.1f} us (min {min(v) * 1e6:.1f}, max {max(v) * 1e6:.1f}; "
                    f"{(med[k] - med['plain']) * 1e6:+.1f} us over plain)")
            # the kernel alone, on the rows the last rollout left
            b = opt._bufs if B is None else opt._bbufs
            group, rows = b["N"], b["rows"]
            n_rows, row_len = rows.shape
            qr, tr = QuadraticReward(X, U), TermReward(X, U)
            tables = {
                "pendulum [B, 1]": (_hip.REWARD_PENDULUM, PlanRewardParams.stack(system.reward, [[PendulumRewardParams(target_angle=0.1 * bb)]
                                                                                                 for bb in range(nb)], dev).table),
                "quadratic [B, H]": (_hip.REWARD_QUADRATIC, PlanRewardParams.stack(qr, [[QuadraticRewardParams(
                    [math.cos(0.1 * bb + 0.02 * t), math.sin(0.1 * bb + 0.02 * t), 0.0], [1.0, 1.0, 0.1], [0.02]) for t in range(H)]
                    for bb in range(nb)], dev).table),
                "12-term table [B, H]": (_hip.REWARD_TERMS, PlanRewardParams.stack(tr, [[term12(bb, t) for t in range(H)] for bb in range(nb)],
                                                                                   dev).table)}
            dense = torch.zeros(n_rows, device=dev)
            for name, (kind, table) in tables.items():
                for place in ("dense", "in place"):
                    kw = dict(out=dense) if place == "dense" else dict(reward_col=X + U)
                    fn = lambda kind=kind, table=table, kw=kw: ops.plan_reward_eval(kind, table, rows, H, nb, group, X, U, next_off=X + U + 2, **kw)
                    t, te = both(fn, 200)
                    # in place every cache line of the rows is dirtied by a 4-byte store and written back whole
                    nbytes = 4 * n_rows * row_len * (1 if place == "dense" else 2) + (4 * n_rows if place == "dense" else 0) + 4 * table.numel()
                    out.append(hbm_entry(f"k_plan_reward, {name}, {place}", "mbpo_plan_reward_eval",
                                         dict(cfg, n_problems=nb, group=group, n_rows=n_rows, row_len=row_len, table=list(table.shape), output=place),
                                         t, nbytes, "the rows' 64 B sectors once (40 B rows: every sector is touched) + the table once + dense: 4 B "
                                         "per row written; in place: the rows' sectors written back"))
                    log(f"plan_reward_eval {name}, {place}, n_rows={n_rows}: {t * 1e6:.1f} us (eager {te * 1e6:.1f})")
            cost = TermCost(X, U, bias=-5.0, groups=[Group([Term("x", 2, "abs")])], reduce="max")
            buf = torch.zeros(nb * group, device=dev)
            t, te = both(lambda: cost.trajectory_cost(rows, H, nb * group, out=buf), 200)
            out.append(hbm_entry("k_traj_cost (yardstick, same rows, same session)", "mbpo_traj_cost_eval",
                                 dict(cfg, n_traj=nb * group, row_len=row_len, reduce="max", terms=1), t, 4 * n_rows * row_len + 4 * nb * group,
                                 "the rows' 64 B sectors once + 4 B per trajectory"))
            log(f"traj_cost_eval (yardstick) n_traj={nb * group}: {t * 1e6:.1f} us (eager {te * 1e6:.1f})")
            opt._bufs = opt._bbufs = None

    if want("icem_plan_reward_case"): icem_plan_reward_case(20)

    # ---------------------------------------------------------------- iCEM terminal value: a learned critic at x_H (one launch per iteration)
    def icem_terminal_value_case():
        """mbpo_terminal_value_eval alone under graph replay at 5150 rows (one problem) and 329 600 rows (batch_size 64), kind V (a twin
        64 x 3 critic) and kind Q (a 64 x 3 policy and twin 64 x 3 Q), x = 3, A = 1, strided exactly as iCEM passes it (states in the
        next-state columns of 10-float rows, the sum into the rows' reward column), next to mbpo_ensemble_mlp_forward with two 64 x 3
        members on the same number of DENSE rows in the same session (the yardstick: the same wave chains, no gather, no policy); and one
        Pendulum `optimize` — H = 20 at the defaults, H = 5 without and with the value — single and at batch_size 64, median of five
        alternating rounds."""
        from mbpo.optimizers import TerminalValue
        from mbpo.optimizers.trajectory_optimizers.icem_optimizer import iCemParams, iCemTO
        from mbpo.systems import PendulumSystem
        X, A, hid = 3, 1, [64, 64, 64]
        vd, qd, pd = [X, *hid, 1], [X + A, *hid, 1], [X, *hid, 2 * A]
        gg = torch.Generator().manual_seed(11)
        noisy = lambda dims, n=1: (lambda p: p + 0.1 * torch.randn(p.shape, generator=gg))(lecun_flat(dims, gg, n)).to(dev)
        mean, std = torch.randn(X, generator=gg).to(dev), (torch.rand(X, generator=gg) + 0.5).to(dev)
        values = {"V": TerminalValue(X, noisy(vd, 2), vd, n_critics=2, norm_mean=mean, norm_std=std, weight=0.95),
                  "Q": TerminalValue(X, noisy(qd, 2), qd, policy_params=noisy(pd), policy_dims=pd, norm_mean=mean, norm_std=std, weight=0.95)}
        row_len, reward_col, next_off = 2 * X + A + 3, X + A, X + A + 2
        macs = {"V": 2 * mlp_macs(vd), "Q": 2 * mlp_macs(qd) + mlp_macs(pd)}
        for n in (5150, 64 * 5150):
            rows = torch.randn(n, row_len, generator=gg).to(dev)
            for kind, tv in values.items():
                t, te = both(lambda tv=tv: tv.eval_into(rows, next_off, row_len, rows, reward_col, row_len, n, accumulate=True), 200)
                rows.copy_(torch.randn(n, row_len, generator=gg))      # (the sums ran away: fresh numbers for the next form)
                out.append(mfma_entry(f"k_terminal_value<64>, kind {kind}", "mbpo_terminal_value_eval",
                                      {"n": n, "x": X, "A": A, "critic": vd if kind == "V" else qd, "n_critics": 2,
                                       "policy": pd if kind == "Q" else None, "x_stride": row_len, "out_stride": row_len, "accumulate": 1},
                                      t, 2 * macs[kind] * n, "2 flop per MAC of every network, per row"))
                log(f"terminal_value_eval kind {kind}, n={n}: {t * 1e6:.1f} us (eager {te * 1e6:.1f})")
            for lean in (1, 0):      # the yardstick: the dispatch's throughput kernel (3 inputs: it applies), and the generic wave-chain kernel
                _hip.load().mbpo_debug_set_ens_lean(lean)
                try:
                    spec = ops.MlpSpec(vd, "swish", 2)
                    pe, xd = noisy(vd, 2), torch.randn(n, X, generator=gg).to(dev)
                    ty, te = both(lambda: ops.ensemble_mlp_forward(pe, spec, xd), 200)
                finally:
                    _hip.load().mbpo_debug_set_ens_lean(-1)
                which = "k_ens_fwd_lean" if lean else "k_ensemble_forward<64>"
                out.append(mfma_entry(f"{which} (yardstick, same rows, same session)", "mbpo_ensemble_mlp_forward",
                                      {"n": n, "dims": vd, "members": 2, "input": "dense", "note": "allocates its output per call"}, ty,
                                      2 * 2 * mlp_macs(vd) * n, "2 flop per MAC of both members, per row"))
                log(f"ensemble_mlp_forward {which} 2 x {vd}, n={n}: {ty * 1e6:.1f} us (eager {te * 1e6:.1f})")
        # one optimize
        system = PendulumSystem()
        p = iCemParams()
        x1 = torch.tensor([math.cos(2.5), math.sin(2.5), 4.5], device=dev)
        forms = {"H20": (20, None), "H5": (5, None), "H5 + V": (5, values["V"]), "H5 + Q": (5, values["Q"])}
        opts = {k: iCemTO(horizon=h, action_dim=A, opt_params=p, system=system, terminal_value=tv) for k, (h, tv) in forms.items()}
        ROUNDS = 5
        for B, reps in ((None, 20), (64, 5)):
            calls = {}
            for k, opt in opts.items():
                st = opt.init(0, batch_size=B)
                x0 = x1 if B is None else x1.expand(B, X).contiguous()
                calls[k] = (lambda opt=opt, x0=x0, st=st: opt.optimize(x0, st))
                timed(calls[k], 2, warm=2)
            times = {k: [] for k in calls}
            for _ in range(ROUNDS):
                for k, fn in calls.items():
                    times[k].append(timed(fn, reps, warm=0))
            med = {k: sorted(v)[ROUNDS // 2] for k, v in times.items()}
            for k, v in times.items():
                out.append({"kernel": f"iCemTO.optimize, {k}", "entry": "mbpo_icem_sample + mbpo_model_rollout"
                            + (" + mbpo_terminal_value_eval" if "+" in k else "") + " + mbpo_icem_update x num_steps",
                            "config": {"num_samples": p.num_samples, "num_particles": p.num_particles, "num_elites": p.num_elites,
                                       "num_steps": p.num_steps, "horizon": forms[k][0], "system": "Pendulum", "B": 1 if B is None else B,
                                       "batched": B is not None, "terminal_value": k.split("+ ")[1] if "+" in k else None},
                            "eager_us": med[k] * 1e6, "eager_us_min": min(v) * 1e6, "eager_us_max": max(v) * 1e6, "rounds": ROUNDS,
                            "calls_per_round": reps, "bound": "launch" if B is None else "rollout", "over_H5_us": (med[k] - med["H5"]) * 1e6,
                            "note": "HIP-event time of one eager optimize call; the forms alternate round by round in one session"})
                log(f"icem optimize B={B or 1} {k}: {med[k] * 1e6:.1f} us (min {min(v) * 1e6:.1f}, max {max(v) * 1e6:.1f}; "
                    f"{(med[k] - med['H5']) * 1e6:+.1f} us over H5)")
            for opt in opts.values():
                opt._bufs = opt._bbufs = None

    if want("icem_terminal_value_case"): icem_terminal_value_case()

    # ---------------------------------------------------------------- iCEM policy prior: a policy's rollouts among the candidates
    def icem_policy_prior_case():
        """One Pendulum `optimize` at the reference's defaults (H = 20) and at H = 5, single and at batch_size 64, without a prior and
        with K = 24 proposals of a 64 x 2 policy seeded in every iteration and in the first only, median of five alternating rounds; and
        mbpo_icem_seed_candidates alone under graph replay on the proposal rows of the last call, next to mbpo_traj_cost_eval on the
        same session's candidate rows (the yardstick)."""
        from mbpo.optimizers import PolicyPrior
        from mbpo.optimizers.trajectory_optimizers.icem_optimizer import iCemParams, iCemTO
        from mbpo.systems import Group, PendulumSystem, Term, TermCost
        X, A, KP = 3, 1, 24
        pd = [X, 64, 64, 2 * A]
        gg = torch.Generator().manual_seed(13)
        pol = (lambda p: p + 0.1 * torch.randn(p.shape, generator=gg))(lecun_flat(pd, gg, 1)).to(dev)
        mean, std = (torch.randn(X, generator=gg) * 0.1).to(dev), (torch.rand(X, generator=gg) + 0.5).to(dev)
        prior = lambda every: PolicyPrior(X, pol, pd, norm_mean=mean, norm_std=std, n_candidates=KP, every_iteration=every)
        system = PendulumSystem()
        p = iCemParams()
        x1 = torch.tensor([math.cos(2.5), math.sin(2.5), 4.5], device=dev)
        ROUNDS = 5
        for H in (20, 5):
            forms = {"plain": None, "prior, every iteration": prior(True), "prior, first iteration": prior(False)}
            opts = {k: iCemTO(horizon=H, action_dim=A, opt_params=p, system=system, policy_prior=pp) for k, pp in forms.items()}
            for B, reps in ((None, 20), (64, 5)):
                nb = 1 if B is None else B
                calls = {}
                for k, opt in opts.items():
                    st = opt.init(0, batch_size=B)
                    x0 = x1 if B is None else x1.expand(B, X).contiguous()
                    calls[k] = (lambda opt=opt, x0=x0, st=st: opt.optimize(x0, st))
                    timed(calls[k], 2, warm=2)
                times = {k: [] for k in calls}
                for _ in range(ROUNDS):
                    for k, fn in calls.items():
                        times[k].append(timed(fn, reps, warm=0))
                med = {k: sorted(v)[ROUNDS // 2] for k, v in times.items()}
                for k, v in times.items():
                    out.append({"kernel": f"iCemTO.optimize, {k}", "entry": "mbpo_icem_sample"
                                + (" + mbpo_icem_seed_candidates" if forms[k] is not None else "") + " + mbpo_model_rollout + mbpo_icem_update x num_steps"
                                + ("; once: mbpo_philox_fill_grouped + mbpo_model_rollout (policy)" if forms[k] is not None else ""),
                                "config": {"num_samples": p.num_samples, "num_particles": p.num_particles, "num_elites": p.num_elites,
                                           "num_steps": p.num_steps, "horizon": H, "system": "Pendulum", "B": nb, "batched": B is not None,
                                           "n_candidates": KP if forms[k] is not None else None, "policy": pd if forms[k] is not None else None},
                                "eager_us": med[k] * 1e6, "eager_us_min": min(v) * 1e6, "eager_us_max": max(v) * 1e6, "rounds": ROUNDS,
                                "calls_per_round": reps, "bound": "launch" if B is None else "rollout",
                                "over_plain_us": (med[k] - med["plain"]) * 1e6,
                                "note": "HIP-event time of one eager optimize call; the forms alternate round by round in one session"})
                    log(f"icem optimize H={H} B={nb} {k}: {med[k] * 1e6:.1f} us (min {min(v) * 1e6:.1f}, max {max(v) * 1e6:.1f}; "
                        f"{(med[k] - med['plain']) * 1e6:+.1f} us over plain)")
                # the seed launch alone, on the proposal rows the last call left, into that optimizer's own candidate buffers
                opt = opts["prior, every iteration"]
                b = opt._bufs if B is None else opt._bbufs
                src, row_len = b["pp_rows"], b["pp_rows"].shape[1]
                NC, P = b["NC"], p.num_particles
                fn = lambda: ops.icem_seed_candidates(src, X, nb * KP * row_len, row_len, nb, KP, NC, H, A, P, b["u_min"], b["u_max"],
                                                      actions=b["actions"], candidates=b["cand"])
                t, te = both(fn, 200)
                n_el = nb * KP * H * A
                out.append(hbm_entry("k_icem_seed", "mbpo_icem_seed_candidates",
                                     {"n_problems": nb, "n_seed": KP, "n_candidates": NC, "horizon": H, "u_dim": A, "n_particles": P,
                                      "src_traj_stride": row_len, "src_step_stride": nb * KP * row_len}, t, 4 * n_el * (2 + 1 + P),
                                     "every proposal element read twice (4 B of a 40 B row each), written once as a candidate and P times as "
                                     "an action"))
                log(f"icem_seed_candidates H={H} B={nb}: {t * 1e6:.1f} us (eager {te * 1e6:.1f})")
                rows = b["rows"]
                cost = TermCost(X, A, bias=-5.0, groups=[Group([Term("x", 2, "abs")])], reduce="max")
                buf = torch.zeros(nb * b["N"], device=dev)
                t, te = both(lambda: cost.trajectory_cost(rows, H, nb * b["N"], out=buf), 200)
                out.append(hbm_entry("k_traj_cost (yardstick, same session's candidate rows)", "mbpo_traj_cost_eval",
                                     {"n_traj": nb * b["N"], "horizon": H, "row_len": rows.shape[1], "reduce": "max", "terms": 1}, t,
                                     4 * rows.numel() + 4 * nb * b["N"], "the rows' 64 B sectors once + 4 B per trajectory"))
                log(f"traj_cost_eval (yardstick) H={H} n_traj={nb * b['N']}: {t * 1e6:.1f} us (eager {te * 1e6:.1f})")
                for o in opts.values():
                    o._bufs = o._bbufs = None

    if want("icem_policy_prior_case"): icem_policy_prior_case()

    res = {"device": torch.cuda.get_device_name(0), "roofs": {"hbm_GBs": HBM_PEAK_GBS, "mfma_f32_TFLOPs": MFMA_F32_PEAK_TF},
           "note": "device_us = HIP-event average per call with the calls captured into a hipGraph and replayed (device time, inputs resident in HBM; multi-launch ops timed whole); eager_us = the same call issued from Python",
           "kernels": out}
    txt = json.dumps(res, indent=1)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
