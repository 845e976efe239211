"""Time-adaptive rollout cases shared by tests/test_cpu_time_adaptive.py and tests/test_gpu_time_adaptive.py: the inputs, the reference
run of tests/time_adaptive_ref.py (computed once per case and dtype, and left unchanged) and the device run.

Every case: N = 40 envs (three 16-row tiles, the last one ragged), S = 4 decisions, episode_length 6 model steps (resets fall inside
the launch), initial steps = env % 3, a few envs entering already done.  Members and policy are lecun-initialised
(oracle.nets.init_mlp_flat) with small non-zero biases; policy_noise is given.  The hold maps tau to [dt, (K + 0.999) dt), so every
k in 1 .. K is taken.

Tolerance.  The project's rollout tolerance atol = rtol = 2e-4 was set for rows at most 5 model steps deep; here a row is up to
S * K steps deep.  Per case TOL is twice the reference's own fp32-fp64 gap (max over the kept envs' rows of |r32 - r64| / (1 + |r64|),
GAP below, measured by test_cpu_time_adaptive.py's condition test, which also asserts gap < TOL / 2), rounded up to one significant
digit, never below 2e-4 and never above 2e-3.
"""
from __future__ import annotations

import functools

import torch

from oracle import nets as onets
from oracle import rollout as oro
from oracle import systems as osys

import fresh_start_cases as fc
import learned_reward_ref as lref
import time_adaptive_ref as taref

N, L, S = 40, 6, 4
SEED, OFFSET = 9876, (7 << 32) + 3      # Philox key of the start-buffer draws (case 4)
DT = 0.05
INF = float("inf")

_C = dict(hidden=(64, 64, 64), E=5, mode="mean", noise=False, ppo=False, env_major=False, normalize=False, reward="quadratic",
          system="ensemble", box=None, start=False, cd=0.0, cost=0.0, seed=0)
CASES = {
    # 1: k_model_rollout64; discounted sum inside the hold and a switch cost                      GAP 4.3e-7 -> TOL 2e-4
    "c1_64_mean_cd": dict(_C, X=3, UE=2, K=4, cd=0.7, cost=0.1),
    # 2: k_model_rollout<128>; 'ts1' with sampled noise, explicit member_idx / model_noise [S, K, N, ...]   GAP 1.6e-6 -> TOL 2e-4
    "c2_128_ts1_noise": dict(_C, X=5, UE=1, E=3, hidden=(128, 128), K=3, mode="ts1", noise=True, seed=1),
    # 3: the PPO layout: log_prob over both action dims, raw_action, env-major rows, normaliser on   GAP 6.9e-7 -> TOL 2e-4
    "c3_ppo_x4": dict(_C, X=4, UE=1, K=2, ppo=True, env_major=True, normalize=True, seed=2),
    # 4: learned reward (2x + 2), a termination box (on x_2) checked at every inner step, a start buffer   GAP 1.3e-7 -> TOL 2e-4
    "c4_lr_box_start": dict(_C, X=3, UE=1, K=4, reward="learned", box=([-INF, -INF, -1.2], [INF, INF, 1.2]), start=True, seed=3),
    # 5: the analytic Pendulum under a 64-wide policy, Pendulum reward, a box on thetadot            GAP 3.6e-7 -> TOL 2e-4
    "c5_pendulum_box": dict(_C, X=3, UE=1, K=4, E=0, system="pendulum", reward="pendulum", box=([-INF, -INF, -2.5], [INF, INF, 2.5]),
                            cd=0.3, seed=4),
    # 6: k_model_rollout<256>                                                                        GAP 9.6e-7 -> TOL 2e-4
    "c6_256_e2": dict(_C, X=3, UE=2, E=2, hidden=(256, 256), K=2, cd=0.5, cost=0.05, seed=5),
}
# per case: (the measured fp32-fp64 gap, the tolerance chosen from it)
GAP_TOL = {
    "c1_64_mean_cd": (4.3e-7, 2e-4),
    "c2_128_ts1_noise": (1.6e-6, 2e-4),
    "c3_ppo_x4": (6.9e-7, 2e-4),
    "c4_lr_box_start": (1.3e-7, 2e-4),
    "c5_pendulum_box": (3.6e-7, 2e-4),
    "c6_256_e2": (9.6e-7, 2e-4),
}
INT_MARGIN = 1e-3        # a decision is kept when t / dt is at least this far from an integer (fp64) and k agrees between fp32 and fp64
MAX_EXCLUDED = 0.10      # at most this share of the envs may be dropped
MIN_HOLD_SHARE = 0.05    # every k in 1 .. K is taken by at least this share of the kept decisions
MIN_INNER_TERMINATIONS = 5


def tol(name: str) -> float:
    return GAP_TOL[name][1]


def time_adaptive(name: str):
    """The host object of the case: its kernel_spec() is what the device run passes."""
    from mbpo.systems import TimeAdaptive
    c = CASES[name]
    ta = TimeAdaptive(DT, (c["K"] + 0.999) * DT, DT, switch_cost=c["cost"], continuous_discounting=c["cd"])
    assert ta.max_steps == c["K"]
    return ta


def hold(name: str) -> taref.Hold:
    ks = time_adaptive(name).kernel_spec()
    return taref.Hold(ks["hold_min_time"], ks["hold_max_time"], ks["hold_dt"], ks["hold_max_steps"], ks["hold_gamma"], ks["hold_switch_cost"])


def member_params(dims, E, g) -> torch.Tensor:
    return torch.cat([onets.init_mlp_flat(dims, g) + 0.05 * torch.randn(onets.n_params(dims), generator=g) for _ in range(E)])


@functools.lru_cache(maxsize=None)
def build(name: str) -> dict:
    c = CASES[name]
    X, UE, E, K = c["X"], c["UE"], c["E"], c["K"]
    A = UE + 1
    g = torch.Generator().manual_seed(2000 + c["seed"])
    pdims = [X, *c["hidden"][:3], 2 * A] if c["system"] == "ensemble" else [X, 64, 64, 2 * A]
    ppar = onets.init_mlp_flat(pdims, g) + 0.02 * torch.randn(onets.n_params(pdims), generator=g)
    ddims = dpar = None
    if c["system"] == "ensemble":
        ddims = [X + UE, *c["hidden"], 2 * X + (2 if c["reward"] == "learned" else 0)]
        dpar = member_params(ddims, E, g)
    tgt, q, r = torch.randn(X, generator=g), torch.rand(X, generator=g), torch.rand(UE, generator=g) * 0.1
    if X == 3 and (c["start"] or c["system"] == "pendulum"):      # pendulum-shaped states (case 4: the true buffer's)
        obs0, first = fc._pendulum_obs(N, g, 2.0), fc._pendulum_obs(N, g, 2.0)
    else:
        obs0, first = torch.randn(N, X, generator=g), torch.randn(N, X, generator=g)
    return dict(c, A=A, pdims=pdims, ddims=ddims, ppar=ppar, dpar=dpar, rparams=torch.cat([tgt, q, r]),
                obs0=obs0, first=first, steps0=(torch.arange(N) % 3).float(), done0=(torch.rand(N, generator=g) < 0.15).float(),
                pnoise=torch.randn(S, N, A, generator=g),
                midx=torch.randint(0, max(E, 1), (S, K, N), generator=g, dtype=torch.int32) if c["mode"] == "ts1" else None,
                mnoise=torch.randn(S, K, N, X, generator=g) if c["noise"] else None,
                nm=torch.randn(X, generator=g) * 0.3 if c["normalize"] else None,
                ns=torch.rand(X, generator=g) + 0.5 if c["normalize"] else None)


def ref_system(name: str, dtype=torch.float32):
    """The inner system of the case in `dtype`: it sees [x, u] only."""
    b = build(name)
    X, UE, E = b["X"], b["UE"], b["E"]
    if b["system"] == "pendulum":
        return osys.PendulumSystem()
    dpar = b["dpar"].to(dtype)
    kw = dict(mode=b["mode"], sample_noise=b["noise"])
    if b["reward"] == "learned":
        return lref.LearnedRewardEnsembleSystem(dpar, b["ddims"], E, X, UE, **kw)
    tgt, q, r = b["rparams"][:X], b["rparams"][X:2 * X], b["rparams"][2 * X:]
    rfn = lambda x, u: osys.quadratic_reward(x, u, tgt.to(x.dtype), q.to(x.dtype), r.to(x.dtype))
    return osys.EnsembleSystem(dpar, b["ddims"], E, X, UE, reward_fn=rfn, **kw)


class _Gather64:
    """oracle.replay.UniformSamplingQueue whose gathered rows are float64 (the same values)."""

    def __init__(self, queue):
        self.queue = queue

    def gather(self, qstate, idx):
        return self.queue.gather(qstate, idx).astype("float64")


def _box(b):
    return None if b["box"] is None else (torch.tensor(b["box"][0]), torch.tensor(b["box"][1]))


@functools.lru_cache(maxsize=None)
def oracle(name: str, dtype=torch.float32) -> dict:
    """The reference run (time_adaptive_ref.rollout's dict)."""
    b = build(name)
    c = lambda t: None if t is None else t.to(dtype)
    st0 = oro.EnvState(c(b["obs0"]), c(b["first"]), c(b["steps0"]), c(b["done0"]))
    start = None
    if b["start"]:
        queue, qstate = fc.oracle_buffer("pendulum")
        start = dict(queue=_Gather64(queue) if dtype == torch.float64 else queue, qstate=qstate, seed=SEED, offset=OFFSET)
    return taref.rollout(ref_system(name, dtype), b["UE"], hold(name), c(b["ppar"]), b["pdims"], st0, S, L, box=_box(b),
                         norm_mean=c(b["nm"]), norm_std=c(b["ns"]), policy_noise=c(b["pnoise"]), model_noise=c(b["mnoise"]),
                         member_idx=b["midx"], ppo_extras=b["ppo"], env_major=b["env_major"], start=start)


def env_rows(rows: torch.Tensor, name: str) -> torch.Tensor:
    """[N, S, D] whatever the case's row order."""
    return rows.reshape(N, S, -1) if build(name)["env_major"] else rows.reshape(S, N, -1).permute(1, 0, 2)


@functools.lru_cache(maxsize=None)
def kept(name: str) -> dict:
    """What the comparison rests on, from the two reference runs alone: dec [S, N] kept decisions (t / dt at least INT_MARGIN from an
    integer in fp64, k equal in fp32 and fp64), env [N] kept envs (all decisions kept; with a box, never within 10 * TOL of a finite
    bound — termination_ref's rule at the case's tolerance — and the same termination record in both runs), gap (the fp32-fp64 row
    gap over the kept envs)."""
    b = build(name)
    o32, o64 = oracle(name, torch.float32), oracle(name, torch.float64)
    X, A = b["X"], b["A"]
    acts = env_rows(o64["rows"], name)[:, :, X:X + A].permute(1, 0, 2)      # [S, N, A]
    dec = (taref.integer_distance(acts, b["UE"], hold(name)) >= INT_MARGIN) & (o32["k"] == o64["k"])
    env = dec.all(dim=0)
    if b["box"] is not None:
        near = ~((o64["box_dist"] >= 10 * tol(name)).all(dim=0)) | ~((o32["box_dist"] >= 10 * tol(name)).all(dim=0))
        env = env & ~near & (o32["term_at"] == o64["term_at"]).all(dim=0)
    r32, r64 = env_rows(o32["rows"], name)[env].double(), env_rows(o64["rows"], name)[env]
    gap = float(((r32 - r64).abs() / (1 + r64.abs())).max())
    return dict(dec=dec, env=env, gap=gap)


def device_kwargs(name: str, dev) -> dict:
    """The system side of the case for ops.model_rollout, the hold through TimeAdaptive.kernel_spec()."""
    from mbpo import _hip, ops
    b = build(name)
    d = lambda t: None if t is None else t.to(dev)
    if b["system"] == "pendulum":
        p = osys.PendulumParams()
        kw = dict(system_kind=_hip.SYS_PENDULUM, sys_params=torch.tensor(p.sys_vector(), device=dev), reward_kind=_hip.REWARD_PENDULUM,
                  reward_params=torch.tensor(p.reward_vector(), device=dev))
    else:
        kw = dict(system_kind=_hip.SYS_ENSEMBLE, dyn_params=d(b["dpar"]), dyn_spec=ops.MlpSpec(b["ddims"], "swish", b["E"]),
                  ens_mode={"mean": _hip.ENS_MEAN, "ts1": _hip.ENS_TS1}[b["mode"]], ens_predict_delta=True, ens_sample_noise=b["noise"],
                  reward_kind=_hip.REWARD_LEARNED if b["reward"] == "learned" else _hip.REWARD_QUADRATIC,
                  reward_params=None if b["reward"] == "learned" else d(b["rparams"]), member_idx=d(b["midx"]), model_noise=d(b["mnoise"]))
    if b["box"] is not None:
        kw.update(term_low=torch.tensor(b["box"][0], device=dev), term_high=torch.tensor(b["box"][1], device=dev))
    if b["start"]:
        data, state = fc.device_buffer("pendulum", dev)
        kw.update(start_rows=data, start_state=state, seed=SEED, offset=OFFSET)
    kw.update(time_adaptive(name).kernel_spec())
    return kw


def run_device(name: str, dev, **override):
    """Case `name` through ops.model_rollout.  Returns (rows, obs, first_obs, steps, done) as host tensors."""
    from mbpo import ops
    b = build(name)
    d = lambda t: None if t is None else t.to(dev)
    obs, first, steps, done = d(b["obs0"]).clone(), d(b["first"]).clone(), d(b["steps0"]).clone(), d(b["done0"]).clone()
    kw = device_kwargs(name, dev)
    kw.update(override)
    rows = ops.model_rollout(policy_params=d(b["ppar"]), policy_spec=ops.MlpSpec(b["pdims"], "swish", 1), x_dim=b["X"], u_dim=b["A"], obs=obs,
                             first_obs=first, steps=steps, done=done, n_steps=S, episode_length=L, norm_mean=d(b["nm"]),
                             norm_std=d(b["ns"]), ppo_extras=b["ppo"], env_major=b["env_major"], policy_noise=d(b["pnoise"]), **kw)
    torch.cuda.synchronize()
    return rows.cpu(), obs.cpu(), first.cpu(), steps.cpu(), done.cpu()
