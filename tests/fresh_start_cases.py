"""Fresh-start rollout cases shared by tests/test_cpu_fresh_starts.py and tests/test_gpu_fresh_starts.py: the inputs
(tests/termination_cases.py's parameter recipe), the true buffer, and the reference run of tests/fresh_start_ref.py — two consecutive
launches, computed once per case and left unchanged.

Common shapes: N = 40 envs (2.5 tiles: a partial tile, and a pair with an empty second slot), S = 5 steps, episode_length = 2 with
initial steps = env % 2 (neighbours of one tile reset on different steps) and a few envs entering already done, a true buffer of
max_size 37 into which 50 rows went in three inserts (wrapped, head != 0) with sample_position set to 5, two launches under
different offsets so that the written-back first_obs is consumed.  The termination case keeps tests/termination_cases.py's own shapes.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from oracle import nets as onets
from oracle import replay as oreplay
from oracle import rollout as oro
from oracle import systems as osys

import fresh_start_ref as fref
import learned_reward_ref as lref
import termination_cases as tc
import termination_ref as tref

BUF_MAX, BUF_INSERTS, BUF_SAMPLE_POSITION = 37, (20, 20, 10), 5
SEED, OFFSETS = 1234, ((7 << 32) + 3, (9 << 32) + 4)       # (seed, offset) of the two launches: high and low offset words in use
LAUNCHES = 2

_C = dict(N=40, S=5, L=2, AR=1, X=4, U=1, system="ensemble", E=5, mode="mean", sample_noise=False, hidden=(64, 64, 64), seed=0,
          reward="quadratic", openloop=False, bounds=None, atol=2e-4)
CASES = {
    "pendulum": dict(_C, X=3, system="pendulum", E=0, reward="pendulum"),
    "ens_ts1_noise": dict(_C, mode="ts1", sample_noise=True),
    "learned_reward_x6": dict(_C, X=6, E=3, reward="learned", mode="tsinf"),
    "wide128_x17": dict(_C, X=17, U=6, E=3, mode="tsinf", hidden=(128, 128), atol=5e-4),
    "wide256": dict(_C, E=2, hidden=(256, 256)),
    "openloop_pendulum": dict(_C, X=3, system="pendulum", E=0, reward="pendulum", openloop=True),
    # tests/termination_cases.py's "a_ragged_n40" (N = 40, S = 6, episode_length 5, a box on x_0 and x_3) with a start buffer
    "termination": dict(tc.CASES["a_ragged_n40"], reward="quadratic", openloop=False, buf_seed=3),
}
LEAN = ("pendulum", "ens_ts1_noise", "termination")      # the shapes k_rollout_lean takes


def _pendulum_obs(n, gen, speed):
    th = (torch.rand(n, generator=gen) * 2 - 1) * math.pi
    thd = (torch.rand(n, generator=gen) * 2 - 1) * speed
    return torch.stack([torch.cos(th), torch.sin(th), thd], dim=1)


def buffer_rows(name: str) -> torch.Tensor:
    """The 50 rows [obs | action | reward | discount | next_obs] inserted into the case's true buffer."""
    c = CASES[name]
    X, U = c["X"], c["U"]
    g = torch.Generator().manual_seed(100 + c.get("buf_seed", 0))
    n = sum(BUF_INSERTS)
    rows = torch.randn(n, 2 * X + U + 2, generator=g)
    rows[:, :X] = _pendulum_obs(n, g, 4.0) if X == 3 else 0.3 * torch.randn(n, X, generator=g)
    return rows


def oracle_buffer(name: str):
    """(queue, state) of oracle.replay.UniformSamplingQueue after the inserts, sample_position moved to BUF_SAMPLE_POSITION."""
    rows = buffer_rows(name).numpy()
    q = oreplay.UniformSamplingQueue(BUF_MAX, rows.shape[1], 1)
    st, at = q.init(), 0
    for n in BUF_INSERTS:
        st = q.insert(st, rows[at:at + n])
        at += n
    assert int(st["insert_position"]) == BUF_MAX
    st["sample_position"] = np.int32(BUF_SAMPLE_POSITION)
    return q, st


def device_buffer(name: str, dev):
    """(data, state) of the same buffer on the device, through mbpo_replay_insert (head != 0)."""
    from mbpo import ops
    rows = buffer_rows(name).to(dev)
    data = torch.zeros(BUF_MAX, rows.shape[1], device=dev)
    state = torch.zeros(4, dtype=torch.int32, device=dev)
    at = 0
    for n in BUF_INSERTS:
        ops.replay_insert(data, state, rows[at:at + n].contiguous())
        at += n
    state[1] = BUF_SAMPLE_POSITION
    return data, state


@functools.lru_cache(maxsize=None)
def build(name: str) -> dict:
    """Host tensors and the oracle system of case `name`; the random tensors cover both launches ([LAUNCHES * S, ...])."""
    c = CASES[name]
    if name == "termination":
        b = dict(tc.build("a_ragged_n40"))
        N, S, AR, X, U, E = b["N"], b["S"], b["AR"], b["X"], b["U"], b["E"]
        g = torch.Generator().manual_seed(77)
        b.update(pnoise=torch.cat([b["pnoise"], torch.randn(S, N, U, generator=g)]), actions=None, reward="quadratic", openloop=False,
                 osystem=tref.TerminatingSystem(b["osystem"], b["low"], b["high"]))
        return b
    N, S, L, AR, X, U, E = c["N"], c["S"], c["L"], c["AR"], c["X"], c["U"], c["E"]
    g = torch.Generator().manual_seed(c["seed"])
    T = LAUNCHES * S
    pdims = [X, *c["hidden"], 2 * U]
    ppar = onets.init_mlp_flat(pdims, g) + 0.02 * torch.randn(onets.n_params(pdims), generator=g)
    if X == 3:
        obs0, first = _pendulum_obs(N, g, 8.0), _pendulum_obs(N, g, 4.0)
    else:
        obs0, first = torch.randn(N, X, generator=g), 0.3 * torch.randn(N, X, generator=g)
    steps0 = (torch.arange(N) % 2).float()
    done0 = (torch.rand(N, generator=g) < 0.2).float()
    pnoise = torch.randn(T, N, U, generator=g)
    mnoise = torch.randn(T, AR, N, X, generator=g) if c["sample_noise"] else None
    midx = torch.randint(0, max(E, 1), (T, AR, N), generator=g, dtype=torch.int32) if c["mode"] == "ts1" else None
    actions = (torch.rand(T, N, U, generator=g) * 2 - 1) if c["openloop"] else None
    out = dict(c, pdims=pdims, ppar=ppar, obs0=obs0, first=first, steps0=steps0, done0=done0, pnoise=pnoise, mnoise=mnoise, midx=midx,
               actions=actions, ppo=False, env_major=False, low=None, high=None)
    if c["system"] == "pendulum":
        pp = osys.PendulumParams()
        out.update(osystem=osys.PendulumSystem(pp), rparams=torch.tensor(pp.reward_vector()), sys_vector=torch.tensor(pp.sys_vector()))
        return out
    learned = c["reward"] == "learned"
    ddims = [X + U, *c["hidden"], 2 * X + (2 if learned else 0)]
    dpar = torch.cat([onets.init_mlp_flat(ddims, g) * 0.5 + 0.01 * torch.randn(onets.n_params(ddims), generator=g) for _ in range(E)])
    kw = dict(mode=c["mode"], predict_delta=True, sample_noise=c["sample_noise"], min_std=1e-3)
    if learned:
        out.update(ddims=ddims, dpar=dpar, rparams=None, osystem=lref.LearnedRewardEnsembleSystem(dpar, ddims, E, X, U, **kw))
    else:
        tgt, q, r = torch.randn(X, generator=g), torch.rand(X, generator=g), torch.rand(U, generator=g) * 0.1
        out.update(ddims=ddims, dpar=dpar, rparams=torch.cat([tgt, q, r]),
                   osystem=osys.EnsembleSystem(dpar, ddims, E, X, U, reward_fn=lambda x, u: osys.quadratic_reward(x, u, tgt, q, r), **kw))
    return out


def _slice(t, k, S):
    return None if t is None else t[k * S:(k + 1) * S]


@functools.lru_cache(maxsize=None)
def oracle(name: str) -> dict:
    """The reference run: per launch the rows and the EnvState after it, every draw, and (termination) the kept-env mask."""
    c = build(name)
    q, qs = oracle_buffer(name)
    S = c["S"]
    st = oro.EnvState(c["obs0"], c["first"], c["steps0"], c["done0"])
    draws = fref.Draws()
    rows, states = [], []
    for k in range(LAUNCHES):
        st, r, draws = fref.rollout(c["osystem"], c["ppar"], c["pdims"], st, S, c["L"], queue=q, qstate=qs, seed=SEED, offset=OFFSETS[k],
                                    action_repeat=c["AR"], policy_noise=_slice(c["pnoise"], k, S), model_noise=_slice(c["mnoise"], k, S),
                                    member_idx=_slice(c["midx"], k, S), actions=_slice(c["actions"], k, S), ppo_extras=c["ppo"],
                                    env_major=c["env_major"], draws=draws, launch=k)
        rows.append(r)
        states.append(st)
    keep = torch.ones(c["N"], dtype=torch.bool)
    if name == "termination":
        keep = tref.check_oracle_run(c["osystem"], torch.cat(rows)[:, -1], last_of=c["AR"])
    return dict(rows=rows, states=states, draws=draws, keep=keep, queue=q, qstate=qs)


def device_kwargs(name: str, dev, launch: int, env=None, start=True) -> dict:
    """ops.model_rollout keyword arguments of launch `launch`; `env` = (obs, first_obs, steps, done) device tensors carried over from
    the launch before (None: fresh ones from the case).  start: (data, state) of device_buffer, True to build it, None for none."""
    from mbpo import _hip, ops
    c = build(name)
    X, U, S = c["X"], c["U"], c["S"]
    mv = lambda t: None if t is None else _slice(t, launch, S).contiguous().to(dev)
    if env is None:
        env = tuple(c[k].to(dev) for k in ("obs0", "first", "steps0", "done0"))
    kw = dict(x_dim=X, u_dim=U, obs=env[0], first_obs=env[1], steps=env[2], done=env[3], n_steps=S, episode_length=c["L"],
              action_repeat=c["AR"], reward_params=None if c["rparams"] is None else c["rparams"].to(dev), ppo_extras=c["ppo"],
              env_major=c["env_major"], model_noise=mv(c["mnoise"]), member_idx=mv(c["midx"]), seed=SEED, offset=OFFSETS[launch])
    if c["openloop"]:
        kw.update(actions=mv(c["actions"]))
    else:
        kw.update(policy_params=c["ppar"].to(dev), policy_spec=ops.MlpSpec(c["pdims"], "swish", 1), policy_noise=mv(c["pnoise"]))
    if c["system"] == "pendulum":
        kw.update(system_kind=_hip.SYS_PENDULUM, sys_params=c["sys_vector"].to(dev), reward_kind=_hip.REWARD_PENDULUM)
    else:
        kw.update(system_kind=_hip.SYS_ENSEMBLE, dyn_params=c["dpar"].to(dev), dyn_spec=ops.MlpSpec(c["ddims"], "swish", c["E"]),
                  ens_mode={"mean": _hip.ENS_MEAN, "ts1": _hip.ENS_TS1, "tsinf": _hip.ENS_TSINF}[c["mode"]],
                  ens_predict_delta=True, ens_sample_noise=c["sample_noise"], ens_min_std=1e-3,
                  reward_kind=_hip.REWARD_LEARNED if c["reward"] == "learned" else _hip.REWARD_QUADRATIC)
    if c["low"] is not None:
        kw.update(term_low=c["low"].to(dev), term_high=c["high"].to(dev))
    if start is True:
        start = device_buffer(name, dev)
    if start is not None:
        kw.update(start_rows=start[0], start_state=start[1])
    return kw
