"""Terminating-rollout cases shared by tests/test_gpu_termination.py: the inputs (tests/test_gpu_rollout.py's parameter recipe, with
first_obs = 0.3 * randn for the ensembles and the Pendulum's first thetadot in +-4), the wrapped oracle system, and the oracle run —
computed once per case, checked for the three conditions of termination_ref.check_oracle_run, and left unchanged."""
from __future__ import annotations

import functools
import math

import torch

from oracle import nets as onets
from oracle import rollout as oro
from oracle import systems as osys

import termination_ref as tref

INF = math.inf


def box(X, intervals):
    low, high = [-INF] * X, [INF] * X
    for d, (lo, hi) in intervals.items():
        low[d], high[d] = lo, hi
    return torch.tensor(low), torch.tensor(high)


# name -> recipe.  (a)-(d) are the four base cases; the others vary (a) along one axis each.
_A = dict(N=48, S=6, L=5, AR=1, X=4, U=1, system="ensemble", E=5, mode="mean", sample_noise=False, hidden=(64, 64, 64), seed=0,
          bounds={0: (-1.0, 1.0), 3: (-INF, 1.0)}, ppo=False, env_major=False, atol=tref.ATOL)
CASES = {
    "a": _A,
    "b": dict(_A, mode="ts1", sample_noise=True),
    "c": dict(_A, X=3, system="pendulum", E=0, bounds={2: (-6.0, 6.0)}),
    "d": dict(_A, N=40, S=4, L=32, X=17, U=6, E=10, mode="tsinf", bounds={0: (-1.5, 1.5), 16: (-INF, 1.5)}, atol=5e-4),
    "a_ppo_env_major": dict(_A, ppo=True, env_major=True),
    "a_64x2": dict(_A, hidden=(64, 64)),
    "a_action_repeat2": dict(_A, AR=2),                 # action_repeat 2: the generic 64-wide kernel
    "a_128wide": dict(_A, hidden=(128, 128)),
    "a_256wide": dict(_A, hidden=(256, 256), E=2),
    "a_ragged_n40": dict(_A, N=40),
}


def _pendulum_obs(N, gen, speed):
    th = (torch.rand(N, generator=gen) * 2 - 1) * math.pi
    thd = (torch.rand(N, generator=gen) * 2 - 1) * speed
    return torch.stack([torch.cos(th), torch.sin(th), thd], dim=1)


@functools.lru_cache(maxsize=None)
def build(name: str) -> dict:
    """Host tensors, the oracle system (unwrapped) and the bounds of case `name`."""
    c = CASES[name]
    N, S, L, AR, X, U, E = c["N"], c["S"], c["L"], c["AR"], c["X"], c["U"], c["E"]
    g = torch.Generator().manual_seed(c["seed"])
    pdims = [X, *c["hidden"], 2 * U]
    ppar = onets.init_mlp_flat(pdims, g) + 0.02 * torch.randn(onets.n_params(pdims), generator=g)
    if X == 3:
        obs0, first = _pendulum_obs(N, g, 8.0), _pendulum_obs(N, g, 4.0)
    else:
        obs0, first = torch.randn(N, X, generator=g), 0.3 * torch.randn(N, X, generator=g)
    steps0 = torch.randint(0, L, (N,), generator=g).float()
    done0 = (torch.rand(N, generator=g) < 0.2).float()
    pnoise = torch.randn(S, N, U, generator=g)
    mnoise = torch.randn(S, AR, N, X, generator=g) if c["sample_noise"] else None
    midx = torch.randint(0, max(E, 1), (S, AR, N), generator=g, dtype=torch.int32) if c["mode"] == "ts1" else None
    pp = osys.PendulumParams()
    out = dict(c, pdims=pdims, ppar=ppar, obs0=obs0, first=first, steps0=steps0, done0=done0, pnoise=pnoise, mnoise=mnoise, midx=midx)
    if c["system"] == "pendulum":
        out.update(osystem=osys.PendulumSystem(pp), rparams=torch.tensor(pp.reward_vector()), sys_vector=torch.tensor(pp.sys_vector()))
    else:
        ddims = [X + U, *c["hidden"], 2 * X]
        dpar = torch.cat([onets.init_mlp_flat(ddims, g) * 0.5 + 0.01 * torch.randn(onets.n_params(ddims), generator=g) for _ in range(E)])
        tgt, q, r = torch.randn(X, generator=g), torch.rand(X, generator=g), torch.rand(U, generator=g) * 0.1
        out.update(ddims=ddims, dpar=dpar, rparams=torch.cat([tgt, q, r]),
                   osystem=osys.EnsembleSystem(dpar, ddims, E, X, U, mode=c["mode"], predict_delta=True, sample_noise=c["sample_noise"],
                                               min_std=1e-3, reward_fn=lambda x, u: osys.quadratic_reward(x, u, tgt, q, r)))
    out["low"], out["high"] = box(X, c["bounds"])
    return out


@functools.lru_cache(maxsize=None)
def oracle(name: str) -> dict:
    """The oracle run of case `name` with the wrapped system; asserts the three conditions on it (no device result involved).
    Returns rows_ref, the final EnvState, the kept-env mask and the counts."""
    c = build(name)
    wrapped = tref.TerminatingSystem(c["osystem"], c["low"], c["high"])
    st0 = oro.EnvState(c["obs0"], c["first"], c["steps0"], c["done0"])
    st_ref, rows_ref = oro.rollout(wrapped, c["ppar"], c["pdims"], st0, c["S"], c["L"], c["AR"], policy_noise=c["pnoise"],
                                   model_noise=c["mnoise"], member_idx=c["midx"], ppo_extras=c["ppo"], env_major=c["env_major"])
    # with action_repeat > 1 the step's sys_done is the LAST inner step's: the near rule looks at every inner step (stricter),
    # the terminating count at the last ones
    keep = tref.check_oracle_run(wrapped, rows_ref[:, -1], last_of=c["AR"])
    return dict(rows=rows_ref, state=st_ref, keep=keep, n_excluded=int((~keep).sum()), n_terminating=int(wrapped.terminated_mask(c["AR"]).sum()),
                n_truncations=int(rows_ref[:, -1].sum()))


def device_kwargs(name: str, dev, with_termination: bool = True) -> dict:
    """The ops.model_rollout keyword arguments of case `name` (fresh env-state tensors on every call)."""
    from mbpo import _hip, ops
    c = build(name)
    X, U = c["X"], c["U"]
    mv = lambda t: None if t is None else t.to(dev)
    kw = dict(policy_params=c["ppar"].to(dev), policy_spec=ops.MlpSpec(c["pdims"], "swish", 1), x_dim=X, u_dim=U,
              obs=c["obs0"].to(dev), first_obs=c["first"].to(dev), steps=c["steps0"].to(dev), done=c["done0"].to(dev),
              n_steps=c["S"], episode_length=c["L"], action_repeat=c["AR"], reward_params=c["rparams"].to(dev),
              ppo_extras=c["ppo"], env_major=c["env_major"], policy_noise=mv(c["pnoise"]), model_noise=mv(c["mnoise"]),
              member_idx=mv(c["midx"]))
    if c["system"] == "pendulum":
        kw.update(system_kind=_hip.SYS_PENDULUM, sys_params=c["sys_vector"].to(dev), reward_kind=_hip.REWARD_PENDULUM)
    else:
        kw.update(system_kind=_hip.SYS_ENSEMBLE, dyn_params=c["dpar"].to(dev), dyn_spec=ops.MlpSpec(c["ddims"], "swish", c["E"]),
                  ens_mode={"mean": _hip.ENS_MEAN, "ts1": _hip.ENS_TS1, "tsinf": _hip.ENS_TSINF}[c["mode"]],
                  ens_predict_delta=True, ens_sample_noise=c["sample_noise"], ens_min_std=1e-3, reward_kind=_hip.REWARD_QUADRATIC)
    if with_termination:
        kw.update(term_low=c["low"].to(dev), term_high=c["high"].to(dev))
    return kw


def env_rows(rows: torch.Tensor, name: str) -> torch.Tensor:
    """rows [S*N, D] -> [N, S, D] whatever the case's layout."""
    c = CASES[name]
    if c["env_major"]:
        return rows.reshape(c["N"], c["S"], -1)
    return rows.reshape(c["S"], c["N"], -1).transpose(0, 1)
