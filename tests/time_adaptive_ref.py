"""Test-tree restatement of time-adaptive rollouts (include/mbpo_hip.h, "time-adaptive rollouts"), built on the oracle.

The policy's action is [u (u_env) | tau].  With t_lo / t_hi / dt / K / gamma / switch_cost the hold's parameters:
    t = (t_hi - t_lo) / 2 * tau + (t_hi + t_lo) / 2                (one fused multiply-add)
    k = clamp((int) floor_divide(t, dt), 1, K)                     floor_divide: jnp.floor_divide on floats, as the header states it
    for j < k, while the row has not terminated:  r_j = reward(x_j, u);  x_{j+1} = system.step(x_j, u)
    R = sum_j w_j r_j - switch_cost,  w_0 = 1, w_{j+1} = w_j * gamma   (each product rounded before it is added)
    with a box: checked after every inner step; a violated x_{j+1} freezes the row there, sys_done = 1
    steps += k_eff;  over = steps >= episode_length;  done = over ? 1 : sys_done;  truncation = over ? 1 - sys_done : 0
The inner system is one of oracle.systems' (or a test-tree subclass): its `step(x, u, member_idx=, model_noise=, env_index=)` sees the
u_env control columns only.  The episode bookkeeping restates oracle.rollout.env_step with `action_repeat` replaced by k_eff; the
policy, the rows and their order are oracle.rollout.rollout's.  With a start buffer every reset is followed by the draw of
tests/fresh_start_ref.py (one per decision).  member_idx is [S, K, N], model_noise [S, K, N, x].

fp32 and fp64: the hold's parameters are the fp32 values the host hands the kernels, in both.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from oracle import nets
from oracle import rollout as oro

import fresh_start_ref as fref
import termination_ref as tref


@dataclass
class Hold:
    t_lo: float
    t_hi: float
    dt: float
    K: int
    gamma: float = 1.0
    switch_cost: float = 0.0


def floor_divide_f(x1: torch.Tensor, x2: torch.Tensor) -> torch.Tensor:
    """jnp.floor_divide for floats: remainder-based, then rounded (halves away from zero, as roundf)."""
    mod = torch.fmod(x1, x2)
    div = (x1 - mod) / x2
    div = torch.where((mod != 0) & ((x2 < 0) != (mod < 0)), div - 1, div)
    return torch.sign(div) * torch.floor(div.abs() + 0.5)


def switch_time(tau: torch.Tensor, h: Hold) -> torch.Tensor:
    """t in tau's dtype.  fp32: the multiply-add is fused on the device — formed here in fp64 (the product of two fp32 numbers is
    exact there) and rounded to fp32."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    a, c = (f(h.t_hi) - f(h.t_lo)) / 2, (f(h.t_hi) + f(h.t_lo)) / 2
    t = a.double() * tau.double() + c.double()
    return t.to(tau.dtype)


def hold_steps(tau: torch.Tensor, h: Hold) -> torch.Tensor:
    """k [n] int64."""
    dt = torch.tensor(h.dt, dtype=torch.float32).to(tau.dtype)
    return floor_divide_f(switch_time(tau, h), dt).long().clamp(1, h.K)


def rollout(system, u_env: int, hold: Hold, policy_params, policy_dims, st: oro.EnvState, n_steps: int, episode_length: int, *,
            box=None, act: str = "swish", norm_mean=None, norm_std=None, policy_noise=None, actions=None, model_noise=None,
            member_idx=None, ppo_extras: bool = False, env_major: bool = False, start=None):
    """S decisions for N envs.  box: (low, high) or None.  actions: open-loop [S, N, A] instead of a policy.  start: dict(queue=,
    qstate=, seed=, offset=) of a true buffer.  Returns dict(state, rows [S*N, D], k [S, N], k_eff [S, N], term_at [S, N] (the inner
    step whose next state left the box, -1: none), box_dist [S, N] (smallest distance to a finite bound over the inner steps the row
    took), reset [S, N])."""
    N, X = st.obs.shape
    A = u_env + 1
    dtype = st.obs.dtype
    D = oro.row_len(X, A, ppo_extras)
    rows = torch.zeros(n_steps, N, D, dtype=dtype)
    st = st.clone()
    env_index = torch.arange(N)
    gamma = torch.tensor(hold.gamma, dtype=torch.float32).to(dtype)
    cost = torch.tensor(hold.switch_cost, dtype=torch.float32).to(dtype)
    rec = dict(k=[], k_eff=[], term_at=[], box_dist=[], reset=[])
    for s in range(n_steps):
        obs = st.obs
        if actions is None:
            logits = nets.mlp_forward(policy_params, policy_dims, nets.normalize(obs, norm_mean, norm_std), act)
            z = nets.sample_no_postprocessing(logits, policy_noise[s])
            action = nets.postprocess(z)
        else:
            action = actions[s]
        u, tau = action[:, :u_env], action[:, u_env]
        k = hold_steps(tau, hold)
        # AutoReset.step: zero `steps` where previously done
        steps = torch.where(st.done != 0, torch.zeros_like(st.steps), st.steps)
        x = obs
        R = torch.zeros(N, dtype=dtype)
        w = torch.ones((), dtype=dtype)
        term = torch.zeros(N, dtype=dtype)
        k_eff = torch.zeros(N, dtype=dtype)
        term_at = torch.full((N,), -1, dtype=torch.long)
        dist = torch.full((N,), float("inf"), dtype=dtype)
        for j in range(int(k.max())):
            live = (j < k) & (term == 0)
            kw = {}
            if member_idx is not None:
                kw["member_idx"] = member_idx[s, j]
            if model_noise is not None:
                kw["model_noise"] = model_noise[s, j]
            xn, r = system.step(x, u, env_index=env_index, **kw)[:2]
            R = torch.where(live, R + w * r, R)
            x = torch.where(live[:, None], xn, x)
            k_eff = k_eff + live.to(dtype)
            if box is not None:
                lo, hi = box[0].to(dtype), box[1].to(dtype)
                left = live & (tref.box_done(xn, lo, hi) != 0)
                term = torch.where(left, torch.ones_like(term), term)
                term_at = torch.where(left, torch.full_like(term_at, j), term_at)
                d = torch.full((N,), float("inf"), dtype=dtype)
                for b in (lo, hi):
                    fin = torch.isfinite(b)
                    if bool(fin.any()):
                        d = torch.minimum(d, (xn[:, fin] - b[fin]).abs().min(dim=1).values)
                dist = torch.where(live, torch.minimum(dist, d), dist)
            w = w * gamma
        R = R - cost
        steps = steps + k_eff
        over = steps >= episode_length
        done = torch.where(over, torch.ones_like(term), term)
        trunc = torch.where(over, 1 - term, torch.zeros_like(term))
        nobs = torch.where(done[:, None] != 0, st.first_obs, x)
        r_ = rows[s]
        r_[:, 0:X] = obs
        r_[:, X:X + A] = action
        r_[:, X + A] = R
        r_[:, X + A + 1] = 1 - done
        r_[:, X + A + 2:2 * X + A + 2] = nobs
        if ppo_extras:
            r_[:, 2 * X + A + 2] = nets.log_prob(logits, z)
            r_[:, 2 * X + A + 3:2 * X + 2 * A + 3] = z
        r_[:, D - 1] = trunc
        first = st.first_obs
        if start is not None:          # the reset consumed first_obs of the envs that came out done: each gets its next start state
            done_envs = np.nonzero(done.numpy() != 0)[0]
            if done_envs.size:
                qs = start["qstate"]
                idx = fref.draw_indices(start["seed"], start["offset"], s, N, done_envs, qs["sample_position"], qs["insert_position"])
                first = first.clone()
                first[torch.from_numpy(done_envs)] = torch.from_numpy(start["queue"].gather(qs, idx)[:, :X].copy()).to(dtype)
        st = oro.EnvState(nobs, first, steps, done)
        for key, v in (("k", k), ("k_eff", k_eff.long()), ("term_at", term_at), ("box_dist", dist), ("reset", done != 0)):
            rec[key].append(v)
    if env_major:
        rows = rows.permute(1, 0, 2)
    out = {key: torch.stack(v) for key, v in rec.items()}
    out.update(state=st, rows=rows.reshape(n_steps * N, D).contiguous())
    return out


def integer_distance(actions: torch.Tensor, u_env: int, hold: Hold) -> torch.Tensor:
    """|t / dt - nearest integer| in fp64 for the actions [..., A]: a decision closer than 1e-3 to an integer may take another k on
    the device, whose tau differs from the reference's in the last bits."""
    q = switch_time(actions[..., u_env].double(), hold) / torch.tensor(hold.dt, dtype=torch.float32).double()
    return (q - torch.round(q)).abs()
