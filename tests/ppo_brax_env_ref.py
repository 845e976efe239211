"""Test-tree restatement of the reference's brax-env PPO variant (ppo/ppo_brax_env.py + ppo/losses_new.py), built on the oracle:

  PPOLoss.loss with non_equidistant_time    losses_new.py:105-120 (per-sample discount), :181-226 (compute_gae with it)
  optax.chain(clip_by_global_norm, adamw)   ppo_brax_env.py:137-141

The loss is oracle.ppo.loss with the scalar discount of compute_gae replaced by a per-step [T,B] array when `neq` is given;
everything else (networks, log-probs, entropy, advantage normalisation) is the oracle's own code.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from oracle import nets, scans
from oracle import ppo as oppo
from oracle.sac import adamw_step


@dataclass
class Neq:
    """non_equidistant_time's parameters (ppo_brax_env.py constructor)."""
    continuous_discounting: float
    min_time_between_switches: float
    max_time_between_switches: float
    env_dt: float


def floor_divide(x, y):
    """jnp.floor_divide for floats: remainder-based, then rounded (numpy's own float floor_divide)."""
    mod = np.fmod(x, y)
    div = (x - mod) / y
    div = np.where((mod != 0) & ((y < 0) != (mod < 0)), div - 1, div)
    return np.round(div)


def per_sample_discount(action_last: np.ndarray, neq: Neq, dtype) -> np.ndarray:
    """losses_new.py:105-112: discount from the switch time encoded in the last action component."""
    a = np.asarray(action_last, dtype)
    tl, tu, dt = dtype(neq.min_time_between_switches), dtype(neq.max_time_between_switches), dtype(neq.env_dt)
    t = (tu - tl) / dtype(2) * a + (tu + tl) / dtype(2)
    t = floor_divide(t, dt) * dt
    return np.exp(-dtype(neq.continuous_discounting) * t).astype(dtype)


def loss(cfg: oppo.PpoConfig, params, data, ent_noise, norm_mean=None, norm_std=None, neq: Optional[Neq] = None):
    """PPOLoss.loss of losses_new.py on data [B, T, D].  Returns (total, the four terms, vs, raw advantages [T,B], normalised ones)."""
    X, U = cfg.x_dim, cfg.u_dim
    np_dtype = np.float64 if data.dtype == torch.float64 else np.float32
    pol, val = params[:cfg.P], params[cfg.P:cfg.P + cfg.V]
    t = {k: v.transpose(0, 1) for k, v in oppo.split_rows(data, X, U).items()}
    obs = nets.normalize(t["obs"], norm_mean, norm_std)
    logits = nets.mlp_forward(pol, cfg.policy_dims, obs, cfg.policy_act)
    baseline = nets.mlp_forward(val, cfg.value_dims, obs, cfg.value_act)[..., 0]
    boot = nets.mlp_forward(val, cfg.value_dims, nets.normalize(t["next_obs"][-1], norm_mean, norm_std), cfg.value_act)[..., 0]
    rewards = t["reward"] * cfg.reward_scaling
    truncation = t["truncation"]
    termination = (1 - t["discount"]) * (1 - truncation)
    target_lp = nets.log_prob(logits, t["raw_action"])
    behaviour_lp = t["log_prob"]
    if neq is not None:
        discounting = per_sample_discount(t["action"][..., -1].detach().numpy(), neq, np_dtype)      # [T, B]
    else:
        discounting = cfg.discounting
    vs_np, adv_np = scans.compute_gae(truncation.detach().numpy(), termination.detach().numpy(), rewards.detach().numpy(),
                                      baseline.detach().numpy(), boot.detach().numpy(), discounting, cfg.gae_lambda, dtype=np_dtype)
    vs, adv_raw = torch.from_numpy(vs_np).to(data.dtype), torch.from_numpy(adv_np).to(data.dtype)
    adv = adv_raw
    if cfg.normalize_advantage:
        adv = (adv - adv.mean()) / (adv.std(unbiased=False) + 1e-8)
    rho = torch.exp(target_lp - behaviour_lp)
    s1 = rho * adv
    s2 = torch.clamp(rho, 1 - cfg.clipping_epsilon, 1 + cfg.clipping_epsilon) * adv
    policy_loss = -torch.minimum(s1, s2).mean()
    v_error = vs - baseline
    v_loss = (v_error * v_error).mean() * 0.5
    entropy = nets.entropy(logits, ent_noise.transpose(0, 1)).mean()
    entropy_loss = cfg.entropy_cost * -entropy
    total = policy_loss + v_loss + entropy_loss
    return total, dict(total_loss=total, policy_loss=policy_loss, v_loss=v_loss, entropy_loss=entropy_loss), vs, adv_raw, adv


def grads(cfg, params, data, ent_noise, norm_mean=None, norm_std=None, neq: Optional[Neq] = None):
    p = params.clone().requires_grad_(True)
    total, terms, vs, adv_raw, _ = loss(cfg, p, data, ent_noise, norm_mean, norm_std, neq)
    total.backward()
    return p.grad.detach(), {k: float(v.detach()) for k, v in terms.items()}, vs, adv_raw


def clip_by_global_norm(g: torch.Tensor, max_norm: Optional[float]) -> torch.Tensor:
    """optax.clip_by_global_norm over the whole flat gradient: g if ||g|| < max_norm else (g / ||g||) * max_norm."""
    if max_norm is None:
        return g
    n = torch.sqrt((g * g).sum())
    return g if bool(n < max_norm) else (g / n) * max_norm


def minibatch_step(cfg, st: oppo.PpoState, data, ent_noise, norm_mean=None, norm_std=None, neq: Optional[Neq] = None,
                   max_grad_norm: Optional[float] = None, grad_override: Optional[torch.Tensor] = None):
    """ppo_brax_env.py's minibatch_step: loss gradient, clip_by_global_norm, adamw."""
    g, terms, _, _ = grads(cfg, st.params, data, ent_noise, norm_mean, norm_std, neq)
    if grad_override is not None:
        g = grad_override
    count = st.count + 1
    p, m, v = adamw_step(st.params, clip_by_global_norm(g, max_grad_norm), st.adam_m, st.adam_v, count, cfg.lr, cfg.wd)
    return oppo.PpoState(p, m, v, count), terms, g
