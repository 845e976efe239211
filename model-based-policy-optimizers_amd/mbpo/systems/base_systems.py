"""System / SystemParams / SystemState — mirrors mbpo/systems/base_systems.py:13-60.

`System.step(x, u, system_params)` keeps the reference signature; x may be a single state [x_dim] (what the reference
writes and vmaps) or a batch [N, x_dim] (batch-native here: one fused launch instead of vmap).
"""
from __future__ import annotations

import dataclasses
from abc import ABC
from dataclasses import dataclass, field
from typing import Any, Generic

import torch

from mbpo.systems.dynamics.base_dynamics import Dynamics, DynamicsParams
from mbpo.systems.rewards.base_rewards import Reward, RewardParams
from mbpo.utils import keys as K


@dataclass
class SystemParams(Generic[DynamicsParams, RewardParams]):
    dynamics_params: Any
    reward_params: Any
    key: int = 0

    def replace(self, **kw):
        return dataclasses.replace(self, **kw)


@dataclass
class SystemState(Generic[DynamicsParams, RewardParams]):
    x_next: torch.Tensor
    reward: torch.Tensor
    system_params: SystemParams
    done: Any = 0.0

    def replace(self, **kw):
        return dataclasses.replace(self, **kw)


class System(ABC, Generic[DynamicsParams, RewardParams]):
    time_adaptive = None      # (a subclass that never calls __init__ is not time-adaptive)

    def __init__(self, dynamics: Dynamics, reward: Reward, time_adaptive=None):
        """time_adaptive: a mbpo.systems.TimeAdaptive — the policy emits [u | tau] and the fused rollout holds u for k(tau) model
        steps (include/mbpo_hip.h "time-adaptive rollouts").  Fused systems only: a user-defined System steps once per call."""
        self.dynamics = dynamics
        self.reward = reward
        self.x_dim = dynamics.x_dim
        self.u_dim = dynamics.u_dim
        if time_adaptive is not None and not self.fused:
            raise ValueError(f"time_adaptive needs a fused system (PendulumSystem, EnsembleSystem): the hold runs inside the rollout "
                             f"kernel, and {type(self).__name__}.step is user code that steps once per call")
        self.time_adaptive = time_adaptive

    @property
    def action_dim(self) -> int:
        """What the policy (or a planner) emits and the model's transition rows carry.  u_dim — what the dynamics and the true buffer
        see — unless the actions hold more than controls: the optimistic EnsembleSystem's hallucinated controls (u_dim + x_dim), a
        time-adaptive system's hold time (u_dim + 1)."""
        return self.u_dim + (1 if self.time_adaptive is not None else 0)

    def env_action(self, a: torch.Tensor) -> torch.Tensor:
        """The controls of a policy action, for acting on the true system: a[..., :u_dim] (the whole action where action_dim == u_dim)."""
        return a[..., :self.u_dim]

    def hold_steps(self, a: torch.Tensor) -> torch.Tensor:
        """int32 [n]: the model steps the fused rollouts hold each of the actions a [n, action_dim] (or one, [action_dim]) for —
        mbpo_hold_steps, the kernels' own function — so that host code acts on the true system for exactly as long."""
        from mbpo import ops
        if self.time_adaptive is None:
            raise ValueError("hold_steps needs a time-adaptive system (time_adaptive=TimeAdaptive(...))")
        ta = self.time_adaptive
        ab = a.reshape(-1, self.action_dim).to(_device_of(a), torch.float32).contiguous()
        k = ops.hold_steps(ab, ta.min_time_between_switches, ta.max_time_between_switches, ta.env_dt, ta.max_steps)
        return k[0] if a.dim() == 1 else k

    @staticmethod
    def system_params_vmap_axes(axes: int = 0):
        return SystemParams(dynamics_params=None, reward_params=None, key=axes)

    def step(self, x: torch.Tensor, u: torch.Tensor, system_params: SystemParams) -> SystemState:
        """Systems that exist as device code (PendulumSystem, EnsembleSystem): one fused launch of the rollout kernel with
        open-loop actions and S=1 (csrc/rollout.hip).  On a time-adaptive system u is an action [u | tau] and the step is one
        decision: x_next after k(tau) model steps (fewer where the box was left), reward the hold's discounted sum less switch_cost.  A user-defined System overrides this with its own BATCHED torch code
        (x [N, x_dim], u [N, u_dim] on the device -> SystemState with x_next [N, x_dim], reward [N]); the trainers then step it
        between the HIP policy and bookkeeping kernels (ops.generic_rollout).
        With a termination set (PendulumSystem / EnsembleSystem(termination=)) SystemState.done is the box's verdict on the next state;
        where done is 1 the kernel's auto-reset has already run, so x_next is the state the env restarts from — here x itself — and a
        non-finite next state never leaves the kernel."""
        return self._fused_step(x, u, system_params, terminate=True)

    def _fused_step(self, x: torch.Tensor, u: torch.Tensor, system_params: SystemParams, terminate: bool) -> SystemState:
        """`step` of a fused system; terminate=False drops the termination (rollout_policy's scan ignores SystemState.done)."""
        from mbpo import ops
        from mbpo.systems.termination import without_termination
        from mbpo.systems.plan_reward import refuse_plan_reward
        refuse_plan_reward(system_params, f"{type(self).__name__}.step")      # (rollout_spec refuses it too; here before any device use)
        if not self.fused:
            raise NotImplementedError(f"{type(self).__name__} must define step(x, u, system_params) itself (batched torch code)")
        dev = _device_of(x)
        single = x.dim() == 1
        xb = x.reshape(-1, self.x_dim).to(dev, torch.float32).contiguous().clone()
        A = self.action_dim
        ub = u.reshape(-1, A).to(dev, torch.float32).contiguous()
        n = xb.shape[0]
        key, sub = K.split(system_params.key)
        spec = self.rollout_spec(system_params, dev)
        if not terminate:
            spec = without_termination(spec)
        rows = ops.model_rollout(x_dim=self.x_dim, u_dim=A, actions=ub.reshape(1, n, A), obs=xb,
                                 first_obs=xb.clone(), steps=torch.zeros(n, device=dev), done=torch.zeros(n, device=dev),
                                 n_steps=1, episode_length=2 ** 30, seed=sub, **spec)
        X, U = self.x_dim, A
        x_next, reward = rows[:, X + U + 2:2 * X + U + 2], rows[:, X + U]
        # the episode cannot run out here (episode_length 2**30): done = 1 - discount is the system's own
        done = 1.0 - rows[:, X + U + 1] if "term_low" in spec else 0.0      # (no termination: SystemState's default)
        if single:
            x_next, reward = x_next[0], reward[0]
            done = done[0] if "term_low" in spec else done
        # a stochastic System must split-and-return its key; the reference's Pendulum drops it (:38)
        return SystemState(x_next=x_next, reward=reward, system_params=system_params.replace(key=key), done=done)

    def init_params(self, key: int) -> SystemParams:
        keys = K.split(key, 3)
        return SystemParams(dynamics_params=self.dynamics.init_params(keys[0]),
                            reward_params=self.reward.init_params(keys[1]), key=keys[2])

    # MI355X seam: keyword arguments describing this system to ops.model_rollout.  PendulumSystem / EnsembleSystem return the
    # description of their device code (one fused launch per unroll); the default is the non-fused path for a user-defined
    # System: its own `step` between the HIP policy and episode-bookkeeping kernels.
    def rollout_spec(self, system_params: SystemParams, device) -> dict:
        from mbpo import _hip
        from mbpo.systems.plan_reward import refuse_plan_reward
        refuse_plan_reward(system_params, f"{type(self).__name__}.rollout_spec")
        return dict(system_kind=_hip.SYS_GENERIC, system=self, system_params=system_params)

    @property
    def fused(self) -> bool:
        """True when the system runs inside the fused rollout kernel (and a training step can be hipGraph-captured)."""
        return type(self).rollout_spec is not System.rollout_spec


def _device_of(t: torch.Tensor) -> torch.device:
    return t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())
