"""PendulumSystem — mirrors mbpo/systems/pendulum_system.py:12-46."""
from __future__ import annotations

import dataclasses
from typing import Optional

import torch

from mbpo import _hip
from mbpo.systems.base_systems import System, SystemParams, SystemState, _device_of
from mbpo.systems.plan_reward import refuse_plan_reward
from mbpo.systems.dynamics.pendulum_dynamics import PendulumDynamics, PendulumDynamicsParams
from mbpo.systems.rewards.pendulum_reward import PendulumReward, PendulumRewardParams
from mbpo.systems.termination import BoxTermination, termination_spec


class PendulumSystem(System[PendulumDynamicsParams, PendulumRewardParams]):
    def __init__(self, termination: Optional[BoxTermination] = None, time_adaptive=None):
        """termination (not in the reference): a BoxTermination on the next state [cos, sin, thetadot]; see EnsembleSystem.
        time_adaptive (not in the reference): a TimeAdaptive — actions are [u | tau]; see EnsembleSystem."""
        super().__init__(dynamics=PendulumDynamics(), reward=PendulumReward(), time_adaptive=time_adaptive)
        if termination is not None and termination.x_dim != self.x_dim:
            raise ValueError(f"the termination has {termination.x_dim} dimensions, the system {self.x_dim}")
        self.termination = termination
        self.min_action = -1.0
        self.max_action = 1.0

    def rollout_spec(self, system_params: SystemParams, device) -> dict:
        refuse_plan_reward(system_params, "PendulumSystem.rollout_spec")      # (only iCEM consumes one, and takes it out first)
        dp = system_params.dynamics_params or PendulumDynamicsParams()
        rp = system_params.reward_params or PendulumRewardParams()
        ck = (dataclasses.astuple(dp), dataclasses.astuple(rp), str(device), None if self.termination is None else self.termination.key,
              self.time_adaptive)
        if getattr(self, "_spec_key", None) != ck:     # device vectors are cached: no H2D copy inside a captured graph
            kind, rvec = self.reward.kernel_spec(rp, device)
            self._spec = dict(system_kind=_hip.SYS_PENDULUM, sys_params=dp.vector(device), reward_kind=kind, reward_params=rvec,
                              **({} if self.time_adaptive is None else self.time_adaptive.kernel_spec()),
                              **termination_spec(self.termination, self.x_dim, device))
            self._spec_key = ck
        return dict(self._spec)

    def reset(self, rng=None, device=None) -> SystemState:
        """pendulum_system.py:41-46: hanging-down start [-1, 0, 0], reward 0."""
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        return SystemState(x_next=torch.tensor([-1.0, 0.0, 0.0], device=dev), reward=torch.zeros((), device=dev),
                           system_params=SystemParams(dynamics_params=PendulumDynamicsParams(),
                                                      reward_params=PendulumRewardParams()))


def _pendulum_step(x, u, dyn_params, rew_params):
    sys = PendulumSystem()
    st = sys.step(x, u, SystemParams(dynamics_params=dyn_params, reward_params=rew_params or PendulumRewardParams()))
    return st.x_next, st.reward
