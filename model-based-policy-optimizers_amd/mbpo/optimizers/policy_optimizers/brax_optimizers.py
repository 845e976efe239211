"""BraxOptimizer / SACOptimizer / PPOOptimizer — mirrors mbpo/optimizers/policy_optimizers/brax_optimizers.py:21-115
(same constructor signatures, `init` / `act` / `train` semantics and key-split structure).

Not in the reference (its SAC and PPO optimizers start every `train` from a fresh initialisation; its BPTT optimizer carries its
state): warm_start=True carries the learner from one `train` to the next in BraxState.learner_state and keeps the trainer, with
its captured training step, between the calls (DESIGN "warm start")."""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass
from typing import Any, List, Optional, Tuple

import torch

from mbpo.optimizers.base_optimizer import BaseOptimizer
from mbpo.replay import ReplayBufferState, UniformSamplingQueue
from mbpo.systems.base_systems import System
from mbpo.systems.brax_wrapper import BraxWrapper
from mbpo.utils import keys as K
from mbpo.utils.type_aliases import OptimizerState, OptimizerTrainingOutPut


@dataclass
class BraxState(OptimizerState):
    policy_params: Any = None          # (normalizer_params, policy_params)  (brax_optimizers.py:69-72)
    learner_state: Any = None          # brax_utils.base.LearnerState with warm_start=True, else None (not in the reference)


@dataclass
class BraxOutput(OptimizerTrainingOutPut):
    optimizer_state: BraxState
    summary: List[dict] = dataclasses.field(default_factory=list)


class BraxOptimizer(BaseOptimizer):
    def __init__(self, agent_class, true_buffer: UniformSamplingQueue, system: Optional[System] = None, warm_start: bool = False,
                 retain_replay_buffer: bool = False, **agent_kwargs):
        """warm_start: `train` resumes the learner of opt_state.learner_state (None: the first call, a fresh initialisation) and
        returns the new one in optimizer_state.learner_state; the trainer is kept between calls until close().
        retain_replay_buffer (SAC, needs warm_start): the learner state also carries the model replay buffer, by reference."""
        if retain_replay_buffer and not warm_start:
            raise ValueError("retain_replay_buffer=True needs warm_start=True: the buffer travels in the learner state")
        super().__init__(system)
        self.agent_class = agent_class
        self.agent_kwargs = agent_kwargs
        self.warm_start = bool(warm_start)
        self.retain_replay_buffer = bool(retain_replay_buffer)
        self._trainer = None               # warm_start: the trainer kept between train() calls
        self.true_buffer = true_buffer
        if system is None:
            self.dummy_trainer = None
            self.make_policy = None
        else:
            self.set_system(system)

    def set_system(self, system: System):
        self.close()                       # a kept trainer was built on the previous system
        super().set_system(system)
        self.key, sys_key, buffer_key = K.split(self.key, 3)
        dummy_true_buffer_state = self.dummy_true_buffer_state(buffer_key)
        dummy_env = BraxWrapper(system=self.system, system_params=self.system.init_params(sys_key),
                                sample_buffer_state=dummy_true_buffer_state, sample_buffer=self.true_buffer)
        self.dummy_trainer = self.agent_class(environment=dummy_env, **self.agent_kwargs)
        self.make_policy = self.dummy_trainer.make_policy

    def init(self, key: int, true_buffer_state: Optional[ReplayBufferState] = None) -> BraxState:
        assert self.system is not None, "Brax optimizer requires system to be defined."
        if true_buffer_state is None:
            dummy_buffer_key, key = K.split(key, 2)
            true_buffer_state = self.dummy_true_buffer_state(dummy_buffer_key)
        keys = K.split(key, 3)
        system_params = self.system.init_params(keys[0])
        training_state = self.dummy_trainer.init_training_state(keys[1])
        norm, pol = training_state.get_policy_params()
        policy_params = (dataclasses.replace(norm, vec=norm.vec.clone()), pol.clone())
        return BraxState(system_params=system_params, true_buffer_state=true_buffer_state, policy_params=policy_params,
                         key=keys[2])

    def act(self, obs: torch.Tensor, opt_state: BraxState, evaluate: bool = True) -> Tuple[torch.Tensor, BraxState]:
        assert self.system is not None, "Brax optimizer requires system to be defined."
        policy = self.make_policy(opt_state.policy_params, evaluate)
        key, subkey = K.split(opt_state.key)
        action = policy(obs, subkey)[0]
        return action, opt_state.replace(key=key)

    def train(self, opt_state: BraxState) -> BraxOutput:
        """brax_optimizers.py:86-99: a NEW trainer per call (policy/critics re-initialised inside run_training)."""
        assert self.system is not None, "Brax optimizer requires system to be defined."
        env = BraxWrapper(system=self.system, system_params=opt_state.system_params,
                          sample_buffer_state=opt_state.true_buffer_state, sample_buffer=self.true_buffer)
        if self.warm_start:
            return self._train_warm(opt_state, env)
        trainer = self.agent_class(environment=env, **self.agent_kwargs)
        key, new_key = K.split(opt_state.key)
        try:
            policy_params, metrics = trainer.run_training(key=new_key)
        finally:
            trainer.close()      # the captured graph and the peer-memory regions belong to this trainer (one per train())
        new_opt_state = opt_state.replace(policy_params=policy_params, key=new_key)
        return BraxOutput(optimizer_state=new_opt_state, summary=metrics)

    def _keeps_trainer(self) -> bool:
        """The trainer is kept for the built-in (fused) Systems on a single rank.  A user-defined System (its own code runs between
        the kernels and may hold state of the environment it was built with) and a process group (the peer-memory regions are
        negotiated per trainer by all ranks together) get a new trainer per call; the learner state is carried all the same."""
        return bool(self.system.fused) and self.agent_kwargs.get("process_group") is None

    def _train_warm(self, opt_state: BraxState, env: BraxWrapper) -> BraxOutput:
        """`train` with warm_start: the same key split; the learner ALWAYS comes from opt_state (a copy of a few hundred KB), so the
        result never depends on which trainer is alive.  A kept trainer is rebound to the new environment; whether its captured
        step replays or is captured again is decided by the trainer's own address check, nothing here forces either."""
        trainer, self._trainer = self._trainer, None
        if trainer is not None:
            trainer.rebind(env)
        else:
            trainer = self.agent_class(environment=env, **self.agent_kwargs)
        key, new_key = K.split(opt_state.key)
        try:
            policy_params, metrics = trainer.run_training(key=new_key, learner_state=opt_state.learner_state)
        except BaseException:
            trainer.close()
            raise
        learner_state = trainer.last_learner_state
        if not self.retain_replay_buffer:
            learner_state = learner_state.replace(replay=None)
        if self._keeps_trainer():
            self._trainer = trainer
        else:
            trainer.close()
        new_opt_state = opt_state.replace(policy_params=policy_params, key=new_key, learner_state=learner_state)
        return BraxOutput(optimizer_state=new_opt_state, summary=metrics)

    def close(self) -> None:
        """Release the kept trainer (its captured graph, and the buffers the graph keeps alive)."""
        trainer, self._trainer = self._trainer, None
        if trainer is not None:
            trainer.close()


class SACOptimizer(BraxOptimizer):
    def __init__(self, true_buffer: UniformSamplingQueue, system: Optional[System] = None, warm_start: bool = False,
                 retain_replay_buffer: bool = False, **sac_kwargs):
        from mbpo.optimizers.policy_optimizers.sac.sac import SAC
        super().__init__(agent_class=SAC, system=system, true_buffer=true_buffer, warm_start=warm_start,
                         retain_replay_buffer=retain_replay_buffer, **sac_kwargs)


class PPOOptimizer(BraxOptimizer):
    def __init__(self, true_buffer: UniformSamplingQueue, system: Optional[System] = None, warm_start: bool = False, **ppo_kwargs):
        from mbpo.optimizers.policy_optimizers.ppo.ppo import PPO
        if ppo_kwargs.get("retain_replay_buffer"):
            raise ValueError("retain_replay_buffer: PPO keeps no replay buffer")
        super().__init__(agent_class=PPO, system=system, true_buffer=true_buffer, warm_start=warm_start, **ppo_kwargs)
