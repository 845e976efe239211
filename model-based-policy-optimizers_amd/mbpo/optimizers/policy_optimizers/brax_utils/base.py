"""State — mirrors mbpo/optimizers/policy_optimizers/brax_utils/base.py:12-23 (brax env State carrying system_params).
All leaves are batched over envs ([N, ...]) — the reference gets the batch axis from VmapWrapper (training.py:50-74)."""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field
from typing import Any, Dict, Optional

import torch


@dataclass
class State:
    pipeline_state: Optional[Any]
    obs: torch.Tensor          # [N, x_dim]
    reward: torch.Tensor       # [N]
    done: torch.Tensor         # [N] float flags
    system_params: Any
    metrics: Dict[str, Any] = field(default_factory=dict)
    info: Dict[str, Any] = field(default_factory=dict)   # 'steps' [N], 'truncation' [N], 'first_obs' [N, x_dim]

    def replace(self, **kw):
        return dataclasses.replace(self, **kw)


@dataclass
class LearnerState:
    """Everything a SAC / PPO learner carries from one run_training to the next (not in the reference, whose SAC and PPO start every
    `train` from init_training_state; its BPTT optimizer carries actor, critic and optimizer state the same way).  A VALUE: the
    tensors are clones, never views of a trainer's live flat buffers — except `replay`.

      params      SAC [P + 2Q + 1] (policy | twin critics | log_alpha); PPO [P + V] (policy | value)
      target_q    SAC [2Q]; PPO None
      adam_m / v  the moments, as params
      step_count  [1] float: the Adam step count (the bias corrections depend on it)
      normalizer  [1 + 3 x_dim]: count, mean, summed variance, std
      signature   which trainer, x_dim, action_dim, the logical and kernel dims of every network, normalize_observations
      replay      SAC only, optional: the model replay buffer's ReplayBufferState.  `data` and the device state words are held BY
                  REFERENCE (a buffer of 2^20 rows is not copied per call): whoever passes a state on gives its buffer to the next
                  call, which inserts into it in place — a state with a buffer resumes ONE run, not two.
    """
    signature: Dict[str, Any]
    params: torch.Tensor
    adam_m: torch.Tensor
    adam_v: torch.Tensor
    step_count: torch.Tensor
    normalizer: torch.Tensor
    target_q: Optional[torch.Tensor] = None
    replay: Optional[Any] = None

    def replace(self, **kw):
        return dataclasses.replace(self, **kw)

    def mismatch(self, signature: Dict[str, Any]) -> Optional[str]:
        """Name of the first signature field in which this state differs from `signature` (a trainer's), None when they agree."""
        for name in list(signature) + [k for k in self.signature if k not in signature]:
            if name not in self.signature or name not in signature or _plain(self.signature[name]) != _plain(signature[name]):
                return name
        return None

    def check(self, signature: Dict[str, Any]) -> None:
        """ValueError naming the differing field — raised before anything is copied."""
        name = self.mismatch(signature)
        if name is not None:
            raise ValueError(f"learner state does not fit this trainer: {name} is {self.signature.get(name)!r} in the state, "
                             f"{signature.get(name)!r} in the trainer")
        for name, t in (("adam_m", self.adam_m), ("adam_v", self.adam_v)):
            if t.shape != self.params.shape:
                raise ValueError(f"learner state is inconsistent: {name} has shape {tuple(t.shape)}, params {tuple(self.params.shape)}")


def _plain(v):
    return [_plain(e) for e in v] if isinstance(v, (list, tuple)) else v


def rehome_state(home: Optional[State], fresh: State) -> State:
    """A trainer that is kept between run_training calls holds a captured graph whose launches read and write the env State tensors
    of the call before.  The values of a fresh reset are copied INTO those tensors (same shapes), so the next call runs on the
    addresses the graph was captured against; everything that is not a device tensor (system_params, metrics) is the fresh State's.
    Without a home, or with one of another shape, the fresh State is used as it is."""
    if home is None:
        return fresh
    pairs = [(home.obs, fresh.obs), (home.reward, fresh.reward), (home.done, fresh.done)]
    if set(home.info) != set(fresh.info):
        return fresh
    pairs += [(home.info[k], fresh.info[k]) for k in fresh.info]
    if any(h.shape != f.shape or h.dtype != f.dtype or h.device != f.device for h, f in pairs):
        return fresh
    for h, f in pairs:
        h.copy_(f)
    return fresh.replace(obs=home.obs, reward=home.reward, done=home.done, info={k: home.info[k] for k in fresh.info})
