"""PolicyPrior — a learned policy's rollouts among iCEM's candidates (include/mbpo_hip.h "policy priors").  Not in the reference, whose iCEM
samples every candidate around (mean, std); build-defined, the actor half of the methods TerminalValue took the critic half from: TD-MPC
puts its policy's trajectories among the CEM samples of every iteration, LOOP starts the search from the actor's sequence.

Once per `optimize` the policy is rolled closed-loop through the model from x0, as n_candidates proposals of H steps:

    a_t = squash(loc(pi(n(x_t))) + noise_scale * scale * eps)

the rollout kernels' own NormalTanh path (ops.model_rollout with a policy and an explicit policy_noise); proposal 0 is the mode sequence
(include_mode).  In every iteration (every_iteration; else only the first) one launch of mbpo_icem_seed_candidates overwrites the sampled
slots [0, n_candidates) with the clipped proposals; a proposal with a non-finite action is dropped and its slot keeps the sample.  With
init_mean the search also starts from the mode sequence instead of the warm start.  `iCemTO(..., policy_prior=prior)` wires it in, single
and batched; with policy_prior=None every path issues exactly the launches it issued before.

Out of scope: proposals re-rolled per iteration, mixing the policy's and CEM's means, an entropy term, BPTT or SAC consuming a prior,
policies wider than 256.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from mbpo import _hip, ops
from mbpo.optimizers.trajectory_optimizers._net_checks import _check_dims, _check_flat, _learner_state_of, _n_params


class PolicyPrior:
    """PolicyPrior(x_dim, policy_params, policy_dims, activation="swish", norm_mean=None, norm_std=None, n_candidates=24, include_mode=True,
    noise_scale=1.0, action_clip=0.0, every_iteration=True, init_mean=False).

    policy_params: flat float32 [params(policy_dims)] (W[in][out] row-major, then b, per layer); policy_dims the KERNEL dims
    [x_dim, hidden..., 2 A], hidden layers sharing one width in 64 / 128 / 256; A is the action width iCEM plans in (on an optimistic system
    u_dim + x_dim).  norm_mean / norm_std [x_dim]: the trainer's normaliser, both or neither.

    All tensors are kept BY REFERENCE and read by the launch, not before: a policy refreshed in place is honoured without a new object.
    One exception: the rollout kernels run policy and ensemble members at one hidden width, so a policy NARROWER than the members of the
    EnsembleSystem it plans on is run through a zero-padded COPY (the same network), made when the system is first checked; after an
    in-place refresh of policy_params call `prior.refresh()` to re-make that copy.  A policy wider than the members is refused."""

    def __init__(self, x_dim: int, policy_params: torch.Tensor, policy_dims: Sequence[int], activation: str = "swish",
                 norm_mean: Optional[torch.Tensor] = None, norm_std: Optional[torch.Tensor] = None, n_candidates: int = 24,
                 include_mode: bool = True, noise_scale: float = 1.0, action_clip: float = 0.0, every_iteration: bool = True,
                 init_mean: bool = False):
        self.x_dim = int(x_dim)
        if self.x_dim < 1:
            raise ValueError(f"x_dim must be >= 1, got {x_dim}")
        if activation not in _hip.ACT_IDS:
            raise ValueError(f"activation must be one of {sorted(_hip.ACT_IDS)}, got {activation!r}")
        pd = [int(v) for v in policy_dims]
        if len(pd) < 2 or pd[-1] < 2 or pd[-1] % 2:
            raise ValueError(f"policy_dims must end in 2 * action_dim outputs, got {pd}")
        self.action_dim = pd[-1] // 2
        if self.action_dim > 64:
            raise ValueError(f"policy_dims: action_dim {self.action_dim} > 64 is not built")
        self.policy_dims = _check_dims("policy_dims", pd, self.x_dim, 2 * self.action_dim, "x_dim -> 2 * action_dim")
        self.policy_params = _check_flat("policy_params", policy_params, _n_params(self.policy_dims))
        if (norm_mean is None) != (norm_std is None):
            raise ValueError("norm_mean and norm_std must both be given or both be None")
        self.norm_mean = None if norm_mean is None else _check_flat("norm_mean", norm_mean, self.x_dim)
        self.norm_std = None if norm_std is None else _check_flat("norm_std", norm_std, self.x_dim)
        dev = self.policy_params.device
        for name, t in (("norm_mean", self.norm_mean), ("norm_std", self.norm_std)):
            if t is not None and t.device != dev:
                raise ValueError(f"{name} lies on {t.device}, policy_params on {dev}")
        self.n_candidates = int(n_candidates)
        if self.n_candidates < 1:
            raise ValueError(f"n_candidates must be >= 1, got {n_candidates}")
        self.include_mode, self.every_iteration, self.init_mean = bool(include_mode), bool(every_iteration), bool(init_mean)
        if self.init_mean and not self.include_mode:
            raise ValueError("init_mean=True starts the search from proposal 0, which is the mode sequence only with include_mode=True")
        self.noise_scale = float(noise_scale)
        if not self.noise_scale >= 0.0:
            raise ValueError(f"noise_scale must be >= 0, got {noise_scale}")
        self.action_clip = float(action_clip)
        if not 0.0 <= self.action_clip <= 1.0:
            raise ValueError(f"action_clip must be in [0, 1] (0: none), got {action_clip}")
        self.activation = activation
        self._embedded, self._embedded_width = None, None      # the zero-padded copy for a wider ensemble, and its width

    # -- from a trainer's state ----------------------------------------------------------------------------------------
    @classmethod
    def _from_learner(cls, trainer: str, learner_state, policy_dims, activation, kw) -> "PolicyPrior":
        who = f"from_{trainer.lower()}"
        ls = _learner_state_of(learner_state, who, trainer)
        sig = getattr(ls, "signature", None) or {}
        if sig.get("trainer", trainer) != trainer:
            raise ValueError(f"{who} needs {trainer}'s learner state, this one is {sig.get('trainer')!r}'s")
        policy_dims = [int(v) for v in (policy_dims if policy_dims is not None else sig.get("policy_dims") or ())]
        if len(policy_dims) < 2:
            raise ValueError("policy_dims is needed (the learner state carries no signature to read it from)")
        X, P = policy_dims[0], _n_params(policy_dims)
        params = _check_flat("learner_state.params", ls.params, P, exact=False)
        mean = std = None
        if sig.get("normalize_observations", True):
            vec = _check_flat("learner_state.normalizer", ls.normalizer, 1 + 3 * X)
            mean, std = vec[1:1 + X], vec[1 + 2 * X:1 + 3 * X]
        return cls(X, params[:P], policy_dims, activation=activation, norm_mean=mean, norm_std=std, **kw)

    @classmethod
    def from_sac(cls, learner_state, policy_dims: Optional[Sequence[int]] = None, activation: str = "swish", **kw) -> "PolicyPrior":
        """From SAC's LearnerState (or the BraxState / SACOptimizer / SAC trainer that carries one, as TerminalValue.from_sac): the policy
        slice of `params` [policy | twin critics | log_alpha], mean / std from the normaliser vector [count | mean | summed variance |
        std] when the learner normalises observations.  policy_dims: the KERNEL dims, read off the state's signature when None.  The
        tensors are views of the state's.  **kw: n_candidates, include_mode, noise_scale, action_clip, every_iteration, init_mean."""
        return cls._from_learner("SAC", learner_state, policy_dims, activation, kw)

    @classmethod
    def from_ppo(cls, learner_state, policy_dims: Optional[Sequence[int]] = None, activation: str = "swish", **kw) -> "PolicyPrior":
        """From PPO's LearnerState (signature "PPO"): the policy slice of `params` [policy | value] and the normaliser, as from_sac."""
        return cls._from_learner("PPO", learner_state, policy_dims, activation, kw)

    @classmethod
    def from_bptt(cls, opt_state, actor_dims: Sequence[int], action_clip: float = 0.999, activation: str = "swish", **kw) -> "PolicyPrior":
        """From a BPTTState: the actor (2 A outputs; squash_action is the rollout kernels' tanh with action_clip 0.999, as BPTT's own
        evaluation rollouts run it) and the state normaliser (BPTT always normalises).  actor_dims: the KERNEL dims,
        `BPTTOptimizer.actor_dims`."""
        actor_dims = [int(v) for v in actor_dims]
        ns = opt_state.state_normalizer_state
        return cls(actor_dims[0], opt_state.actor_params, actor_dims, activation=activation, norm_mean=ns.mean, norm_std=ns.std,
                   action_clip=action_clip, **kw)

    # -- use -----------------------------------------------------------------------------------------------------------
    @property
    def width(self) -> Optional[int]:
        return self.policy_dims[1] if len(self.policy_dims) > 2 else None

    def check_system(self, system) -> None:
        """The widths against a system's: x_dim, the action width against system.action_dim (on an optimistic system u + x), and the
        hidden width against an EnsembleSystem's members — equal: the tensor as is; narrower: the zero-padded copy is made here (once per
        width; `refresh()` re-makes it); wider: refused."""
        if system is None:
            return
        if self.x_dim != system.x_dim:
            raise ValueError(f"policy_prior is built at x_dim {self.x_dim}, the system has x_dim {system.x_dim}")
        if self.action_dim != system.action_dim:
            raise ValueError(f"policy_prior acts at action_dim {self.action_dim}, the system has action_dim {system.action_dim} "
                             f"(u_dim {system.u_dim}; an optimistic system acts in u_dim + x_dim)")
        target = self._member_width(system)
        if target is None or self.width is None or target == self.width:
            self._embedded, self._embedded_width = None, None
            return
        if target < self.width:
            raise ValueError(f"policy_prior's hidden width {self.width} exceeds the width {target} of the system's ensemble members: the "
                             f"rollout kernels run both at one width and a network cannot be narrowed")
        if self._embedded_width != target:
            self._embedded_width = target
            self.refresh()

    @staticmethod
    def _member_width(system) -> Optional[int]:
        """The hidden width the rollout kernels run this system's learned members at; None: no such constraint (the analytic Pendulum, a
        user-defined System)."""
        dyn = getattr(system, "dynamics", None)
        if not getattr(system, "fused", False) or dyn is None or not hasattr(dyn, "kernel_width"):
            return None
        if dyn.kernel_width is None:
            raise ValueError("policy_prior: this ensemble's members are wider than 256 and do not run in the rollout kernels")
        return int(dyn.kernel_width) if len(dyn.dims) > 2 else None

    def refresh(self) -> None:
        """Re-make the zero-padded copy a narrower policy is run through (see the class docstring); nothing to do otherwise."""
        if self._embedded_width is not None:
            self._embedded = ops.embed_mlp_params(self.policy_params, self.policy_dims, self._embedded_width)

    def check_optimizer(self, num_samples: int) -> None:
        if self.n_candidates > int(num_samples):
            raise ValueError(f"policy_prior seeds n_candidates = {self.n_candidates} sampled slots, iCEM samples only num_samples = "
                             f"{num_samples}")

    def rollout_kwargs(self) -> dict:
        """The policy half of an ops.model_rollout call: the (possibly zero-padded) parameters, their spec, normaliser and clip."""
        if self._embedded is not None:
            params, dims = self._embedded, ops.padded_dims(self.policy_dims, self._embedded_width)
        else:
            params, dims = self.policy_params, self.policy_dims
        return dict(policy_params=params, policy_spec=ops.MlpSpec(dims, self.activation, 1), norm_mean=self.norm_mean,
                    norm_std=self.norm_std, action_clip=self.action_clip)

    @staticmethod
    def proposal_spec(spec: dict) -> dict:
        """The system's rollout descriptor as the proposal rollout runs under it: a stochastic fused ensemble in ENS_MEAN without model
        noise (proposals are action sequences: their only randomness is the policy's).  The optimistic mode already is ENS_MEAN plus
        halluc_beta; a user-defined System is stepped as it is."""
        if spec.get("system_kind") != _hip.SYS_ENSEMBLE:
            return spec
        if spec.get("ens_mode", _hip.ENS_MEAN) == _hip.ENS_MEAN and not spec.get("ens_sample_noise"):
            return spec
        return dict(spec, ens_mode=_hip.ENS_MEAN, ens_sample_noise=False)

    def __repr__(self):
        return (f"PolicyPrior(x_dim {self.x_dim}, action_dim {self.action_dim}, policy {self.policy_dims}, n_candidates {self.n_candidates}, "
                f"include_mode {self.include_mode}, noise_scale {self.noise_scale}, every_iteration {self.every_iteration}, "
                f"init_mean {self.init_mean})")
