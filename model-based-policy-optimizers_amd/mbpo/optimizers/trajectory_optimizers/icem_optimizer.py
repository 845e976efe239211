"""iCEM trajectory optimizer — mirrors mbpo/optimizers/trajectory_optimizers/icem_optimizer.py:25-330 on the MI355X kernels.

One `optimize` = num_steps iterations of
    mbpo_icem_sample   coloured-noise candidates around (mean, std), previous elites appended                (:168-190)
    mbpo_model_rollout open-loop rollouts of every candidate x particle through System.step               (rollout_actions)
    mbpo_icem_update   objective, elites, soft mean/std update, best-so-far, elites carried over              (:193-232)
with all optimizer state in flat device vectors; the host only sequences launches.  Keys are integers (mbpo.utils.keys);
device noise is Philox(seed = split key, offset = iteration).  A user `cost_fn` (icem_optimizer.py:99,161-166: a callable over one
trajectory, `cost_fn(observation [H, x], action [H, u]) -> scalar`) cannot run inside the kernels: it is evaluated between the
rollout launch and the update launch, vmapped over all (candidate, particle) trajectories with torch.func.vmap on the device rows
(the reference vmaps it too).  A cost written as data, `cost_fn=TermCost(...)` (mbpo.systems), needs no Python there: one launch of
mbpo_traj_cost_eval evaluates its term table on the rollout's rows — (x_t, u_t, x_{t+1}) of every step, summed or maximised over the
horizon — into a preallocated buffer, and the iteration stays a pure launch chain, single and batched.  Either way the cost enters the
objective inside mbpo_icem_update_constrained: reward - lambda_constraint * relu(cost), cost summarised over particles by mean
(use_pessimism: max).  use_optimism -> max over particles of the reward.

Plan rewards: `opt_state.system_params.reward_params` may be a `PlanRewardParams(reward, table [PB, PH, param_len])` (mbpo.systems) —
reward parameters per problem (PB = B) and per planned step (PH = horizon), an axis of size 1 broadcast.  The rollout then runs under
one ordinary parameter object (its reward column is computed and not used), one launch of mbpo_plan_reward_eval writes the rewards
under the table into a dense buffer, and the unchanged update launch reads that buffer as (rows = buffer, row_len = 1, reward_col = 0).  The table is read by that launch: refilled in place between two `act`
calls it is honoured without a new object.  Without a PlanRewardParams every path issues exactly the launches it issued before.

Terminal value: `iCemTO(..., terminal_value=TerminalValue(...))` (mbpo.optimizers) adds weight * V(x_H) — a learned critic at the state the
horizon ends in: SAC's twin Q under its policy's mode action, BPTT's twin target critic, PPO's value network — to every trajectory's
objective.  One launch of mbpo_terminal_value_eval, after the reward source and before the update, adds it into the last step's rewards
the update launch reads (the rows' own reward column, or the plan reward's dense buffer); the update kernels are unchanged, and a
trajectory whose terminal state is not finite gets -inf there.  It composes with a TermCost, a callable cost_fn, use_optimism /
use_pessimism, the TS modes and warm starts, none of which reads the reward column.  With terminal_value=None every path issues exactly
the launches it issued before.

Policy prior: `iCemTO(..., policy_prior=PolicyPrior(...))` (mbpo.optimizers; include/mbpo_hip.h "policy priors") puts a learned policy's
closed-loop rollouts among the candidates.  Once per `optimize`, before the first iteration, the policy is rolled through the model from
the initial state — K proposals per problem, one mbpo_philox_fill_grouped for their noise under split(optimizer_key, 3)[2] and one
mbpo_model_rollout with the policy — and in every iteration (every_iteration; else the first only) one launch of
mbpo_icem_seed_candidates, between the sample launch and the candidate rollout, overwrites the sampled slots [0, K) with the clipped
proposals, reading the action columns of the proposal rollout's rows in place.  A proposal with a non-finite action is dropped: its slot
keeps the sample.  init_mean also writes the mode proposal into the mean the first sample launch reads.  The existing key chain is
untouched (split(k, 3)[:2] == split(k, 2)); with policy_prior=None every path issues exactly the launches it issued before.

Batched MPC: `init(key, batch_size=B)` makes a state for B independent problems (best_sequence [B, H, U], best_reward [B], key = B
host integers) and `optimize` / `act` on such a state plan for obs [B, x] in one launch chain per iteration —
mbpo_icem_sample_batched -> one rollout over all B*NC*P envs -> mbpo_icem_update_batched (one workgroup per problem).  Problem b
is bit for bit the single-problem `optimize` with key[b], best_sequence[b] and obs[b]: its noise is drawn under its own split
keys, and a stochastic EnsembleSystem's members and model noise are drawn per problem up front (mbpo_philox_fill_grouped) instead
of from the global env index in the rollout kernel.  A user-defined (non-fused) System has its `step` called once per horizon step
over all B*NC*P rows; bit-equality with the single calls then needs that step to be row-independent and deterministic.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from dataclasses import dataclass
from typing import Any, Generic, List, Mapping, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from mbpo import _hip, ops
from mbpo.optimizers.base_optimizer import BaseOptimizer
from mbpo.optimizers.trajectory_optimizers.policy_prior import PolicyPrior
from mbpo.optimizers.trajectory_optimizers.terminal_value import TerminalValue
from mbpo.replay import ReplayBufferState
from mbpo.systems.base_systems import System
from mbpo.systems.dynamics.base_dynamics import DynamicsParams
from mbpo.systems.plan_reward import PlanRewardParams
from mbpo.systems.rewards.base_rewards import RewardParams
from mbpo.systems.term_cost import TermCost
from mbpo.systems.termination import without_termination
from mbpo.systems.time_adaptive import refuse_time_adaptive
from mbpo.utils import keys as K
from mbpo.utils.type_aliases import OptimizerState, OptimizerTrainingOutPut


class iCemParams(NamedTuple):
    """icem_optimizer.py:25-50 (same fields and defaults)."""
    num_particles: int = 10
    num_samples: int = 500
    num_elites: int = 50
    init_std: float = 0.5
    alpha: float = 0.0
    num_steps: int = 5
    exponent: float = 0.0
    elite_set_fraction: float = 0.3
    u_min: Union[float, Sequence[float]] = -1.0
    u_max: Union[float, Sequence[float]] = 1.0
    warm_start: bool = True
    lambda_constraint: float = 1e4


@dataclass
class iCemOptimizerState(OptimizerState, Generic[DynamicsParams, RewardParams]):
    best_sequence: torch.Tensor = None     # [horizon, action_dim]; batched: [B, horizon, action_dim]
    best_reward: torch.Tensor = None       # scalar; batched: [B]

    @property
    def batched(self) -> bool:
        return self.best_sequence is not None and self.best_sequence.dim() == 3

    @property
    def action(self):
        return self.best_sequence[..., 0, :]      # [action_dim]; batched: [B, action_dim]


@dataclass
class iCemTrainingOutput(OptimizerTrainingOutPut, Generic[DynamicsParams, RewardParams]):
    optimizer_state: iCemOptimizerState = None
    summary: List[Mapping[str, Any]] = None


class iCemTO(BaseOptimizer, Generic[DynamicsParams, RewardParams]):
    def __init__(self, horizon: int, action_dim: int, key: int = K.PRNGKey(0), opt_params: iCemParams = iCemParams(), cost_fn=None,
                 use_optimism: bool = False, use_pessimism: bool = False, *args, terminal_value: Optional[TerminalValue] = None,
                 policy_prior: Optional[PolicyPrior] = None, **kwargs):
        super().__init__(*args, **kwargs)
        refuse_time_adaptive(self.system, "iCEM")
        if policy_prior is not None and not isinstance(policy_prior, PolicyPrior):
            raise ValueError(f"policy_prior must be a PolicyPrior (mbpo.optimizers) or None, got {type(policy_prior).__name__}")
        self.policy_prior = policy_prior          # a learned policy's rollouts among the candidates (see the module docstring)
        if policy_prior is not None:
            policy_prior.check_optimizer(opt_params.num_samples)
        self._check_policy_prior(self.system)
        if terminal_value is not None and not isinstance(terminal_value, TerminalValue):
            raise ValueError(f"terminal_value must be a TerminalValue (mbpo.optimizers) or None, got {type(terminal_value).__name__}")
        self.terminal_value = terminal_value      # a learned critic at x_H, added on the device (see the module docstring)
        self._check_terminal_value(self.system)
        self.cost_fn = cost_fn       # evaluated on the host side of the seam, between two launches (see the module docstring)
        self._term_cost = cost_fn if isinstance(cost_fn, TermCost) else None      # ... or on the device, by mbpo_traj_cost_eval
        self._check_term_cost(self.system)
        self.lib = _hip.load()
        self.horizon, self.action_dim = int(horizon), int(action_dim)
        self.opt_params, self.key = opt_params, key
        self.opt_dim = (self.horizon, self.action_dim)
        self.use_optimism, self.use_pessimism = use_optimism, use_pessimism
        p = opt_params
        self.num_prev = max(int(p.elite_set_fraction * p.num_elites), 1)
        if not (0 < p.num_elites <= p.num_samples + self.num_prev):
            raise ValueError("num_elites must be in (0, num_samples + carried elites]")
        self._bufs = None
        self._bbufs = None

    def set_system(self, system):
        refuse_time_adaptive(system, "iCEM")      # (single and batched: the candidates' objective sums per-step rewards)
        self._check_term_cost(system)
        self._check_terminal_value(system)
        self._check_policy_prior(system)
        super().set_system(system)

    def _check_policy_prior(self, system):
        """A PolicyPrior's widths against the system's: x_dim, its action width against system.action_dim, its hidden width against an
        ensemble's members (a narrower policy gets its zero-padded copy here)."""
        if self.policy_prior is not None:
            self.policy_prior.check_system(system)

    def _proposal_buffers(self, d: dict, B: int, dev) -> None:
        """The proposal rollout's buffers for B problems, allocated with the others: B * K envs of H steps."""
        pp = self.policy_prior
        if pp is None:
            return
        H, U, X, n = self.horizon, self.action_dim, self.system.x_dim, B * pp.n_candidates
        f = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)
        d.update(pp_obs=f(n, X), pp_first=f(n, X), pp_steps=f(n), pp_done=f(n), pp_rows=f(H * n, 2 * X + U + 3), pp_noise=f(H, n, U),
                 pp_seeds=torch.zeros(B, device=dev, dtype=torch.int64))

    def _propose(self, b: dict, B: int, x0: torch.Tensor, prior_keys, spec: dict) -> None:
        """Once per `optimize`: K closed-loop rollouts of the policy per problem from x0 [B, x] into b["pp_rows"] (step-major, B * K envs),
        their noise drawn per problem under prior_keys (B integers) — include/mbpo_hip.h "policy priors"."""
        pp = self.policy_prior
        H, U, X, Kp = self.horizon, self.action_dim, self.system.x_dim, pp.n_candidates
        if "pp_rows" not in b or b["pp_rows"].shape[0] != H * B * Kp:      # (a prior assigned, or resized, after the buffers were made)
            pp.check_optimizer(self.opt_params.num_samples)
            self._proposal_buffers(b, B, b["dev"])
        b["pp_seeds"].copy_(torch.from_numpy(np.asarray([int(k) & K.MASK for k in prior_keys], dtype=np.uint64).view(np.int64)))
        _hip.check(self.lib.mbpo_philox_fill_grouped(b["pp_seeds"].data_ptr(), 0, _hip.STREAM_POLICY_NOISE, H, B, Kp * U, 0, 0, 0,
                                                     b["pp_noise"].data_ptr(), _hip.current_stream_ptr()), "mbpo_philox_fill_grouped")
        if pp.include_mode:
            b["pp_noise"].view(H, B, Kp, U)[:, :, 0].zero_()      # proposal 0: the policy's mode sequence
        if pp.noise_scale != 1.0:
            b["pp_noise"].mul_(pp.noise_scale)
        b["pp_obs"].view(B, Kp, X).copy_(x0.reshape(B, 1, X).expand(B, Kp, X))
        b["pp_first"].copy_(b["pp_obs"])
        b["pp_steps"].zero_(); b["pp_done"].zero_()
        ops.model_rollout(x_dim=X, u_dim=U, obs=b["pp_obs"], first_obs=b["pp_first"], steps=b["pp_steps"], done=b["pp_done"], n_steps=H,
                          episode_length=2 ** 30, seed=0, offset=0, out=b["pp_rows"], policy_noise=b["pp_noise"], **pp.rollout_kwargs(),
                          **PolicyPrior.proposal_spec(spec))

    def _seed(self, b: dict, B: int, candidates: bool, mean: bool) -> None:
        """One launch of mbpo_icem_seed_candidates on the action columns of the proposal rows: into the sampled slots [0, K) of every
        problem (candidates and their particle-replicated actions) and / or proposal 0 into the mean."""
        pp, X = self.policy_prior, self.system.x_dim
        row_len = b["pp_rows"].shape[1]
        ops.icem_seed_candidates(b["pp_rows"], X, B * pp.n_candidates * row_len, row_len, B, pp.n_candidates, b["NC"], self.horizon,
                                 self.action_dim, self.opt_params.num_particles, b["u_min"], b["u_max"],
                                 actions=b["actions"] if candidates else None, candidates=b["cand"] if candidates else None,
                                 mean=b["mean"] if mean else None)

    def _check_terminal_value(self, system):
        """A TerminalValue's widths against the system's: x_dim, and kind Q's action width against system.action_dim."""
        if self.terminal_value is not None:
            self.terminal_value.check_system(system)

    def _add_terminal_value(self, b: dict, prp: Optional[PlanRewardParams], rew_len: int, rew_col: int, n: int) -> None:
        """One launch of mbpo_terminal_value_eval (accumulate): weight * V(x_H) of every trajectory — x_H the next-state columns of its
        last-step row — added into the last step's reward of whichever source the update reads (the rows' own reward column, or the
        plan reward's dense buffer).  Only those n values are touched."""
        tv = self.terminal_value
        if tv is None:
            return
        rows, H, X, U = b["rows"], self.horizon, self.system.x_dim, self.action_dim
        row_len, last = rows.shape[1], (H - 1) * n
        tv.eval_into(rows, last * row_len + X + U + 2, row_len, rows if prp is None else b["plan_reward"], last * rew_len + rew_col,
                     rew_len, n, accumulate=True)

    def _check_term_cost(self, system):
        """A TermCost's widths against the system's: u_dim is the control width the dynamics see, not action_dim."""
        tc = self._term_cost
        if tc is None or system is None:
            return
        if tc.x_dim != system.x_dim:
            raise ValueError(f"cost_fn is a TermCost at x_dim {tc.x_dim}, the system has x_dim {system.x_dim}")
        if tc.u_dim != system.u_dim:
            raise ValueError(f"cost_fn is a TermCost at u_dim {tc.u_dim}, the system has u_dim {system.u_dim} (the control width the "
                             f"dynamics see; its action_dim is {system.action_dim})")

    def _plan_reward(self, opt_state, batch: Optional[int]):
        """(plan reward or None, the system parameters the rollout runs under).  A PlanRewardParams is checked against the system, the
        horizon and the batch and taken out of the parameters `rollout_spec` sees (it refuses one: iCEM alone consumes it)."""
        sp = opt_state.system_params
        prp = sp.reward_params
        if not isinstance(prp, PlanRewardParams):
            return None, sp
        prp.check_plan(self.system, self.horizon, batch)
        if not self.system.fused:
            raise ValueError(f"a PlanRewardParams needs a fused system (PendulumSystem, EnsembleSystem): {type(self.system).__name__}.step "
                             f"is user code that computes its own reward")
        return prp, sp.replace(reward_params=prp.rollout_reward_params(self.system, sp))

    def _reward_source(self, prp: Optional[PlanRewardParams], b: dict, n_problems: int, group: int):
        """(pointer, row_len, reward_col) the update launch reads the rewards through: the rollout's own rows, or — one launch of
        mbpo_plan_reward_eval — a dense [H * n_problems * group] buffer holding the rewards under the table.  Dense, not in place: a
        4-byte store into every 40-byte row dirties every cache line of the rows, which then go back to memory whole (the Pendulum kind
        at batch_size 64: 86.8 us in place against 42.3 us dense, profiles/r16_icem_plan_reward.json), and the update reads 4 bytes per
        row instead of a strided column."""
        rows = b["rows"]
        if prp is None:
            return rows.data_ptr(), rows.shape[1], self.system.x_dim + self.action_dim
        X, U = self.system.x_dim, self.action_dim
        if "plan_reward" not in b:
            b["plan_reward"] = torch.zeros(rows.shape[0], device=rows.device, dtype=torch.float32)
        out = ops.plan_reward_eval(prp.kind, prp.table, rows, self.horizon, n_problems, group, X, self.system.u_dim, next_off=X + U + 2,
                                   out=b["plan_reward"])
        return out.data_ptr(), 1, 0

    # -- reference API ------------------------------------------------------------------------------------------------
    def init(self, key: int, true_buffer_state: Optional[ReplayBufferState] = None, batch_size: Optional[int] = None) -> iCemOptimizerState:
        """batch_size=B: a state for B independent problems (see the module docstring); key = K.split(k, B) of the key k the
        single-problem state would hold."""
        assert self.system is not None, "iCem optimizer requires system to be defined."
        init_key, dummy_buffer_key, key = K.split(key, 3)
        dev = torch.device("cuda", torch.cuda.current_device())
        if batch_size is None:
            return iCemOptimizerState(true_buffer_state=self.dummy_true_buffer_state(dummy_buffer_key),
                                      system_params=self.system.init_params(init_key), best_sequence=torch.zeros(self.opt_dim, device=dev),
                                      best_reward=torch.zeros((), device=dev), key=key)
        B = int(batch_size)
        if B < 1:
            raise ValueError("batch_size must be >= 1")
        return iCemOptimizerState(true_buffer_state=self.dummy_true_buffer_state(dummy_buffer_key), system_params=self.system.init_params(init_key),
                                  best_sequence=torch.zeros((B,) + self.opt_dim, device=dev), best_reward=torch.zeros(B, device=dev),
                                  key=K.split(key, B))

    def _buffers(self, dev):
        if self._bufs is None or self._bufs["dev"] != dev:
            p, H, U = self.opt_params, self.horizon, self.action_dim
            NC = p.num_samples + self.num_prev
            N = NC * p.num_particles
            f = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)

            vec = lambda v: _bound_vec(v, U, dev)
            self._bufs = dict(dev=dev, NC=NC, N=N, mean=f(H, U), std=f(H, U), best_value=f(1), best_seq=f(H, U), prev=f(self.num_prev, H, U),
                              actions=f(H, N, U), cand=f(NC, H, U), values=f(NC), rank=torch.zeros(NC, device=dev, dtype=torch.int32),
                              u_min=vec(p.u_min), u_max=vec(p.u_max), obs=f(N, self.system.x_dim), first=f(N, self.system.x_dim),
                              steps=f(N), done=f(N), rows=f(H * N, 2 * self.system.x_dim + U + 3))
            if self._term_cost is not None:
                self._bufs["term_cost"] = f(N)
            self._proposal_buffers(self._bufs, 1, dev)
        return self._bufs

    def _batched_buffers(self, dev, B: int):
        """The buffers of `_buffers` for B problems.  rows alone is H*B*NC*P*(2x+u+3) floats: about 1 GB at B = 256 with the
        default iCemParams on the Pendulum (H = 20, NC*P = 5150, x = 3)."""
        bb = self._bbufs
        if bb is None or bb["dev"] != dev or bb["B"] != B:
            self._bbufs = None      # (release the old set before allocating the new one)
            p, H, U, X = self.opt_params, self.horizon, self.action_dim, self.system.x_dim
            NC = p.num_samples + self.num_prev
            N = NC * p.num_particles
            NT = B * N
            f = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)
            self._bbufs = dict(dev=dev, B=B, NC=NC, N=N, NT=NT, mean=f(B, H, U), std=f(B, H, U), best_value=f(B), best_seq=f(B, H, U),
                               prev=f(B, self.num_prev, H, U), actions=f(H, NT, U), cand=f(B, NC, H, U), values=f(B * NC),
                               rank=torch.zeros(B * NC, device=dev, dtype=torch.int32), u_min=_bound_vec(p.u_min, U, dev),
                               u_max=_bound_vec(p.u_max, U, dev), obs=f(NT, X), first=f(NT, X), steps=f(NT), done=f(NT),
                               rows=f(H * NT, 2 * X + U + 3))
            if self._term_cost is not None:
                self._bbufs["term_cost"] = f(NT)
            self._proposal_buffers(self._bbufs, B, dev)
        return self._bbufs

    def optimize(self, initial_state: torch.Tensor, opt_state: iCemOptimizerState) -> iCemOptimizerState:
        assert self.system is not None, "iCem optimizer requires system to be defined."
        self._check_term_cost(self.system)      # (a system assigned without set_system)
        self._check_terminal_value(self.system)
        self._check_policy_prior(self.system)
        if opt_state.batched:
            return self._optimize_batched(initial_state, opt_state)
        p, H, U = self.opt_params, self.horizon, self.action_dim
        dev = initial_state.device if initial_state.is_cuda else torch.device("cuda", torch.cuda.current_device())
        b = self._buffers(dev)
        X = self.system.x_dim
        x0 = initial_state.reshape(-1).to(dev, torch.float32)
        # initial distribution; warm start = previous best sequence shifted by one, last action repeated (:240-246)
        b["mean"].zero_()
        if p.warm_start:
            b["mean"][:-1].copy_(opt_state.best_sequence[1:])
            b["mean"][-1].copy_(opt_state.best_sequence[-1])
        b["std"].fill_(p.init_std)
        b["best_value"].fill_(float("-inf"))
        b["best_seq"].copy_(b["mean"])
        b["prev"].zero_()
        optimizer_key, key = K.split(opt_state.key, 2)
        prp, sys_params = self._plan_reward(opt_state, None)
        spec = without_termination(self.system.rollout_spec(sys_params, dev))      # (rollout_actions ignores done)
        st = _hip.current_stream_ptr()
        lib = self.lib
        pp = self.policy_prior
        if pp is not None:
            self._propose(b, 1, x0, [K.split(optimizer_key, 3)[2]], spec)
            if pp.init_mean:      # LOOP's scheme: the search starts from the mode proposal (a non-finite one keeps the warm start)
                self._seed(b, 1, candidates=False, mean=True)
                b["best_seq"].copy_(b["mean"])
        carry_key = optimizer_key
        for it in range(p.num_steps):
            sampling_key, particles_key = K.split(carry_key, 2)          # :170-173 (the carried key is the first sampling split)
            carry_key = K.split(sampling_key, 2)[0]
            _hip.check(lib.mbpo_icem_sample(b["mean"].data_ptr(), b["std"].data_ptr(), b["prev"].data_ptr(), b["u_min"].data_ptr(),
                                            b["u_max"].data_ptr(), p.num_samples, self.num_prev, H, U, p.num_particles, float(p.exponent),
                                            sampling_key, it, None, b["actions"].data_ptr(), b["cand"].data_ptr(), st), "mbpo_icem_sample")
            if pp is not None and (it == 0 or pp.every_iteration):
                self._seed(b, 1, candidates=True, mean=False)
            b["obs"].copy_(x0.expand(b["N"], X))
            b["first"].copy_(b["obs"])
            b["steps"].zero_(); b["done"].zero_()
            ops.model_rollout(x_dim=X, u_dim=U, actions=b["actions"], obs=b["obs"], first_obs=b["first"], steps=b["steps"], done=b["done"],
                              n_steps=H, episode_length=2 ** 30, seed=particles_key, offset=it, out=b["rows"], **spec)
            rew_ptr, rew_len, rew_col = self._reward_source(prp, b, 1, b["N"])
            self._add_terminal_value(b, prp, rew_len, rew_col, b["N"])
            cost_ptr = None
            if self._term_cost is not None:
                cost_ptr = self._term_cost.trajectory_cost(b["rows"], H, b["N"], next_off=X + U + 2, out=b["term_cost"]).data_ptr()
            elif self.cost_fn is not None:
                rows3 = b["rows"].reshape(H, b["N"], -1)
                obs_t = rows3[:, :, :X].transpose(0, 1)                    # [N, H, x]: transitions.observation per (candidate, particle)
                act_t = rows3[:, :, X:X + U].transpose(0, 1)               # [N, H, u]
                cost = torch.func.vmap(self.cost_fn)(obs_t, act_t)         # :162  vmap(self.cost_fn)(observation, action)
                cost = torch.as_tensor(cost, device=dev, dtype=torch.float32).reshape(-1).contiguous()
                assert cost.numel() == b["N"], "cost_fn must return one scalar per trajectory"       # :163
                b["cost"] = cost
                cost_ptr = cost.data_ptr()
            _hip.check(lib.mbpo_icem_update_constrained(
                rew_ptr, rew_len, rew_col, b["NC"], p.num_particles, H, U, b["cand"].data_ptr(), p.num_elites,
                self.num_prev, float(p.alpha), int(self.use_optimism), cost_ptr, float(p.lambda_constraint), int(self.use_pessimism),
                b["mean"].data_ptr(), b["std"].data_ptr(), b["best_value"].data_ptr(), b["best_seq"].data_ptr(), b["prev"].data_ptr(),
                b["values"].data_ptr(), b["rank"].data_ptr(), st), "mbpo_icem_update_constrained")
        return opt_state.replace(key=key, best_sequence=b["best_seq"].clone(), best_reward=b["best_value"][0].clone())

    def _optimize_batched(self, initial_state: torch.Tensor, opt_state: iCemOptimizerState) -> iCemOptimizerState:
        """`optimize` for B problems in one launch chain per iteration: problem b equals the single call on (initial_state[b],
        best_sequence[b], key[b]) bit for bit."""
        p, H, U = self.opt_params, self.horizon, self.action_dim
        B = opt_state.best_sequence.shape[0]
        keys = list(opt_state.key)
        if len(keys) != B:
            raise ValueError(f"a batched state needs {B} keys, got {len(keys)}")
        dev = initial_state.device if initial_state.is_cuda else torch.device("cuda", torch.cuda.current_device())
        b = self._batched_buffers(dev, B)
        X, N, NT = self.system.x_dim, b["N"], b["NT"]
        x0 = initial_state.reshape(B, X).to(dev, torch.float32)
        b["mean"].zero_()
        if p.warm_start:
            b["mean"][:, :-1].copy_(opt_state.best_sequence[:, 1:])
            b["mean"][:, -1].copy_(opt_state.best_sequence[:, -1])
        b["std"].fill_(p.init_std)
        b["best_value"].fill_(float("-inf"))
        b["best_seq"].copy_(b["mean"])
        b["prev"].zero_()
        # the single path's key chain, for all problems at once: seeds[it] = (sampling keys, particle keys), uploaded once
        ks = K.split_many(keys, 2)
        carry, next_keys = ks[:, 0], ks[:, 1]
        seeds = np.empty((p.num_steps, 2, B), dtype=np.uint64)
        for it in range(p.num_steps):
            sk = K.split_many(carry, 2)
            seeds[it, 0], seeds[it, 1] = sk[:, 0], sk[:, 1]
            carry = K.split_many(sk[:, 0], 2)[:, 0]
        seeds_dev = torch.from_numpy(seeds.view(np.int64)).to(dev)
        prp, sys_params = self._plan_reward(opt_state, B)
        spec = without_termination(self.system.rollout_spec(sys_params, dev))      # (rollout_actions ignores done)
        draw = self._batched_ensemble_draws(spec, b)
        st = _hip.current_stream_ptr()
        lib = self.lib
        pp = self.policy_prior
        if pp is not None:
            self._propose(b, B, x0, K.split_many(ks[:, 0], 3)[:, 2], spec)      # (the proposals run in ENS_MEAN: `draw` is not theirs)
            if pp.init_mean:
                self._seed(b, B, candidates=False, mean=True)
                b["best_seq"].copy_(b["mean"])
        for it in range(p.num_steps):
            _hip.check(lib.mbpo_icem_sample_batched(b["mean"].data_ptr(), b["std"].data_ptr(), b["prev"].data_ptr(), b["u_min"].data_ptr(),
                                                    b["u_max"].data_ptr(), p.num_samples, self.num_prev, H, U, p.num_particles,
                                                    float(p.exponent), B, seeds_dev[it, 0].data_ptr(), it, b["actions"].data_ptr(),
                                                    b["cand"].data_ptr(), st), "mbpo_icem_sample_batched")
            if pp is not None and (it == 0 or pp.every_iteration):
                self._seed(b, B, candidates=True, mean=False)
            b["obs"].view(B, N, X).copy_(x0[:, None, :].expand(B, N, X))
            b["first"].copy_(b["obs"])
            b["steps"].zero_(); b["done"].zero_()
            pseeds = seeds_dev[it, 1].data_ptr()
            if draw.get("draw_member"):
                _hip.check(lib.mbpo_philox_fill_grouped(pseeds, it, _hip.STREAM_MEMBER, H, B, N, 1, 0, draw["E"], draw["member_idx"].data_ptr(), st),
                           "mbpo_philox_fill_grouped")
            if draw.get("model_noise") is not None:
                _hip.check(lib.mbpo_philox_fill_grouped(pseeds, it, _hip.STREAM_MODEL_NOISE, H, B, N * X, 0, 0, 0, draw["model_noise"].data_ptr(),
                                                        st), "mbpo_philox_fill_grouped")
            ops.model_rollout(x_dim=X, u_dim=U, actions=b["actions"], obs=b["obs"], first_obs=b["first"], steps=b["steps"], done=b["done"],
                              n_steps=H, episode_length=2 ** 30, seed=0, offset=it, out=b["rows"], member_idx=draw.get("member_idx"),
                              model_noise=draw.get("model_noise"), **spec)
            rew_ptr, rew_len, rew_col = self._reward_source(prp, b, B, N)
            self._add_terminal_value(b, prp, rew_len, rew_col, NT)
            cost_ptr = None
            if self._term_cost is not None:
                cost_ptr = self._term_cost.trajectory_cost(b["rows"], H, NT, next_off=X + U + 2, out=b["term_cost"]).data_ptr()
            elif self.cost_fn is not None:
                rows3 = b["rows"].reshape(H, NT, -1)
                obs_t = rows3[:, :, :X].transpose(0, 1)
                act_t = rows3[:, :, X:X + U].transpose(0, 1)
                cost = torch.func.vmap(self.cost_fn)(obs_t, act_t)
                cost = torch.as_tensor(cost, device=dev, dtype=torch.float32).reshape(-1).contiguous()
                assert cost.numel() == NT, "cost_fn must return one scalar per trajectory"
                b["cost"] = cost
                cost_ptr = cost.data_ptr()
            _hip.check(lib.mbpo_icem_update_batched(
                rew_ptr, rew_len, rew_col, B, b["NC"], p.num_particles, H, U, b["cand"].data_ptr(), p.num_elites,
                self.num_prev, float(p.alpha), int(self.use_optimism), cost_ptr, float(p.lambda_constraint), int(self.use_pessimism),
                b["mean"].data_ptr(), b["std"].data_ptr(), b["best_value"].data_ptr(), b["best_seq"].data_ptr(), b["prev"].data_ptr(),
                b["values"].data_ptr(), b["rank"].data_ptr(), st), "mbpo_icem_update_batched")
        return opt_state.replace(key=[int(k) for k in next_keys], best_sequence=b["best_seq"].clone(), best_reward=b["best_value"].clone())

    def _batched_ensemble_draws(self, spec: dict, b: dict) -> dict:
        """A stochastic EnsembleSystem draws its members / model noise in the rollout kernel from the GLOBAL env index, so a rollout
        over all problems would not reproduce problem b's single-call draws.  Here they are drawn per problem (each under its
        particle key) into member_idx [H, B*NC*P] / model_noise [H, B*NC*P, x] buffers the rollout consumes instead.  'tsinf'
        (member = env % E in the kernel) runs as 'ts1' with member_idx = problem-local env % E: the two modes differ only in the
        member selection in every rollout kernel the open-loop dispatch can pick.  Edits `spec` in place."""
        if spec.get("system_kind") != _hip.SYS_ENSEMBLE or spec.get("ens_mode", _hip.ENS_MEAN) == _hip.ENS_MEAN:
            return {}
        H, X, B, N, dev = self.horizon, self.system.x_dim, b["B"], b["N"], b["dev"]
        E = int(spec["dyn_spec"].n_nets)
        out = dict(E=E)
        if spec["ens_mode"] == _hip.ENS_TSINF:
            if b.get("tsinf_E") != E:
                b["tsinf_member"] = (torch.arange(N, device=dev, dtype=torch.int32) % E).repeat(H * B).contiguous()
                b["tsinf_E"] = E
            out["member_idx"] = b["tsinf_member"]
            spec["ens_mode"] = _hip.ENS_TS1
        else:
            if "member" not in b:
                b["member"] = torch.zeros(H * b["NT"], device=dev, dtype=torch.int32)
            out["member_idx"], out["draw_member"] = b["member"], True
        if spec.get("ens_sample_noise"):
            if "model_noise" not in b:
                b["model_noise"] = torch.zeros(H * b["NT"] * X, device=dev, dtype=torch.float32)
            out["model_noise"] = b["model_noise"]
        return out

    def act(self, obs: torch.Tensor, opt_state: iCemOptimizerState, evaluate: bool = True) -> Tuple[torch.Tensor, iCemOptimizerState]:
        new_opt_state = self.optimize(initial_state=obs, opt_state=opt_state)
        return new_opt_state.action, new_opt_state


def _bound_vec(v, U: int, dev) -> torch.Tensor:
    """scalar or per-dimension bound -> [U] device vector"""
    t = torch.as_tensor(v, dtype=torch.float32).reshape(-1)
    return (t.expand(U) if t.numel() == 1 else t.reshape(U)).contiguous().to(dev)


class iCEMOptimizer(BaseOptimizer):
    """iCEM wrapper with the SAC/PPO optimizers' interface (icem_optimizer.py:259-320).  batch_size=B: plans for B environments at
    once (init makes a batched state, act(obs [B, x]) returns actions [B, u]); None keeps the single-state interface."""

    def __init__(self, horizon: int, opt_params: iCemParams = iCemParams(), system: Optional[System] = None, key: int = K.PRNGKey(0),
                 batch_size: Optional[int] = None, terminal_value: Optional[TerminalValue] = None,
                 policy_prior: Optional[PolicyPrior] = None, **agent_kwargs):
        refuse_time_adaptive(system, "iCEM")
        if policy_prior is not None:
            if not isinstance(policy_prior, PolicyPrior):
                raise ValueError(f"policy_prior must be a PolicyPrior (mbpo.optimizers) or None, got {type(policy_prior).__name__}")
            policy_prior.check_optimizer(opt_params.num_samples)
            policy_prior.check_system(system)
            agent_kwargs = dict(agent_kwargs, policy_prior=policy_prior)
        self.policy_prior = policy_prior
        if terminal_value is not None:
            if not isinstance(terminal_value, TerminalValue):
                raise ValueError(f"terminal_value must be a TerminalValue (mbpo.optimizers) or None, got {type(terminal_value).__name__}")
            terminal_value.check_system(system)
            agent_kwargs = dict(agent_kwargs, terminal_value=terminal_value)
        self.terminal_value = terminal_value
        super().__init__(system, key)
        self.horizon, self.key, self.opt_params = horizon, key, opt_params
        self.batch_size = None if batch_size is None else int(batch_size)
        if self.batch_size is not None and self.batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        self.agent_class, self.agent_kwargs = iCemTO, agent_kwargs
        if system is not None:
            self.set_system(system)

    def set_system(self, system):
        refuse_time_adaptive(system, "iCEM")
        if self.terminal_value is not None:
            self.terminal_value.check_system(system)
        if self.policy_prior is not None:
            self.policy_prior.check_system(system)
        super().set_system(system)

    @property
    def can_act_in_batches(self):
        return self.batch_size is not None

    def init(self, key: int, true_buffer_state=None) -> iCemOptimizerState:
        assert self.system is not None, "iCEM optimizer requires system to be defined."
        self.agent = self.agent_class(horizon=self.horizon, action_dim=self.system.action_dim, key=self.key, opt_params=self.opt_params,
                                      **self.agent_kwargs)
        self.agent.set_system(self.system)
        if true_buffer_state is None:
            dummy_buffer_key, key = K.split(key, 2)
            true_buffer_state = self.dummy_true_buffer_state(dummy_buffer_key)
        agent_state = self.agent.init(key, batch_size=self.batch_size)
        return agent_state.replace(true_buffer_state=true_buffer_state)

    def act(self, obs: torch.Tensor, opt_state: iCemOptimizerState, evaluate: bool = True) -> Tuple[torch.Tensor, iCemOptimizerState]:
        assert self.system is not None, "iCEM optimizer requires system to be defined."
        if self.batch_size is not None:
            action, opt_state = self.agent.act(obs.reshape(self.batch_size, -1), opt_state, evaluate)
            return action.reshape(self.batch_size, -1), opt_state
        action, opt_state = self.agent.act(obs.reshape(-1), opt_state, evaluate)
        return action.reshape(1, -1), opt_state

    def train(self, opt_state: iCemOptimizerState) -> iCemTrainingOutput:
        training_output = super().train(opt_state)
        return iCemTrainingOutput(optimizer_state=training_output.optimizer_state, summary=[])
