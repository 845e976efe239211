"""EnsembleDynamics / EnsembleSystem — the learned-ensemble System behind the reference's Dynamics/System seam
(base_dynamics.py:15-20, base_systems.py:40-52).

NOT IN THE REFERENCE: `bsm` is declared in setup.py:22 but never imported; this is the slot MBPO's learned
model plugs into.  Semantics (build-defined, parity-unpinned; restated in oracle/systems.py):
    out_e = MLP_e([x, u]) = [mu_e (x_dim), raw_std_e (x_dim)],  sigma_e = softplus(raw_std_e) + min_std
    base  = x if predict_delta else 0
    'mean' : x' = base + mean_e(mu_e)               — what System.step's `.mean()` consumes
    'ts1'  : member drawn per (env, step);  x' = base + mu_m (+ sigma_m * eps when sample_noise)   — MBPO-style
    'tsinf': member = env % E
    'optimistic': hallucinated control (include/mbpo_hip.h "hallucinated control"; H-UCRL-style optimistic exploration): the policy
             emits [u | eta], eta in [-1, 1]^x, and x' = base + mean_e(mu_e) + beta * std_e(mu_e) * eta (population std over members)
BPTT differentiates every mode but 'optimistic' (include/mbpo_hip.h, mbpo_bptt_desc): in 'ts1' / 'tsinf' by reparameterisation through the selected
member — mu_m, and with sample_noise sigma_m * eps — with the member and eps drawn from Philox per train step (the reference threads
SystemParams.key through rollout_policy, utils/optimizer_utils.py:81-97).  sample_noise has no effect in 'mean' mode.

Learned reward (EnsembleDynamics(learn_reward=True) + LearnedReward): the members also predict the reward,
    out_e = [mu_e (x_dim), raw_std_e (x_dim), mu_r,e, raw_r,e]
and the reward of a step is the head at the pre-step (x, u): 'mean' r = mean_e mu_r,e; 'ts1' / 'tsinf' r = mu_r,m with the member m
the state takes.  sample_noise perturbs the state only.  `fit` adds the reward's Gaussian NLL (target: the rows' reward column).

Model selection (MBPO's model-training procedure, Janner et al. 2019 — not the reference's, which has no model): `fit(holdout_ratio=)`
holds rows out, evaluates every member on them once per epoch (mbpo_ens_eval), keeps each member's best parameters on the device
(mbpo_ens_keep_best) and stops when no member improved for a few evaluations; `fit(n_elites=)` / `select_elites` pick the members
of lowest held-out squared error (mbpo_ens_pick_elites).  EnsembleDynamicsParams.elite_params, when set, is what every rollout
consumer runs: the kernels see an ensemble of n_elites members, so 'mean' averages the elites, 'ts1' draws among them and 'tsinf'
binds env i to elite i % n_elites.

Input scaler (MBPO's, fitted on the training inputs; only the inputs are scaled): `fit(normalize_inputs=True)` fits per-column mean / std
of [x, u] on the training rows (mbpo_ens_scaler_fit), trains on a matrix prepared once — inputs normalised, target encoded
(mbpo_ens_scaler_prepare) — and leaves EnsembleDynamicsParams.params in NORMALISED coordinates.  Consumers never normalise: they run
folded_params, the same members with the scaler folded into the first Dense layer (mbpo_ens_fold_scaler; W' = diag(1/std) W,
b' = b - W'^T mean), on raw inputs — the same affine map, so no rollout, planning or BPTT kernel knows about the scaler.

Calibration (what the reference's declared-but-unimported `bsm` does after a fit; restated as remembered, so include/mbpo_hip.h "N3d"
is the definition): `calibrate` / `fit(calibrate=True)` pick one factor per state dimension on held-out rows (mbpo_ens_calibrate) so
that mean +- z * calibration * std_e(mu_e) covers the true next state as often as a Gaussian's interval would, at 19 levels;
`coverage` reads the covered fractions.  EnsembleSystem(mode="optimistic", calibrated=True) then hands the kernels
halluc_beta = beta * calibration, and next_state reports std = sqrt(E[sigma^2] + calibration^2 Var[mu]).
"""
from __future__ import annotations

import dataclasses
import math
from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from mbpo import _hip, ops
from mbpo.systems.base_systems import System, SystemParams
from mbpo.systems.dynamics.base_dynamics import Dynamics, Normal
from mbpo.systems.rewards.base_rewards import Reward
from mbpo.systems.termination import BoxTermination, termination_spec
from mbpo.utils import keys as K

# ('optimistic' is ENS_MEAN plus halluc_beta: the mean of the members, moved inside their spread by the policy's eta)
_MODES = {"mean": _hip.ENS_MEAN, "ts1": _hip.ENS_TS1, "tsinf": _hip.ENS_TSINF, "optimistic": _hip.ENS_MEAN}


FIT_SITE_HOLDOUT = 1            # high word of the Philox offset of fit's holdout permutation (the sampler draws at offsets 0, 1, ...)


@dataclass
class EnsembleDynamicsParams:
    """elite_params is a COPY of the elite members' parameters (in elite_idx order), taken when they were selected: a later `fit`
    without re-selection leaves it stale (the rollouts then still run the old elites); `fit(..., n_elites=)` always refreshes it, and
    `select_elites` does on request.  Set both elite fields to None to roll out through all members again.

    scaler, when set, says that `params` live in normalised input coordinates (they are what `fit` trains and `evaluate` scores) and
    that every consumer runs folded_params instead: a COPY of params with the scaler folded into layer one, taken at the end of
    `fit(normalize_inputs=True)` and by `select_elites` / `EnsembleDynamics.fold`.  Changing params or scaler by hand leaves it stale
    until `fold` is called; elite_params of a scaler-bearing object are picked from folded_params and go stale the same way.

    calibration, when set, holds one factor per state dimension for the spread of the members the rollouts used WHEN IT WAS PICKED
    (`calibrate`, `fit(calibrate=True)`): a later `fit`, `fold` or elite selection without a new `calibrate` leaves it stale, as
    elite_params goes stale; `calibrate` rewrites the tensor in place, so consumers that hold it see the new factors.  Set it to None
    to report and roll out the uncalibrated spread again."""
    params: torch.Tensor          # flat [E * P] device tensor (layout: include/mbpo_hip.h)
    elite_idx: Optional[torch.Tensor] = None       # int32 [n_elites]: the members the rollouts use, best first
    elite_params: Optional[torch.Tensor] = None    # [n_elites * P]
    holdout: Optional[torch.Tensor] = None         # [2, E]: held-out (NLL, squared error) of the members fit(holdout_ratio=) kept
    scaler: Optional[torch.Tensor] = None          # [2, x+u]: (mean; std) of the training inputs, fit(normalize_inputs=True)
    folded_params: Optional[torch.Tensor] = None   # [E * P]: params with the scaler folded into layer one (what consumers run)
    calibration: Optional[torch.Tensor] = None     # [x_dim]: the factor on the members' spread picked on held-out rows (calibrate)

    def replace(self, **kw):
        return dataclasses.replace(self, **kw)


def lecun_uniform_flat(dims: Sequence[int], gen: torch.Generator) -> torch.Tensor:
    """flax lecun_uniform kernels U(+-sqrt(3/fan_in)), zero biases (sac/networks.py:23)."""
    parts = []
    for i in range(len(dims) - 1):
        bound = math.sqrt(3.0 / dims[i])
        parts.append(((torch.rand(dims[i], dims[i + 1], generator=gen, dtype=torch.float64) * 2 - 1) * bound).reshape(-1).float())
        parts.append(torch.zeros(dims[i + 1]))
    return torch.cat(parts)


def kernel_width_for(hidden_layer_sizes: Sequence[int]) -> Optional[int]:
    """The hidden width an ensemble of these hidden sizes is stored at: the smallest of ops.ROLLOUT_WIDTHS that holds every layer
    (200 -> 256, (200, 100) -> 256), so that the rollout kernels take it; None above 256 (the logical sizes, layer by layer only)."""
    hid = [int(h) for h in hidden_layer_sizes]
    if not hid or max(hid) > ops.ROLLOUT_WIDTHS[-1]:
        return None
    return ops.common_width(hid, supported=ops.ROLLOUT_WIDTHS, what="EnsembleDynamics")


class EnsembleDynamics(Dynamics[EnsembleDynamicsParams]):
    """learn_reward: the members also predict the reward (two more outputs, [mu_r, raw_r]); see LearnedReward.

    Any hidden sizes.  dims_logical are the sizes asked for; dims / spec are the KERNEL shapes the parameters are stored at: every
    hidden layer zero-padded to kernel_width (kernel_width_for; ops.py "hidden-width padding"), so that the rollout kernels run the
    members.  64, 128 and 256 wide stacks are their own kernel shapes.  The padding is a fixed point of `fit` (padded entries get
    exactly zero gradient and AdamW keeps them at zero), so the stored network stays the logical one; logical_params /
    from_logical_params convert.  Above 256 kernel_width is None and the parameters are logical: fit, member_outputs and
    next_state run layer by layer; the rollout consumers refuse the shape."""

    def __init__(self, x_dim: int, u_dim: int, n_members: int = 5, hidden_layer_sizes: Sequence[int] = (64, 64, 64),
                 activation: str = "swish", device=None, learn_reward: bool = False):
        super().__init__(x_dim, u_dim)
        self.n_members = n_members
        self.learn_reward = bool(learn_reward)
        self.dims_logical = [x_dim + u_dim, *[int(h) for h in hidden_layer_sizes], 2 * x_dim + (2 if self.learn_reward else 0)]
        self.kernel_width = kernel_width_for(hidden_layer_sizes)
        self.dims = ops.padded_dims(self.dims_logical, self.kernel_width)
        self.spec = ops.MlpSpec(self.dims, activation, n_members)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())

    def init_params(self, key: int) -> EnsembleDynamicsParams:
        gen = torch.Generator().manual_seed(K.PRNGKey(key) % (2 ** 63))
        flat = torch.cat([lecun_uniform_flat(self.dims_logical, gen) for _ in range(self.n_members)])
        return self.from_logical_params(flat)

    def logical_params(self, dynamics_params: EnsembleDynamicsParams) -> torch.Tensor:
        """The members' flat parameters at dims_logical ([E * P_logical], on the parameters' device)."""
        if self.kernel_width is None:
            return dynamics_params.params
        return ops.extract_mlp_params(dynamics_params.params, self.dims_logical, self.kernel_width, self.n_members)

    def from_logical_params(self, flat: torch.Tensor) -> EnsembleDynamicsParams:
        """Flat parameters at dims_logical ([E * P_logical]) -> EnsembleDynamicsParams stored at the kernel shapes."""
        flat = flat.reshape(-1).to(torch.float32)
        if self.kernel_width is not None:
            flat = ops.embed_mlp_params(flat, self.dims_logical, self.kernel_width, self.n_members)
        return EnsembleDynamicsParams(params=flat.to(self.device).contiguous())

    def fit(self, dynamics_params: EnsembleDynamicsParams, rows: torch.Tensor, num_steps: int, batch_size: int = 256,
            learning_rate: float = 1e-3, weight_decay: float = 0.0, key: int = 0, predict_delta: bool = True,
            min_std: float = 1e-3, n_rows: Optional[int] = None, next_obs_off: Optional[int] = None,
            reward_off: Optional[int] = None, holdout_ratio: float = 0.0, max_holdout: int = 5000, eval_every: Optional[int] = None,
            max_evals_since_improvement: int = 5, rel_tol: float = 0.01, n_elites: Optional[int] = None,
            normalize_inputs: bool = False, scaler_std_floor: float = ops.SCALER_STD_FLOOR, calibrate: bool = False):
        """Model learning (N3 — not in the reference, whose model would come from `bsm`): `num_steps` AdamW steps on the
        members' Gaussian negative log-likelihood, each member on its own bootstrapped minibatch (sampling with replacement
        from rows[:n_rows]; Philox randint on the device).  `rows` are true-buffer transition rows (obs, action, reward,
        discount, next_obs, ...).  With learn_reward the reward head is fitted to column `reward_off` (default x_dim + u_dim, the
        Transition's reward).  Updates dynamics_params.params in place; returns (dynamics_params, losses [steps run, E]).

        holdout_ratio > 0 (MBPO's model selection): rows[:n_rows] are permuted (device Philox permutation keyed by `key`); the first
        min(max_holdout, floor(holdout_ratio * R)) are held out, the rest are copied once into the training matrix the sampler draws
        from.  Every `eval_every` steps (default: one epoch, ceil(R_train / batch_size)) the members are evaluated on the holdout and
        each member whose squared error improved by the relative margin `rel_tol` is snapshotted; the fit stops when no member improved
        for more than `max_evals_since_improvement` evaluations, or at `num_steps` (then after one last evaluation).  The snapshots are
        copied back into dynamics_params.params in place; dynamics_params.holdout = their held-out [NLL; squared error] ([2, E]).
        n_elites: dynamics_params.elite_idx / elite_params = the n_elites members of lowest held-out squared error.

        normalize_inputs (MBPO's input scaler): the per-column mean / std of [x, u] are fitted on the TRAINING rows (after the holdout
        split; a std below scaler_std_floor counts as 1) and the training and holdout rows are prepared once — inputs normalised,
        target delta-encoded as `predict_delta` says, columns [x, u | reward | target] — so the steps above run unchanged on the
        prepared matrices and the scaler costs nothing per step.  dynamics_params.params are then in normalised coordinates;
        dynamics_params.scaler = the scaler and dynamics_params.folded_params = the members every consumer runs on raw inputs (`fold`);
        the elites are picked from folded_params.  A refit refits the scaler on the new rows and continues from the same weights.

        calibrate (needs a holdout: factors picked on training rows would be biased): after the snapshots are restored, and after the
        fold and the elite selection if any, `self.calibrate` runs on the RAW held-out rows with this fit's predict_delta and
        next_obs_off, through the members the rollouts use; dynamics_params.calibration = its factors.  False changes nothing."""
        dev = self.device
        if dynamics_params.scaler is not None and not normalize_inputs:
            raise ValueError("these parameters were fitted on normalised inputs (scaler is set): refit with normalize_inputs=True")
        if reward_off is not None and not self.learn_reward:
            raise ValueError("reward_off needs EnsembleDynamics(learn_reward=True)")
        if self.learn_reward and reward_off is None:
            reward_off = self.x_dim + self.u_dim
        if n_elites is not None and not holdout_ratio > 0:
            raise ValueError("n_elites needs a holdout (holdout_ratio > 0): the elites are picked by held-out error")
        if calibrate and not holdout_ratio > 0:
            raise ValueError("calibrate needs a holdout (holdout_ratio > 0): factors picked on the training rows are biased")
        rows = rows.to(dev, torch.float32).contiguous()
        R = int(rows.shape[0] if n_rows is None else n_rows)
        if R <= 0:
            raise ValueError("no transitions to fit on")
        E = self.n_members
        seed = K.PRNGKey(key)
        train, hold_idx = rows, None
        # what the NLL / eval kernels are told: the caller's row layout, or the prepared one (target already encoded)
        X, U = self.x_dim, self.u_dim
        k_delta, k_next, k_rew, hold_rows, scaler = predict_delta, next_obs_off, reward_off, rows, None
        if normalize_inputs:
            k_delta, k_next = False, ops.prepared_next_obs_off(X, U)
            k_rew = ops.prepared_reward_off(X, U) if self.learn_reward else None
        if holdout_ratio > 0:
            n_hold = min(int(max_holdout), int(math.floor(holdout_ratio * R)))
            if n_hold <= 0 or n_hold >= R:
                raise ValueError(f"holdout_ratio {holdout_ratio} of {R} rows leaves an empty holdout or training set")
            perm = ops.philox_permutation(R, seed=seed, offset=FIT_SITE_HOLDOUT << 32)
            hold_idx = perm[:n_hold]
            if normalize_inputs:
                train_idx = perm[n_hold:].contiguous()
                scaler = ops.ens_scaler_fit(rows, X + U, idx=train_idx, std_floor=scaler_std_floor)
                train = ops.ens_scaler_prepare(rows, scaler, X, U, idx=train_idx, next_obs_off=next_obs_off, reward_off=reward_off,
                                               predict_delta=predict_delta)
                hold_rows = ops.ens_scaler_prepare(rows, scaler, X, U, idx=hold_idx.contiguous(), next_obs_off=next_obs_off,
                                                   reward_off=reward_off, predict_delta=predict_delta)
                hold_idx = torch.arange(n_hold, device=dev, dtype=torch.int32)
            else:
                train = ops.replay_gather(rows, torch.tensor([R, 0, 0, R], device=dev, dtype=torch.int32), perm[n_hold:])
            R = R - n_hold
        elif normalize_inputs:
            scaler = ops.ens_scaler_fit(rows, X + U, n=R, std_floor=scaler_std_floor)
            train = ops.ens_scaler_prepare(rows, scaler, X, U, n=R, next_obs_off=next_obs_off, reward_off=reward_off,
                                           predict_delta=predict_delta)
        if getattr(self, "_fit_cfg", None) != (batch_size, k_delta, min_std, learning_rate, weight_decay):
            self._nll = ops.EnsembleNllGrad(x_dim=self.x_dim, u_dim=self.u_dim, spec=self.spec, batch=batch_size, device=dev,
                                            predict_delta=k_delta, min_std=min_std)
            self._opt = ops.AdamW(E * self.spec.n_params, dev, learning_rate, weight_decay, apply_if_finite=True)
            self._fit_cfg = (batch_size, k_delta, min_std, learning_rate, weight_decay)
            self._fit_state = torch.tensor([R, 0, 0, R], device=dev, dtype=torch.int32)
            self._fit_idx = torch.zeros(E * batch_size, device=dev, dtype=torch.int32)
            self._fit_scratch = torch.zeros(E * batch_size, 1, device=dev, dtype=torch.float32)
        self._fit_state[0] = R
        self._fit_state[3] = R
        losses = torch.zeros(num_steps, E, device=dev, dtype=torch.float32)
        col0 = train[:, :1].contiguous()         # the sampler gathers something; one column keeps that cheap
        if hold_idx is not None:
            every = int(eval_every) if eval_every is not None else -(-R // batch_size)
            if every <= 0:
                raise ValueError("eval_every must be positive")
            ev = self._evaluator(k_delta, min_std)
            best_params = dynamics_params.params.clone()
            best_score = torch.full((E,), float("inf"), device=dev, dtype=torch.float32)
            sel_state = torch.zeros(2, device=dev, dtype=torch.int32)
            sel_ws = torch.zeros(E, device=dev, dtype=torch.int32)

            def evaluate_and_keep() -> int:
                m = ev(dynamics_params.params, hold_rows, hold_idx, next_obs_off=k_next, reward_off=k_rew)
                ops.ens_keep_best(dynamics_params.params, best_params, E, m[1], best_score, rel_tol, sel_state, sel_ws)
                return int(sel_state[0])         # the epoch's one read-back: evaluations since any member improved
        steps_run, evaluated_at = num_steps, -1
        for it in range(num_steps):
            ops.replay_sample(col0, self._fit_state, E * batch_size, seed=seed, offset=it, out=self._fit_scratch, idx_out=self._fit_idx)
            g = self._nll(dynamics_params.params, train, self._fit_idx.view(E, batch_size), next_obs_off=k_next, reward_off=k_rew)
            self._opt.step(dynamics_params.params, g)
            losses[it].copy_(self._nll.metrics)
            if hold_idx is not None and (it + 1) % every == 0:
                evaluated_at = it + 1
                if evaluate_and_keep() > max_evals_since_improvement:
                    steps_run = it + 1
                    break
        if hold_idx is None:
            if scaler is not None:
                dynamics_params.scaler = scaler
                self.fold(dynamics_params)
            return dynamics_params, losses
        if steps_run == num_steps and evaluated_at != num_steps:
            evaluate_and_keep()                  # num_steps ended the fit: the last steps can still be snapshotted
        dynamics_params.params.copy_(best_params)
        # the snapshots' metrics: their squared error as it was scored, their NLL from one more evaluation of the restored parameters
        holdout = ev(dynamics_params.params, hold_rows, hold_idx, next_obs_off=k_next, reward_off=k_rew).clone()
        holdout[1].copy_(best_score)
        dynamics_params.holdout = holdout
        members = dynamics_params.params
        if scaler is not None:
            dynamics_params.scaler = scaler
            members = self.fold(dynamics_params).folded_params
        if n_elites is not None:
            dynamics_params.elite_idx, dynamics_params.elite_params = ops.ens_pick_elites(members, E, holdout[1], n_elites)
        if calibrate:
            self.calibrate(dynamics_params, rows, idx=perm[:n_hold], next_obs_off=next_obs_off, predict_delta=predict_delta)
        return dynamics_params, losses[:steps_run]

    def fold(self, dynamics_params: EnsembleDynamicsParams) -> EnsembleDynamicsParams:
        """Refresh dynamics_params.folded_params from its params and scaler (mbpo_ens_fold_scaler, in place when the buffer exists);
        without a scaler folded_params is cleared.  Returns dynamics_params."""
        if dynamics_params.scaler is None:
            dynamics_params.folded_params = None
            return dynamics_params
        out = dynamics_params.folded_params
        if out is not None and out.shape != dynamics_params.params.shape:
            out = None
        dynamics_params.folded_params = ops.ens_fold_scaler(dynamics_params.params, self.n_members, self.dims[0], self.dims[1],
                                                            dynamics_params.scaler.to(self.device, torch.float32).contiguous(), out=out)
        return dynamics_params

    def _consumer_params(self, dynamics_params: EnsembleDynamicsParams) -> torch.Tensor:
        """All members as a consumer of raw inputs must see them: folded when a scaler is set (folded on first use if nobody has)."""
        if dynamics_params.scaler is None:
            return dynamics_params.params
        if dynamics_params.folded_params is None:
            self.fold(dynamics_params)
        return dynamics_params.folded_params

    def _evaluator(self, predict_delta: bool, min_std: float) -> "ops.EnsembleEval":
        if getattr(self, "_eval_cfg", None) != (predict_delta, min_std):
            self._eval = ops.EnsembleEval(x_dim=self.x_dim, u_dim=self.u_dim, spec=self.spec, device=self.device,
                                          predict_delta=predict_delta, min_std=min_std)
            self._eval_cfg = (predict_delta, min_std)
        return self._eval

    def evaluate(self, dynamics_params: EnsembleDynamicsParams, rows: torch.Tensor, idx: Optional[torch.Tensor] = None,
                 next_obs_off: Optional[int] = None, reward_off: Optional[int] = None, predict_delta: bool = True,
                 min_std: float = 1e-3) -> torch.Tensor:
        """[2, E]: every member's mean Gaussian NLL (row 0, `fit`'s loss) and mean squared error of its mean prediction (row 1, MBPO's
        selection metric) on rows[idx] (idx int32, shared by the members; None: all rows) — mbpo_ens_eval, forward only.  reward_off
        defaults as in `fit`.  With a scaler, rows[idx] are prepared with it first (as `fit` prepares its holdout) and the stored
        params — normalised coordinates — are evaluated on them: the figures `fit` reports for the same rows."""
        if reward_off is not None and not self.learn_reward:
            raise ValueError("reward_off needs EnsembleDynamics(learn_reward=True)")
        if self.learn_reward and reward_off is None:
            reward_off = self.x_dim + self.u_dim
        rows = rows.to(self.device, torch.float32).contiguous()
        if idx is None:
            idx = torch.arange(rows.shape[0], device=self.device, dtype=torch.int32)
        idx = idx.to(self.device, torch.int32).contiguous()
        if dynamics_params.scaler is not None:
            X, U = self.x_dim, self.u_dim
            rows = ops.ens_scaler_prepare(rows, dynamics_params.scaler, X, U, idx=idx, next_obs_off=next_obs_off, reward_off=reward_off,
                                          predict_delta=predict_delta)
            idx = torch.arange(rows.shape[0], device=self.device, dtype=torch.int32)
            predict_delta, next_obs_off = False, ops.prepared_next_obs_off(X, U)
            reward_off = ops.prepared_reward_off(X, U) if self.learn_reward else None
        return self._evaluator(predict_delta, min_std)(dynamics_params.params, rows, idx, next_obs_off=next_obs_off,
                                                       reward_off=reward_off).clone()

    def select_elites(self, dynamics_params: EnsembleDynamicsParams, score: torch.Tensor, n_elites: int) -> EnsembleDynamicsParams:
        """The n_elites members of lowest `score` ([E]; NaN last, ties by lower index) become the members every rollout consumer runs:
        returns the params with elite_idx / elite_params set (mbpo_ens_pick_elites; elite_params is a copy, see EnsembleDynamicsParams).
        With a scaler the fold is refreshed first and the elites are copies of folded_params."""
        score = score.to(self.device, torch.float32).contiguous()
        members = self._consumer_params(self.fold(dynamics_params))
        elite_idx, elite_params = ops.ens_pick_elites(members, self.n_members, score, int(n_elites))
        return dynamics_params.replace(elite_idx=elite_idx, elite_params=elite_params)

    def elite_spec(self, n_elites: int) -> "ops.MlpSpec":
        """The kernel shapes of an ensemble of n_elites of these members (cached per n_elites)."""
        cache = self.__dict__.setdefault("_elite_specs", {})
        if n_elites not in cache:
            cache[n_elites] = ops.MlpSpec(self.dims, self.spec.activation, int(n_elites))
        return cache[n_elites]

    def _rollout_members(self, dynamics_params: EnsembleDynamicsParams):
        """(params, spec) of the members the rollouts use: the elites when selected, else all — with a scaler, the folded members."""
        if dynamics_params.elite_params is None:
            return self._consumer_params(dynamics_params), self.spec
        return dynamics_params.elite_params, self.elite_spec(int(dynamics_params.elite_idx.numel()))

    def _calibration_call(self, dynamics_params, rows, idx, next_obs_off, predict_delta, alphas, n_levels, scale):
        """The rollouts' members on the raw [x, u] of rows[idx], then mbpo_ens_calibrate: (calibration, best_idx, counts, n)."""
        params, spec = self._rollout_members(dynamics_params)
        if spec.n_nets < 2:
            raise ValueError("calibration needs at least 2 rollout members: the spread of one member is identically zero")
        rows = rows.to(self.device, torch.float32).contiguous()
        if idx is not None:
            idx = idx.to(self.device, torch.int32).contiguous()
        xu = (rows if idx is None else rows[idx.long()])[:, :self.x_dim + self.u_dim].contiguous()
        y = ops.ensemble_mlp_forward(params, spec, xu)
        cal, best, counts = ops.ens_calibrate(y, rows, self.x_dim, self.u_dim, idx=idx, next_obs_off=next_obs_off,
                                              predict_delta=predict_delta, alphas=alphas, n_levels=n_levels, scale=scale)
        return cal, best, counts, int(xu.shape[0])

    def calibrate(self, dynamics_params: EnsembleDynamicsParams, rows: torch.Tensor, idx: Optional[torch.Tensor] = None,
                  next_obs_off: Optional[int] = None, predict_delta: bool = True, alphas=None, n_levels: int = 19,
                  return_counts: bool = False):
        """Pick dynamics_params.calibration ([x_dim], on the device) on rows[idx] (true-buffer transition rows the members were NOT
        fitted on; idx None: all rows): the members the rollouts use — the elites when selected, the folded members with a scaler —
        run on the raw [x, u] and mbpo_ens_calibrate picks, per state dimension, the factor of `alphas` (default: 61 values from 0.1 to
        100) whose intervals' coverage at the n_levels equispaced levels is closest to nominal (include/mbpo_hip.h "N3d").  The
        existing tensor is rewritten in place.  Nothing is read back.  Returns dynamics_params (return_counts: also best_idx and
        counts [x, A, P])."""
        cal, best, counts, _ = self._calibration_call(dynamics_params, rows, idx, next_obs_off, predict_delta, alphas, n_levels, None)
        old = dynamics_params.calibration
        if old is not None and old.shape == cal.shape and old.device == cal.device and old.dtype == cal.dtype:
            old.copy_(cal)                       # in place: a system that caches beta * calibration sees the tensor's version change
        else:
            dynamics_params.calibration = cal
        return (dynamics_params, best, counts) if return_counts else dynamics_params

    def coverage(self, dynamics_params: EnsembleDynamicsParams, rows: torch.Tensor, idx: Optional[torch.Tensor] = None,
                 next_obs_off: Optional[int] = None, predict_delta: bool = True, n_levels: int = 19,
                 calibrated: bool = True) -> torch.Tensor:
        """[x_dim, n_levels] float: the fraction of rows[idx] whose true next state lies inside the interval of level p_j =
        j / (n_levels + 1) around the members' mean, per state dimension — nominal coverage is p_j.  calibrated: the intervals are
        scaled by dynamics_params.calibration when one is set (else, or with False, the raw spread).  The same kernel as `calibrate`,
        at the single factor 1."""
        scale = dynamics_params.calibration if calibrated else None
        if scale is not None:
            scale = scale.to(self.device, torch.float32).contiguous()
        _, _, counts, n = self._calibration_call(dynamics_params, rows, idx, next_obs_off, predict_delta, [1.0], n_levels, scale)
        return counts[:, 0, :].to(torch.float32) / n

    def member_outputs(self, x: torch.Tensor, u: torch.Tensor, dynamics_params: EnsembleDynamicsParams,
                       elites: bool = False) -> torch.Tensor:
        """[E, N, 2*x_dim] raw member outputs (+ [mu_r, raw_r] with learn_reward) — mbpo_ensemble_mlp_forward.  All members, also
        when elites are selected; elites=True: the members the rollouts use ([n_elites, N, ...] when selected).  x, u are RAW: with a
        scaler the folded members run."""
        xu = torch.cat([x.reshape(-1, self.x_dim), u.reshape(-1, self.u_dim)], dim=1).to(self.device, torch.float32).contiguous()
        params, spec = self._rollout_members(dynamics_params) if elites else (self._consumer_params(dynamics_params), self.spec)
        return ops.ensemble_mlp_forward(params, spec, xu)

    def next_state(self, x, u, dynamics_params, predict_delta: bool = True, min_std: float = 1e-3):
        """Mixture moments over members (the elites when selected): mean = E_e[mu_e], std = sqrt(E_e[sigma_e^2] + Var_e[mu_e]); with a
        calibration set, std = sqrt(E_e[sigma_e^2] + calibration^2 Var_e[mu_e])."""
        y = self.member_outputs(x, u, dynamics_params, elites=True)
        X = self.x_dim
        mu = y[..., :X] + (x.reshape(-1, X) if predict_delta else 0.0)
        sig = torch.nn.functional.softplus(y[..., X:2 * X]) + min_std
        mean = mu.mean(dim=0)
        var_mu = mu.var(dim=0, unbiased=False)
        if dynamics_params.calibration is not None:
            var_mu = dynamics_params.calibration.to(var_mu.device, torch.float32) ** 2 * var_mu
        std = torch.sqrt((sig ** 2).mean(dim=0) + var_mu)
        if x.dim() == 1:
            mean, std = mean[0], std[0]
        return Normal(mean, std), dynamics_params

    def reward(self, x, u, dynamics_params, min_std: float = 1e-3) -> Normal:
        """The reward head's mixture moments over members (the elites when selected) at (x, u): mean = E_e[mu_r,e],
        std = sqrt(E_e[sigma_r,e^2] + Var_e[mu_r,e])."""
        if not self.learn_reward:
            raise ValueError("this ensemble has no reward head (EnsembleDynamics(learn_reward=True))")
        y = self.member_outputs(x, u, dynamics_params, elites=True)
        X = self.x_dim
        mu = y[..., 2 * X]
        sig = torch.nn.functional.softplus(y[..., 2 * X + 1]) + min_std
        mean = mu.mean(dim=0)
        std = torch.sqrt((sig ** 2).mean(dim=0) + mu.var(dim=0, unbiased=False))
        if x.dim() == 1:
            mean, std = mean[0], std[0]
        return Normal(mean, std)


class LearnedReward(Reward[EnsembleDynamicsParams]):
    """The reward an EnsembleDynamics(learn_reward=True) predicts (MBPO_REWARD_LEARNED): its parameters ARE the dynamics'
    (EnsembleSystem.init_params binds the same EnsembleDynamicsParams object to both, so fit's in-place updates reach both).
    min_std (the floor of the reported std): None takes the EnsembleSystem's own min_std when the reward is bound to one, 1e-3 alone."""

    def __init__(self, dynamics: EnsembleDynamics, min_std: Optional[float] = None):
        if not isinstance(dynamics, EnsembleDynamics) or not dynamics.learn_reward:
            raise ValueError("LearnedReward needs an EnsembleDynamics(learn_reward=True)")
        super().__init__(dynamics.x_dim, dynamics.u_dim)
        self.dynamics, self.min_std = dynamics, min_std

    def init_params(self, key: int) -> EnsembleDynamicsParams:
        return self.dynamics.init_params(key)

    def kernel_spec(self, reward_params, device):
        return _hip.REWARD_LEARNED, None        # the kernels read the reward head of the dynamics' own parameters

    def __call__(self, x, u, reward_params, x_next=None):
        """Host evaluation: Normal(mean_e mu_r,e, mixture std) — the mean is what System.step returns in 'mean' mode."""
        return self.dynamics.reward(x, u, reward_params, 1e-3 if self.min_std is None else self.min_std), reward_params


class EnsembleSystem(System):
    """termination: a BoxTermination on the next state (mbpo/systems/termination.py) — the model episodes of the SAC / PPO trainers
    and of the evaluators then end where the box is left or the state stops being finite (discount 0, truncation 0, reset to the
    env's first obs), and `step` reports SystemState.done.  iCEM, BPTT and rollout_actions / rollout_policy IGNORE it, as the
    reference's scans ignore SystemState.done (utils/optimizer_utils.py:31-47, 85-93): their trajectories run on through the box.

    mode='optimistic' (hallucinated control): two widths exist.  u_dim stays what the dynamics and the true buffer see; action_dim =
    u_dim + x_dim is what the policy emits, the model's rows carry and SAC's critics see: an action is [u | eta] and the next state is
    mean + beta * std_over_members * eta.  beta: a float or a length-x_dim sequence / tensor.  env_action(a) cuts the controls out
    for the true system.  The reward is unchanged (eta never enters it).  Out of scope and refused: BPTT (the gradient through the
    spread is not built), SAC's real_ratio > 0 (real rows carry u_dim action columns, model rows action_dim), members wider than 256.
    calibrated=True (optimistic only): the kernels get halluc_beta = beta * dynamics_params.calibration, one fp32 multiply on the
    device into a buffer the system keeps, refreshed when the calibration tensor or its contents change; `beta` stays the user's
    value.  rollout_spec refuses parameters without a calibration (run `calibrate` or `fit(calibrate=True)` first).

    time_adaptive (a TimeAdaptive; every mode but 'optimistic'): action_dim = u_dim + 1, an action is [u | tau] and the fused rollouts
    hold u for k(tau) steps of the members (mbpo/systems/time_adaptive.py).  The members stay a model of one env_dt, fitted on
    base-rate transitions with u_dim action columns as before."""

    def __init__(self, dynamics: EnsembleDynamics, reward: Reward, mode: str = "mean", predict_delta: bool = True,
                 sample_noise: bool = False, min_std: float = 1e-3, termination: Optional[BoxTermination] = None, beta=1.0,
                 calibrated: bool = False, time_adaptive=None):
        if time_adaptive is not None and mode == "optimistic":
            raise ValueError("time_adaptive together with mode='optimistic' is not built: the action would be [u | eta | tau] and no "
                             "rollout kernel holds a hallucinated control")
        if time_adaptive is not None and dynamics.kernel_width is None:
            raise ValueError("time_adaptive runs inside the fused rollout kernels, which take members up to 256 wide")
        super().__init__(dynamics=dynamics, reward=reward, time_adaptive=time_adaptive)
        if termination is not None and termination.x_dim != dynamics.x_dim:
            raise ValueError(f"the termination has {termination.x_dim} dimensions, the system {dynamics.x_dim}")
        self.termination = termination
        if mode not in _MODES:
            raise ValueError(f"mode must be one of {sorted(_MODES)}")
        if isinstance(reward, LearnedReward):
            if reward.dynamics is not dynamics or not dynamics.learn_reward:
                raise ValueError("a LearnedReward must wrap this system's own EnsembleDynamics(learn_reward=True)")
            if reward.min_std is None:
                reward.min_std = min_std                   # one std floor for the state and the reward heads
            elif reward.min_std != min_std:
                raise ValueError(f"LearnedReward.min_std {reward.min_std} differs from the system's min_std {min_std}")
        self.mode, self.predict_delta, self.sample_noise, self.min_std = mode, predict_delta, sample_noise, min_std
        self.optimistic = mode == "optimistic"
        self.calibrated = bool(calibrated)
        if self.calibrated and not self.optimistic:
            raise ValueError("calibrated=True scales the hallucinated control's beta: it needs mode='optimistic'")
        self.beta = None
        if self.optimistic:
            if dynamics.kernel_width is None:
                raise ValueError("mode='optimistic' runs inside the fused rollout kernels, which take members up to 256 wide")
            b = torch.as_tensor(beta, dtype=torch.float32).detach().cpu().reshape(-1)
            if b.numel() == 1:
                b = b.expand(dynamics.x_dim)
            if b.numel() != dynamics.x_dim:
                raise ValueError(f"beta must be a float or hold x_dim = {dynamics.x_dim} values, got {b.numel()}")
            self.beta = b.clone()
            self._beta_dev = {}
            self._beta_cal = {}                  # device -> [buffer of beta * calibration, (calibration's data_ptr, version)]

    @property
    def action_dim(self) -> int:
        return self.u_dim + self.x_dim if self.optimistic else super().action_dim

    def _halluc_beta(self, device) -> torch.Tensor:
        """beta as a device tensor, cached per device: nothing is copied host to device inside a captured graph."""
        k = str(device)
        if k not in self._beta_dev:
            self._beta_dev[k] = self.beta.to(device).contiguous()
        return self._beta_dev[k]

    def _calibrated_beta(self, device, dynamics_params) -> torch.Tensor:
        """beta * calibration in a buffer that lives as long as the system (one per device: the pointer a captured step holds stays
        valid), multiplied again only when the calibration is another tensor or was written to since."""
        cal = dynamics_params.calibration.to(device, torch.float32)
        if cal.numel() != self.x_dim:
            raise ValueError(f"the calibration must hold x_dim = {self.x_dim} values, got {cal.numel()}")
        k, tag = str(device), (cal.data_ptr(), cal._version)
        if k not in self._beta_cal:
            self._beta_cal[k] = [torch.empty(self.x_dim, device=device, dtype=torch.float32), None]
        slot = self._beta_cal[k]
        if slot[1] != tag:
            torch.mul(self._halluc_beta(device), cal.reshape(-1), out=slot[0])
            slot[1] = tag
        return slot[0]

    def init_params(self, key: int) -> SystemParams:
        if not isinstance(self.reward, LearnedReward):
            return super().init_params(key)
        keys = K.split(key, 3)                                     # System.init_params's split: the same dynamics parameters
        dp = self.dynamics.init_params(keys[0])
        return SystemParams(dynamics_params=dp, reward_params=dp, key=keys[2])      # one parameter object: fit updates both

    def rollout_spec(self, system_params: SystemParams, device) -> dict:
        from mbpo.systems.plan_reward import refuse_plan_reward
        refuse_plan_reward(system_params, "EnsembleSystem.rollout_spec")      # (only iCEM consumes one, and takes it out first)
        rp = system_params.reward_params
        if self.calibrated and system_params.dynamics_params.calibration is None:      # (refused before anything touches the device)
            raise ValueError("calibrated=True but these dynamics parameters have no calibration: run EnsembleDynamics.calibrate "
                             "(or fit(..., calibrate=True)) first")
        # (the learned reward has no parameter vector: its params hold a device tensor, whose repr would copy it to the host)
        # (the termination's device tensors are cached per device by BoxTermination.kernel_spec itself; its key here only makes the
        # spec's cache key change with the bounds)
        ck = ("learned" if isinstance(self.reward, LearnedReward) else repr(rp), str(device),
              None if self.termination is None else self.termination.key)
        if getattr(self, "_rspec_key", None) != ck:    # cached: no H2D copy inside a captured graph
            self._rspec = self.reward.kernel_spec(rp, device)
            self._rspec_key = ck
        kind, rvec = self._rspec
        # the elites, when selected, ARE the ensemble the kernels see (every consumer takes E from dyn_spec.n_nets)
        dyn_params, dyn_spec = self.dynamics._rollout_members(system_params.dynamics_params)
        return dict(system_kind=_hip.SYS_ENSEMBLE, dyn_params=dyn_params, dyn_spec=dyn_spec,
                    ens_mode=_MODES[self.mode], ens_predict_delta=self.predict_delta, ens_sample_noise=self.sample_noise,
                    ens_min_std=self.min_std, reward_kind=kind, reward_params=rvec,
                    **({"halluc_beta": self._calibrated_beta(device, system_params.dynamics_params) if self.calibrated
                        else self._halluc_beta(device)} if self.optimistic else {}),
                    **({} if self.time_adaptive is None else self.time_adaptive.kernel_spec()),
                    **termination_spec(self.termination, self.x_dim, device))
