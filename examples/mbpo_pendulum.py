#!/usr/bin/env python
"""End-to-end MBPO on the Pendulum with every stage on the MI355X path:

    true transitions  ->  EnsembleDynamics.fit (N3, mbpo_ens_nll_grads + mbpo_adamw_step)
                      ->  SACOptimizer on EnsembleSystem (short model rollouts branched from true states + SAC updates)
                      ->  the policy acts on the TRUE PendulumSystem.

    python examples/mbpo_pendulum.py [--iters 2 --model-steps 1500 --sac-steps 40000] [--learn-reward] [--elites] [--terminate-speed V] [--term-reward]
                                     [--real-ratio R] [--normalize-inputs] [--resample-starts] [--optimistic BETA] [--calibrate]
                                     [--warm-start [--retain-buffer]] [--time-adaptive TMIN TMAX [--switch-cost C]]

--learn-reward: the ensemble also learns the reward from the true transitions (EnsembleDynamics(learn_reward=True) + LearnedReward),
so the model rollouts never see the Pendulum's reward formula.
--elites: MBPO's model selection — 7 members, a 20 % holdout, per-member early stopping with --model-steps as the cap, and rollouts
through the 5 members of lowest held-out error (fit(holdout_ratio=0.2, n_elites=5)).
--terminate-speed V: the MODEL system (not the true one) gets a termination function, BoxTermination on |thetadot| <= V: a model episode
ends where the predicted speed leaves the interval (discount 0, truncation 0, restart from the env's first state).  After every SAC
epoch the share of the last collection's model transitions that ended this way is printed.
--real-ratio R: MBPO's mixed minibatches — int(batch_size * R) rows of every SAC minibatch are true transitions from the environment
buffer, the others model transitions (SACOptimizer(real_ratio=R); MBPO's published runs use 0.05).  0, the default, trains on model
transitions only.
--normalize-inputs: MBPO's input scaler — fit(normalize_inputs=True) standardises the members' inputs [x, u] with the training rows'
mean / std; the rollouts run the members with the scaler folded into their first layer.
--resample-starts: MBPO's branched rollouts — SACOptimizer(resample_starts=True): every reset inside the fused model rollout is followed
by a fresh draw from the true buffer, so an env's consecutive model episodes start at different real states instead of the one state
its first reset chose.
--optimistic BETA: hallucinated control (optimistic exploration in the style of H-UCRL) — the MODEL system becomes
EnsembleSystem(mode="optimistic", beta=BETA): the policy emits [u | eta] and the model's next state is the members' mean moved by
beta * (std over members) * eta, anywhere inside the ensemble's confidence set; on the TRUE system only the controls act
(model.env_action).  Not with --real-ratio (real rows have no eta columns).  No learning curve is claimed for it.
--calibrate: the spread of the members is calibrated on the fit's held-out rows (fit(holdout_ratio=0.2, calibrate=True): one factor per
state dimension, EnsembleDynamics.calibrate); with --optimistic the model system is built with calibrated=True, so the policy moves
the state inside mean +- BETA * calibration * std.  Every iteration prints the calibration vector and the coverage of the intervals at
the 0.5 and 0.9 levels, before and after calibration, on the held-out rows and on 2000 fresh transitions.  No learning curve is claimed.
--warm-start: MBPO's outer loop continues its learner — ONE SACOptimizer(warm_start=True) for all iterations, and the learner state
(policy, critics, target critics, log_alpha, Adam moments and step count, observation normaliser) of one iteration's `train` is handed to
the next in BraxState.learner_state, instead of SAC starting from a fresh initialisation after every model refit.  The optimizer keeps
its trainer between the calls.  --retain-buffer: the model replay buffer is carried too (retain_replay_buffer=True), so an iteration
starts on the previous iterations' model transitions and prefills nothing.  Every iteration prints its true_return.  Not with
--terminate-speed (its reporting builds a trainer of its own).
--time-adaptive TMIN TMAX: the policy also chooses how long its torque is held — the MODEL system is built with
TimeAdaptive(TMIN, TMAX, env_dt = the Pendulum's dt, switch_cost=C): the policy emits [u | tau], the fused rollouts hold u for k(tau)
steps of the learned model, sum the rewards of the hold discounted by 0.99 per step and charge C per decision; SAC gets the matching
non_equidistant_time options, so its target discounts every row by the time the row was held.  On the TRUE system an action is applied
for model.hold_steps(a) steps (the kernels' own k); every iteration also reports the mean hold of that evaluation.  Not with
--optimistic or --real-ratio.  No learning curve is claimed for it.
--term-reward: the MODEL's reward is a TermReward written as data instead of the Pendulum's formula — on the observation
(cos th, sin th, thdot): -(cos th - 1)^2 - sin^2 th - 0.1 thdot^2 - 0.02 u^2 plus the tolerance bonus
exp(-4 ((cos th - 1)^2 + sin^2 th)) around upright, evaluated inside the fused rollouts.  The true system keeps the Pendulum's own
reward, which is what the evaluation reports.  Not with --learn-reward.  No learning curve is claimed for it.
"""
from __future__ import annotations

import argparse
import math
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "model-based-policy-optimizers_amd"))

import torch  # noqa: E402


def collect_uniform(system, n, gen, dev):
    """n true transitions from states / actions drawn uniformly over the Pendulum's range (full state coverage)."""
    th = (torch.rand(n, generator=gen) * 2 - 1) * math.pi
    x = torch.stack([torch.cos(th), torch.sin(th), (torch.rand(n, generator=gen) * 2 - 1) * 8], 1).to(dev)
    u = (torch.rand(n, 1, generator=gen) * 2 - 1).to(dev)
    nxt = system.step(x, u, system.reset().system_params)
    return x, u, nxt.reward, nxt.x_next


def true_return(system, optimizer, opt_state, steps=200, env_action=lambda a: a, hold_steps=None, holds=None):
    """env_action: the controls of a policy action (System.env_action: an optimistic model's policy also emits eta, a time-adaptive
    one tau).  hold_steps (a time-adaptive model's System.hold_steps): every action is applied for hold_steps(a) true steps, `steps`
    true steps in all; the holds taken are appended to `holds`."""
    start = system.reset()
    x, total, true_params = start.x_next, 0.0, start.system_params      # the TRUE system's own parameters
    t = 0
    while t < steps:
        u, opt_state = optimizer.act(x, opt_state, evaluate=True)
        k = 1 if hold_steps is None else min(int(hold_steps(u.reshape(1, -1))[0]), steps - t)
        if holds is not None:
            holds.append(k)
        for _ in range(k):
            nxt = system.step(x, env_action(u), true_params)
            x, total = nxt.x_next, total + float(nxt.reward)
        t += k
    return total


def train_reporting_terminations(optimizer, opt_state, verbose=True):
    """SACOptimizer.train (a new trainer per call) with a progress_fn: after every epoch, the share of the last collection's model
    transitions with discount == 0 and truncation == 0 — the ones the termination function ended.  Returns (output, shares).
    KEEP IN STEP with BraxOptimizer.train (mbpo/optimizers/policy_optimizers/brax_optimizers.py), whose body this repeats because the
    progress_fn needs the trainer: the rows of its last collection are the trainer's `_rollout_rows` (what tests/ read too)."""
    from mbpo.optimizers.policy_optimizers.brax_optimizers import BraxOutput
    from mbpo.systems.brax_wrapper import BraxWrapper
    from mbpo.utils import keys as K
    env = BraxWrapper(system=optimizer.system, system_params=opt_state.system_params, sample_buffer_state=opt_state.true_buffer_state,
                      sample_buffer=optimizer.true_buffer)
    trainer = optimizer.agent_class(environment=env, **optimizer.agent_kwargs)
    X, U = optimizer.system.x_dim, optimizer.system.action_dim      # (the model rows' action width)
    shares = []

    def progress(env_steps, metrics):
        if env_steps == 0:
            return
        rows = trainer._rollout_rows                  # the last get_experience's rows: [..., reward, discount, next_obs, truncation]
        shares.append(float(((rows[:, X + U + 1] == 0) & (rows[:, -1] == 0)).float().mean()))
        if verbose:
            print(f"  env_steps {env_steps}: {100 * shares[-1]:.1f} % of the model transitions terminated", flush=True)

    key, new_key = K.split(opt_state.key)
    try:
        policy_params, metrics = trainer.run_training(key=new_key, progress_fn=progress)
    finally:
        trainer.close()
    return BraxOutput(optimizer_state=opt_state.replace(policy_params=policy_params, key=new_key), summary=metrics), shares


def calibration_report(dyn, dyn_params, rows, n_rows, fit_key, true_system, dev, verbose=True, n_fresh=2000):
    """The calibration vector and the coverage at the 0.5 and 0.9 levels (of 19), raw spread and calibrated, on the rows `fit` held
    out (the same Philox permutation) and on n_fresh transitions the model has never seen."""
    from mbpo import ops
    from mbpo.systems.ensemble_system import FIT_SITE_HOLDOUT
    from mbpo.utils import keys as K
    n_hold = min(5000, int(math.floor(0.2 * n_rows)))
    hold = ops.philox_permutation(n_rows, seed=K.PRNGKey(fit_key), offset=FIT_SITE_HOLDOUT << 32)[:n_hold].contiguous()
    x, u, r, xn = collect_uniform(true_system, n_fresh, torch.Generator().manual_seed(fit_key + 12345), dev)
    fresh = torch.cat([x, u, r[:, None], torch.ones(n_fresh, 1, device=dev), xn], 1).contiguous()
    out = dict(calibration=[round(float(v), 4) for v in dyn_params.calibration])
    levels = (9, 17)                                  # p = 10 / 20 and 18 / 20 of the 19 equispaced levels
    for name, data, idx in (("holdout", rows, hold), ("fresh", fresh, None)):
        for tag, flag in (("before", False), ("after", True)):
            cov = dyn.coverage(dyn_params, data, idx=idx, calibrated=flag)[:, levels]
            out[f"coverage_{name}_{tag}"] = [[round(float(v), 4) for v in row] for row in cov]
    if verbose:
        print(f"  calibration {out['calibration']}; coverage at levels (0.5, 0.9) per state dimension:", flush=True)
        for name in ("holdout", "fresh"):
            print(f"    {name:8s} before {out[f'coverage_{name}_before']}  after {out[f'coverage_{name}_after']}", flush=True)
    return out


def run(iters=2, n_true=4000, model_steps=1500, sac_steps=40_000, seed=0, verbose=True, learn_reward=False, elites=False,
        terminate_speed=None, real_ratio=0.0, normalize_inputs=False, resample_starts=False, optimistic=None, calibrate=False,
        warm_start=False, retain_buffer=False, time_adaptive=None, switch_cost=0.0, term_reward=False):
    from mbpo.optimizers import SACOptimizer
    from mbpo.replay import UniformSamplingQueue
    from mbpo.systems import (BoxTermination, EnsembleDynamics, EnsembleSystem, LearnedReward, PendulumReward, PendulumSystem,
                              TimeAdaptive, Group, Term, TermReward)
    from mbpo.systems.dynamics.pendulum_dynamics import PendulumDynamicsParams
    from mbpo.types import Transition
    if time_adaptive is not None and (optimistic is not None or real_ratio > 0):
        raise ValueError("--time-adaptive is not combined with --optimistic or --real-ratio")
    ta = None
    if time_adaptive is not None:      # one model step is one step of the true Pendulum; 0.99 per step, as SAC's discounting below
        dt = PendulumDynamicsParams().dt
        ta = TimeAdaptive(time_adaptive[0], time_adaptive[1], dt, switch_cost=switch_cost, continuous_discounting=-math.log(0.99) / dt)
    if warm_start and terminate_speed is not None:
        raise ValueError("--warm-start is not combined with --terminate-speed here: train_reporting_terminations builds its own trainer")
    if retain_buffer and not warm_start:
        raise ValueError("--retain-buffer needs --warm-start")
    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator().manual_seed(seed)
    true_system = PendulumSystem()
    s0 = true_system.reset()
    dummy = Transition(observation=s0.x_next, action=torch.zeros(1, device=dev), reward=s0.reward,
                       discount=torch.tensor(0.99, device=dev), next_observation=s0.x_next)
    true_buffer = UniformSamplingQueue(max_replay_size=iters * n_true, dummy_data_sample=dummy, sample_batch_size=1, device=dev)
    tbs = true_buffer.init(seed)
    dyn = EnsembleDynamics(3, 1, n_members=7 if elites else 5, learn_reward=learn_reward)
    termination = None if terminate_speed is None else BoxTermination.from_intervals(3, {2: (-terminate_speed, terminate_speed)})
    if term_reward and learn_reward:
        raise ValueError("--term-reward is not combined with --learn-reward")
    upright = [Term("x", 0, "square", 1.0, 1.0), Term("x", 1, "square", 1.0)]          # (cos th - 1)^2 + sin^2 th
    known = TermReward(3, 1, groups=[Group(upright + [Term("x", 2, "square", 0.1), Term("u", 0, "square", 0.02)], weight=-1.0),
                                     Group([Term("x", 0, "square", -4.0, 1.0), Term("x", 1, "square", -4.0)], link="exp")])
    reward = known if term_reward else (LearnedReward(dyn) if learn_reward else PendulumReward())
    model = EnsembleSystem(dyn, reward, predict_delta=True, termination=termination,
                           time_adaptive=ta,
                           **(dict(mode="mean") if optimistic is None else dict(mode="optimistic", beta=optimistic, calibrated=calibrate)))
    dyn_params = dyn.init_params(seed + 1)
    history = []
    optimizer, learner_state = None, None      # --warm-start: one optimizer, and the learner handed from iteration to iteration
    for it in range(iters):
        t0 = time.time()
        x, u, r, xn = collect_uniform(true_system, n_true, gen, dev)
        tbs = true_buffer.insert(tbs, Transition(observation=x, action=u, reward=r, discount=torch.ones(n_true, device=dev), next_observation=xn))
        n_rows = true_buffer.size(tbs)
        fit_kw = dict(holdout_ratio=0.2, n_elites=5) if elites else {}
        if calibrate:
            fit_kw.update(holdout_ratio=0.2, calibrate=True)
        dyn_params, losses = dyn.fit(dyn_params, true_buffer.logical_data(tbs), num_steps=model_steps, batch_size=256, learning_rate=3e-3,
                                     key=seed + 10 * it, n_rows=n_rows, normalize_inputs=normalize_inputs, **fit_kw)
        coverage = calibration_report(dyn, dyn_params, true_buffer.logical_data(tbs), n_rows, seed + 10 * it, true_system, dev,
                                      verbose) if calibrate else None
        if optimizer is None or not warm_start:
            optimizer = SACOptimizer(system=model, true_buffer=true_buffer, num_timesteps=sac_steps, num_evals=2, reward_scaling=1,
                                     episode_length=10, episode_length_eval=10, normalize_observations=True, action_repeat=1,
                                     discounting=0.99, lr_policy=3e-4, lr_alpha=3e-4, lr_q=3e-4, num_envs=64, batch_size=128,
                                     grad_updates_per_step=64, max_replay_size=2 ** 15, min_replay_size=2 ** 9, num_eval_envs=16,
                                     deterministic_eval=True, tau=0.005, num_env_steps_between_updates=5, real_ratio=real_ratio,
                                     **(dict(resample_starts=True) if resample_starts else {}),
                                     **({} if ta is None else ta.trainer_kwargs()),
                                     **(dict(warm_start=True, retain_replay_buffer=retain_buffer) if warm_start else {}))
        state = optimizer.init(key=seed + 3, true_buffer_state=tbs)
        sp = state.system_params.replace(dynamics_params=dyn_params)
        if learn_reward:
            sp = sp.replace(reward_params=dyn_params)      # the learned reward's parameters are the model's
        state = state.replace(system_params=sp)
        if warm_start:
            state = state.replace(learner_state=learner_state)      # None in the first iteration: a fresh initialisation
        if termination is None:
            out, shares = optimizer.train(opt_state=state), None
        else:
            out, shares = train_reporting_terminations(optimizer, state, verbose)
        learner_state = out.optimizer_state.learner_state
        holds = []
        ret = true_return(true_system, optimizer, out.optimizer_state, env_action=model.env_action,
                          hold_steps=None if ta is None else model.hold_steps, holds=holds)
        history.append(dict(iteration=it, true_transitions=n_rows, model_nll=float(losses[-20:].mean()), true_return=ret,
                            seconds=time.time() - t0))
        if elites:
            history[-1].update(steps_run=int(losses.shape[0]), elite_idx=dyn_params.elite_idx.tolist(),
                               holdout_mse=[round(float(v), 6) for v in dyn_params.holdout[1]])
        if shares is not None:
            history[-1].update(terminated_share=[round(s, 4) for s in shares])
        if coverage is not None:
            history[-1].update(coverage)
        if ta is not None:
            history[-1].update(mean_hold=sum(holds) / len(holds), max_hold=ta.max_steps)
        if verbose:
            print(history[-1], flush=True)
            if warm_start:
                print(f"iteration {it}: true_return {ret:.1f} (SAC optimizer steps so far: {int(learner_state.step_count)})", flush=True)
    if warm_start:
        optimizer.close()
    return history


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--model-steps", type=int, default=1500)
    ap.add_argument("--sac-steps", type=int, default=40_000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--learn-reward", action="store_true")
    ap.add_argument("--elites", action="store_true")
    ap.add_argument("--terminate-speed", type=float, default=None, metavar="V",
                    help="end a MODEL episode where the predicted |thetadot| exceeds V (BoxTermination on the model system only)")
    ap.add_argument("--real-ratio", type=float, default=0.0, metavar="R",
                    help="share of true transitions in every SAC minibatch (MBPO's real_ratio; 0 = model transitions only)")
    ap.add_argument("--normalize-inputs", action="store_true",
                    help="standardise the model's inputs with the training rows' mean / std (MBPO's input scaler)")
    ap.add_argument("--resample-starts", action="store_true",
                    help="after every reset inside the model rollouts draw the env's next start state from the true buffer (MBPO's "
                         "branched rollouts) instead of returning to the same state every time")
    ap.add_argument("--calibrate", action="store_true",
                    help="calibrate the members' spread on the fit's held-out rows and report the coverage before and after; with "
                         "--optimistic the model system uses beta * calibration")
    ap.add_argument("--optimistic", type=float, default=None, metavar="BETA",
                    help="hallucinated control: the policy also picks the model's next state inside mean +- BETA * (std over members)")
    ap.add_argument("--warm-start", action="store_true",
                    help="one SACOptimizer(warm_start=True) for all iterations: every iteration continues the previous one's learner")
    ap.add_argument("--retain-buffer", action="store_true",
                    help="with --warm-start: carry the model replay buffer from iteration to iteration too")
    ap.add_argument("--time-adaptive", type=float, nargs=2, default=None, metavar=("TMIN", "TMAX"),
                    help="the policy also chooses how long its torque is held, between TMIN and TMAX seconds (multiples of the Pendulum's dt)")
    ap.add_argument("--switch-cost", type=float, default=0.0, metavar="C", help="with --time-adaptive: charged once per decision")
    ap.add_argument("--term-reward", action="store_true",
                    help="the model's reward is a TermReward (a quadratic cost on (cos th, sin th, thdot, u) plus an exp tolerance bonus)")
    a = ap.parse_args()
    run(a.iters, model_steps=a.model_steps, sac_steps=a.sac_steps, seed=a.seed, learn_reward=a.learn_reward, elites=a.elites,
        terminate_speed=a.terminate_speed, real_ratio=a.real_ratio, normalize_inputs=a.normalize_inputs,
        resample_starts=a.resample_starts, optimistic=a.optimistic, calibrate=a.calibrate, warm_start=a.warm_start,
        retain_buffer=a.retain_buffer, time_adaptive=a.time_adaptive, switch_cost=a.switch_cost, term_reward=a.term_reward)
