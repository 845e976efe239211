"""TimeAdaptive — the policy also chooses how long its control is held (include/mbpo_hip.h, "time-adaptive rollouts").

The environment side of the trainers' non_equidistant_time options (sac/losses.py:90-96, ppo/losses_new.py:105-112 carry the loss
side): on a system built with `time_adaptive=TimeAdaptive(...)` the policy emits [u | tau], the fused rollout holds u for
    t = (t_hi - t_lo) / 2 * tau + (t_hi + t_lo) / 2,   k = clamp(floor_divide(t, env_dt), 1, max_steps)
steps of the (learned or Pendulum) model inside one launch, sums the rewards of the hold with weights
exp(-continuous_discounting * env_dt)^j, charges switch_cost once, and hands SAC / PPO a row whose time is the one their discount
exp(-continuous_discounting * floor_divide(t, env_dt) * env_dt) assumes.  The model stays a model of one env_dt; only the decision
rate becomes the policy's.  Not in the reference tree (its wrapper lives elsewhere): the header is the definition.

Under non_equidistant_time=False the trainers discount every decision by their constant `discounting`, however long it was held:
legal, and a different objective.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

MAX_HOLD_STEPS = 64          # the kernels' bound on K (include/mbpo_hip.h)
_F32 = np.float32


def _round_f32(v: Fraction) -> np.float32:
    """v rounded once to fp32, to nearest even — what one fused multiply-add leaves."""
    f = _F32(float(v))
    best = None
    for c in (np.nextafter(f, _F32(-np.inf)), f, np.nextafter(f, _F32(np.inf))):
        if not np.isfinite(c):
            continue
        err = abs(Fraction(float(c)) - v)
        even = (int(np.array(c, dtype=_F32).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even and not best[2]):
            best = (err, c, even)
    return best[1]


def floor_divide_f32(x1, x2) -> np.float32:
    """jnp.floor_divide on fp32, as csrc/common.hpp's floor_divide_f states it."""
    x1, x2 = _F32(x1), _F32(x2)
    mod = _F32(math.fmod(float(x1), float(x2)))          # fmodf is exact
    div = _F32(_F32(x1 - mod) / x2)
    if mod != 0 and ((x2 < 0) != (mod < 0)):
        div = _F32(div - _F32(1))
    return _F32(math.copysign(math.floor(abs(float(div)) + 0.5), float(div)))      # roundf: halves away from zero


def hold_steps_f32(tau, t_lo, t_hi, env_dt, max_steps=None) -> int:
    """The k of csrc/common.hpp's hold_steps for one tau, restated in fp32 on the host (max_steps None: no upper clamp)."""
    tau, t_lo, t_hi = _F32(tau), _F32(t_lo), _F32(t_hi)
    a, c = _F32(_F32(t_hi - t_lo) / _F32(2)), _F32(_F32(t_hi + t_lo) / _F32(2))
    t = _round_f32(Fraction(float(a)) * Fraction(float(tau)) + Fraction(float(c)))
    k = max(int(floor_divide_f32(t, env_dt)), 1)
    return k if max_steps is None else min(k, int(max_steps))


@dataclass(frozen=True)
class TimeAdaptive:
    """min_time_between_switches / max_time_between_switches / env_dt / continuous_discounting: the values the trainer's
    non_equidistant_time options of the same names must carry.  switch_cost >= 0 is charged once per decision.
    max_steps (K): the hold of tau = 1, by the fp32 restatement above — the kernels' loop bound and the stride of their random
    numbers.  gamma: exp(-continuous_discounting * env_dt), formed in float64 and rounded once to fp32."""
    min_time_between_switches: float
    max_time_between_switches: float
    env_dt: float
    switch_cost: float = 0.0
    continuous_discounting: float = 0.0

    def __post_init__(self):
        lo, hi, dt = float(self.min_time_between_switches), float(self.max_time_between_switches), float(self.env_dt)
        if not (0.0 < dt <= lo <= hi) or not math.isfinite(hi):
            raise ValueError(f"TimeAdaptive needs 0 < env_dt <= min_time_between_switches <= max_time_between_switches, got "
                             f"env_dt={dt}, min_time_between_switches={lo}, max_time_between_switches={hi}")
        if not self.switch_cost >= 0.0:
            raise ValueError(f"switch_cost must be >= 0, got {self.switch_cost}")
        if not self.continuous_discounting >= 0.0:
            raise ValueError(f"continuous_discounting must be >= 0, got {self.continuous_discounting}")
        k = hold_steps_f32(1.0, lo, hi, dt)
        if k > MAX_HOLD_STEPS:
            raise ValueError(f"max_time_between_switches={hi} is {k} steps of env_dt={dt}; the fused rollouts hold for at most "
                             f"{MAX_HOLD_STEPS}")
        object.__setattr__(self, "max_steps", k)

    @property
    def gamma(self) -> float:
        return float(_F32(math.exp(-float(self.continuous_discounting) * float(self.env_dt))))

    def kernel_spec(self) -> dict:
        """The hold_* keywords of ops.model_rollout."""
        return dict(hold_max_steps=self.max_steps, hold_min_time=float(self.min_time_between_switches),
                    hold_max_time=float(self.max_time_between_switches), hold_dt=float(self.env_dt), hold_gamma=self.gamma,
                    hold_switch_cost=float(self.switch_cost))

    def trainer_kwargs(self) -> dict:
        """The matching non_equidistant_time options of SAC / PPO."""
        return dict(non_equidistant_time=True, continuous_discounting=self.continuous_discounting,
                    min_time_between_switches=self.min_time_between_switches,
                    max_time_between_switches=self.max_time_between_switches, env_dt=self.env_dt)


def check_trainer(system, who: str, *, action_repeat: int, non_equidistant_time: bool, continuous_discounting: float,
                  min_time_between_switches: float, max_time_between_switches: float, env_dt: float, real_ratio: float = 0.0) -> None:
    """What SAC / PPO refuse on a time-adaptive system, before anything touches a device."""
    ta = getattr(system, "time_adaptive", None)
    if ta is None:
        return
    if action_repeat != 1:
        raise ValueError(f"{who}: action_repeat={action_repeat} on a time-adaptive system: the hold is the repeat, and the policy "
                         "chooses it; use action_repeat=1")
    if real_ratio > 0:
        raise ValueError(f"{who}: real_ratio={real_ratio} > 0 on a time-adaptive system: real rows have no tau column (they carry "
                         "u_dim action columns, model rows u_dim + 1), so they cannot share a minibatch")
    if non_equidistant_time:
        for name, mine in (("continuous_discounting", continuous_discounting), ("min_time_between_switches", min_time_between_switches),
                           ("max_time_between_switches", max_time_between_switches), ("env_dt", env_dt)):
            if float(mine) != float(getattr(ta, name)):
                raise ValueError(f"{who}: non_equidistant_time with {name}={mine}, but the system's TimeAdaptive has "
                                 f"{name}={getattr(ta, name)}: the loss would discount by another time than the rollout held")


def refuse_time_adaptive(system, who: str) -> None:
    """BPTT and iCEM sum per-step rewards with no notion of a hold."""
    if getattr(system, "time_adaptive", None) is not None:
        raise ValueError(f"{who} does not take a time-adaptive system: its objective sums per-step rewards with no notion of how "
                         "long an action is held; use SAC or PPO")
