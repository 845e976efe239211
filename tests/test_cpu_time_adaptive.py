"""CPU: the descriptor layout of the hold_* fields, every MBPO_ERR_ARG of a time-adaptive rollout on an empty launch, the Python surface
(TimeAdaptive, the systems' two widths, the refusals) on device="cpu" objects, TimeAdaptive.max_steps against the restatement, and the
conditions every GPU case must meet in the reference runs alone (tests/time_adaptive_cases.py)."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest
import torch

import time_adaptive_cases as tc
import time_adaptive_ref as taref

ROOT = Path(__file__).resolve().parent.parent
HOLD_FIELDS = ["hold_max_steps", "hold_min_time", "hold_max_time", "hold_dt", "hold_gamma", "hold_switch_cost"]


# ------------------------------------------------------------------------------------------------ descriptor layout
def test_hold_fields_sit_in_front_of_the_termination_pair(tmp_path):
    from mbpo import _hip
    header = (ROOT / "include" / "mbpo_hip.h").read_text()
    body = re.search(r"typedef struct mbpo_rollout_desc \{(.*?)\} mbpo_rollout_desc;", header, re.S).group(1)
    code = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    pos = [code.index(f) for f in HOLD_FIELDS]
    assert pos == sorted(pos) and code.index("start_state") < pos[0] and pos[-1] < code.index("term_low")
    names = [f[0] for f in _hip.RolloutDesc._fields_]
    assert names[-8:] == HOLD_FIELDS + ["term_low", "term_high"]
    src = tmp_path / "off.c"
    offs = ", ".join(f"offsetof(mbpo_rollout_desc, {f})" for f in HOLD_FIELDS + ["term_low"])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mbpo_hip.h"\nint main(void) {\n'
                   f'  printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", {offs}, sizeof(mbpo_rollout_desc));\n  return 0;\n}}\n')
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert out == [getattr(_hip.RolloutDesc, f).offset for f in HOLD_FIELDS + ["term_low"]] + [C.sizeof(_hip.RolloutDesc)]
    d = _hip.RolloutDesc()
    assert d.hold_max_steps == 0 and d.hold_gamma == 0.0        # a zero-initialised descriptor: off


def test_hold_steps_is_exported_and_declared():
    from mbpo import _hip
    lib = _hip.load()
    assert hasattr(lib, "mbpo_hold_steps")
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mbpo_hip.h").read_text(), flags=re.S)
    m = re.search(r"\bmbpo_hold_steps\s*\(([^;{}]*?)\)\s*;", header, re.S)
    assert m and "workspace" not in m.group(1)
    # its argument checks need no device (n = 0 returns before any pointer is looked at)
    call = lambda n, A, lo, hi, dt, K: lib.mbpo_hold_steps(None, n, A, lo, hi, dt, K, None, None)
    assert call(0, 2, 0.05, 0.2, 0.05, 4) == 0, lib.mbpo_last_error()
    for args, what in (((-1, 2, 0.05, 0.2, 0.05, 4), b"n < 0"), ((0, 0, 0.05, 0.2, 0.05, 4), b"action_dim"),
                       ((0, 2, 0.05, 0.2, 0.0, 4), b"env_dt"), ((0, 2, 0.3, 0.2, 0.05, 4), b"min_time"),
                       ((0, 2, 0.05, 0.2, 0.05, 0), b"max_steps"), ((0, 2, 0.05, 0.2, 0.05, 65), b"max_steps"),
                       ((3, 2, 0.05, 0.2, 0.05, 4), b"null pointer")):
        assert call(*args) == -1 and what in lib.mbpo_last_error(), (args, lib.mbpo_last_error())


# ------------------------------------------------------------------------------------------------ C-ABI, no device
def _mlp_desc_raw(dims, n_nets):
    """An MlpDesc over a fake non-null parameter pointer (validated by the library, never dereferenced)."""
    from mbpo import _hip
    m = _hip.MlpDesc()
    m.params, m.n_nets, m.n_layers, m.activation = 64, n_nets, len(dims) - 1, 0
    m.net_stride = sum(dims[i] * dims[i + 1] + dims[i + 1] for i in range(len(dims) - 1))
    for i, v in enumerate(dims):
        m.dims[i] = v
    return m


def _desc(X=3, UE=2, dyn_in=None, u_dim=None, **hold):
    """An empty (n_envs = 0) time-adaptive rollout over fake non-null pointers: validated, never launched."""
    from mbpo import _hip
    d = _hip.RolloutDesc()
    A = UE + 1 if u_dim is None else u_dim
    d.x_dim, d.u_dim, d.n_envs, d.n_steps, d.episode_length, d.action_repeat = X, A, 0, 0, 5, 1
    d.system_kind, d.ens_mode = _hip.SYS_ENSEMBLE, _hip.ENS_MEAN
    d.reward_kind, d.row_len = _hip.REWARD_QUADRATIC, 2 * X + A + 3
    d.reward_params = d.sys_params = d.actions = 64          # (never dereferenced: n_envs = 0)
    d.dynamics = _mlp_desc_raw([X + UE if dyn_in is None else dyn_in, 64, 64, 2 * X], 3)
    h = dict(hold_max_steps=4, hold_min_time=0.05, hold_max_time=0.2, hold_dt=0.05, hold_gamma=0.97, hold_switch_cost=0.1)
    h.update(hold)
    for k, v in h.items():
        setattr(d, k, v)
    return d


def test_every_hold_argument_check_needs_no_device():
    from mbpo import _hip
    lib = _hip.load()
    call = lambda d: lib.mbpo_model_rollout(C.byref(d), None)
    assert call(_desc()) == 0, lib.mbpo_last_error()
    assert call(_desc(hold_gamma=1.0, hold_switch_cost=0.0, hold_max_steps=64, hold_min_time=0.2)) == 0, lib.mbpo_last_error()
    # Pendulum dynamics and reward: x_dim == 3 && u_env == 1
    d = _desc(UE=1)
    d.system_kind, d.reward_kind = _hip.SYS_PENDULUM, _hip.REWARD_PENDULUM
    assert call(d) == 0, lib.mbpo_last_error()
    d = _desc(UE=2)
    d.reward_kind = _hip.REWARD_PENDULUM
    assert call(d) == -1 and b"pendulum reward" in lib.mbpo_last_error()
    d = _desc(UE=2)
    d.system_kind = _hip.SYS_PENDULUM
    assert call(d) == -1 and b"pendulum system" in lib.mbpo_last_error()
    bad = {"action_repeat": (_desc(), b"action_repeat"), "halluc_beta": (_desc(), b"halluc_beta"),
           "u_dim < 2": (_desc(UE=1, u_dim=1, dyn_in=3), b"u_dim"), "dynamics input": (_desc(dyn_in=3 + 3), b"dynamics input"),
           "hold_dt": (_desc(hold_dt=0.0), b"hold_dt"), "hold_dt < 0": (_desc(hold_dt=-0.05), b"hold_dt"),
           "min > max": (_desc(hold_min_time=0.3), b"hold_min_time"),
           "K > 64": (_desc(hold_max_steps=65), b"hold_max_steps"), "K < 0": (_desc(hold_max_steps=-1), b"hold_max_steps"),
           "gamma 0": (_desc(hold_gamma=0.0), b"hold_gamma"), "gamma > 1": (_desc(hold_gamma=1.01), b"hold_gamma"),
           "cost < 0": (_desc(hold_switch_cost=-0.1), b"hold_switch_cost")}
    bad["action_repeat"][0].action_repeat = 2
    bad["halluc_beta"][0].halluc_beta = 64
    for what, (d, field) in bad.items():
        assert call(d) == -1, f"{what} was accepted"
        assert field in lib.mbpo_last_error(), (what, lib.mbpo_last_error())
    # off: the same descriptor without a hold keeps the plain width rule
    d = _desc(hold_max_steps=0)
    assert call(d) == -1 and b"dynamics input must be x_dim+u_dim" in lib.mbpo_last_error()


# ------------------------------------------------------------------------------------------------ the Python surface
TA = dict(min_time_between_switches=0.05, max_time_between_switches=0.2, env_dt=0.05, switch_cost=0.1, continuous_discounting=0.5)


def _systems(**kw):
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, QuadraticReward, TimeAdaptive
    dyn = EnsembleDynamics(3, 1, n_members=3, hidden_layer_sizes=(64, 64), device="cpu")
    return EnsembleSystem(dyn, QuadraticReward(3, 1), time_adaptive=TimeAdaptive(**TA), **kw)


def test_time_adaptive_validates_and_carries_max_steps():
    from mbpo.systems import TimeAdaptive
    ta = TimeAdaptive(**TA)
    assert ta.max_steps == 4 and ta.kernel_spec()["hold_max_steps"] == 4
    import math
    import numpy as np
    assert ta.gamma == float(np.float32(math.exp(-0.5 * 0.05))) and TimeAdaptive(0.05, 0.2, 0.05).gamma == 1.0
    for lo, hi, dt in ((0.05, 0.2, 0.0), (0.05, 0.2, -0.05), (0.04, 0.2, 0.05), (0.3, 0.2, 0.05), (0.05, 0.05 * 66, 0.05)):
        with pytest.raises(ValueError):
            TimeAdaptive(lo, hi, dt)
    with pytest.raises(ValueError, match="switch_cost"):
        TimeAdaptive(0.05, 0.2, 0.05, switch_cost=-1.0)
    assert ta.trainer_kwargs() == dict(non_equidistant_time=True, continuous_discounting=0.5, min_time_between_switches=0.05,
                                       max_time_between_switches=0.2, env_dt=0.05)


@pytest.mark.parametrize("lo,hi,dt", [(0.05, 0.05, 0.05), (0.05, 0.2, 0.05), (0.05, 0.24995, 0.05), (0.1, 0.35, 0.1), (0.0625, 0.25, 0.0625),
                                      (0.01, 0.64, 0.01), (0.05, 0.15000001, 0.05), (0.3, 0.3, 0.1), (1.0, 7.5, 0.5)])
def test_max_steps_is_the_restatement_at_tau_one(lo, hi, dt):
    from mbpo.systems import TimeAdaptive
    k = int(taref.hold_steps(torch.ones(1), taref.Hold(lo, hi, dt, K=10 ** 6))[0])
    assert TimeAdaptive(lo, hi, dt).max_steps == k
    if lo == hi == dt:
        assert k == 1


def test_the_restatement_of_floor_divide():
    f = lambda a, b: float(taref.floor_divide_f(torch.tensor(a), torch.tensor(b)))
    assert [f(0.2, 0.05), f(0.19, 0.05), f(0.05, 0.05), f(0.04, 0.05), f(-0.01, 0.05), f(7.0, 2.0)] == [4.0, 3.0, 1.0, 0.0, -1.0, 3.0]
    # tau = -1 with t_lo = dt: the floor gives 1 (or 0 to rounding); the rollout's clamp makes it 1 either way
    h = taref.Hold(0.05, 0.2, 0.05, 4)
    assert taref.hold_steps(torch.tensor([-1.0, -0.999999, 0.0, 1.0]), h).tolist() == [1, 1, 2, 4]


def test_systems_report_both_widths():
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, PendulumSystem, QuadraticReward, TimeAdaptive
    from mbpo.systems.brax_wrapper import BraxWrapper
    cpu = torch.device("cpu")
    s = _systems()
    assert (s.u_dim, s.action_dim) == (1, 2) and BraxWrapper(s, None, None, None).action_size == 2
    a = torch.arange(6.0).reshape(3, 2)
    assert torch.equal(s.env_action(a), a[:, :1])
    spec = s.rollout_spec(s.init_params(0), cpu)
    assert {k: spec[k] for k in spec if k.startswith("hold_")} == TimeAdaptive(**TA).kernel_spec()
    plain = EnsembleSystem(EnsembleDynamics(3, 1, n_members=3, hidden_layer_sizes=(64, 64), device="cpu"), QuadraticReward(3, 1))
    assert plain.action_dim == 1 and not any(k.startswith("hold_") for k in plain.rollout_spec(plain.init_params(0), cpu))
    assert torch.equal(plain.env_action(a[:, :1]), a[:, :1])
    with pytest.raises(ValueError, match="time-adaptive"):
        plain.hold_steps(a)
    p = PendulumSystem(time_adaptive=TimeAdaptive(**TA))
    assert (p.u_dim, p.action_dim) == (1, 2)
    pspec = p.rollout_spec(p.init_params(0), cpu)
    assert pspec["hold_max_steps"] == 4 and pspec["hold_switch_cost"] == pytest.approx(0.1)
    assert PendulumSystem().action_dim == 1 and "hold_max_steps" not in PendulumSystem().rollout_spec(p.init_params(0), cpu)
    # another TimeAdaptive on the same system: another cached spec
    p.time_adaptive = TimeAdaptive(0.05, 0.1, 0.05)
    assert p.rollout_spec(p.init_params(0), cpu)["hold_max_steps"] == 2


def test_the_refusals_need_no_device():
    from mbpo import _hip, ops
    from mbpo.optimizers.policy_optimizers.bptt_optimizer import BPTTOptimizer
    from mbpo.optimizers.policy_optimizers.ppo.ppo import PPO
    from mbpo.optimizers.policy_optimizers.sac.sac import SAC
    from mbpo.optimizers.trajectory_optimizers.icem_optimizer import iCEMOptimizer, iCemTO
    from mbpo.systems import PendulumDynamics, PendulumReward, System, TimeAdaptive
    s = _systems()

    class Env:
        system = s

    base = dict(environment=Env(), num_timesteps=1000, episode_length=10)
    for cls in (SAC, PPO):
        with pytest.raises(ValueError, match="action_repeat"):
            cls(action_repeat=2, **base)
        for field, value in (("continuous_discounting", 0.4), ("min_time_between_switches", 0.1), ("max_time_between_switches", 0.25),
                             ("env_dt", 0.025)):
            kw = TimeAdaptive(**TA).trainer_kwargs()
            kw[field] = value
            with pytest.raises(ValueError, match=field):
                cls(**base, **kw)
    with pytest.raises(ValueError, match="real_ratio"):
        SAC(real_ratio=0.05, **base)
    # optimistic together with time_adaptive
    with pytest.raises(ValueError, match="optimistic"):
        _systems(mode="optimistic")
    # BPTT, fused and wide (both start at the same check), and through set_system
    with pytest.raises(ValueError, match="time-adaptive"):
        BPTTOptimizer(obs_dim=3, action_dim=2, device="cpu", system=s)
    opt = BPTTOptimizer.__new__(BPTTOptimizer)
    opt.system = None
    with pytest.raises(ValueError, match="time-adaptive"):
        opt.set_system(s)
    opt.system = s
    with pytest.raises(ValueError, match="time-adaptive"):
        opt._system_kwargs(None)
    # iCEM, single and batched, and the planner itself
    for kw in ({}, {"batch_size": 4}):
        with pytest.raises(ValueError, match="time-adaptive"):
            iCEMOptimizer(horizon=5, system=s, **kw)
        o = iCEMOptimizer(horizon=5, **kw)
        with pytest.raises(ValueError, match="time-adaptive"):
            o.set_system(s)
    with pytest.raises(ValueError, match="time-adaptive"):
        iCemTO(horizon=5, action_dim=2, system=s)
    # a user-defined (non-fused) System

    class Mine(System):      # (its own step: not fused)
        def __init__(self, **kw):
            super().__init__(PendulumDynamics(), PendulumReward(), **kw)

    assert Mine().action_dim == 1
    with pytest.raises(ValueError, match="fused"):
        Mine(time_adaptive=TimeAdaptive(**TA))
    with pytest.raises(ValueError, match="hold_max_steps"):
        ops.model_rollout(system_kind=_hip.SYS_GENERIC, x_dim=3, u_dim=2, obs=None, first_obs=None, steps=None, done=None, n_steps=1,
                          episode_length=5, hold_max_steps=4)


# ------------------------------------------------------------------------------------------------ the conditions of the GPU cases
@pytest.mark.parametrize("name", sorted(tc.CASES))
def test_gpu_cases_meet_their_conditions(name):
    """On the reference runs alone (fp32 and fp64), before any device result is looked at."""
    b, k = tc.build(name), tc.kept(name)
    o32, o64 = tc.oracle(name, torch.float32), tc.oracle(name, torch.float64)
    gap, tol = k["gap"], tc.tol(name)
    print(f"{name}: fp32-fp64 gap {gap:.3g}, recorded {tc.GAP_TOL[name][0]:.3g}, tol {tol:.3g}, kept envs {int(k['env'].sum())} / {tc.N}")
    assert 2e-4 <= tol <= 2e-3 and gap < tol / 2
    assert gap <= 1.5 * tc.GAP_TOL[name][0], "the recorded gap is out of date"
    assert int(k["env"].sum()) >= (1 - tc.MAX_EXCLUDED) * tc.N
    dec = k["dec"][:, k["env"]]
    ks = o64["k"][:, k["env"]][dec]
    for v in range(1, b["K"] + 1):
        assert float((ks == v).float().mean()) >= tc.MIN_HOLD_SHARE, f"k = {v} is taken by too few kept decisions"
    assert int(o64["k"].max()) == b["K"] == tc.time_adaptive(name).max_steps
    assert bool(o64["reset"][:-1].any()), "no reset inside the launch"
    assert float(tc.env_rows(o64["rows"], name)[:, :, -1].sum()) >= 1, "no truncation in the reference run"
    if b["box"] is not None:
        inner = ((o64["term_at"] >= 0) & (o64["term_at"] < o64["k"] - 1))[:, k["env"]]
        assert int(inner.sum()) >= tc.MIN_INNER_TERMINATIONS, f"only {int(inner.sum())} kept rows terminate at an inner step j < k - 1"
        assert torch.equal(o32["k_eff"][:, k["env"]], o64["k_eff"][:, k["env"]])
    else:
        assert torch.equal(o64["k_eff"], o64["k"])
    if b["start"]:
        assert not torch.equal(o64["state"].first_obs, b["first"].double()), "no reset drew a fresh start"


def test_fixed_hold_is_action_repeat_in_the_reference():
    """t_lo = t_hi = K dt, gamma = 1, no cost, no box: the restatement's rows are oracle.rollout's at action_repeat = K, bit for bit."""
    from oracle import rollout as oro
    name = "c1_64_mean_cd"
    b = tc.build(name)
    K, X, UE = 3, b["X"], b["UE"]
    g = torch.Generator().manual_seed(5)
    acts = torch.rand(tc.S, tc.N, UE + 1, generator=g) * 2 - 1
    st0 = oro.EnvState(b["obs0"], b["first"], b["steps0"], b["done0"])
    out = taref.rollout(tc.ref_system(name), UE, taref.Hold(K * 0.0625, K * 0.0625, 0.0625, K), None, None, st0, tc.S, tc.L, actions=acts)
    st, rows = st0.clone(), []
    for s in range(tc.S):
        nst, r, tr = oro.env_step(tc.ref_system(name), st, acts[s, :, :UE], tc.L, K, s)
        rows.append(torch.cat([st.obs, acts[s], r[:, None], (1 - nst.done)[:, None], nst.obs, tr[:, None]], dim=1))
        st = nst
    assert torch.equal(out["rows"], torch.cat(rows)) and torch.equal(out["state"].steps, st.steps)
