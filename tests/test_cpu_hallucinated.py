"""CPU: the hallucinated-control restatement on its own (tests/halluc_ref.py), the conditions every GPU case must meet in the
reference run alone, the Python surface (EnsembleSystem(mode="optimistic"), the refusals) and the C-ABI checks of halluc_beta, which
need no device."""
import ctypes as C
import subprocess
from pathlib import Path

import pytest
import torch

import halluc_cases as hc
import halluc_ref as href
from oracle import nets as onets
from oracle import rollout as oro
from oracle import systems as osys

ROOT = Path(__file__).resolve().parent.parent


def _pair(X=3, UE=2, E=5, beta=1.0, seed=0):
    """(hallucinated restatement, oracle 'mean' system) over the same members, a batch of states, controls and eta."""
    g = torch.Generator().manual_seed(seed)
    dims = [X + UE, 64, 64, 2 * X]
    par = hc.member_params(dims, E, g)
    tgt, q, r = torch.randn(X, generator=g), torch.rand(X, generator=g), torch.rand(UE, generator=g)
    rfn = lambda x, u: osys.quadratic_reward(x, u, tgt, q, r)
    h = href.HallucinatedEnsembleSystem(par, dims, E, X, UE, beta, reward_fn=rfn)
    m = osys.EnsembleSystem(par, dims, E, X, UE, mode="mean", reward_fn=rfn)
    x, u = torch.randn(33, X, generator=g), torch.rand(33, UE, generator=g) * 2 - 1
    eta = torch.rand(33, X, generator=g) * 2 - 1
    return h, m, x, u, eta


def test_beta_zero_is_the_mean_step_exactly():
    h, m, x, u, eta = _pair(beta=0.0)
    xn, r = h.step(x, torch.cat([u, eta], dim=1))
    xm, rm = m.step(x, u)
    assert torch.equal(xn, xm) and torch.equal(r, rm)


def test_one_member_is_the_mean_step_exactly_for_any_eta():
    h, m, x, u, eta = _pair(E=1, beta=[0.5, 1.0, 2.0], seed=1)
    xn, r = h.step(x, torch.cat([u, 5.0 * eta], dim=1))
    xm, rm = m.step(x, u)
    assert torch.equal(xn, xm) and torch.equal(r, rm)


def test_the_term_is_beta_times_population_std_times_eta():
    h, m, x, u, eta = _pair(beta=[0.5, 1.0, 2.0], seed=2)
    X = 3
    y = onets.ensemble_forward(h.params, h.dims, h.E, torch.cat([x, u], dim=1))[..., :X]
    want = x + y.mean(0) + h.beta * y.var(dim=0, unbiased=False).sqrt() * eta
    xn, _ = h.step(x, torch.cat([u, eta], dim=1))
    torch.testing.assert_close(xn, want, atol=1e-6, rtol=1e-6)
    # and it moves the state: the members disagree
    assert float((xn - m.step(x, u)[0]).abs().mean()) > 10 * hc.ATOL


@pytest.mark.parametrize("name", list(hc.CASES))
def test_gpu_cases_meet_their_conditions(name):
    """On the reference run alone: fp32 against fp64 stays below half the GPU tolerance, the mean of |beta sd eta| exceeds ten times
    that tolerance (a kernel that drops the term cannot pass), resets fall inside the launch, and the case with a termination box
    stays within tests/termination_ref.py's caps (asserted inside hc.oracle)."""
    b = hc.build(name)
    r32, r64 = hc.oracle(name), hc.oracle(name, torch.float64)
    keep = r32["keep"] & r64["keep"]
    gap = float((hc.env_rows(r32["rows"], name)[keep].double() - hc.env_rows(r64["rows"], name)[keep]).abs().max())
    print(f"{name}: fp32-fp64 gap {gap:.3g}, mean |beta sd eta| {r32['term_mean']:.3g}, kept {int(keep.sum())} of {hc.N}")
    assert gap < 0.5 * hc.ATOL
    assert r32["term_mean"] > 10 * hc.ATOL
    disc = b["X"] + b["A"] + 1
    rows = hc.env_rows(r32["rows"], name)
    assert int((rows[..., disc] == 0).sum()) >= hc.N      # every env resets at least once on average: episode_length 3 < S
    assert int(keep.sum()) >= 0.9 * hc.N


def _systems(mode="optimistic", beta=1.0, X=3, U=1, **kw):
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, QuadraticReward
    dyn = EnsembleDynamics(X, U, n_members=3, hidden_layer_sizes=kw.pop("hidden", (64, 64)), device="cpu")
    return EnsembleSystem(dyn, QuadraticReward(X, U), mode=mode, beta=beta, **kw)


def test_optimistic_system_reports_both_widths():
    from mbpo import _hip
    s = _systems()
    assert (s.x_dim, s.u_dim, s.action_dim) == (3, 1, 4) and s.optimistic
    a = torch.arange(8.0).reshape(2, 4)
    assert torch.equal(s.env_action(a), a[:, :1]) and torch.equal(s.env_action(a[0]), a[0, :1])
    assert torch.equal(s.beta, torch.ones(3))
    assert torch.equal(_systems(beta=[0.5, 1.0, 2.0]).beta, torch.tensor([0.5, 1.0, 2.0]))
    assert torch.equal(_systems(beta=torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)).beta, torch.tensor([0.5, 1.0, 2.0]))
    plain = _systems(mode="mean")
    assert (plain.u_dim, plain.action_dim) == (1, 1) and not plain.optimistic and plain.beta is None
    a1 = torch.arange(2.0).reshape(2, 1)
    assert torch.equal(plain.env_action(a1), a1)
    # 'optimistic' is the mean of the members plus halluc_beta
    from mbpo.systems import ensemble_system
    assert ensemble_system._MODES["optimistic"] == _hip.ENS_MEAN
    # every System has the property
    from mbpo.systems import PendulumSystem
    assert PendulumSystem().action_dim == 1
    # the wrapper's action_size is the policy's width; the true buffer's layout stays on u_dim
    from mbpo.systems.brax_wrapper import BraxWrapper
    assert BraxWrapper(s, None, None, None).action_size == 4 and BraxWrapper(plain, None, None, None).action_size == 1


def test_beta_of_the_wrong_length_is_refused():
    for bad in ([1.0, 2.0], torch.ones(4), []):
        with pytest.raises(ValueError, match="beta"):
            _systems(beta=bad)


def test_members_wider_than_256_are_refused():
    with pytest.raises(ValueError, match="256"):
        _systems(hidden=(300, 300))


def test_bptt_refuses_an_optimistic_system():
    from mbpo import _hip
    from mbpo.optimizers.policy_optimizers.bptt_optimizer import BPTTOptimizer
    from mbpo.systems.torch_steps import DifferentiableBuiltin
    s = _systems()
    with pytest.raises(ValueError, match="optimistic"):
        BPTTOptimizer(obs_dim=3, action_dim=4, device="cpu", system=s)
    opt = BPTTOptimizer.__new__(BPTTOptimizer)      # (an optimizer built without a system, as set_system's callers have it)
    opt.system = None
    with pytest.raises(ValueError, match="optimistic"):
        opt.set_system(s)
    opt.system = s
    with pytest.raises(ValueError, match="optimistic"):
        opt._system_kwargs(None)                    # the fused and the wide path both start here
    with pytest.raises(ValueError, match="optimistic"):
        opt.init(0)
    # the wide path's torch form of the step
    with pytest.raises(ValueError, match="optimistic"):
        DifferentiableBuiltin(s, dict(system_kind=_hip.SYS_ENSEMBLE, halluc_beta=torch.ones(3)))
    with pytest.raises(ValueError, match="optimistic"):
        DifferentiableBuiltin(_systems(mode="mean"), dict(system_kind=_hip.SYS_ENSEMBLE, halluc_beta=torch.ones(3)))


def test_sac_refuses_real_ratio_on_an_optimistic_system():
    """Real rows carry u_dim action columns, model rows action_dim: refused before anything touches a device."""
    from mbpo.optimizers.policy_optimizers.sac.sac import SAC

    class Env:
        system = _systems()

    with pytest.raises(ValueError, match="optimistic"):
        SAC(environment=Env(), num_timesteps=1000, episode_length=10, real_ratio=0.05)


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


def _desc(X=3, UE=2, ens_mode=None, system_kind=None, dyn_in=None, u_dim=None):
    """An empty (n_envs = 0) hallucinated rollout over fake non-null pointers: validated, never launched."""
    from mbpo import _hip
    d = _hip.RolloutDesc()
    A = UE + X if u_dim is None else u_dim
    d.x_dim, d.u_dim, d.n_envs, d.n_steps, d.episode_length, d.action_repeat = X, A, 0, 0, 5, 1
    d.system_kind = _hip.SYS_ENSEMBLE if system_kind is None else system_kind
    d.ens_mode = _hip.ENS_MEAN if ens_mode is None else ens_mode
    d.reward_kind, d.row_len = _hip.REWARD_QUADRATIC, 2 * X + A + 3
    d.reward_params = d.sys_params = d.actions = 64          # (never dereferenced: n_envs = 0)
    d.dynamics = _mlp_desc_raw([X + UE if dyn_in is None else dyn_in, 64, 64, 2 * X], 3)
    d.halluc_beta = 64
    return d


def test_halluc_argument_checks_need_no_device():
    from mbpo import _hip
    lib = _hip.load()
    call = lambda d: lib.mbpo_model_rollout(C.byref(d), None)
    assert call(_desc()) == 0, lib.mbpo_last_error()
    # mean-only members (dyn_out == x_dim) are accepted
    d = _desc()
    d.dynamics = _mlp_desc_raw([5, 64, 64, 3], 3)
    assert call(d) == 0, lib.mbpo_last_error()
    # the pendulum reward needs x = 3 and u_env = 1
    d = _desc(UE=1)
    d.reward_kind = _hip.REWARD_PENDULUM
    assert call(d) == 0, lib.mbpo_last_error()
    d = _desc(UE=2)
    d.reward_kind = _hip.REWARD_PENDULUM
    assert call(d) == -1 and b"pendulum reward" in lib.mbpo_last_error()
    # the four conditions
    bad = {"system_kind": _desc(X=3, UE=1, u_dim=4, system_kind=_hip.SYS_PENDULUM),
           "ens_mode": _desc(ens_mode=_hip.ENS_TS1),
           "u_dim <= x_dim": _desc(X=3, UE=2, u_dim=3, dyn_in=3),
           "dynamics input": _desc(dyn_in=3 + 2 + 3)}
    bad["system_kind"].reward_kind = _hip.REWARD_PENDULUM
    for what, d in bad.items():
        assert call(d) == -1, f"{what} was accepted"
        assert b"halluc_beta" in lib.mbpo_last_error(), (what, lib.mbpo_last_error())
    d = _desc(ens_mode=_hip.ENS_TSINF)
    assert call(d) == -1 and b"halluc_beta" in lib.mbpo_last_error()
    # off: the same descriptors without halluc_beta fail or pass as they did (the plain width rule)
    d = _desc()
    d.halluc_beta = None
    assert call(d) == -1 and b"dynamics input must be x_dim+u_dim" in lib.mbpo_last_error()
    assert _hip.RolloutDesc().halluc_beta is None


def test_descriptor_mirror_matches_the_header(tmp_path):
    from mbpo import _hip
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mbpo_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu\\n", offsetof(mbpo_rollout_desc, halluc_beta), sizeof(mbpo_rollout_desc));\n  return 0;\n}\n')
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert out == [_hip.RolloutDesc.halluc_beta.offset, C.sizeof(_hip.RolloutDesc)]
