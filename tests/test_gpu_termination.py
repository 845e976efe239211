"""GPU: termination functions in the fused model rollouts (mbpo_rollout_desc.term_low / term_high; include/mbpo_hip.h "termination")
against oracle.rollout given a system that reports done (tests/termination_ref.py), on every rollout kernel: k_rollout_lean (one
tile and two tiles in flight), the generic 64-wide kernel, the 128- and 256-wide kernel and the per-env open-loop Pendulum kernel.

`done` is a discontinuous decision and rows match the oracle only to atol = rtol = 2e-4 (5e-4 for the x = 17 case, as
tests/test_gpu_rollout.py), so an env whose next state ever comes within 2e-3 (10 x the tolerance) of a finite bound in the ORACLE
run is excluded from the comparison as a whole; tests/termination_cases.py asserts on the oracle run alone that at most 10 % of the
envs are excluded, at least 10 % terminate by sys_done and a truncation occurs.  On the kept envs discount, truncation, steps and
done are exact.
"""
import ctypes as C
import math

import pytest
import torch

import termination_cases as tc
import termination_ref as tref

pytestmark = pytest.mark.gpu
INF = math.inf


def _set_rollout_lean(mode: int) -> None:
    from mbpo import _hip
    lib = _hip.load()
    lib.mbpo_debug_set_rollout_lean.argtypes = [C.c_int]
    lib.mbpo_debug_set_rollout_lean.restype = C.c_int
    assert lib.mbpo_debug_set_rollout_lean(mode) == 0


def _run(name, dev, with_termination=True):
    """rows (host), and the env state the launch left (host)."""
    from mbpo import ops
    kw = tc.device_kwargs(name, dev, with_termination)
    rows = ops.model_rollout(**kw)
    torch.cuda.synchronize()
    return rows.cpu(), kw["obs"].cpu(), kw["steps"].cpu(), kw["done"].cpu()


# ------------------------------------------------------------------------------------------------ 1. oracle parity
@pytest.mark.parametrize("name", list(tc.CASES))
def test_terminating_rollout_matches_oracle(dev, name):
    ref = tc.oracle(name)                      # (asserts the three conditions on the oracle run before anything runs on the device)
    c = tc.CASES[name]
    X, U, atol = c["X"], c["U"], c["atol"]
    rows, obs, steps, done = _run(name, dev)
    keep = ref["keep"]
    got, want = tc.env_rows(rows, name)[keep], tc.env_rows(ref["rows"], name)[keep]
    D = got.shape[-1]
    disc, trunc = X + U + 1, D - 1
    print(f"{name}: excluded {ref['n_excluded']}, terminating {ref['n_terminating']}, truncations {ref['n_truncations']}, "
          f"max |rows - oracle| on kept envs {float((got - want).abs().max()):.3e}")
    assert torch.equal(got[..., disc], want[..., disc])
    assert torch.equal(got[..., trunc], want[..., trunc])
    assert torch.equal(steps[keep], ref["state"].steps[keep])
    assert torch.equal(done[keep], ref["state"].done[keep])
    # terminations that are not truncations do occur in what is compared
    assert int(((got[..., disc] == 0) & (got[..., trunc] == 0)).sum()) >= 1
    torch.testing.assert_close(got, want, atol=atol, rtol=atol)
    torch.testing.assert_close(obs[keep], ref["state"].obs[keep], atol=atol, rtol=atol)


# ------------------------------------------------------------------------------------------------ 2. lean == generic
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_terminating_rollout_lean_equals_generic_kernel(dev, name):
    """k_rollout_lean with one tile per workgroup (mode 3) and two in flight (mode 2) against the generic 64-wide kernel (mode 0),
    termination set: rows and env state bit for bit, near-bound envs included (the kernels form x' with the same operations)."""
    out = {}
    try:
        for mode in (0, 3, 2):
            _set_rollout_lean(mode)
            out[mode] = _run(name, dev)
    finally:
        _set_rollout_lean(-1)
    for mode in (3, 2):
        for got, want in zip(out[mode], out[0]):
            assert torch.equal(got, want), f"mode {mode}"
    disc, trunc = tc.CASES[name]["X"] + tc.CASES[name]["U"] + 1, -1
    assert int(((out[0][0][:, disc] == 0) & (out[0][0][:, trunc] == 0)).sum()) >= 1


# ------------------------------------------------------------------------------------------------ 3. neutrality
@pytest.mark.parametrize("name", ["a", "b", "c"])
@pytest.mark.parametrize("mode", [0, 3, 2])
def test_unbounded_box_equals_no_termination(dev, name, mode):
    """low = -inf, high = +inf on finite states: rows and env state bit-identical to the run without a termination."""
    from mbpo import ops
    X = tc.CASES[name]["X"]
    try:
        _set_rollout_lean(mode)
        plain = _run(name, dev, with_termination=False)
        kw = tc.device_kwargs(name, dev, with_termination=False)
        kw.update(term_low=torch.full((X,), -INF, device=dev), term_high=torch.full((X,), INF, device=dev))
        rows = ops.model_rollout(**kw)
        torch.cuda.synchronize()
    finally:
        _set_rollout_lean(-1)
    for got, want in zip((rows.cpu(), kw["obs"].cpu(), kw["steps"].cpu(), kw["done"].cpu()), plain):
        assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ 4. non-finite states
def test_non_finite_states_terminate_and_reset(dev):
    """Open-loop actions (the generic kernel), predict_delta, every bound +-inf.  The members are zero networks with a non-zero output
    bias, so a finite state steps to x + mean_e(bias) whatever its size: the envs started at +inf and NaN step to a non-finite state
    and get discount 0, truncation 0 and next_obs == first_obs; the env at 3e38 (finite) and all the others continue."""
    from mbpo import _hip, ops
    X, U, E, N, S = 4, 1, 3, 20, 2
    g = torch.Generator().manual_seed(0)
    ddims = [X + U, 64, 64, 64, 2 * X]
    P = sum(ddims[i] * ddims[i + 1] + ddims[i + 1] for i in range(4))
    dpar = torch.zeros(E, P)
    bias = 0.01 * torch.randn(E, X, generator=g)
    dpar[:, P - 2 * X:P - X] = bias                      # the mean outputs' biases (the last layer's bias vector closes the network)
    obs0 = torch.randn(N, X, generator=g)
    first = torch.randn(N, X, generator=g)
    i_inf, i_nan, i_big = 3, 7, 18
    obs0[i_inf], obs0[i_nan], obs0[i_big] = INF, float("nan"), 3e38
    actions = torch.rand(S, N, U, generator=g) * 2 - 1
    obs_d, steps_d, done_d = obs0.to(dev), torch.zeros(N, device=dev), torch.zeros(N, device=dev)
    rows = ops.model_rollout(x_dim=X, u_dim=U, actions=actions.to(dev), obs=obs_d, first_obs=first.to(dev), steps=steps_d, done=done_d,
                             n_steps=S, episode_length=1000, system_kind=_hip.SYS_ENSEMBLE, dyn_params=dpar.reshape(-1).to(dev),
                             dyn_spec=ops.MlpSpec(ddims, "swish", E), ens_mode=_hip.ENS_MEAN, ens_predict_delta=True,
                             reward_kind=_hip.REWARD_QUADRATIC, reward_params=torch.cat([torch.zeros(X), torch.ones(X), torch.ones(U)]).to(dev),
                             term_low=torch.full((X,), -INF, device=dev), term_high=torch.full((X,), INF, device=dev))
    torch.cuda.synchronize()                              # (no fault)
    r = rows.cpu().reshape(S, N, -1)
    disc, trunc, nobs = X + U + 1, -1, slice(X + U + 2, 2 * X + U + 2)
    bad = torch.zeros(N, dtype=torch.bool)
    bad[[i_inf, i_nan]] = True
    assert torch.equal(r[0, :, disc], (~bad).float()) and torch.equal(r[0, :, trunc], torch.zeros(N))
    assert torch.equal(r[0, bad][:, nobs], first[bad])
    step = bias.mean(dim=0)
    torch.testing.assert_close(r[0, ~bad][:, nobs], obs0[~bad] + step, atol=1e-6, rtol=1e-6)
    assert float(r[0, i_big, nobs].min()) > 2.9e38 and bool(torch.isfinite(r[0, i_big, nobs]).all())
    # the second step: the two reset envs run on from first_obs; nothing non-finite in any next_obs, observation or carried obs
    assert torch.equal(r[1, :, :X][bad], first[bad])
    assert torch.equal(r[1, :, disc], torch.ones(N)) and torch.equal(r[1, :, trunc], torch.zeros(N))
    assert bool(torch.isfinite(r[:, :, nobs]).all()) and bool(torch.isfinite(r[1, :, :X]).all())
    assert bool(torch.isfinite(obs_d.cpu()).all())
    assert torch.equal(done_d.cpu(), torch.zeros(N))
    assert torch.equal(steps_d.cpu(), torch.where(bad, 1.0, 2.0))      # (AutoReset zeroes the steps of an env that was done)


def test_one_null_bound_is_an_argument_error(dev):
    from mbpo import _hip, ops
    kw = tc.device_kwargs("a", dev)
    kw.pop("term_high")
    with pytest.raises(_hip.MbpoHipError, match="term_low and term_high"):
        ops.model_rollout(**kw)


# ------------------------------------------------------------------------------------------------ 5. System.step
def _host_system(dev, termination=None, mode="mean", sample_noise=False, E=5, X=4, U=1):
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, QuadraticReward
    dyn = EnsembleDynamics(X, U, n_members=E, device=dev)
    rew = QuadraticReward(X, U, target=[0.1, 0, 0, 0], q=[1, 2, 0.5, 0.1], r=[0.3] * U)
    return EnsembleSystem(dyn, rew, mode=mode, sample_noise=sample_noise, termination=termination)


def test_system_step_reports_done(dev):
    from mbpo.systems import BoxTermination, PendulumSystem
    X, U, N = 4, 1, 100
    term = BoxTermination([-0.8, -INF, -INF, -INF], [0.8, INF, INF, 1.0])
    system, plain = _host_system(dev, term), _host_system(dev)
    sp = system.init_params(1)
    g = torch.Generator().manual_seed(2)
    x, u = torch.randn(N, X, generator=g).to(dev), (torch.rand(N, U, generator=g) * 2 - 1).to(dev)
    free = plain.step(x, u, sp)                          # the same members, no termination: the un-reset next state
    assert int(torch.count_nonzero(torch.as_tensor(free.done))) == 0
    st = system.step(x, u, sp)
    want = term(free.x_next.cpu())
    assert 0.1 * N <= float(want.sum()) <= 0.9 * N
    assert torch.equal(st.done.cpu(), want)
    assert torch.equal(st.done.cpu(), term(free.x_next).cpu())               # __call__ on the device tensor too
    live = want == 0
    assert torch.equal(st.x_next.cpu()[live], free.x_next.cpu()[live])
    assert torch.equal(st.x_next.cpu()[~live], x.cpu()[~live])               # where done: the state the env restarts from
    assert torch.equal(st.reward, free.reward)
    one = system.step(x[0], u[0], sp)
    assert one.done.shape == () and float(one.done) == float(want[0])
    # PendulumSystem: |thetadot| <= 1
    pterm = BoxTermination([-INF, -INF, -1.0], [INF, INF, 1.0])
    psys, pplain = PendulumSystem(termination=pterm), PendulumSystem()
    psp = psys.init_params(0)
    th = (torch.rand(N, generator=g) * 2 - 1) * math.pi
    px = torch.stack([torch.cos(th), torch.sin(th), (torch.rand(N, generator=g) * 2 - 1) * 3], dim=1).to(dev)
    pfree, pst = pplain.step(px, u, psp), psys.step(px, u, psp)
    assert torch.equal(pst.done.cpu(), pterm(pfree.x_next.cpu())) and 0 < float(pst.done.sum()) < N
    assert float(torch.as_tensor(pfree.done)) == 0.0


# ------------------------------------------------------------------------------------------------ 7. iCEM and BPTT ignore it
_TIGHT = ([-0.05, -INF, -INF, -INF], [0.05, INF, INF, INF])          # left within a step or two by most trajectories


def test_icem_ignores_the_termination(dev):
    from mbpo.optimizers import iCemParams, iCemTO
    from mbpo.systems import BoxTermination
    X, U, H = 4, 1, 8
    params = iCemParams(num_particles=2, num_samples=120, num_elites=12, num_steps=3, exponent=1.0, alpha=0.1, init_std=0.6)
    x0 = (torch.randn(X, generator=torch.Generator().manual_seed(3)) * 0.5).to(dev)
    out = []
    for term in (None, BoxTermination(*_TIGHT)):
        system = _host_system(dev, term, mode="ts1", sample_noise=True)
        opt = iCemTO(horizon=H, action_dim=U, opt_params=params, key=5)
        opt.set_system(system)
        new = opt.optimize(x0, opt.init(7))
        out.append((new.best_sequence.cpu().clone(), new.best_reward.cpu().clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_bptt_and_rollout_utils_ignore_the_termination(dev):
    from mbpo.optimizers import BPTTOptimizer
    from mbpo.replay import UniformSamplingQueue
    from mbpo.systems import BoxTermination
    from mbpo.types import Transition
    from mbpo.utils.optimizer_utils import rollout_actions, rollout_policy
    X, U, H = 4, 1, 6
    g = torch.Generator().manual_seed(3)
    q = UniformSamplingQueue(16, Transition(observation=torch.zeros(X), action=torch.zeros(U), reward=torch.zeros(1),
                                            discount=torch.zeros(1), next_observation=torch.zeros(X)), 1, device=dev)
    sbs = q.insert_rows(q.init(0), torch.randn(16, 2 * X + U + 2, generator=g).to(dev))
    out, trs = [], []
    for term in (None, BoxTermination(*_TIGHT)):
        system = _host_system(dev, term, E=3)
        opt = BPTTOptimizer(action_dim=U, obs_dim=X, horizon=H, num_samples_per_gradient_update=24, train_steps=1,
                            critic_updates_per_policy_update=2, sampling_buffer_size=4096)
        opt.set_system(system)
        res = opt.train(bptt_state=opt.init(key=11, true_buffer_state=sbs))
        torch.cuda.synchronize()
        st = res.optimizer_state
        out.append((opt._actor_grad.grads.cpu().clone(), st.actor_params.cpu().clone(), st.critic_params.cpu().clone()))
        sp = system.init_params(1)
        x0 = torch.randn(5, X, generator=torch.Generator().manual_seed(4)).to(dev)
        acts = (torch.rand(H, 5, U, generator=torch.Generator().manual_seed(5)) * 2 - 1).to(dev)
        ta = rollout_actions(system, sp, x0, acts, H)
        tp = rollout_policy(system, sp, x0, lambda o, s: (torch.tanh(o[:, :U]), s), None, H)
        trs.append([t.cpu().clone() for t in (ta.next_observation, ta.reward, tp.next_observation, tp.reward)])
    for a, b in zip(out[0], out[1]):
        assert torch.equal(a, b)
    for a, b in zip(trs[0], trs[1]):
        assert torch.equal(a, b)
    # ... and the box is one these trajectories do leave
    assert float(BoxTermination(*_TIGHT)(trs[0][0]).mean()) > 0.5
