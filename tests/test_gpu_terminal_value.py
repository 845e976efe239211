"""Terminal values on the device (include/mbpo_hip.h "terminal values", mbpo.optimizers.TerminalValue): mbpo_terminal_value_eval against
the test tree's restatement (tests/terminal_value_ref.py, fp32 and fp64) at the project's forward tolerances, its accumulate, -inf,
row-independence and capture contracts bit for bit, and the launch inside iCemTO (single, plan reward, batched, optimistic).

Tolerances: test_ensemble_forward_parity's — atol = rtol = 2e-5 against the fp32 restatement, 5e-5 against the fp64 one;
tests/test_cpu_terminal_value.py shows on the restatement alone that the two agree to 3.3e-6 and that the values spread over the rows
by 4 and more at every case."""
import functools
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

import plan_reward_ref as pref
import terminal_value_cases as cases
import terminal_value_ref as tref
from test_gpu_icem_batched import _compare_with_single_calls, _same

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
NAN = float("nan")


def _tv(case, dev, norm=True, weight=1.0):
    from mbpo.optimizers import TerminalValue
    d = lambda t: None if t is None else t.to(dev)
    return TerminalValue(case.x_dim, d(case.critic), case.critic_dims, n_critics=case.n_critics, activation=case.act,
                         policy_params=d(case.policy), policy_dims=case.policy_dims, policy_activation=case.act,
                         norm_mean=d(case.mean) if norm else None, norm_std=d(case.std) if norm else None, weight=weight)


def _grid_cap() -> int:
    """the launch's largest grid: 8 workgroups per compute unit (csrc/terminal_value.hip)"""
    return 8 * torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def _reference(si: int, kind: str, norm: bool):
    """(case, states [n_big, x], v32 [n_big], v64 [n_big]) on the host, computed once: n_big = 16 k + 1 with k + 1 tiles, two more than
    the launch's grid.  A row's value does not depend on n, so every smaller n reads a prefix."""
    case = cases.make_case(cases.SHAPES[si], kind)
    n_big = 16 * (_grid_cap() + 1) + 1
    x = cases.make_states(case, n_big, norm=norm)
    args, kw = case.ref_args(norm)
    return case, x, tref.v_hat(x, *args, **kw), tref.v_hat(x.double(), *args, **kw)


def _icem_rows(x: torch.Tensor, action_width: int, dev, fill=NAN):
    """States laid out as iCEM passes them: the next-state columns of rows [n, 2 x + A + 3] (an odd stride whenever A is even, rows off
    16-byte alignment), every other column `fill`.  (rows on the device, reward_col, next_off)"""
    n, X = x.shape
    row_len, reward_col, next_off = cases.icem_layout(X, action_width)
    rows = torch.full((n, row_len), fill, dtype=torch.float32)
    rows[:, next_off:next_off + X] = x
    return rows.to(dev), reward_col, next_off


# ------------------------------------------------------------------------------------------------ 1: parity
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("si", range(len(cases.SHAPES)), ids=[cases.shape_id(s) for s in cases.SHAPES])
def test_parity_with_the_restatement(dev, si, kind):
    A = cases.SHAPES[si][1]
    worst32 = worst64 = 0.0
    for norm in (True, False):
        case, x, v32, v64 = _reference(si, kind, norm)
        tv = _tv(case, dev, norm)
        for n in (1, 16, 17, x.shape[0]):
            for strided in (False, True):
                if strided:
                    rows, _, next_off = _icem_rows(x[:n], A, dev)
                    out = torch.full((n,), NAN, device=dev)
                    tv.eval_into(rows, next_off, rows.shape[1], out, 0, 1, n, accumulate=False)
                else:
                    out = tv(x[:n].to(dev))
                got = out.cpu()
                assert got.shape == (n,)
                worst32 = max(worst32, float((got - v32[:n]).abs().max()))
                worst64 = max(worst64, float((got.double() - v64[:n]).abs().max()))
                torch.testing.assert_close(got, v32[:n], atol=cases.TOL32, rtol=cases.TOL32)
                torch.testing.assert_close(got.double(), v64[:n], atol=cases.TOL64, rtol=cases.TOL64)
    print(f"{cases.shape_id(cases.SHAPES[si])} {kind}: max |kernel - fp32 ref| {worst32:.3g}, max |kernel - fp64 ref| {worst64:.3g}")


def test_weight_scales_the_value(dev):
    case, x, _, v64 = _reference(0, "Q", True)
    got = _tv(case, dev, weight=0.37)(x[:100].to(dev)).cpu()
    w = float(torch.tensor(0.37, dtype=torch.float32))
    torch.testing.assert_close(got.double(), w * v64[:100], atol=cases.TOL64, rtol=cases.TOL64)
    one = _tv(case, dev, weight=1.0)(x[:100].to(dev)).cpu()
    assert _same(got, torch.tensor(0.37, dtype=torch.float32) * one)            # the product is rounded on its own


# ------------------------------------------------------------------------------------------------ 2: accumulate
@pytest.mark.parametrize("si,kind", [(0, "Q"), (1, "Q"), (2, "V2"), (4, "V1")])
def test_accumulate_adds_bit_for_bit_and_touches_nothing_else(dev, si, kind):
    """accumulate = 1 on a random out == fl(out + fl(w v)), v from the accumulate = 0 call on the same input; out strided as iCEM passes
    it (the reward column of the rows the states are read from); every other float of the buffer keeps its bits."""
    A = cases.SHAPES[si][1]
    case, x, _, _ = _reference(si, kind, True)
    n, w = 16 * 9 + 5, 0.73
    tv1, tvw = _tv(case, dev, weight=1.0), _tv(case, dev, weight=w)
    g = torch.Generator().manual_seed(5)
    rows, reward_col, next_off = _icem_rows(x[:n], A, dev, fill=0.0)
    rows.copy_(torch.where(rows == 0, torch.randn(rows.shape, generator=g).to(dev), rows))     # poison: random bits in every other column
    rows[:, next_off:next_off + case.x_dim] = x[:n].to(dev)
    before = rows.clone()
    v = tv1.eval_into(rows, next_off, rows.shape[1], torch.empty(n, device=dev), 0, 1, n, accumulate=False)
    assert _same(rows, before)
    tvw.eval_into(rows, next_off, rows.shape[1], rows, reward_col, rows.shape[1], n, accumulate=True)
    want = before.clone()
    want[:, reward_col] = before[:, reward_col] + torch.tensor(w, dtype=torch.float32, device=dev) * v
    assert _same(rows, want)
    assert not _same(rows[:, reward_col], before[:, reward_col])
    # accumulate = 0 into the same strided positions: a store
    tvw.eval_into(rows, next_off, rows.shape[1], rows, reward_col, rows.shape[1], n, accumulate=False)
    want[:, reward_col] = torch.tensor(w, dtype=torch.float32, device=dev) * v
    assert _same(rows, want)


# ------------------------------------------------------------------------------------------------ 3: states that are not finite
@pytest.mark.parametrize("si,kind", [(0, "Q"), (2, "V2"), (3, "Q")])
def test_rows_that_are_not_finite_read_minus_inf_and_leave_their_tile_alone(dev, si, kind):
    case, x, _, _ = _reference(si, kind, True)
    n, X = 16 + 9, case.x_dim
    tv = _tv(case, dev, weight=0.5)
    clean = x[:n].clone()
    bad = clean.clone()
    bad[3, 0], bad[7, X - 1], bad[9, X // 2], bad[20, 0] = float("inf"), float("-inf"), NAN, NAN
    bad[12] = float("inf")
    bad_rows = [3, 7, 9, 12, 20]
    fine = [r for r in range(n) if r not in bad_rows]
    v_clean = tv(clean.to(dev))
    v_bad = tv(bad.to(dev))
    assert bool((v_bad[bad_rows] == float("-inf")).all())
    assert _same(v_bad[fine], v_clean[fine]) and bool(torch.isfinite(v_clean).all())
    # accumulate: -inf is stored over whatever was there (a NaN, +inf), the others are added to
    out = torch.randn(n, generator=torch.Generator().manual_seed(1)).to(dev)
    out[3], out[7] = NAN, float("inf")
    start = out.clone()
    tv.eval_into(bad.to(dev), 0, X, out, 0, 1, n, accumulate=True)
    assert bool((out[bad_rows] == float("-inf")).all())
    assert _same(out[fine], start[fine] + v_clean[fine])
    want = tref.bonus(bad.double(), 0.5, *case.ref_args()[0], **case.ref_args()[1])
    torch.testing.assert_close(v_bad.cpu().double(), want, atol=cases.TOL64, rtol=cases.TOL64)


# ------------------------------------------------------------------------------------------------ 4: row independence
@pytest.mark.parametrize("si,kind", [(0, "Q"), (2, "V2"), (5, "Q")])
def test_a_rows_value_does_not_depend_on_its_place(dev, si, kind):
    """The same states in another order, as a prefix, one by one and behind a tile boundary give the same bits: what makes the batched
    planner equal the single one."""
    case, x, _, _ = _reference(si, kind, True)
    n = 16 * 6 + 11
    tv = _tv(case, dev)
    xs = x[:n].to(dev)
    v = tv(xs)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(2)).to(dev)
    assert _same(tv(xs[perm].contiguous()), v[perm])
    assert _same(tv(xs[:37].contiguous()), v[:37])
    assert _same(tv(xs[50:].contiguous()), v[50:])
    for r in (0, 15, 16, n - 1):
        assert _same(tv(xs[r:r + 1].contiguous()), v[r:r + 1])
    big = tv(x.to(dev))                                                          # more tiles than workgroups: rows of a later trip
    assert _same(big[:n], v)
    assert _same(tv(x[-40:].to(dev)), big[-40:])


# ------------------------------------------------------------------------------------------------ 5: capture
@pytest.mark.parametrize("kind", ["V2", "Q"])
def test_captured_launch_replays_on_refreshed_tensors(dev, kind):
    case, x, _, _ = _reference(0, kind, True)
    n = 16 * 40 + 3
    tv = _tv(case, dev, weight=0.9)
    rows, reward_col, next_off = _icem_rows(x[:n], 1, dev, fill=0.25)
    L = rows.shape[1]
    rows[:, reward_col] = torch.randn(n, generator=torch.Generator().manual_seed(3)).to(dev)
    start = rows.clone()
    tv.eval_into(rows, next_off, L, rows, reward_col, L, n, accumulate=True)     # (one eager call first: the code object)
    eager = rows.clone()
    torch.cuda.synchronize()
    rows.copy_(start)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tv.eval_into(rows, next_off, L, rows, reward_col, L, n, accumulate=True)
    rows.copy_(start)
    graph.replay()
    torch.cuda.synchronize()
    assert _same(rows, eager)
    # the parameters, the normaliser and the states are read by the launch: refreshed in place, the replay honours them
    other = cases.make_case(cases.SHAPES[0], kind, seed=1)
    tv.critic_params.copy_(other.critic.to(dev))
    tv.norm_mean.copy_(other.mean.to(dev))
    if kind == "Q":
        tv.policy_params.copy_(other.policy.to(dev))
    start[:, next_off:next_off + 3] = x[n:2 * n].to(dev)
    rows.copy_(start)
    graph.replay()
    torch.cuda.synchronize()
    replayed = rows.clone()
    rows.copy_(start)
    tv.eval_into(rows, next_off, L, rows, reward_col, L, n, accumulate=True)
    assert _same(replayed, rows) and not _same(replayed[:, reward_col], eager[:, reward_col])


# ------------------------------------------------------------------------------------------------ 6: through iCemTO
_PARAMS = dict(num_particles=2, num_samples=126, num_elites=12, num_steps=2, exponent=1.0, alpha=0.1, init_std=0.6)   # NC = 129
H = 5


def _opt(system, tv, **kw):
    from mbpo.optimizers import iCemParams, iCemTO
    params = iCemParams(**{**_PARAMS, **kw.pop("params", {})})
    opt = iCemTO(horizon=H, action_dim=system.action_dim, opt_params=params, key=5, terminal_value=tv, **kw)
    opt.set_system(system)
    return opt


def _pendulum_starts(dev, B, seed=0):
    g = torch.Generator().manual_seed(seed)
    ang = torch.rand(B, generator=g) * 6.28
    x0 = torch.stack([torch.cos(ang), torch.sin(ang), torch.randn(B, generator=g)], dim=1)
    warm = (torch.rand(B, H, 1, generator=g) - 0.5) * 1.5
    return x0.to(dev), warm.to(dev)


def _pendulum_value(dev, kind="Q", weight=1.0):
    case = cases.make_case(cases.SHAPES[0], kind)          # x 3, A 1: the Pendulum's widths
    return case, _tv(case, dev, weight=weight)


@pytest.mark.parametrize("kind", ["Q", "V2"])
def test_icem_weight_zero_changes_nothing(dev, kind):
    from mbpo.systems import PendulumSystem
    system = PendulumSystem()
    x0, warm = _pendulum_starts(dev, 1)
    _, tv = _pendulum_value(dev, kind, weight=0.0)
    res = []
    for value in (None, tv):
        opt = _opt(system, value)
        st = opt.init(7).replace(best_sequence=warm[0].clone())
        res.append(opt.optimize(x0[0], st))
    assert _same(res[0].best_sequence, res[1].best_sequence) and _same(res[0].best_reward, res[1].best_reward)
    assert res[0].key == res[1].key


def _check_last_step(opt, case, reward64, col, n, dev):
    """The buffer the update read, after the call: its last-step slice is the step's own reward plus the restatement's value of the
    row's next state; every earlier step is the reward alone; `values` is the particle mean of the column sums over the horizon."""
    b = opt._bufs
    rows = b["rows"].cpu()
    X, A = 3, 1
    _, _, next_off = cases.icem_layout(X, A)
    xn = rows[(H - 1) * n:, next_off:next_off + X]
    args, kw = case.ref_args()
    v64 = tref.v_hat(xn.double(), *args, **kw)
    col = col.cpu().double().reshape(H, n)
    r = reward64.reshape(H, n)
    assert float(v64.abs().min()) > 1e-3                                          # (a bonus that could not hide inside the tolerance)
    torch.testing.assert_close(col[H - 1], r[H - 1] + v64, atol=cases.TOL64 + 1e-5, rtol=cases.TOL64)
    torch.testing.assert_close(col[:H - 1], r[:H - 1], atol=1e-5, rtol=0)
    P = opt.opt_params.num_particles
    want = (col.sum(dim=0) / H).reshape(-1, P).mean(dim=1)
    torch.testing.assert_close(b["values"].cpu().double(), want, atol=1e-5, rtol=1e-5)


def test_icem_adds_the_value_into_the_last_steps_reward_column(dev):
    from mbpo.systems import PendulumSystem
    system = PendulumSystem()
    x0, warm = _pendulum_starts(dev, 1)
    case, tv = _pendulum_value(dev, "Q")
    opt = _opt(system, tv)
    st = opt.init(7).replace(best_sequence=warm[0].clone())
    new = opt.optimize(x0[0], st)
    assert bool(torch.isfinite(new.best_reward)) and bool(torch.isfinite(new.best_sequence).all())
    rows = opt._bufs["rows"]
    n = opt._bufs["N"]
    vec = system.reward.kernel_spec(st.system_params.reward_params, dev)[1].cpu()
    r64 = pref.reward(pref.PENDULUM, vec, rows[:, :3].cpu().double(), rows[:, 3:4].cpu().double(), rows[:, 6:9].cpu().double())
    _check_last_step(opt, case, r64, rows[:, 4], n, dev)
    # one iteration from the same state, with the value and without: the launch touched the last step's reward column and nothing else
    one, plain = _opt(system, tv, params=dict(num_steps=1)), _opt(system, None, params=dict(num_steps=1))
    one.optimize(x0[0], st), plain.optimize(x0[0], st)
    a, p = one._bufs["rows"].clone(), plain._bufs["rows"].clone()
    assert not _same(a[(H - 1) * n:, 4], p[(H - 1) * n:, 4])
    a[(H - 1) * n:, 4] = p[(H - 1) * n:, 4]
    assert _same(a, p)


def test_icem_adds_the_value_into_the_plan_rewards_dense_buffer(dev):
    from mbpo.systems import PendulumSystem, PlanRewardParams
    from mbpo.systems.rewards.pendulum_reward import PendulumRewardParams
    system = PendulumSystem()
    x0, warm = _pendulum_starts(dev, 1)
    case, tv = _pendulum_value(dev, "V2")
    prp = PlanRewardParams.stack(system.reward, [[PendulumRewardParams(target_angle=0.3 * t - 0.5) for t in range(H)]], dev)      # [1, H, 3]
    opt = _opt(system, tv)
    st = opt.init(7).replace(best_sequence=warm[0].clone())
    st = st.replace(system_params=st.system_params.replace(reward_params=prp))
    new = opt.optimize(x0[0], st)
    assert bool(torch.isfinite(new.best_reward))
    n = opt._bufs["N"]
    rows = opt._bufs["rows"].cpu()
    r64 = pref.rows_reward(pref.PENDULUM, prp.table.cpu(), rows.double(), H, 1, n, 3, 1, 6)
    _check_last_step(opt, case, r64, opt._bufs["plan_reward"], n, dev)
    # the rows' own reward column was left to the rollout (which ran under the plan's base parameters): no value was added there
    vec = system.reward.kernel_spec(prp.base, dev)[1].cpu()
    own = pref.reward(pref.PENDULUM, vec, rows[:, :3].double(), rows[:, 3:4].double(), rows[:, 6:9].double())
    torch.testing.assert_close(rows[:, 4].double(), own, atol=1e-5, rtol=0)


@pytest.mark.parametrize("kind", ["Q", "V2"])
def test_icem_batched_equals_single_calls(dev, kind):
    from mbpo.systems import PendulumSystem
    _, tv = _pendulum_value(dev, kind)
    opt = _opt(PendulumSystem(), tv)
    x0, warm = _pendulum_starts(dev, 3, seed=1)
    new = _compare_with_single_calls(opt, x0, warm)
    assert bool(torch.isfinite(new.best_reward).all()) and len(set(float(v) for v in new.best_reward)) == 3
    plain = _compare_with_single_calls(_opt(PendulumSystem(), None), x0, warm)
    assert not _same(plain.best_reward, new.best_reward)                          # the value took part


def test_icem_on_an_optimistic_ensemble_takes_the_policys_action_width(dev):
    from mbpo.optimizers import iCemParams, iCemTO
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, QuadraticReward
    X, U = 3, 1
    system = EnsembleSystem(EnsembleDynamics(X, U, n_members=5, device=dev), QuadraticReward(X, U), mode="optimistic", beta=1.5)
    assert system.action_dim == U + X
    case = cases.make_case(cases.SHAPES[1], "Q")                                  # x 3, A 4 = u + x
    tv = _tv(case, dev)
    opt = _opt(system, tv, use_optimism=True)
    g = torch.Generator().manual_seed(3)
    x0, warm = (torch.randn(X, generator=g) * 0.5).to(dev), ((torch.rand(H, U + X, generator=g) - 0.5) * 1.5).to(dev)
    st = opt.init(7).replace(best_sequence=warm.clone())
    new = opt.optimize(x0, st)
    assert bool(torch.isfinite(new.best_reward)) and new.best_sequence.shape == (H, U + X)
    n = opt._bufs["N"]
    rows = opt._bufs["rows"].cpu()
    row_len, reward_col, next_off = cases.icem_layout(X, U + X)
    assert rows.shape[1] == row_len
    xn = rows[(H - 1) * n:, next_off:next_off + X].double()
    u = rows[(H - 1) * n:, X:X + U].double()
    rp = st.system_params.reward_params
    r64 = -(torch.tensor(rp.q).double() * (rows[(H - 1) * n:, :X].double() - torch.tensor(rp.target).double()) ** 2).sum(dim=1) \
        - (torch.tensor(rp.r).double() * u ** 2).sum(dim=1)
    args, kw = case.ref_args()
    torch.testing.assert_close(rows[(H - 1) * n:, reward_col].double(), r64 + tref.v_hat(xn, *args, **kw), atol=cases.TOL64 + 1e-5,
                               rtol=cases.TOL64)
    narrow = _tv(cases.make_case(cases.SHAPES[0], "Q"), dev)                      # a kind-Q value at A = u
    with pytest.raises(ValueError, match="kind-Q value at action_dim 1, the system has action_dim 4"):
        iCemTO(horizon=H, action_dim=system.action_dim, opt_params=iCemParams(**_PARAMS), terminal_value=narrow).set_system(system)
    assert _opt(system, _tv(cases.make_case(cases.SHAPES[0], "V2"), dev)) is not None      # kind V knows no action width


def test_unsupported_widths_are_a_value_error(dev):
    from mbpo import ops
    dims = [3, 96, 96, 1]
    with pytest.raises(ValueError, match="MBPO_ERR_UNSUPPORTED"):
        ops.terminal_value_eval(x_dim=3, action_dim=0, critic_params=torch.zeros(2 * 9793, device=dev), critic_dims=dims, n_critics=2,
                                x=torch.zeros(4, 3, device=dev))


# ------------------------------------------------------------------------------------------------ 7: from a trainer's state
def test_from_sac_reads_the_learner_state(dev):
    from mbpo import ops
    from mbpo.optimizers import SACOptimizer, TerminalValue
    from test_gpu_trainer_parity import SAC_KW, _make_system, _true_buffer
    system, sp, _, X, U = _make_system(dev, "pendulum")
    tb, tbs = _true_buffer(dev, X, U, 512)
    N, S = SAC_KW["num_envs"], SAC_KW["num_env_steps_between_updates"]
    opt = SACOptimizer(system=system, true_buffer=tb, num_timesteps=64 + N * S * 2, use_graph=True, warm_start=True, **SAC_KW)
    out = opt.train(opt.init(key=3, true_buffer_state=tbs).replace(system_params=sp))      # two training steps
    ls = out.optimizer_state.learner_state
    pd, qd = opt._trainer.policy_dims, opt._trainer.q_dims
    opt.close()
    assert float(ls.step_count) == 2 * SAC_KW["grad_updates_per_step"]
    P, Q = ops.MlpSpec(pd).n_params, ops.MlpSpec(qd).n_params
    mean, std = ls.normalizer[1:1 + X], ls.normalizer[1 + 2 * X:1 + 3 * X]
    assert not _same(ls.params[P:P + 2 * Q], ls.target_q) and float(ls.normalizer[0]) > 0
    obs = tb.logical_data(tbs)[:200, :X].contiguous()
    for target in (True, False):
        tv = TerminalValue.from_sac(ls, weight=0.8, target=target)
        assert (tv.policy_dims, tv.critic_dims, tv.action_dim, tv.n_critics) == (list(pd), list(qd), U, 2)
        q = ls.target_q if target else ls.params[P:P + 2 * Q]
        built = TerminalValue(X, q, qd, policy_params=ls.params[:P], policy_dims=pd, norm_mean=mean, norm_std=std, weight=0.8)
        assert _same(tv(obs), built(obs))
        assert _same(TerminalValue.from_sac(out.optimizer_state, pd, qd, weight=0.8, target=target)(obs), tv(obs))
        # the product's own pieces: the deterministic policy's action, then the Q forward on [n(obs) | action]
        act = ops.policy_act(ls.params[:P].contiguous(), ops.MlpSpec(pd), obs, mean.contiguous(), std.contiguous(), deterministic=True)
        q_in = torch.cat([(obs - mean) / std, act], dim=1).contiguous()
        qs = ops.ensemble_mlp_forward(q.contiguous(), ops.MlpSpec(qd, "swish", 2), q_in)[:, :, 0]
        torch.testing.assert_close(tv(obs), 0.8 * qs.min(dim=0).values, atol=cases.TOL32, rtol=cases.TOL32)
    # against the restatement, on the trained tensors
    want = tref.v_hat(obs.cpu().double(), ls.target_q.cpu(), list(qd), 2, "swish", policy=ls.params[:P].cpu(), policy_dims=list(pd),
                      mean=mean.cpu(), std=std.cpu())
    torch.testing.assert_close(TerminalValue.from_sac(ls)(obs).cpu().double(), want, atol=cases.TOL64, rtol=cases.TOL64)


def test_from_bptt_reads_the_target_critic_and_the_state_normaliser(dev):
    from mbpo.optimizers import BPTTOptimizer, TerminalValue
    from test_gpu_host_api import _bptt_pendulum_setup
    system, _, sbs = _bptt_pendulum_setup(dev, buffer_rows=64)
    opt = BPTTOptimizer(action_dim=1, obs_dim=3, horizon=6, num_samples_per_gradient_update=24, train_steps=2, init_stddev=1.5,
                        sampling_buffer_size=4096)
    opt.set_system(system)
    st = opt.train(bptt_state=opt.init(key=11, true_buffer_state=sbs)).optimizer_state        # two train steps
    ns = st.state_normalizer_state
    assert not _same(st.target_critic_params, st.critic_params) and float(ns.size) > 0
    tv = TerminalValue.from_bptt(st, opt.critic_dims, weight=1.7)
    assert (tv.kind, tv.n_critics, tv.critic_dims) == ("V", 2, list(opt.critic_dims))
    assert tv.critic_params.data_ptr() == st.target_critic_params.data_ptr() and tv.norm_std.data_ptr() == ns.std.data_ptr()
    g = torch.Generator().manual_seed(4)
    x = (ns.mean.cpu() + 2 * ns.std.cpu() * torch.randn(150, 3, generator=g)).to(dev)
    built = TerminalValue(3, st.target_critic_params, opt.critic_dims, n_critics=2, norm_mean=ns.mean, norm_std=ns.std, weight=1.7)
    assert _same(tv(x), built(x))
    want = float(torch.tensor(1.7, dtype=torch.float32)) * tref.v_hat(x.cpu().double(), st.target_critic_params.cpu(),
                                                                     list(opt.critic_dims), 2, "swish", mean=ns.mean.cpu(), std=ns.std.cpu())
    torch.testing.assert_close(tv(x).cpu().double(), want, atol=cases.TOL64, rtol=cases.TOL64)


# ------------------------------------------------------------------------------------------------ 8: the example
def test_example_runs_with_a_terminal_value(dev):
    env = dict(os.environ)
    r = subprocess.run([sys.executable, str(ROOT / "examples" / "icem_pendulum.py"), "--terminal-value", "--tv-horizon", "3", "--steps", "3",
                        "--sac-steps", "1500"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("horizon 3")]
    assert len(lines) == 2 and "with the critic" in lines[0] and "without" in lines[1] and "TerminalValue(kind Q" in r.stdout
