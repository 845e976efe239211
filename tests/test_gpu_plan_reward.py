"""Plan rewards on the device (include/mbpo_hip.h "plan rewards"): mbpo_plan_reward_eval alone — the term-table and quadratic kinds bit
for bit against mbpo_reward_eval per (b, t) slice, the Pendulum kind against the fp64 oracle, in all four broadcast forms, dense and in
place, on aligned rows and rows offset by one float, with nothing else written, and under graph replay on changed contents — and through
iCemTO: shared parameters change nothing, problem b of a batched call equals its single call, the schedule against the CPU loop, the
table read late, and a reward that is not the system's own."""
import functools

import numpy as np
import pytest
import torch

import plan_reward_cases as cases
import plan_reward_ref as pref
from test_gpu_icem_batched import _SMALL, _same

pytestmark = pytest.mark.gpu

_POISON = 0x7FC0BEEF      # a quiet NaN with a payload


def _poison(t: torch.Tensor) -> torch.Tensor:
    t.view(torch.int32).fill_(_POISON)
    return t


# ------------------------------------------------------------------------------------------------ the kernel alone
@functools.lru_cache(maxsize=None)
def _host_case(si: int, kind: int):
    """(rows, {form: table}) on the host, built once and left unchanged; the term kind has one row whose next state holds an inf."""
    shape = cases.SHAPES[si]
    rows = cases.make_rows(shape, seed=si, pendulum=kind == pref.PENDULUM)
    if kind == pref.TERMS:
        _, _, next_off = cases.layout(shape[3], shape[5])
        rows[rows.shape[0] // 2, next_off + shape[3] - 1] = float("inf")
    return rows, {form: cases.make_table(kind, form, shape, seed=si) for form in cases.FORMS}


def _expected_bits(kind, table, rows, shape):
    """mbpo_reward_eval per (b, t) slice with that slice's parameters: [n_rows] on the device."""
    from mbpo import ops
    H, B, G, X, U, A = shape
    _, _, next_off = cases.layout(X, A)
    PB, PH, _ = table.shape
    r3 = rows.reshape(H, B, G, -1)
    out = torch.empty(H, B, G, device=rows.device)
    for t in range(H):
        for b in range(B):
            s = r3[t, b]
            out[t, b] = ops.reward_eval(kind, table[b if PB > 1 else 0, t if PH > 1 else 0].contiguous(), s[:, :X].contiguous(),
                                        s[:, X:X + U].contiguous(), s[:, next_off:next_off + X].contiguous())
    return out.reshape(-1)


def _offset_view(t: torch.Tensor, off: int) -> torch.Tensor:
    """A copy of t that starts `off` floats past an allocation's (256-byte aligned) start."""
    flat = torch.empty(t.numel() + off, device=t.device, dtype=t.dtype)
    v = flat[off:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (4 * off) % 16 and v.is_contiguous()
    return v


def _run_all_forms(dev, si, kind, check):
    """Every broadcast form x {dense, in place} x {aligned, offset by one float}: check(form, got [n_rows], shape, table, rows)."""
    from mbpo import ops
    shape = cases.SHAPES[si]
    H, B, G, X, U, A = shape
    row_len, reward_col, next_off = cases.layout(X, A)
    n = H * B * G
    host_rows, tables = _host_case(si, kind)
    for form in cases.FORMS:
        table = tables[form].to(dev)
        want = check(form, None, shape, table, host_rows.to(dev))
        for off in (0, 1):
            rows = _offset_view(host_rows.to(dev), off)
            # the columns the launch must not read or write — reward, discount, truncation, the action columns past u_dim — are poisoned
            dead = [c for c in range(row_len) if not (c < X + U or next_off <= c < next_off + X)]
            for c in dead:
                rows[:, c].view(torch.int32).fill_(_POISON)
            before = rows.clone()
            # dense, between guard words, into a poisoned buffer that starts `off` floats past alignment
            buf = _poison(torch.empty(n + 8 + off, device=dev))
            out = buf[4 + off:4 + off + n]
            ret = ops.plan_reward_eval(kind, table, rows, H, B, G, X, U, next_off, out=out)
            assert ret is out and _same(rows, before), (form, off, "dense: rows changed")
            guards = torch.cat([buf[:4 + off], buf[4 + off + n:]]).view(torch.int32)
            assert bool((guards == _POISON).all()), (form, off, "dense: a guard word was written")
            assert not bool((out.view(torch.int32) == _POISON).any()), (form, off, "dense: an output was not written")
            check(form, out, shape, table, rows, want)
            # in place into the reward column: every other column keeps its bits, and the column holds the dense result's
            ret = ops.plan_reward_eval(kind, table, rows, H, B, G, X, U, next_off, reward_col=reward_col)
            assert ret is rows
            assert _same(rows[:, reward_col].contiguous(), out.contiguous()), (form, off, "in place != dense")
            keep = [c for c in range(row_len) if c != reward_col]
            assert _same(rows[:, keep].contiguous(), before[:, keep].contiguous()), (form, off, "in place: another column changed")
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", [pref.TERMS, pref.QUADRATIC], ids=["terms", "quadratic"])
@pytest.mark.parametrize("si", range(len(cases.SHAPES)))
def test_terms_and_quadratic_equal_reward_eval_bit_for_bit(dev, si, kind):
    def check(form, got, shape, table, rows, want=None):
        if got is None:
            return _expected_bits(kind, table, rows, shape)
        assert _same(got.contiguous(), want), (form, int((got.view(torch.int32) != want.view(torch.int32)).sum()))

    _run_all_forms(dev, si, kind, check)


@pytest.fixture
def force_flat_kernel():
    import ctypes as C
    from mbpo import _hip
    lib = _hip.load()
    lib.mbpo_debug_set_plan_reward_flat.argtypes, lib.mbpo_debug_set_plan_reward_flat.restype = [C.c_int], C.c_int
    assert lib.mbpo_debug_set_plan_reward_flat(1) == 0
    yield
    assert lib.mbpo_debug_set_plan_reward_flat(-1) == 0


@pytest.mark.parametrize("kind", [pref.TERMS, pref.QUADRATIC], ids=["terms", "quadratic"])
@pytest.mark.parametrize("si", [i for i, s in enumerate(cases.SHAPES) if s[2] >= 256])
def test_flat_kernel_on_large_groups_equals_reward_eval_bit_for_bit(dev, force_flat_kernel, si, kind):
    """From group 256 on the dispatch picks the kernel with one (problem, step) per workgroup unless there are more than 65535 problems
    or steps; the flat kernel's branch for such groups (a row's pair is the tile's first or the next) runs here through the hook."""
    def check(form, got, shape, table, rows, want=None):
        if got is None:
            return _expected_bits(kind, table, rows, shape)
        assert _same(got.contiguous(), want), (form, int((got.view(torch.int32) != want.view(torch.int32)).sum()))

    _run_all_forms(dev, si, kind, check)


def test_term_tables_differ_per_problem_and_step(dev):
    """The comparison above has teeth: on shape 2 the [B, H] result differs from the one every slice's first table would give."""
    from mbpo import ops
    shape = cases.SHAPES[2]
    H, B, G, X, U, A = shape
    _, _, next_off = cases.layout(X, A)
    rows, tables = _host_case(2, pref.TERMS)
    rows = rows.to(dev)
    full = ops.plan_reward_eval(pref.TERMS, tables["BH"].to(dev), rows, H, B, G, X, U, next_off).reshape(H, B, G)
    first = ops.plan_reward_eval(pref.TERMS, tables["BH"][:1, :1].contiguous().to(dev), rows, H, B, G, X, U, next_off).reshape(H, B, G)
    assert _same(full[0, 0], first[0, 0])
    for t in range(H):
        for b in range(B):
            if (t, b) != (0, 0):
                assert not bool((full[t, b] == first[t, b]).any()), (t, b)
    assert bool(torch.isfinite(full).all())                                   # the row with the inf next state included


@pytest.mark.parametrize("si", [i for i, s in enumerate(cases.SHAPES) if (s[3], s[4]) == (3, 1)])
def test_pendulum_kind_against_the_fp64_oracle(dev, si):
    def check(form, got, shape, table, rows, want=None):
        H, B, G, X, U, A = shape
        if got is None:
            return pref.rows_reward(pref.PENDULUM, table.cpu(), rows.cpu().double(), H, B, G, X, U, cases.layout(X, A)[2])
        err = (got.cpu().double() - want).abs()
        print(f"pendulum kind, shape {si} form {form}: max |err| {float(err.max()):.3e} at max |r| {float(want.abs().max()):.2f}")
        assert bool((err <= 5e-5 + 5e-5 * want.abs()).all()), (form, float(err.max()))

    _run_all_forms(dev, si, pref.PENDULUM, check)


@pytest.mark.parametrize("kind", [pref.TERMS, pref.PENDULUM], ids=["terms", "pendulum"])
def test_captured_launch_replays_on_changed_table_and_rows(dev, kind):
    from mbpo import ops
    si = 4 if kind == pref.PENDULUM else 2
    shape = cases.SHAPES[si]
    H, B, G, X, U, A = shape
    _, _, next_off = cases.layout(X, A)
    host_rows, tables = _host_case(si, kind)
    rows, table = host_rows.to(dev), tables["BH"].to(dev)
    n = H * B * G
    out = torch.full((n,), float("nan"), device=dev)
    first = ops.plan_reward_eval(kind, table, rows, H, B, G, X, U, next_off, out=out).clone()      # (one eager call first: the code object)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.plan_reward_eval(kind, table, rows, H, B, G, X, U, next_off, out=out)
    ptrs = (table.data_ptr(), rows.data_ptr())
    for r in range(2):
        rows.copy_(cases.make_rows(shape, seed=50 + r, pendulum=kind == pref.PENDULUM).to(dev))
        table.copy_(cases.make_table(kind, "BH", shape, seed=50 + r).to(dev))
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        eager = ops.plan_reward_eval(kind, table, rows, H, B, G, X, U, next_off)
        assert _same(out, eager) and not bool((out == first).all())
    assert ptrs == (table.data_ptr(), rows.data_ptr())


# ------------------------------------------------------------------------------------------------ through iCemTO
def _with(st, prp):
    return st.replace(system_params=st.system_params.replace(reward_params=prp))


def _opt(system, H, **kw):
    from mbpo.optimizers import iCemParams, iCemTO
    params = kw.pop("params", None) or iCemParams(**_SMALL)
    opt = iCemTO(horizon=H, action_dim=system.action_dim, opt_params=params, key=5, **kw)
    opt.set_system(system)
    return opt


def _pendulum_starts(dev, B, H, seed=0):
    g = torch.Generator().manual_seed(seed)
    ang = torch.rand(B, generator=g) * 6.28
    x0 = torch.stack([torch.cos(ang), torch.sin(ang), torch.randn(B, generator=g)], dim=1)
    warm = (torch.rand(B, H, 1, generator=g) - 0.5) * 1.5
    return x0.to(dev), warm.to(dev)


def _ensemble_starts(dev, B, H, X, A, seed=3):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, X, generator=g) * 0.5).to(dev), ((torch.rand(B, H, A, generator=g) - 0.5) * 1.5).to(dev)


def _slice_problem(prp, b):
    from mbpo.systems import PlanRewardParams
    return PlanRewardParams(prp.reward, prp.table[b:b + 1].contiguous() if prp.problems > 1 else prp.table, base=prp.base)


def _compare_with_sliced_single_calls(opt, x0, warm, prp, init_key=7):
    """_compare_with_single_calls of tests/test_gpu_icem_batched.py with the state's parameters sliced per problem: problem b of the
    batched optimize under `prp` vs the single optimize on (x0[b], warm[b], key[b]) under table[b:b + 1]."""
    from mbpo.utils import keys as K
    B = x0.shape[0]
    bst = _with(opt.init(init_key, batch_size=B).replace(best_sequence=warm.clone()), prp)
    bnew = opt.optimize(x0, bst)
    sst = opt.init(init_key)
    assert bst.key == K.split(sst.key, B)
    for b in range(B):
        one = opt.optimize(x0[b], _with(sst.replace(key=bst.key[b], best_sequence=warm[b].clone()), _slice_problem(prp, b)))
        assert _same(bnew.best_sequence[b], one.best_sequence), f"problem {b}: best_sequence"
        assert _same(bnew.best_reward[b], one.best_reward), f"problem {b}: best_reward"
        assert bnew.key[b] == one.key == K.split(bst.key[b], 2)[1], f"problem {b}: key"
    torch.cuda.synchronize()
    assert bool(torch.isfinite(bnew.best_reward).all())
    assert bnew.system_params.reward_params is prp
    return bnew


def _xnext_term_reward(X, U):
    from mbpo.systems import Group, Term, TermReward
    return TermReward(X, U, bias=0.1, groups=[
        Group([Term("x", c, "square", 0.5 + 0.1 * c, 0.1) for c in range(X)], weight=-1.0),
        Group([Term("u", d, "square", 0.3) for d in range(U)], weight=-1.0),
        Group([Term("x_next", 0, "square", -1.5, 0.1), Term("x_next", X - 1, "cos", 0.2, 0.0)], weight=0.5, link="exp")])


def _shared_changes_nothing(dev, system, H, B, exact=True):
    """A [1, 1, P] table holding the system's own reward vector against the plain optimize, single and batched."""
    from mbpo.systems import PlanRewardParams
    opt = _opt(system, H)
    X, A = system.x_dim, system.action_dim
    x0, warm = _pendulum_starts(dev, B, H) if X == 3 and A == 1 else _ensemble_starts(dev, B, H, X, A)
    same = True
    for batch in (None, B):
        st = opt.init(7, batch_size=batch)
        st = st.replace(best_sequence=(warm if batch else warm[0]).clone())
        xs = x0 if batch else x0[0]
        plain = opt.optimize(xs, st)
        vec = system.reward.kernel_spec(st.system_params.reward_params, dev)[1]
        prp = PlanRewardParams(system.reward, vec.reshape(1, 1, -1).clone())
        planned = opt.optimize(xs, _with(st, prp))
        assert planned.key == plain.key
        bits = _same(planned.best_sequence, plain.best_sequence) and _same(planned.best_reward, plain.best_reward)
        same &= bits
        if exact:
            assert bits, f"batch {batch}"
        else:
            print(f"shared Pendulum parameters, batch {batch}: bits equal = {bits}, max |d best_reward| = "
                  f"{float((planned.best_reward - plain.best_reward).abs().max()):.3e}")
            torch.testing.assert_close(planned.best_reward, plain.best_reward, atol=1e-5, rtol=0)
            torch.testing.assert_close(planned.best_sequence, plain.best_sequence, atol=1e-5, rtol=0)
    return same


def test_shared_quadratic_parameters_change_nothing(dev):
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, QuadraticReward
    X, U = 4, 2
    system = EnsembleSystem(EnsembleDynamics(X, U, n_members=5, device=dev),
                            QuadraticReward(X, U, target=[0.1, 0.0, 0.0, 0.0], q=[1.0, 2.0, 0.5, 0.1], r=[0.3] * U))
    _shared_changes_nothing(dev, system, 8, 3)


@pytest.mark.parametrize("mode,noise", [("mean", False), ("ts1", True)])
def test_shared_term_table_with_next_state_terms_changes_nothing(dev, mode, noise):
    from mbpo.systems import EnsembleDynamics, EnsembleSystem
    X, U = 4, 2
    system = EnsembleSystem(EnsembleDynamics(X, U, n_members=5, device=dev), _xnext_term_reward(X, U), mode=mode, sample_noise=noise)
    _shared_changes_nothing(dev, system, 8, 3)


def test_shared_pendulum_parameters_change_nothing(dev):
    """One inlined function at two sites need not contract identically: atol 1e-5, the bits are reported (DESIGN.md has the record)."""
    from mbpo.systems import PendulumSystem
    _shared_changes_nothing(dev, PendulumSystem(), 10, 3, exact=False)


def _pendulum_plan(dev, targets):
    """PlanRewardParams of the Pendulum's own reward from nested target angles [PB][PH]."""
    from mbpo.systems import PlanRewardParams
    from mbpo.systems.rewards.pendulum_reward import PendulumRewardParams
    return lambda reward: PlanRewardParams.stack(reward, [[PendulumRewardParams(target_angle=float(a)) for a in row] for row in targets], dev)


@pytest.mark.parametrize("schedule", [False, True], ids=["per_problem", "per_problem_and_step"])
def test_batched_pendulum_targets_equal_single_calls(dev, schedule):
    from mbpo.systems import PendulumSystem
    B, H = 5, 10
    system = PendulumSystem()
    opt = _opt(system, H)
    x0, warm = _pendulum_starts(dev, B, H)
    base = [0.0, 0.7, -2.0, 3.0, 1.5]
    targets = [[a + 0.05 * t for t in range(H)] for a in base] if schedule else [[a] for a in base]
    prp = _pendulum_plan(dev, targets)(system.reward)
    assert (prp.problems, prp.steps) == (B, H if schedule else 1)
    new = _compare_with_sliced_single_calls(opt, x0, warm, prp)
    assert len(set(float(v) for v in new.best_reward)) == B


def _quadratic_plan(dev, system, B, X, U):
    from mbpo.systems import PlanRewardParams
    from mbpo.systems.rewards.pendulum_reward import QuadraticRewardParams
    g = torch.Generator().manual_seed(11)
    nested = [[QuadraticRewardParams((torch.rand(X, generator=g) - 0.5).tolist(), [1.0, 2.0, 0.5, 0.1][:X], [0.3] * U)] for _ in range(B)]
    return PlanRewardParams.stack(system.reward, nested, dev)


def test_batched_ensemble_ts1_noise_with_quadratic_targets_equals_single_calls(dev):
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, QuadraticReward
    X, U, E, H, B = 4, 2, 5, 8, 3
    system = EnsembleSystem(EnsembleDynamics(X, U, n_members=E, device=dev), QuadraticReward(X, U), mode="ts1", sample_noise=True)
    opt = _opt(system, H)
    x0, warm = _ensemble_starts(dev, B, H, X, U)
    _compare_with_sliced_single_calls(opt, x0, warm, _quadratic_plan(dev, system, B, X, U))


def test_batched_optimistic_ensemble_eta_never_enters(dev):
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, QuadraticReward
    X, U, H, B = 4, 2, 8, 3
    system = EnsembleSystem(EnsembleDynamics(X, U, n_members=5, device=dev), QuadraticReward(X, U), mode="optimistic", beta=1.5)
    assert system.action_dim == U + X
    opt = _opt(system, H)
    x0, warm = _ensemble_starts(dev, B, H, X, U + X)
    _compare_with_sliced_single_calls(opt, x0, warm, _quadratic_plan(dev, system, B, X, U))


def test_batched_targets_with_a_term_cost_under_pessimism_equal_single_calls(dev):
    from mbpo.optimizers import iCemParams
    from mbpo.systems import Group, PendulumSystem, Term, TermCost
    B, H = 4, 10
    system = PendulumSystem()
    cost = TermCost(3, 1, bias=-3.0, groups=[Group([Term("x_next", 2, "abs")])], reduce="max")
    opt = _opt(system, H, params=iCemParams(**dict(_SMALL, lambda_constraint=50.0)), cost_fn=cost, use_pessimism=True)
    x0, warm = _pendulum_starts(dev, B, H, seed=2)
    _compare_with_sliced_single_calls(opt, x0, warm, _pendulum_plan(dev, [[0.0], [1.0], [-1.0], [2.5]])(system.reward))


def test_single_pendulum_schedule_against_the_cpu_loop(dev):
    """A [1, H] target schedule against tests/plan_reward_ref.py's loop: the parameters and the tolerance of
    tests/test_gpu_icem.py::test_icem_optimize_matches_oracle_loop_on_pendulum."""
    from mbpo.optimizers import iCemParams
    from mbpo.systems import PendulumSystem
    params = iCemParams(num_particles=2, num_samples=120, num_elites=12, num_steps=3, exponent=1.0, alpha=0.1, init_std=0.6)
    H = 10
    system = PendulumSystem()
    opt = _opt(system, H, params=params)
    st = opt.init(7)
    st = st.replace(best_sequence=(torch.rand(H, 1, device=dev) - 0.5))
    x0 = torch.tensor([-0.8, 0.6, 0.5], device=dev)
    targets = [float(np.float32(0.1 * t)) for t in range(H)]
    prp = _pendulum_plan(dev, [targets])(system.reward)
    new = opt.optimize(x0, _with(st, prp))
    torch.cuda.synchronize()
    best_v, best_s = pref.icem_loop(pref.pendulum_step_t(targets), x0.cpu().double().numpy(), st.best_sequence.cpu().double().numpy(),
                                    params, H, 1, st.key)
    print(f"schedule vs CPU loop: best_reward {float(new.best_reward):.6f} / {best_v:.6f}, max |d best_sequence| "
          f"{float(np.abs(new.best_sequence.cpu().numpy() - best_s).max()):.3e}")
    assert abs(float(new.best_reward) - best_v) <= 2e-3 * max(1.0, abs(best_v))
    np.testing.assert_allclose(new.best_sequence.cpu().numpy(), best_s, atol=5e-3)
    # and the schedule matters: the loop under the constant first target ends elsewhere
    flat_v, _ = pref.icem_loop(pref.pendulum_step_t([targets[0]] * H), x0.cpu().double().numpy(), st.best_sequence.cpu().double().numpy(),
                               params, H, 1, st.key)
    assert abs(flat_v - best_v) > 1e-2


def test_the_table_is_read_and_read_late(dev):
    from mbpo.systems import PendulumSystem
    H = 10
    system = PendulumSystem()
    opt = _opt(system, H)
    x0, warm = _pendulum_starts(dev, 1, H, seed=5)
    st = opt.init(7).replace(best_sequence=warm[0].clone())
    a = _pendulum_plan(dev, [[0.0]])(system.reward)
    c = _pendulum_plan(dev, [[1.5]])(system.reward)
    ra, rc = opt.optimize(x0[0], _with(st, a)), opt.optimize(x0[0], _with(st, c))
    assert ra.key == rc.key
    assert not _same(ra.best_sequence, rc.best_sequence) and float(ra.best_reward) != float(rc.best_reward)
    # the same object, refilled in place between two calls: the second call is a fresh object's that holds the new numbers
    ptr = a.table.data_ptr()
    a.table.copy_(c.table)
    again = opt.optimize(x0[0], _with(st, a))
    assert a.table.data_ptr() == ptr
    assert _same(again.best_sequence, rc.best_sequence) and _same(again.best_reward, rc.best_reward)
    # a schedule, batched, refilled the same way
    B = 3
    xb, wb = _pendulum_starts(dev, B, H, seed=6)
    bst = opt.init(7, batch_size=B).replace(best_sequence=wb.clone())
    sched = _pendulum_plan(dev, [[0.1 * t + b for t in range(H)] for b in range(B)])(system.reward)
    other = _pendulum_plan(dev, [[0.5 * b - 0.05 * t for t in range(H)] for b in range(B)])(system.reward)
    r1, r2 = opt.optimize(xb, _with(bst, sched)), opt.optimize(xb, _with(bst, other))
    assert not _same(r1.best_sequence, r2.best_sequence)
    sched.table.copy_(other.table)
    r3 = opt.optimize(xb, _with(bst, sched))
    assert _same(r3.best_sequence, r2.best_sequence) and _same(r3.best_reward, r2.best_reward)


def test_a_foreign_term_reward_on_the_pendulum(dev):
    """PendulumSystem planned under -(cos - c)^2 - (sin - s)^2 - 0.1 thetadot^2 - 0.02 u^2 with (c, s) per problem: equal to its single
    calls bit for bit, and the objective values of the last iteration equal to the reference on the rollout's own rows."""
    from mbpo.systems import Group, PendulumSystem, PlanRewardParams, Term, TermReward, TermRewardParams
    B, H = 3, 8
    system = PendulumSystem()
    reward = TermReward(3, 1)
    goals = [(1.0, 0.0), (0.0, 1.0), (-0.6, 0.8)]
    nested = [[TermRewardParams(3, 1, 0.0, (Group((Term("x", 0, "square", -1.0, c), Term("x", 1, "square", -1.0, s),
                                                       Term("x", 2, "square", -0.1, 0.0), Term("u", 0, "square", -0.02, 0.0))),))]
              for c, s in goals]
    prp = PlanRewardParams.stack(reward, nested, dev)
    assert prp.reward is not system.reward and prp.param_len == 580
    opt = _opt(system, H)
    x0, warm = _pendulum_starts(dev, B, H, seed=8)
    new = _compare_with_sliced_single_calls(opt, x0, warm, prp)
    assert len(set(float(v) for v in new.best_reward)) == B
    # one more batched call, then its buffers: rows [H * B * NC * P, row_len], the rewards under the table [H * B * NC * P], values [B * NC]
    opt.optimize(x0, _with(opt.init(7, batch_size=B).replace(best_sequence=warm.clone()), prp))
    torch.cuda.synchronize()
    b = opt._bbufs
    NC, P = b["NC"], opt.opt_params.num_particles
    rows = b["rows"].cpu().double()
    want_r = pref.rows_reward(pref.TERMS, prp.table.cpu(), rows, H, B, NC * P, 3, 1, next_off=3 + 1 + 2)
    got_r = b["plan_reward"].cpu().double()                                  # the dense buffer the update read
    # (|r| <= 1 + 1 + 6.4 + 0.02 at |thetadot| <= 8: four products and four sums, each rounded to within ulp(8) / 2 = 4.8e-7)
    assert float((got_r - want_r).abs().max()) <= 1e-5
    want_v = want_r.reshape(H, B, NC, P).mean(dim=0).mean(dim=2).reshape(-1)
    err = float((b["values"].cpu().double() - want_v).abs().max())
    print(f"foreign term reward: max |objective - reference| = {err:.3e}")
    assert err <= 1e-5
    # by hand, one row: the reference is the formula
    x, u = rows[0, :3], rows[0, 3]
    c, s = goals[0]
    assert abs(float(want_r[0]) - float(-(x[0] - c) ** 2 - (x[1] - s) ** 2 - 0.1 * x[2] ** 2 - np.float32(0.02) * u ** 2)) <= 1e-6


def test_quadratic_reward_call_goes_through_reward_eval(dev):
    """QuadraticReward.__call__ (it raised NotImplementedError): mbpo_reward_eval's bits, Normal(reward, 0), batched and on one state."""
    from mbpo import _hip, ops
    from mbpo.systems import QuadraticReward
    from oracle import systems as osys
    X, U, n = 4, 2, 300
    reward = QuadraticReward(X, U, target=[0.1, -0.2, 0.0, 0.3], q=[1.0, 2.0, 0.5, 0.1], r=[0.3, 0.05])
    p = reward.init_params(0)
    g = torch.Generator().manual_seed(21)
    x, u = (torch.rand(n, X, generator=g) * 2 - 1).to(dev), (torch.rand(n, U, generator=g) * 2 - 1).to(dev)
    dist, back = reward(x, u, p)
    assert back is p and dist.mean().shape == (n,) and not bool(dist.scale.any())
    assert _same(dist.mean(), ops.reward_eval(_hip.REWARD_QUADRATIC, reward.kernel_spec(p, dev)[1], x, u))
    c = lambda v: torch.tensor(v, dtype=torch.float32).double()
    want = osys.quadratic_reward(x.cpu().double(), u.cpu().double(), c(p.target), c(p.q), c(p.r))
    # (|r| <= 1.21 + 2.88 + 0.5 + 0.17 + 0.35 at inputs in [-1, 1]: six fused multiply-adds and a subtraction, each within ulp(8) / 2 = 4.8e-7)
    assert float((dist.mean().cpu().double() - want).abs().max()) <= 1e-5
    one, _ = reward(x[7], u[7], p)
    assert one.mean().shape == () and _same(one.mean(), dist.mean()[7])
