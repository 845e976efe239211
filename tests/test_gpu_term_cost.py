"""GPU: the term cost (mbpo.systems.TermCost, include/mbpo_hip.h "term costs") — mbpo_traj_cost_eval against the sequential fp32 sum /
maximum of mbpo_reward_eval's values bit for bit (past the grid cap, off 16-byte alignment, under every number of step slots the launch
code can pick), against the fp64 torch form, NaN and non-finite rows, poisoned outputs and guards, iCEM with a TermCost on the Pendulum
against the callable path, batched against single calls, an optimistic system's [u | eta] action columns, and a captured launch.

Tolerances: bits wherever the same fp32 operations run in the same order; against fp64, H times the tolerance
tests/test_gpu_term_reward.py uses for one evaluation (a sum of H values carries H evaluation errors; its own H - 1 roundings are below
one of them at these magnitudes).
"""
import ctypes as C
import functools
import re
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
ICEM_HIP = (ROOT / "model-based-policy-optimizers_amd" / "csrc" / "icem.hip").read_text()


def _launch_define(name):
    m = re.search(rf"#define {name} (\d+)\s", ICEM_HIP)
    assert m, name
    return int(m.group(1))


GRID_CAP_THREADS = _launch_define("TRAJ_COST_MAX_BLOCKS") * _launch_define("TRAJ_COST_BLOCK")      # the launch code's own cap
SLOTS = [1 << k for k in range(_launch_define("TRAJ_COST_MAX_SLOTS").bit_length())]                 # 1, 2, .., 32: steps in flight per workgroup
# (x, u, A, H, n_traj): smallest; ragged last wave; action wider than u (the optimistic layout, odd row_len); wide rows; past the grid
# cap, where every thread walks two or three trajectories
SHAPES = [(3, 1, 1, 1, 1), (3, 1, 1, 20, 37), (3, 1, 4, 5, 513), (17, 6, 6, 3, 4097), (3, 1, 1, 2, 2 * GRID_CAP_THREADS + 37)]
SHAPE_IDS = ["smallest", "ragged_wave", "wide_action", "wide_rows", "past_grid_cap"]


def _set_slots(slots):
    from mbpo import _hip
    lib = _hip.load()
    lib.mbpo_debug_set_traj_cost_slots.argtypes = [C.c_int]
    lib.mbpo_debug_set_traj_cost_slots.restype = C.c_int
    assert lib.mbpo_debug_set_traj_cost_slots(slots) == 0


@pytest.fixture
def traj_cost_slots():
    yield _set_slots
    _set_slots(-1)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _table12(X, U, reduce):
    """12 terms in 5 groups: cos / sin / square / abs / relu terms under identity, exp, sqrt and tanh links, two of them on x_next; the
    last control column and the last state column are read, so that a wrong column offset shows."""
    from mbpo.systems import Group, Term, TermCost
    groups = [
        Group([Term("x", 0, "cos", 1.0, 0.1), Term("x", X - 1, "sin", 0.7, -0.2), Term("u", 0, "square", 0.3, 0.0)], weight=0.5),
        Group([Term("x", 1, "square", -0.9, 0.2), Term("x_next", 0, "square", -0.6, -0.1)], weight=0.8, link="exp"),
        Group([Term("x", 2, "square", 1.0, 0.3), Term("x_next", X - 1, "square", 0.5, 0.0), Term("u", U - 1, "square", 0.2, 0.1)],
              weight=-0.4, link="sqrt"),
        Group([Term("x", X // 2, "identity", 1.2, 0.0), Term("u", U - 1, "identity", -0.7, 0.0)], weight=0.3, link="tanh"),
        Group([Term("x", 1, "abs", 0.5, 0.15), Term("x", 0, "relu", 0.6, -0.1)], weight=-0.25),
    ]
    assert sum(len(g.terms) for g in groups) == 12
    return TermCost(X, U, bias=0.05, groups=groups, reduce=reduce)


def _off_by_one_float(rows):
    """The same rows one float past their allocation's start: the buffer is off 16-byte (and 8-byte) alignment."""
    buf = torch.empty(rows.numel() + 1, device=rows.device, dtype=rows.dtype)
    buf[1:].copy_(rows.reshape(-1))
    out = buf[1:].view(rows.shape)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Rows of one shape, uniform in [-1, 1], and the per-row reference computed once and left unchanged: mbpo_reward_eval on the rows'
    own columns, then the sum / maximum over the steps accumulated on the host in ascending t over float32 tensors."""
    from mbpo import _hip, ops
    X, U, A, H, n = shape
    dev = torch.device("cuda:0")
    row_len, next_off = 2 * X + A + 3, X + A + 2
    g = torch.Generator().manual_seed(900 + SHAPES.index(shape))
    rows = (torch.rand(H * n, row_len, generator=g) * 2 - 1).to(dev)
    table = _table12(X, U, "sum").table(dev)
    stage = ops.reward_eval(_hip.REWARD_TERMS, table, rows[:, :X].contiguous(), rows[:, X:X + U].contiguous(),
                            rows[:, next_off:next_off + X].contiguous()).cpu().reshape(H, n)
    acc, top = torch.zeros(n, dtype=torch.float32), stage[0].clone()
    for t in range(H):
        acc = acc + stage[t]
        top = torch.maximum(top, stage[t])
    return dict(rows=rows, row_len=row_len, next_off=next_off, stage=stage, sum=acc, max=top)


# ------------------------------------------------------------------------------------------------ 1. bits
@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "off_by_one_float"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_cost_is_the_sequential_sum_of_reward_eval_bit_for_bit(dev, shape, offset):
    X, U, A, H, n = shape
    c = _case(shape)
    rows = _off_by_one_float(c["rows"]) if offset else c["rows"]
    if SHAPE_IDS[SHAPES.index(shape)] == "past_grid_cap":
        assert n > 2 * GRID_CAP_THREADS
    for reduce in ("sum", "max"):
        got = _table12(X, U, reduce).trajectory_cost(rows, H, n, next_off=c["next_off"]).cpu()
        assert got.shape == (n,) and _same(got, c[reduce]), f"{reduce}: {int((_bits(got) != _bits(c[reduce])).sum())} of {n} differ"
    assert H * n == 1 or float(c["stage"].std()) > 0.05                  # the rows are not all alike
    # the rollout's own layout is the default next_off
    assert _same(_table12(X, U, "sum").trajectory_cost(rows, H, n).cpu(), c["sum"])


@pytest.mark.parametrize("slots", SLOTS)
@pytest.mark.parametrize("shape", SHAPES[:4], ids=SHAPE_IDS[:4])
def test_every_slot_count_gives_the_same_bits(dev, traj_cost_slots, shape, slots):
    """The launch code spreads the steps of a trajectory over 1 .. 32 slots of a workgroup by horizon and trajectory count; forced to each
    value in turn (more slots than steps included), the cost is the same sequential sum / maximum, off alignment too."""
    X, U, A, H, n = shape
    c = _case(shape)
    traj_cost_slots(slots)
    rows = _off_by_one_float(c["rows"])
    for reduce in ("sum", "max"):
        cost = _table12(X, U, reduce)
        assert _same(cost.trajectory_cost(c["rows"], H, n).cpu(), c[reduce]), reduce
        assert _same(cost.trajectory_cost(rows, H, n).cpu(), c[reduce]), reduce


@pytest.mark.parametrize("slots", [2, SLOTS[-1]])
def test_slots_past_the_grid_cap(dev, traj_cost_slots, slots):
    """More tiles than the grid cap with the steps spread over slots: a workgroup walks several tiles through its barriers."""
    shape = SHAPES[4]
    X, U, A, H, n = shape
    c = _case(shape)
    assert n * slots > 2 * GRID_CAP_THREADS
    traj_cost_slots(slots)
    for reduce in ("sum", "max"):
        assert _same(_table12(X, U, reduce).trajectory_cost(c["rows"], H, n).cpu(), c[reduce]), reduce


# ------------------------------------------------------------------------------------------------ 2. fp64
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_cost_against_the_fp64_torch_form(dev, shape):
    import test_gpu_term_reward as tgr
    X, U, A, H, n = shape
    c = _case(shape)
    tol = H * tgr.EVAL_TOL
    r3 = c["rows"].double().reshape(H, n, -1).transpose(0, 1)          # [n, H, row_len]
    obs, act, nxt = r3[..., :X], r3[..., X:X + A], r3[..., c["next_off"]:c["next_off"] + X]
    for reduce in ("sum", "max"):
        cost = _table12(X, U, reduce)
        want = torch.func.vmap(lambda o, a, nx: cost(o, a, next_observation=nx))(obs, act, nxt).cpu()
        assert want.dtype == torch.float64
        got = c[reduce].double()
        print(f"{SHAPE_IDS[SHAPES.index(shape)]} {reduce}: max |kernel - fp64| = {float((got - want).abs().max()):.3e} (tol {tol:.1e})")
        torch.testing.assert_close(got, want, atol=tol, rtol=tol)


# ------------------------------------------------------------------------------------------------ 3. NaN and non-finite rows
def test_nan_stage_cost_and_non_finite_next_state(dev):
    shape = SHAPES[1]
    X, U, A, H, n = shape
    c = _case(shape)
    row = lambda t, i: t * n + i
    # a NaN in a column the table reads through cos: that step's cost is NaN, and so is the trajectory's, in both reduces
    rows = c["rows"].clone()
    rows[row(7, 5), 0] = float("nan")
    for reduce in ("sum", "max"):
        got = _table12(X, U, reduce).trajectory_cost(rows, H, n).cpu()
        keep = torch.arange(n) != 5
        assert bool(torch.isnan(got[5])) and _same(got[keep], c[reduce][keep]), reduce
    # the NaN step first and last: the running maximum neither starts past it nor drops it at the end
    for t in (0, H - 1):
        rows = c["rows"].clone()
        rows[row(t, 11), 0] = float("nan")
        got = _table12(X, U, "max").trajectory_cost(rows, H, n).cpu()
        assert bool(torch.isnan(got[11])) and int(torch.isnan(got).sum()) == 1
    # a next state with a non-finite component reads the observation: finite, and the bits of the rows with x_next = x
    rows, fixed = c["rows"].clone(), c["rows"].clone()
    no = c["next_off"]
    for (t, i, col, v) in ((3, 9, 1, float("inf")), (11, 20, 0, float("nan")), (19, 36, X - 1, float("-inf"))):
        rows[row(t, i), no + col] = v
        fixed[row(t, i), no:no + X] = fixed[row(t, i), :X]
    for reduce in ("sum", "max"):
        cost = _table12(X, U, reduce)
        got, want = cost.trajectory_cost(rows, H, n).cpu(), cost.trajectory_cost(fixed, H, n).cpu()
        assert bool(torch.isfinite(got).all()) and _same(got, want), reduce
        if reduce == "sum":                                              # (a maximum need not move when one step's cost does)
            changed = (_bits(got) != _bits(c[reduce])).nonzero().flatten().tolist()
            assert changed == [9, 20, 36]                                # the three trajectories did change, and only they


# ------------------------------------------------------------------------------------------------ 4. poison
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2]], ids=[SHAPE_IDS[1], SHAPE_IDS[2]])
def test_cost_is_fully_overwritten_and_nothing_else_is_written(dev, shape):
    X, U, A, H, n = shape
    c = _case(shape)
    G = 64
    before = c["rows"].clone()
    for reduce in ("sum", "max"):
        buf = torch.full((G + n + G,), float("nan"), device=dev)
        out = _table12(X, U, reduce).trajectory_cost(c["rows"], H, n, out=buf[G:G + n])
        torch.cuda.synchronize()
        assert out.data_ptr() == buf[G:].data_ptr()
        got = buf.cpu()
        assert _same(got[G:G + n], c[reduce])                            # every element written (none is still NaN)
        assert bool(torch.isnan(got[:G]).all()) and bool(torch.isnan(got[G + n:]).all())
    assert _same(c["rows"], before)


# ------------------------------------------------------------------------------------------------ 5. iCEM on the Pendulum
LIMIT = 5.0
_ICEM = dict(num_particles=4, num_samples=40, num_elites=8, exponent=1.0, alpha=0.1, init_std=0.6, lambda_constraint=100.0)
H_ICEM = 10


def _speed_cost(on):
    """max_t(|theta_dot| - 5) on the pre-step state ("x") or on the step's next state ("x_next")."""
    from mbpo.systems import Group, Term, TermCost
    return TermCost(3, 1, bias=-LIMIT, groups=[Group([Term(on, 2, "abs")])], reduce="max")


def _pendulum_x0(dev):
    th = 2.5
    return torch.tensor([torch.cos(torch.tensor(th)), torch.sin(torch.tensor(th)), 4.5], device=dev)      # falling, close to the limit


def _optimize(dev, cost_fn, num_steps, **kw):
    from mbpo.optimizers import iCemParams, iCemTO
    from mbpo.systems import PendulumSystem
    opt = iCemTO(horizon=H_ICEM, action_dim=1, opt_params=iCemParams(num_steps=num_steps, **_ICEM), key=5, cost_fn=cost_fn, **kw)
    opt.set_system(PendulumSystem())
    new = opt.optimize(_pendulum_x0(dev), opt.init(7))
    torch.cuda.synchronize()
    return opt, new


def test_icem_values_equal_the_callable_paths(dev):
    """One iteration with the same table on both paths — the kernel (cost_fn is the TermCost) and torch.func.vmap (cost_fn is a lambda
    around it; the x-only variant, which a cost_fn(observation, action) can express).  The costs differ by fp32 rounding at most (one
    evaluation each, then a maximum) and lambda_constraint multiplies the difference: rtol 1e-5 plus atol lambda_constraint * 1e-5."""
    cost = _speed_cost("x")
    kern, _ = _optimize(dev, cost, 1)
    call, _ = _optimize(dev, lambda o, a: cost(o, a), 1)
    assert kern._term_cost is cost and call._term_cost is None and "term_cost" not in call._bufs
    kc, cc = kern._bufs["term_cost"].cpu(), call._bufs["cost"].cpu()
    assert int((kc > 0).sum()) >= 4 and int((kc < 0).sum()) >= 4         # the constraint binds for some candidates and not for others
    torch.testing.assert_close(kc, cc, rtol=1e-5, atol=1e-5)
    lam = _ICEM["lambda_constraint"]
    kv, cv = kern._bufs["values"].cpu(), call._bufs["values"].cpu()
    print(f"max |values(kernel) - values(callable)| = {float((kv - cv).abs().max()):.3e}")
    torch.testing.assert_close(kv, cv, rtol=1e-5, atol=lam * 1e-5)
    free, _ = _optimize(dev, None, 1)
    assert not torch.allclose(kv, free._bufs["values"].cpu(), rtol=1e-3, atol=1e-3)      # and it does enter the objective


def test_icem_term_cost_steers_the_plan(dev):
    """The constraint max_t(|theta_dot_{t+1}| - 5) through an x_next term: the constrained plan's true speed violation over the horizon
    is smaller than the unconstrained plan's (same keys), on the oracle's Pendulum in fp64."""
    from oracle import systems as osys
    _, free = _optimize(dev, None, 3)
    _, con = _optimize(dev, _speed_cost("x_next"), 3)
    osystem = osys.PendulumSystem()

    def violation(seq):
        x, worst = _pendulum_x0(dev).cpu().double()[None], 0.0
        for t in range(H_ICEM):
            x, _ = osystem.step(x, seq[t].cpu().double()[None])
            worst = max(worst, float(x[0, 2].abs()) - LIMIT)
        return worst

    v_free, v_con = violation(free.best_sequence), violation(con.best_sequence)
    print(f"speed violation: unconstrained {v_free:.3f}, constrained {v_con:.3f}")
    assert v_free > 0.3                                                  # the unconstrained plan does exceed the limit
    assert v_con < v_free


# ------------------------------------------------------------------------------------------------ 6. batched equals single
@pytest.mark.parametrize("optimism", [False, True])
def test_batched_term_cost_with_pessimism_equals_single_calls(dev, optimism):
    import test_gpu_icem_batched as tb
    from mbpo.optimizers import iCemParams
    params = iCemParams(**dict(tb._SMALL, lambda_constraint=50.0))
    from mbpo.systems import Group, Term, TermCost
    cost = TermCost(3, 1, bias=-2.0, reduce="max", groups=[Group([Term("x_next", 2, "abs")]),
                                                           Group([Term("u", 0, "relu", 1.0, 0.2)], weight=0.5)])
    opt, x0, warm = tb._pendulum_case(dev, 4, 10, params, seed=2, cost_fn=cost, use_pessimism=True, use_optimism=optimism)
    new = tb._compare_with_single_calls(opt, x0, warm)
    assert bool(torch.isfinite(new.best_reward).all())
    assert opt._bbufs["term_cost"].shape == (opt._bbufs["NT"],) and int((opt._bbufs["term_cost"] > 0).sum()) > 0


# ------------------------------------------------------------------------------------------------ 7. optimistic system
def test_optimistic_system_reads_the_controls_only(dev):
    """iCEM on EnsembleSystem(mode="optimistic"): the action columns are [u | eta] (A = u + x) and the TermCost is written at (x, u).
    The cost iCEM computed equals trajectory_cost on the rows' [obs | action[:u] | next_obs] columns alone, and eta never enters."""
    from mbpo.optimizers import iCemParams, iCemTO
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, QuadraticReward
    X, U, E, H = 4, 2, 5, 6
    A = U + X
    system = EnsembleSystem(EnsembleDynamics(X, U, n_members=E, device=dev), QuadraticReward(X, U, target=[0.1, 0.0, 0.0, 0.0], q=[1.0, 2.0, 0.5, 0.1],
                                                                                           r=[0.3] * U), mode="optimistic")
    assert system.action_dim == A
    cost = _table12(X, U, "max")
    params = iCemParams(num_particles=2, num_samples=62, num_elites=8, num_steps=1, exponent=1.0, alpha=0.1, init_std=0.6, lambda_constraint=10.0)
    opt = iCemTO(horizon=H, action_dim=A, opt_params=params, key=5, cost_fn=cost)
    opt.set_system(system)
    x0 = (torch.randn(X, generator=torch.Generator().manual_seed(3)) * 0.5).to(dev)
    opt.optimize(x0, opt.init(7))
    torch.cuda.synchronize()
    b = opt._bufs
    rows, n, got = b["rows"], b["N"], b["term_cost"].clone()
    assert rows.shape == (H * n, 2 * X + A + 3) and bool(torch.isfinite(got).all()) and float(got.std()) > 0
    assert float(rows[:, X + U:X + A].abs().max()) > 0.1                 # eta columns are in use
    no = X + A + 2
    compact = torch.cat([rows[:, :X], rows[:, X:X + U], torch.zeros(H * n, 2, device=dev), rows[:, no:no + X], torch.zeros(H * n, 1, device=dev)],
                        dim=1).contiguous()
    assert compact.shape[1] == 2 * X + U + 3
    assert _same(got, cost.trajectory_cost(compact, H, n))
    garbled = rows.clone()
    garbled[:, X + U:X + A] = float("nan")                               # eta, then reward / discount / truncation
    garbled[:, X + A:X + A + 2] = float("nan")
    garbled[:, -1] = float("nan")
    assert _same(got, cost.trajectory_cost(garbled, H, n))
    r3 = rows.double().reshape(H, n, -1).transpose(0, 1)
    want = torch.func.vmap(lambda o, a, nx: cost(o, a, next_observation=nx))(r3[..., :X], r3[..., X:X + A], r3[..., no:no + X])
    import test_gpu_term_reward as tgr
    torch.testing.assert_close(got.double(), want, atol=H * tgr.EVAL_TOL, rtol=H * tgr.EVAL_TOL)


# ------------------------------------------------------------------------------------------------ 8. capture
@pytest.mark.parametrize("reduce", ["sum", "max"])
def test_captured_launch_replays_on_changed_rows(dev, reduce):
    shape = SHAPES[2]
    X, U, A, H, n = shape
    c = _case(shape)
    cost = _table12(X, U, reduce)
    rows, out = c["rows"].clone(), torch.full((n,), float("nan"), device=dev)
    cost.trajectory_cost(rows, H, n, out=out)                            # (one eager call first: the table's upload, the code object)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cost.trajectory_cost(rows, H, n, out=out)
    g = torch.Generator().manual_seed(77)
    for _ in range(2):
        rows.copy_((torch.rand(rows.shape, generator=g) * 2 - 1).to(dev))
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        eager = cost.trajectory_cost(rows, H, n)
        assert _same(out, eager) and not _same(out.cpu(), c[reduce])
