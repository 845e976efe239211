"""Plan rewards (mbpo.systems.PlanRewardParams, include/mbpo_hip.h "plan rewards") without a device: the class's shapes, `stack` against
hand-built tables for the three kinds, the table held by reference, every refusal matched on its message, mbpo_plan_reward_eval's
declaration, export and argument checks, and the test tree's reference against hand-computed rows."""
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import plan_reward_cases as cases
import plan_reward_ref as pref

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "mbpo_hip.h").read_text()
MBPO_OK, MBPO_ERR_ARG, MBPO_ERR_UNSUPPORTED = 0, -1, -2


@pytest.fixture(scope="module")
def lib():
    from mbpo import _hip
    return _hip.load()


def test_error_codes_and_kinds_match_the_header():
    from mbpo import _hip
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    val = lambda name: int(re.search(rf"\b{name}\b\s*=?\s*\(?(-?\d+)", code).group(1))
    assert (val("MBPO_ERR_ARG"), val("MBPO_ERR_UNSUPPORTED")) == (MBPO_ERR_ARG, MBPO_ERR_UNSUPPORTED)
    assert (pref.PENDULUM, pref.QUADRATIC, pref.TERMS) == (_hip.REWARD_PENDULUM, _hip.REWARD_QUADRATIC, _hip.REWARD_TERMS)
    assert pref.TERMS_FLOATS == _hip.REWARD_TERMS_FLOATS
    assert "plan rewards" in HEADER.lower()


# ------------------------------------------------------------------------------------------------ PlanRewardParams
def test_stack_builds_the_three_layouts():
    from mbpo import _hip
    from mbpo.systems import PendulumSystem, PlanRewardParams, QuadraticReward, TermReward
    from mbpo.systems.rewards.pendulum_reward import PendulumReward, PendulumRewardParams, QuadraticRewardParams
    # Pendulum: [angle_cost, control_cost, target_angle], [B, 1]
    pr = PendulumReward()
    nested = [[PendulumRewardParams(target_angle=a, control_cost=0.25 * (i + 1))] for i, a in enumerate([0.0, 0.5, -2.0])]
    prp = PlanRewardParams.stack(pr, nested, "cpu")
    assert (prp.problems, prp.steps, prp.param_len, prp.kind) == (3, 1, 3, _hip.REWARD_PENDULUM)
    assert prp.table.dtype == torch.float32 and prp.base is nested[0][0] and prp.reward is pr
    assert torch.equal(prp.table, torch.tensor([[[1.0, 0.25, 0.0]], [[1.0, 0.5, 0.5]], [[1.0, 0.75, -2.0]]]))
    # quadratic: [target | q | r], [1, H]
    qr = QuadraticReward(2, 1)
    nested = [[QuadraticRewardParams([float(t), -1.0], [1.0, 2.0], [0.5]) for t in range(4)]]
    prp = PlanRewardParams.stack(qr, nested, "cpu")
    assert (prp.problems, prp.steps, prp.param_len, prp.kind) == (1, 4, 5, _hip.REWARD_QUADRATIC)
    assert torch.equal(prp.table[0], torch.tensor([[float(t), -1.0, 1.0, 2.0, 0.5] for t in range(4)]))
    prp.table[..., :2] = torch.tensor([7.0, 8.0])                          # the documented way to set targets
    assert prp.table[0, 3].tolist() == [7.0, 8.0, 1.0, 2.0, 0.5]
    # terms: the full-length packed table, [B, H]
    g = torch.Generator().manual_seed(0)
    datas = [[cases.term_data(3, 1, g, extra=(b + t) % 2 == 1) for t in range(2)] for b in range(2)]
    tr = TermReward(3, 1)
    nested = [[cases.term_params(d) for d in row] for row in datas]
    prp = PlanRewardParams.stack(tr, nested, "cpu")
    assert (prp.problems, prp.steps, prp.param_len, prp.kind) == (2, 2, _hip.REWARD_TERMS_FLOATS, _hip.REWARD_TERMS)
    for b in range(2):
        for t in range(2):
            assert torch.equal(prp.table[b, t], nested[b][t].vector())
            assert prp.table[b, t, 1] == sum(len(terms) for _, _, terms in datas[b][t][3])
    assert prp.table[0, 0, 1] != prp.table[0, 1, 1]                         # the tables of one plan differ in their term counts
    assert "PlanRewardParams" in repr(prp)
    assert PendulumSystem is not None


def test_table_is_held_by_reference_and_base_defaults():
    from mbpo.systems import PlanRewardParams
    from mbpo.systems.rewards.pendulum_reward import PendulumReward, PendulumRewardParams
    table = torch.zeros(1, 6, 3)
    prp = PlanRewardParams(PendulumReward(), table)
    assert prp.table is table and prp.table.data_ptr() == table.data_ptr()
    table[0, :, 2] = torch.arange(6.0)
    assert prp.table[0, 4, 2] == 4.0
    ptr = prp.table.data_ptr()
    prp.table.copy_(torch.ones(1, 6, 3))
    assert prp.table.data_ptr() == ptr and table[0, 0, 0] == 1.0
    assert prp.base == PendulumRewardParams() and (prp.problems, prp.steps) == (1, 6)


def test_constructor_refusals():
    from mbpo.systems import EnsembleDynamics, LearnedReward, PlanRewardParams, QuadraticReward, TermReward
    from mbpo.systems.rewards.pendulum_reward import PendulumReward, PendulumRewardParams
    pr = PendulumReward()
    with pytest.raises(ValueError, match="float32 tensor"):
        PlanRewardParams(pr, torch.zeros(1, 1, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="float32 tensor"):
        PlanRewardParams(pr, [[[1.0, 0.02, 0.0]]])
    with pytest.raises(ValueError, match=r"\[PB, PH, param_len\].*got \(1, 3\)"):
        PlanRewardParams(pr, torch.zeros(1, 3))
    with pytest.raises(ValueError, match=r"PB, PH >= 1"):
        PlanRewardParams(pr, torch.zeros(0, 1, 3))
    with pytest.raises(ValueError, match="param_len 4.*PendulumReward.*holds 3 floats"):
        PlanRewardParams(pr, torch.zeros(1, 1, 4))
    with pytest.raises(ValueError, match="param_len 3.*QuadraticReward.*x_dim 4, u_dim 2 holds 10 floats"):
        PlanRewardParams(QuadraticReward(4, 2), torch.zeros(1, 1, 3))
    with pytest.raises(ValueError, match="param_len 10.*TermReward.*holds 580 floats"):
        PlanRewardParams(TermReward(4, 2), torch.zeros(1, 1, 10))
    with pytest.raises(ValueError, match="contiguous"):
        PlanRewardParams(pr, torch.zeros(1, 3, 2).transpose(1, 2))
    learned = LearnedReward(EnsembleDynamics(3, 1, n_members=2, device="cpu", learn_reward=True))
    with pytest.raises(ValueError, match="LearnedReward cannot be a plan reward.*not a function of the row"):
        PlanRewardParams(learned, torch.zeros(1, 1, 3))
    with pytest.raises(ValueError, match="QuadraticReward, TermReward or PendulumReward, got int"):
        PlanRewardParams(3, torch.zeros(1, 1, 3))
    with pytest.raises(ValueError, match="rectangular"):
        PlanRewardParams.stack(pr, [[PendulumRewardParams()], []], "cpu")
    with pytest.raises(ValueError, match="rectangular"):
        PlanRewardParams.stack(pr, [], "cpu")
    with pytest.raises(ValueError, match="not a term table at x_dim 3, u_dim 1"):
        PlanRewardParams.stack(TermReward(3, 1), [[TermReward(4, 1).init_params(0)]], "cpu")


def _icem(system, H=6, **kw):
    from mbpo.optimizers import iCemParams, iCemTO
    opt = iCemTO(horizon=H, action_dim=system.action_dim, opt_params=iCemParams(num_particles=2, num_samples=20, num_elites=4, num_steps=1), **kw)
    opt.set_system(system)
    return opt


class _State:
    """What _plan_reward reads of an optimizer state."""

    def __init__(self, system_params):
        self.system_params = system_params


def test_icem_refuses_tables_that_do_not_fit():
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, PendulumSystem, PlanRewardParams, QuadraticReward, SystemParams, TermReward
    from mbpo.systems.rewards.pendulum_reward import PendulumReward
    system = PendulumSystem()
    opt = _icem(system, H=6)
    st = lambda prp: _State(SystemParams(dynamics_params=None, reward_params=prp))
    ok = PlanRewardParams(system.reward, torch.zeros(1, 6, 3))
    prp, sp = opt._plan_reward(st(ok), None)
    assert prp is ok and sp.reward_params is ok.base                       # the system's own reward: the rollout runs under base
    assert opt._plan_reward(st(PlanRewardParams(system.reward, torch.zeros(4, 1, 3))), 4)[0] is not None
    assert opt._plan_reward(st(PlanRewardParams(system.reward, torch.zeros(1, 1, 3))), 4)[0] is not None
    with pytest.raises(ValueError, match="holds 4 problems: a single state needs PB = 1"):
        opt._plan_reward(st(PlanRewardParams(system.reward, torch.zeros(4, 1, 3))), None)
    with pytest.raises(ValueError, match="holds 3 problems, the state has batch_size 4: PB must be 1 or 4"):
        opt._plan_reward(st(PlanRewardParams(system.reward, torch.zeros(3, 1, 3))), 4)
    with pytest.raises(ValueError, match="holds 5 steps, the horizon is 6: PH must be 1 or 6"):
        opt._plan_reward(st(PlanRewardParams(system.reward, torch.zeros(1, 5, 3))), None)
    with pytest.raises(ValueError, match="QuadraticReward at x_dim 4, u_dim 1; the system has x_dim 3, u_dim 1"):
        opt._plan_reward(st(PlanRewardParams(QuadraticReward(4, 1), torch.zeros(1, 1, 9))), None)
    with pytest.raises(ValueError, match="TermReward at x_dim 3, u_dim 2; the system has x_dim 3, u_dim 1"):
        opt._plan_reward(st(PlanRewardParams(TermReward(3, 2), torch.zeros(1, 1, 580))), None)
    # a foreign reward of the system's widths is taken; the rollout then runs under the system's own default parameters
    foreign = PlanRewardParams(TermReward(3, 1), torch.zeros(1, 1, 580))
    prp, sp = opt._plan_reward(st(foreign), None)
    assert prp is foreign and sp.reward_params == system.reward.init_params(0)
    # an optimistic system: the widths are the dynamics' (u_dim), not action_dim; a learned reward's parameters are the dynamics'
    X, U = 4, 2
    dyn = EnsembleDynamics(X, U, n_members=3, device="cpu")
    esys = EnsembleSystem(dyn, QuadraticReward(X, U), mode="optimistic")
    eopt = _icem(esys)
    assert eopt._plan_reward(st(PlanRewardParams(QuadraticReward(X, U), torch.zeros(1, 1, 2 * X + U))), None)[0] is not None
    with pytest.raises(ValueError, match=f"u_dim {U + X}; the system has x_dim {X}, u_dim {U}.*action_dim is {U + X}"):
        eopt._plan_reward(st(PlanRewardParams(QuadraticReward(X, U + X), torch.zeros(1, 1, 3 * X + U))), None)
    assert PendulumReward is not None
    # without a PlanRewardParams the state's parameters pass through untouched
    plain = SystemParams(dynamics_params=None, reward_params=system.reward.init_params(0))
    assert opt._plan_reward(_State(plain), None) == (None, plain)


def test_every_other_consumer_refuses_a_plan_reward():
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, PendulumSystem, PlanRewardParams, QuadraticReward, System, SystemParams
    from mbpo.systems.plan_reward import refuse_plan_reward
    psys = PendulumSystem()
    sp = SystemParams(dynamics_params=None, reward_params=PlanRewardParams(psys.reward, torch.zeros(1, 1, 3)))
    with pytest.raises(ValueError, match="PendulumSystem.rollout_spec.*only iCEM consumes"):
        psys.rollout_spec(sp, "cpu")
    with pytest.raises(ValueError, match="only iCEM consumes.*System.step.*BraxWrapper.*BPTT"):
        psys.step(torch.zeros(3), torch.zeros(1), sp)                       # refused before anything touches a device
    X, U = 4, 2
    esys = EnsembleSystem(EnsembleDynamics(X, U, n_members=3, device="cpu"), QuadraticReward(X, U))
    esp = esys.init_params(0).replace(reward_params=PlanRewardParams(esys.reward, torch.zeros(1, 1, 2 * X + U)))
    with pytest.raises(ValueError, match="EnsembleSystem.rollout_spec.*only iCEM consumes"):
        esys.rollout_spec(esp, "cpu")

    class Mine(System):
        def step(self, x, u, system_params):
            raise AssertionError("never reached")

    mine = Mine(esys.dynamics, esys.reward)
    with pytest.raises(ValueError, match="Mine.rollout_spec.*only iCEM consumes"):
        mine.rollout_spec(esp, "cpu")
    with pytest.raises(ValueError, match="needs a fused system.*Mine.step is user code"):
        _icem(mine)._plan_reward(_State(esp), None)
    refuse_plan_reward(esys.init_params(0), "x")                            # ordinary parameters pass


def test_ops_wrapper_refuses_before_the_device():
    from mbpo import _hip, ops
    rows = torch.zeros(2 * 3 * 4, 10)
    with pytest.raises(_hip.MbpoHipError, match="GPU tensor"):
        ops.plan_reward_eval(_hip.REWARD_PENDULUM, torch.zeros(1, 1, 3), rows, 2, 3, 4, 3, 1, next_off=6)      # host tensors: no CPU fallback


# ------------------------------------------------------------------------------------------------ the entry point
def test_plan_reward_eval_is_declared_exported_and_checks_its_arguments(lib):
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    m = re.search(r"int mbpo_plan_reward_eval\(([^;]*?)\);", code, re.S)
    assert m
    args = [a.strip() for a in m.group(1).split(",")]
    names = ["reward_kind", "params", "param_problems", "param_steps", "param_len", "rows", "row_len", "next_off", "n_steps", "n_problems",
             "group", "x_dim", "u_dim", "out", "out_stride", "stream"]
    assert [a.split()[-1].lstrip("*") for a in args] == names
    assert [" ".join(a.replace("*", " * ").split()[:-1]) for a in args] == [
        "int32_t", "const float *", "int32_t", "int32_t", "int32_t", "const float *", "int32_t", "int32_t", "int32_t", "int32_t", "int64_t",
        "int32_t", "int32_t", "float *", "int64_t", "void *"]
    assert hasattr(lib, "mbpo_plan_reward_eval") and lib.mbpo_plan_reward_eval.argtypes is not None
    assert len(lib.mbpo_plan_reward_eval.argtypes) == len(names)
    # Pendulum iCEM sizes: x = 3, A = u = 1, row_len = 10, next_off = 6; B = 4 problems, H = 20
    good = dict(reward_kind=pref.PENDULUM, params=16, param_problems=4, param_steps=20, param_len=3, rows=16, row_len=10, next_off=6,
                n_steps=20, n_problems=4, group=64, x_dim=3, u_dim=1, out=16, out_stride=1)

    def ev(**kw):
        a = dict(good, **kw)
        return lib.mbpo_plan_reward_eval(*[a[n] for n in names[:-1]], None)

    quad = dict(reward_kind=pref.QUADRATIC, param_len=7)
    terms = dict(reward_kind=pref.TERMS, param_len=pref.TERMS_FLOATS)
    bad = [dict(params=None), dict(rows=None), dict(out=None), dict(n_steps=0), dict(n_steps=-3), dict(n_problems=0), dict(n_problems=-1),
           dict(group=-1), dict(x_dim=0), dict(u_dim=0),
           dict(param_problems=2), dict(param_problems=0), dict(param_problems=5),       # neither 1 nor n_problems
           dict(param_steps=19), dict(param_steps=0), dict(param_steps=21),              # neither 1 nor n_steps
           dict(param_len=2), dict(quad, param_len=6), dict(terms, param_len=pref.TERMS_FLOATS - 1), dict(param_len=-1),
           dict(quad, x_dim=4, next_off=6, u_dim=1, param_len=9, row_len=9),             # next_off + x_dim = 10 > row_len
           dict(next_off=8), dict(row_len=8),                                            # the next state leaves the row
           dict(next_off=3),                                                             # x_dim + u_dim = 4 > next_off
           dict(quad, u_dim=4, param_len=10),                                            # 3 + 4 > 6
           dict(reward_kind=pref.PENDULUM, x_dim=2, u_dim=1), dict(reward_kind=pref.PENDULUM, x_dim=3, u_dim=2),
           dict(out_stride=0), dict(out_stride=-10),
           dict(reward_kind=4), dict(reward_kind=-1),
           dict(group=1 << 62),                                                          # n_steps * n_problems * group overflows int64
           dict(group=1 << 55, row_len=1 << 20, next_off=100),                           # ... times row_len does
           dict(group=1 << 55, out_stride=1 << 20),                                      # ... times out_stride does
           dict(group=1 << 42)]                                                          # more tiles than a grid holds
    for kw in bad:
        assert ev(**kw) == MBPO_ERR_ARG, kw
        assert b"plan_reward_eval" in lib.mbpo_last_error(), kw
    assert ev(params=None) == MBPO_ERR_ARG and b"null" in lib.mbpo_last_error()
    assert ev(param_problems=2) == MBPO_ERR_ARG and b"param_problems" in lib.mbpo_last_error()
    assert ev(param_steps=19) == MBPO_ERR_ARG and b"param_steps" in lib.mbpo_last_error()
    assert ev(param_len=2) == MBPO_ERR_ARG and b"param_len" in lib.mbpo_last_error()
    assert ev(out_stride=0) == MBPO_ERR_ARG and b"out_stride" in lib.mbpo_last_error()
    # the learned reward is not a function of the row
    assert ev(reward_kind=2) == MBPO_ERR_UNSUPPORTED and b"learned" in lib.mbpo_last_error()
    # what is allowed: both broadcast forms, longer parameter vectors, the in-place stride, the row's edges; nothing is launched at group 0
    for kw in [dict(), dict(param_problems=1), dict(param_steps=1), dict(param_problems=1, param_steps=1), dict(param_len=8),
               dict(out_stride=10), dict(row_len=9), dict(quad), dict(terms), dict(terms, x_dim=4, u_dim=2), dict(n_steps=1, param_steps=1),
               dict(quad, u_dim=3, param_len=9), dict(params=None, rows=None, out=None)]:
        assert ev(group=0, **kw) == MBPO_OK, kw
    assert ev(group=0, out_stride=0) == MBPO_ERR_ARG                        # the sizes are checked first
    assert ev(group=0, reward_kind=2) == MBPO_ERR_UNSUPPORTED


def test_flat_kernel_hook_without_a_device(lib):
    """The kernel-selection hook the GPU tests use: exported, not declared, refuses anything but -1, 0 and 1."""
    import ctypes as C
    assert hasattr(lib, "mbpo_debug_set_plan_reward_flat")
    assert "mbpo_debug_set_plan_reward_flat" not in re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    lib.mbpo_debug_set_plan_reward_flat.argtypes, lib.mbpo_debug_set_plan_reward_flat.restype = [C.c_int], C.c_int
    for bad in (2, -2, 256):
        assert lib.mbpo_debug_set_plan_reward_flat(bad) == MBPO_ERR_ARG and b"mode" in lib.mbpo_last_error()
    for ok in (1, 0, -1):
        assert lib.mbpo_debug_set_plan_reward_flat(ok) == MBPO_OK


# ------------------------------------------------------------------------------------------------ the reference
def test_reference_against_hand_computed_rows():
    # Pendulum: x = [1, 0, 0] (theta 0), u = 1, target 0.5: r = -(0.5^2) - 0.02 = -0.27
    x, u = torch.tensor([[1.0, 0.0, 0.0]], dtype=torch.float64), torch.tensor([[1.0]], dtype=torch.float64)
    r = pref.reward(pref.PENDULUM, [1.0, 0.02, 0.5], x, u, x)
    assert abs(float(r) - (-(0.25) - float(np.float32(0.02)))) < 1e-15
    # theta = pi / 2, thetadot 2, u = -0.5, target -pi (as fp32): the difference 3 pi / 2 wraps to -pi / 2; angle_cost 2, control_cost 0.5
    x = torch.tensor([[0.0, 1.0, 2.0]], dtype=torch.float64)
    r = pref.reward(pref.PENDULUM, [2.0, 0.5, -math.pi], x, torch.tensor([[-0.5]], dtype=torch.float64), x)
    want = -(2.0 * ((math.pi / 2 - float(np.float32(-math.pi))) - 2 * math.pi) ** 2 + 0.1 * 4.0) - 0.5 * 0.25
    assert abs(float(r) - want) < 1e-12
    # quadratic: -(1 (2 - 1)^2 + 2 (0 + 1)^2) - 0.5 3^2 = -7.5
    r = pref.reward(pref.QUADRATIC, [1.0, -1.0, 1.0, 2.0, 0.5], torch.tensor([[2.0, 0.0]]), torch.tensor([[3.0]]), torch.zeros(1, 2))
    assert float(r) == -7.5
    # terms: the packed table decodes to the data it was packed from, and evaluates to tests/term_reward_ref.py's number
    g = torch.Generator().manual_seed(3)
    data = cases.term_data(4, 2, g, extra=True)
    vec = cases.term_params(data).vector()
    back = pref.unpack_term_vector(vec, 4, 2)
    f32 = lambda v: float(np.float32(v))
    assert back[:2] == (4, 2) and back[2] == f32(data[2]) and len(back[3]) == len(data[3])
    for (w, link, terms), (w2, link2, terms2) in zip(data[3], back[3]):
        assert (f32(w), link) == (w2, link2) and [(t[0], t[1], t[2], f32(t[3]), f32(t[4])) for t in terms] == terms2
    import term_reward_ref as tref
    x, u, xn = torch.rand(9, 4, dtype=torch.float64), torch.rand(9, 2, dtype=torch.float64), torch.rand(9, 4, dtype=torch.float64)
    xn[4, 1] = float("inf")
    assert torch.equal(pref.reward(pref.TERMS, vec, x, u, xn), tref.reward(data, x, u, xn))
    hand = (1, 1, 0.5, [(2.0, "identity", [("x_next", 0, "square", 1.0, 1.0)]), (-1.0, "sqrt", [("u", 0, "square", 4.0, 0.0)])])
    vec = cases.term_params(hand).vector()
    r = pref.reward(pref.TERMS, vec, torch.tensor([[5.0]]), torch.tensor([[1.5]]), torch.tensor([[3.0]]))
    assert float(r) == 0.5 + 2.0 * 4.0 - 3.0                                  # 0.5 + 2 (3 - 1)^2 - sqrt(4 * 1.5^2)
    r = pref.reward(pref.TERMS, vec, torch.tensor([[5.0]]), torch.tensor([[1.5]]), torch.tensor([[float("nan")]]))
    assert float(r) == 0.5 + 2.0 * 16.0 - 3.0                                 # x_next reads x = 5


def test_rows_reward_indexes_problem_and_step():
    """Row (t, b, j) under table[b or 0][t or 0]: a quadratic whose only non-zero number is the target makes the index visible."""
    H, B, G, X, U, A = 3, 2, 4, 2, 1, 3
    row_len, _, next_off = cases.layout(X, A)
    rows = torch.zeros(H * B * G, row_len, dtype=torch.float64)
    for form in cases.FORMS:
        PB, PH = cases.form_shape(form, H, B)
        table = torch.zeros(PB, PH, 2 * X + U)
        table[:, :, X] = 1.0                                                  # q_0 = 1: r = -(0 - target_0)^2
        for b in range(PB):
            for t in range(PH):
                table[b, t, 0] = 1 + b + 10 * t
        got = pref.rows_reward(pref.QUADRATIC, table, rows, H, B, G, X, U, next_off).reshape(H, B, G)
        for t in range(H):
            for b in range(B):
                want = -float(1 + (b if PB > 1 else 0) + 10 * (t if PH > 1 else 0)) ** 2
                assert got[t, b].tolist() == [want] * G, (form, t, b)


def test_icem_loop_with_a_constant_schedule_is_the_plain_loop():
    """objective_t / icem_loop against oracle.icem.objective on the Pendulum: the same numbers when every step has the same target."""
    from oracle import icem as oicem
    from oracle import systems as osys
    rng = np.random.default_rng(0)
    cand = rng.uniform(-1, 1, (9, 5, 1))
    x0 = np.array([-0.8, 0.6, 0.5])
    osystem = osys.PendulumSystem(osys.PendulumParams(target_angle=0.7))

    def step(x, u):
        xn, r = osystem.step(torch.from_numpy(x), torch.from_numpy(u))
        return xn.numpy(), r.numpy()

    np.testing.assert_array_equal(pref.objective_t(pref.pendulum_step_t([0.7] * 5), x0, cand), oicem.objective(step, x0, cand, 2))
    moving = pref.objective_t(pref.pendulum_step_t([0.7, 0.7, 0.7, 0.7, 2.0]), x0, cand)
    assert not np.array_equal(moving, oicem.objective(step, x0, cand, 2))


def test_cases_cover_both_table_paths():
    """From group 256 on another kernel runs (one (problem, step) per workgroup, term tables staged in LDS): the shapes have groups on
    both sides, one where 256 consecutive rows straddle two problems, and one with eta columns."""
    groups = [s[2] for s in cases.SHAPES]
    assert min(groups) < 256 <= max(groups) and 7 in groups and 300 in groups
    assert any(s[5] > s[4] for s in cases.SHAPES)
    for shape in cases.SHAPES:
        for kind in (pref.QUADRATIC, pref.TERMS):
            t = cases.make_table(kind, "BH", shape)
            assert t.shape == (shape[1], shape[0], pref.param_len(kind, shape[3], shape[4])) and bool(torch.isfinite(t).all())
            if t.shape[0] * t.shape[1] > 1:
                flat = t.reshape(-1, t.shape[2])
                assert len({tuple(v.tolist()) for v in flat}) == flat.shape[0]           # distinct parameters per (b, t)
        rows = cases.make_rows(shape)
        assert rows.shape == (shape[0] * shape[1] * shape[2], cases.layout(shape[3], shape[5])[0])
