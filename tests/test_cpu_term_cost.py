"""The term cost (mbpo.systems.TermCost, include/mbpo_hip.h "term costs") without a device: construction and every refusal, the packed
table against TermReward's, the torch form against hand-computed numbers for both reduces and under vmap, the refusal of next-state terms
without next_observation, mbpo_traj_cost_eval's declaration, export and argument checks, and iCEM's check of the table's widths."""
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "mbpo_hip.h").read_text()
MBPO_OK, MBPO_ERR_ARG = 0, -1


@pytest.fixture(scope="module")
def lib():
    from mbpo import _hip
    return _hip.load()


def _hand_case(reduce):
    """c_t = -5 + |x_t[2]| + 2 * (0.5 u_t^2) - (x_{t+1}[0] - 0.25); every number below is exact in fp32."""
    from mbpo.systems import Group, Term, TermCost
    cost = TermCost(3, 1, bias=-5.0, reduce=reduce, groups=[
        Group([Term("x", 2, "abs")]),
        Group([Term("u", 0, "square", coef=0.5)], weight=2.0),
        Group([Term("x_next", 0, "identity", 1.0, 0.25)], weight=-1.0)])
    obs = torch.tensor([[9.0, 9.0, 1.0], [9.0, 9.0, -6.0], [9.0, 9.0, 4.5]])
    act = torch.tensor([[1.0], [2.0], [-1.0]])
    nxt = torch.tensor([[0.25, 7.0, 7.0], [1.25, 7.0, 7.0], [-0.75, 7.0, 7.0]])
    stage = [-5 + 1 + 1 - 0.0, -5 + 6 + 4 - 1.0, -5 + 4.5 + 1 + 1.0]          # -3, 4, 1.5
    return cost, obs, act, nxt, stage


def test_constants_and_export():
    from mbpo import _hip, systems
    assert _hip.COST_REDUCE_IDS == {"sum": 0, "max": 1}
    assert systems.TermCost is not None and "term costs" in HEADER.lower()


def test_construction_reuses_the_term_rewards_table():
    from mbpo import _hip
    from mbpo.systems import Group, Term, TermCost, TermReward
    groups = [Group([Term("x", 0, "cos", 0.5, 0.1), Term("x_next", 2, "abs", 1.0, 0.0)], weight=0.7, link="exp"),
              Group([Term("u", 0, "square", 0.3)], weight=-1.0, link="sqrt")]
    cost = TermCost(3, 1, bias=-0.4, groups=groups, reduce="max")
    assert (cost.x_dim, cost.u_dim, cost.reduce) == (3, 1, "max") and cost.has_next_state_terms
    v = cost.table("cpu")
    assert v.dtype == torch.float32 and v.shape == (_hip.REWARD_TERMS_FLOATS,)
    assert torch.equal(v, TermReward(3, 1, bias=-0.4, groups=groups).init_params(0).vector())       # one format, one packing
    assert cost.table("cpu") is v                                                                     # cached per device
    assert TermCost(3, 1).reduce == "sum" and not TermCost(3, 1, groups=[Group([Term("x", 1)])]).has_next_state_terms


def test_constructor_refusals():
    from mbpo.systems import Group, Term, TermCost
    ok = Group([Term("x", 0)])
    TermCost(3, 1, groups=[ok] * 16)
    TermCost(3, 1, groups=[Group([Term("u", 0)] * 128)], reduce="max")
    with pytest.raises(ValueError, match="unknown reduce 'mean'"):
        TermCost(3, 1, groups=[ok], reduce="mean")
    with pytest.raises(ValueError, match="group 1 term 0.*index 3"):
        TermCost(3, 1, groups=[ok, Group([Term("x", 3)])])
    with pytest.raises(ValueError, match="group 0 term 1.*index 1"):
        TermCost(3, 1, groups=[Group([Term("u", 0), Term("u", 1)])])
    with pytest.raises(ValueError, match="group 0 term 0.*index -1"):
        TermCost(3, 1, groups=[Group([Term("x_next", -1)])])
    with pytest.raises(ValueError, match="group 0 term 0.*unknown fn 'cube'"):
        TermCost(3, 1, groups=[Group([Term("x", 0, fn="cube")])])
    with pytest.raises(ValueError, match="group 2.*unknown link 'log'"):
        TermCost(3, 1, groups=[ok, ok, Group([Term("x", 0)], link="log")])
    with pytest.raises(ValueError, match="group 0 term 0.*unknown part 'xn'"):
        TermCost(3, 1, groups=[Group([Term("xn", 0)])])
    with pytest.raises(ValueError, match="17 groups"):
        TermCost(3, 1, groups=[ok] * 17)
    with pytest.raises(ValueError, match="129 terms"):
        TermCost(3, 1, groups=[Group([Term("x", 0)] * 100), Group([Term("x", 1)] * 29)])
    with pytest.raises(ValueError, match="group 1 is empty"):
        TermCost(3, 1, groups=[ok, Group([])])
    with pytest.raises(ValueError, match="expected a Group"):
        TermCost(3, 1, groups=[Term("x", 0)])


@pytest.mark.parametrize("reduce", ["sum", "max"])
def test_torch_form_against_hand_computed_numbers(reduce):
    cost, obs, act, nxt, stage = _hand_case(reduce)
    want = sum(stage) if reduce == "sum" else max(stage)               # 2.5, 4.0
    got = cost(obs, act, next_observation=nxt)
    assert got.shape == () and got.dtype == torch.float32 and float(got) == want
    assert cost.stage_costs(obs, act, nxt).tolist() == stage
    assert float(cost(obs.double(), act.double(), nxt.double())) == want and cost(obs.double(), act.double(), nxt.double()).dtype == torch.float64
    # action columns past u_dim (an optimistic system's eta) never enter
    wide = torch.cat([act, torch.full((3, 3), 100.0)], dim=1)
    assert float(cost(obs, wide, nxt)) == want
    # a next state that is not finite reads the observation: step 1's x_next[0] becomes obs[1, 0] = 9
    bad = nxt.clone()
    bad[1, 2] = float("inf")
    stage_bad = [stage[0], -5 + 6 + 4 - (9.0 - 0.25), stage[2]]
    assert float(cost(obs, act, bad)) == (sum(stage_bad) if reduce == "sum" else max(stage_bad))
    # a NaN stage cost is a NaN trajectory cost in both reduces (torch's max keeps it)
    nan_obs = obs.clone()
    nan_obs[0, 2] = float("nan")
    assert bool(torch.isnan(cost(nan_obs, act, nxt)))


@pytest.mark.parametrize("reduce", ["sum", "max"])
def test_torch_form_is_vmappable(reduce):
    cost, obs, act, nxt, stage = _hand_case(reduce)
    g = torch.Generator().manual_seed(1)
    N, H = 7, 5
    o, a, n = torch.randn(N, H, 3, generator=g), torch.randn(N, H, 1, generator=g), torch.randn(N, H, 3, generator=g)
    n[2, 3, 1] = float("nan")                                           # one non-finite next state among the batch
    got = torch.func.vmap(lambda oo, aa, nn: cost(oo, aa, next_observation=nn))(o, a, n)
    want = torch.stack([cost(o[i], a[i], n[i]) for i in range(N)])
    assert got.shape == (N,) and torch.equal(got, want) and bool(torch.isfinite(got).all())
    # without next-state terms it is a plain cost_fn(observation, action)
    from mbpo.systems import Group, Term, TermCost
    plain = TermCost(3, 1, bias=-5.0, groups=[Group([Term("x", 2, "abs")])], reduce=reduce)
    got = torch.func.vmap(plain)(o, a)
    c = o[:, :, 2].abs() - 5.0
    assert torch.equal(got, c.sum(dim=1) if reduce == "sum" else c.max(dim=1).values)


def test_next_state_terms_need_next_observation():
    cost, obs, act, nxt, _ = _hand_case("sum")
    with pytest.raises(ValueError, match="next_observation"):
        cost(obs, act)
    with pytest.raises(ValueError, match="next_observation"):
        torch.func.vmap(cost)(obs[None], act[None])


def test_traj_cost_eval_is_declared_exported_and_checks_its_arguments(lib):
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    m = re.search(r"int mbpo_traj_cost_eval\(([^;]*?)\);", code, re.S)
    assert m
    args = [a.strip() for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["table", "rows", "row_len", "next_off", "n_steps", "n_traj", "x_dim", "u_dim",
                                                         "reduce", "cost", "stream"]
    assert [" ".join(a.replace("*", " * ").split()[:-1]) for a in args] == [
        "const float *", "const float *", "int32_t", "int32_t", "int32_t", "int64_t", "int32_t", "int32_t", "int32_t", "float *", "void *"]
    assert hasattr(lib, "mbpo_traj_cost_eval") and lib.mbpo_traj_cost_eval.argtypes is not None
    # Pendulum iCEM sizes: x = 3, A = u = 1, row_len = 2x + A + 3 = 10, next_off = x + A + 2 = 6
    good = dict(table=16, rows=16, row_len=10, next_off=6, n_steps=20, n_traj=64, x_dim=3, u_dim=1, reduce=0, cost=16)

    def ev(**kw):
        a = dict(good, **kw)
        return lib.mbpo_traj_cost_eval(a["table"], a["rows"], a["row_len"], a["next_off"], a["n_steps"], a["n_traj"], a["x_dim"], a["u_dim"],
                                       a["reduce"], a["cost"], None)

    bad = [dict(table=None), dict(rows=None), dict(cost=None), dict(n_steps=0), dict(n_steps=-3), dict(n_traj=-1), dict(x_dim=0),
           dict(u_dim=0), dict(x_dim=-2), dict(next_off=8),                 # next_off + x_dim = 11 > row_len
           dict(row_len=8),                                                 # 6 + 3 > 8
           dict(next_off=3, row_len=10),                                    # x_dim + u_dim = 4 > next_off
           dict(u_dim=4),                                                   # 3 + 4 > 6
           dict(reduce=2), dict(reduce=-1)]
    for kw in bad:
        assert ev(**kw) == MBPO_ERR_ARG, kw
        assert b"traj_cost_eval" in lib.mbpo_last_error(), kw
    assert ev(table=None) == MBPO_ERR_ARG and b"null" in lib.mbpo_last_error()
    assert ev(reduce=2) == MBPO_ERR_ARG and b"reduce" in lib.mbpo_last_error()
    # the edges that are allowed: the next state ends the row, the controls end where it begins; nothing is launched at n_traj == 0
    assert ev(n_traj=0) == MBPO_OK
    assert ev(n_traj=0, row_len=9, next_off=6) == MBPO_OK and ev(n_traj=0, next_off=4, row_len=7) == MBPO_OK
    assert ev(n_traj=0, reduce=1, n_steps=1) == MBPO_OK
    assert ev(n_traj=0, table=None, rows=None, cost=None) == MBPO_OK      # nothing to do: no pointer is read
    assert ev(n_traj=0, reduce=2) == MBPO_ERR_ARG                         # the sizes are checked first


def test_slot_hook_without_a_device(lib):
    """The kernel-selection hook the GPU tests use: exported, not declared, refuses anything but -1 and the powers of two up to 32."""
    import ctypes as C
    assert hasattr(lib, "mbpo_debug_set_traj_cost_slots")
    assert "mbpo_debug_set_traj_cost_slots" not in re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    lib.mbpo_debug_set_traj_cost_slots.argtypes, lib.mbpo_debug_set_traj_cost_slots.restype = [C.c_int], C.c_int
    for bad in (0, 3, 6, 64, -2):
        assert lib.mbpo_debug_set_traj_cost_slots(bad) == MBPO_ERR_ARG and b"slots" in lib.mbpo_last_error()
    for ok in (1, 2, 4, 8, 16, 32, -1):
        assert lib.mbpo_debug_set_traj_cost_slots(ok) == MBPO_OK


def test_ops_wrapper_refuses_before_the_device():
    from mbpo import _hip
    cost, *_ = _hand_case("sum")
    rows = torch.zeros(6, 10)
    with pytest.raises(_hip.MbpoHipError, match="GPU tensor"):
        cost.trajectory_cost(rows, 3, 2)                                # host rows: no CPU fallback


def test_icem_checks_the_tables_widths():
    from mbpo.optimizers import iCemParams, iCemTO
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, Group, PendulumSystem, QuadraticReward, Term, TermCost
    params = iCemParams(num_particles=2, num_samples=20, num_elites=4, num_steps=1)
    speed = [Group([Term("x_next", 2, "abs")])]
    ok = iCemTO(horizon=5, action_dim=1, opt_params=params, cost_fn=TermCost(3, 1, bias=-5.0, groups=speed, reduce="max"))
    ok.set_system(PendulumSystem())
    assert ok._term_cost is ok.cost_fn
    with pytest.raises(ValueError, match="x_dim 4.*x_dim 3"):
        iCemTO(horizon=5, action_dim=1, opt_params=params, cost_fn=TermCost(4, 1, groups=speed)).set_system(PendulumSystem())
    with pytest.raises(ValueError, match="u_dim 2.*u_dim 1"):
        iCemTO(horizon=5, action_dim=1, opt_params=params, cost_fn=TermCost(3, 2, groups=speed)).set_system(PendulumSystem())
    with pytest.raises(ValueError, match="x_dim 4.*x_dim 3"):
        iCemTO(horizon=5, action_dim=1, opt_params=params, cost_fn=TermCost(4, 1, groups=speed), system=PendulumSystem())
    # an optimistic system: the table is written at u_dim, not at action_dim = u_dim + x_dim
    X, U = 4, 2
    system = EnsembleSystem(EnsembleDynamics(X, U, n_members=3, device="cpu"), QuadraticReward(X, U, target=[0.0] * X, q=[1.0] * X, r=[0.1] * U),
                            mode="optimistic")
    assert system.action_dim == U + X
    iCemTO(horizon=5, action_dim=system.action_dim, opt_params=params, cost_fn=TermCost(X, U, groups=speed)).set_system(system)
    with pytest.raises(ValueError, match=f"u_dim {U + X}.*u_dim {U}.*action_dim is {U + X}"):
        iCemTO(horizon=5, action_dim=system.action_dim, opt_params=params, cost_fn=TermCost(X, U + X, groups=speed)).set_system(system)
    # any other callable is not a term cost: the vmap path
    fn = lambda o, a: o.sum()
    other = iCemTO(horizon=5, action_dim=1, opt_params=params, cost_fn=fn)
    other.set_system(PendulumSystem())
    assert other._term_cost is None and other.cost_fn is fn
    assert iCemTO(horizon=5, action_dim=1, opt_params=params)._term_cost is None
