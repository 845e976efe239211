"""Terminal values (mbpo.optimizers.TerminalValue, include/mbpo_hip.h "terminal values") without a device: mbpo_terminal_value_eval's
declaration, export, struct layout and every argument refusal (before any device use: this machine has none), the Python refusals, the
tensors held by reference, and the test tree's restatement on its own — fp32 against fp64 and the spread of the values over the rows at
every shape the GPU parity test runs, so that its tolerances are known to discriminate."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest
import torch

import terminal_value_cases as cases
import terminal_value_ref as tref

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "mbpo_hip.h").read_text()
MBPO_OK, MBPO_ERR_ARG, MBPO_ERR_UNSUPPORTED = 0, -1, -2


@pytest.fixture(scope="module")
def lib():
    from mbpo import _hip
    return _hip.load()


# ------------------------------------------------------------------------------------------------ the C boundary
def test_symbol_is_declared_exported_and_bound(lib):
    from mbpo import _hip
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    assert re.search(r"\bint\s+mbpo_terminal_value_eval\s*\(\s*const\s+mbpo_terminal_value_desc\s*\*", code)
    assert "terminal values" in HEADER.lower() and "THIS TEXT IS THE DEFINITION" in HEADER
    assert hasattr(lib, "mbpo_terminal_value_eval")
    assert lib.mbpo_terminal_value_eval.argtypes == [C.POINTER(_hip.TerminalValueDesc), C.c_void_p]
    assert (_hip.ERR_ARG, _hip.ERR_UNSUPPORTED) == (MBPO_ERR_ARG, MBPO_ERR_UNSUPPORTED)


def test_struct_layout_matches_the_header(tmp_path):
    """sizeof and every field offset of mbpo_terminal_value_desc as gcc sees the header == the ctypes mirror's."""
    from mbpo import _hip
    fields = [f[0] for f in _hip.TerminalValueDesc._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mbpo_hip.h"\nint main(void) {\n'
                   '  printf("sizeof %zu\\n", sizeof(mbpo_terminal_value_desc));\n' +
                   "".join(f'  printf("{f} %zu\\n", offsetof(mbpo_terminal_value_desc, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    assert int(out["sizeof"]) == C.sizeof(_hip.TerminalValueDesc)
    for f in fields:
        assert int(out[f]) == getattr(_hip.TerminalValueDesc, f).offset, f


FAKE = 4096      # a non-NULL pointer nothing may dereference: every refusal below comes before any device use


def _mlp(m, dims, n_nets=1, act=0, params=FAKE, stride=None):
    m.params, m.n_nets, m.n_layers, m.activation = params, n_nets, len(dims) - 1, act
    for i, v in enumerate(dims):
        m.dims[i] = v
    m.net_stride = sum(dims[i] * dims[i + 1] + dims[i + 1] for i in range(len(dims) - 1)) if stride is None else stride


def _desc(X=3, A=1, hidden=(64, 64, 64), n_critics=2, n=100):
    from mbpo import _hip
    d = _hip.TerminalValueDesc()
    d.x_dim, d.action_dim = X, A
    _mlp(d.critic, [X + A, *hidden, 1], n_critics, stride=1 << 20)      # (roomy: the refusals below change single sizes)
    if A:
        _mlp(d.policy, [X, *hidden, 2 * A])
    d.x, d.x_stride, d.out, d.out_stride = FAKE, 2 * X + A + 3, FAKE, 2 * X + A + 3
    d.n, d.weight, d.accumulate = n, 1.0, 1
    return d


def _refused(lib, d, code, *words):
    rc = lib.mbpo_terminal_value_eval(C.byref(d), None)
    msg = lib.mbpo_last_error().decode()
    assert rc == code, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def test_n_zero_is_ok_and_launches_nothing(lib):
    for A in (0, 1):
        d = _desc(A=A, n=0)
        assert lib.mbpo_terminal_value_eval(C.byref(d), None) == MBPO_OK
        d.x = d.out = None                    # n == 0 asks for nothing: NULL buffers and parameters are fine
        d.critic.params = d.policy.params = None
        assert lib.mbpo_terminal_value_eval(C.byref(d), None) == MBPO_OK


def test_argument_refusals_name_the_field(lib):
    assert lib.mbpo_terminal_value_eval(None, None) == MBPO_ERR_ARG and b"null descriptor" in lib.mbpo_last_error()
    d = _desc(); d.x_dim = 0
    _refused(lib, d, MBPO_ERR_ARG, "x_dim")
    d = _desc(); d.action_dim = -1
    _refused(lib, d, MBPO_ERR_ARG, "action_dim")
    d = _desc(); d.n = -1
    _refused(lib, d, MBPO_ERR_ARG, "n < 0")
    d = _desc(); d.accumulate = 2
    _refused(lib, d, MBPO_ERR_ARG, "accumulate")
    # bad sizes of a network
    d = _desc(); d.critic.n_layers = 0
    _refused(lib, d, MBPO_ERR_ARG, "critic", "n_layers")
    d = _desc(); d.critic.n_layers = 9
    _refused(lib, d, MBPO_ERR_ARG, "critic", "n_layers")
    d = _desc(); d.critic.dims[2] = 0
    _refused(lib, d, MBPO_ERR_ARG, "critic", "dims[2]")
    d = _desc(); d.critic.activation = 7
    _refused(lib, d, MBPO_ERR_ARG, "critic", "activation")
    d = _desc(); d.policy.dims[1] = -3
    _refused(lib, d, MBPO_ERR_ARG, "policy", "dims[1]")
    d = _desc(); d.critic.net_stride = 10
    _refused(lib, d, MBPO_ERR_ARG, "critic", "net_stride")
    # n_nets outside {1, 2}; kind Q with one critic
    for k in (0, 3):
        d = _desc(A=0); d.critic.n_nets = k
        _refused(lib, d, MBPO_ERR_ARG, "n_nets")
    d = _desc(A=1); d.critic.n_nets = 1
    _refused(lib, d, MBPO_ERR_ARG, "kind Q", "critic.n_nets")
    d = _desc(); d.policy.n_nets = 2
    _refused(lib, d, MBPO_ERR_ARG, "policy.n_nets")
    # dims that do not chain
    d = _desc(A=1); d.critic.dims[0] = 3
    _refused(lib, d, MBPO_ERR_ARG, "critic.dims[0]", "x_dim + action_dim")
    d = _desc(A=0); d.critic.dims[0] = 4
    _refused(lib, d, MBPO_ERR_ARG, "critic.dims[0]")
    d = _desc(); d.critic.dims[4] = 2
    _refused(lib, d, MBPO_ERR_ARG, "critic.dims[4]", "one output")
    d = _desc(); d.policy.dims[0] = 4
    _refused(lib, d, MBPO_ERR_ARG, "policy.dims[0]", "x_dim")
    d = _desc(); d.policy.dims[4] = 3
    _refused(lib, d, MBPO_ERR_ARG, "policy.dims[4]", "2 * action_dim")
    # exactly one normaliser pointer
    d = _desc(); d.norm_mean = FAKE
    _refused(lib, d, MBPO_ERR_ARG, "norm_mean", "norm_std")
    d = _desc(); d.norm_std = FAKE
    _refused(lib, d, MBPO_ERR_ARG, "norm_mean", "norm_std")
    # strides smaller than the width read
    d = _desc(); d.x_stride = 2
    _refused(lib, d, MBPO_ERR_ARG, "x_stride")
    d = _desc(); d.out_stride = 0
    _refused(lib, d, MBPO_ERR_ARG, "out_stride")
    d = _desc(); d.n, d.x_stride = 1 << 40, 1 << 40
    _refused(lib, d, MBPO_ERR_ARG, "overflows")
    # n > 0 with NULL params, x or out
    d = _desc(); d.critic.params = None
    _refused(lib, d, MBPO_ERR_ARG, "critic.params")
    d = _desc(); d.policy.params = None
    _refused(lib, d, MBPO_ERR_ARG, "policy.params")
    d = _desc(); d.x = None
    _refused(lib, d, MBPO_ERR_ARG, "x is NULL")
    d = _desc(); d.out = None
    _refused(lib, d, MBPO_ERR_ARG, "out is NULL")


def test_unsupported_widths_are_refused_by_name(lib):
    for hidden in [(96, 96), (64, 128, 64), (512, 512), (32,)]:
        d = _desc(A=0, hidden=hidden)
        _refused(lib, d, MBPO_ERR_UNSUPPORTED, "MBPO_ERR_UNSUPPORTED", "critic", "{64,128,256}")
    d = _desc(A=1)
    _mlp(d.policy, [3, 200, 200, 2])
    _refused(lib, d, MBPO_ERR_UNSUPPORTED, "MBPO_ERR_UNSUPPORTED", "policy", "{64,128,256}")
    d = _desc(A=65)
    _refused(lib, d, MBPO_ERR_UNSUPPORTED, "MBPO_ERR_UNSUPPORTED", "action_dim")
    # an argument error wins over an unsupported width: it is the caller's bug
    d = _desc(A=0, hidden=(96, 96)); d.out_stride = 0
    _refused(lib, d, MBPO_ERR_ARG, "out_stride")


# ------------------------------------------------------------------------------------------------ the Python class
def _tv(case, **kw):
    from mbpo.optimizers import TerminalValue
    args = dict(n_critics=case.n_critics, activation=case.act, policy_params=case.policy, policy_dims=case.policy_dims,
                policy_activation=case.act, norm_mean=case.mean, norm_std=case.std)
    args.update(kw)
    return TerminalValue(case.x_dim, case.critic, case.critic_dims, **args)


def test_constructor_holds_its_tensors_by_reference():
    case = cases.make_case(cases.SHAPES[0], "Q")
    tv = _tv(case, weight=0.25)
    assert (tv.kind, tv.x_dim, tv.action_dim, tv.n_critics, tv.weight) == ("Q", 3, 1, 2, 0.25)
    assert tv.critic_params is case.critic and tv.policy_params is case.policy and tv.norm_mean is case.mean and tv.norm_std is case.std
    ptr = tv.critic_params.data_ptr()
    tv.critic_params.copy_(torch.ones_like(case.critic))          # the documented refresh: in place, no new object
    assert tv.critic_params.data_ptr() == ptr and case.critic[0] == 1.0
    v = _tv(cases.make_case(cases.SHAPES[0], "V1"))
    assert (v.kind, v.action_dim, v.n_critics, v.policy_params) == ("V", 0, 1, None)
    assert "TerminalValue" in repr(v)


def test_constructor_refusals_name_the_field():
    from mbpo.optimizers import TerminalValue
    q, v = cases.make_case(cases.SHAPES[0], "Q"), cases.make_case(cases.SHAPES[0], "V2")
    with pytest.raises(ValueError, match="x_dim"):
        TerminalValue(0, v.critic, v.critic_dims)
    with pytest.raises(ValueError, match="n_critics must be 1 or 2"):
        _tv(v, n_critics=3)
    with pytest.raises(ValueError, match="n_critics must be 2 with a policy"):
        TerminalValue(3, q.critic[:q.critic.numel() // 2], q.critic_dims, n_critics=1, policy_params=q.policy, policy_dims=q.policy_dims)
    with pytest.raises(ValueError, match="activation must be one of"):
        _tv(v, activation="gelu")
    with pytest.raises(ValueError, match="policy_activation must be one of"):
        _tv(q, policy_activation="gelu")
    with pytest.raises(ValueError, match="policy_params and policy_dims must both"):
        _tv(q, policy_dims=None)
    with pytest.raises(ValueError, match="policy_dims must end in 2 \\* action_dim"):
        _tv(q, policy_dims=[3, 64, 64, 64, 3])
    with pytest.raises(ValueError, match=r"policy_dims must run \[3\] -> \[2\]"):
        _tv(q, policy_dims=[4, 64, 64, 64, 2])
    with pytest.raises(ValueError, match=r"critic_dims must run \[4\] -> \[1\]"):
        TerminalValue(3, q.critic, [3, 64, 64, 64, 1], policy_params=q.policy, policy_dims=q.policy_dims)
    with pytest.raises(ValueError, match=r"critic_dims must run \[3\] -> \[1\]"):
        TerminalValue(3, v.critic, [3, 64, 64, 64, 2])
    with pytest.raises(ValueError, match="critic_dims: hidden layers .* must share one width in"):
        TerminalValue(3, torch.zeros(10), [3, 96, 96, 1], n_critics=1)
    with pytest.raises(ValueError, match="critic_dims: hidden layers .* must share one width in"):
        TerminalValue(3, torch.zeros(10), [3, 64, 128, 1], n_critics=1)
    with pytest.raises(ValueError, match="critic_params holds .* floats, expected"):
        TerminalValue(3, v.critic[:-1], v.critic_dims)
    with pytest.raises(ValueError, match="critic_params must be a float32 tensor"):
        TerminalValue(3, v.critic.double(), v.critic_dims)
    with pytest.raises(ValueError, match="policy_params holds"):
        _tv(q, policy_params=q.policy[:-2])
    with pytest.raises(ValueError, match="norm_mean and norm_std must both"):
        _tv(v, norm_std=None)
    with pytest.raises(ValueError, match="norm_std holds 2 floats, expected 3"):
        _tv(v, norm_std=v.std[:2])
    with pytest.raises(ValueError, match="critic_params must be contiguous"):
        TerminalValue(3, torch.zeros(2 * v.critic.numel())[::2], v.critic_dims)


def test_icem_checks_the_widths_at_construction_and_in_set_system():
    from mbpo.optimizers import TerminalValue, iCEMOptimizer, iCemParams, iCemTO
    from mbpo.systems import PendulumSystem
    system = PendulumSystem()
    p = iCemParams(num_particles=2, num_samples=20, num_elites=4, num_steps=1)
    good_v, good_q = _tv(cases.make_case(cases.SHAPES[0], "V2")), _tv(cases.make_case(cases.SHAPES[0], "Q"))
    for tv in (good_v, good_q, None):
        opt = iCemTO(horizon=5, action_dim=1, opt_params=p, terminal_value=tv)
        opt.set_system(system)
        assert opt.terminal_value is tv
    wrong_x = _tv(cases.make_case(cases.SHAPES[4], "V2"))              # x_dim 4
    wrong_a = _tv(cases.make_case(cases.SHAPES[1], "Q"))               # x_dim 3, action_dim 4: an optimistic system's, not this one's
    opt = iCemTO(horizon=5, action_dim=1, opt_params=p, terminal_value=wrong_x)
    with pytest.raises(ValueError, match="terminal_value is built at x_dim 4, the system has x_dim 3"):
        opt.set_system(system)
    opt = iCemTO(horizon=5, action_dim=1, opt_params=p, terminal_value=wrong_a)
    with pytest.raises(ValueError, match="kind-Q value at action_dim 4, the system has action_dim 1"):
        opt.set_system(system)
    with pytest.raises(ValueError, match="terminal_value is built at x_dim 4"):
        iCemTO(horizon=5, action_dim=1, opt_params=p, terminal_value=wrong_x, system=system)
    with pytest.raises(ValueError, match="must be a TerminalValue"):
        iCemTO(horizon=5, action_dim=1, opt_params=p, terminal_value=lambda x: x)
    with pytest.raises(ValueError, match="terminal_value is built at x_dim 4"):
        iCEMOptimizer(horizon=5, opt_params=p, system=system, terminal_value=wrong_x)
    with pytest.raises(ValueError, match="kind-Q value at action_dim 4"):
        iCEMOptimizer(horizon=5, opt_params=p, system=system, terminal_value=wrong_a)
    o = iCEMOptimizer(horizon=5, opt_params=p, terminal_value=wrong_x)
    with pytest.raises(ValueError, match="terminal_value is built at x_dim 4"):
        o.set_system(system)
    assert iCEMOptimizer(horizon=5, opt_params=p, system=system, terminal_value=good_q).agent_kwargs["terminal_value"] is good_q
    assert TerminalValue is not None


def test_from_sac_and_from_bptt_slice_the_states():
    """The factories against the constructor on hand-built states (no trainer, no device): the slices, held as views."""
    from types import SimpleNamespace
    from mbpo.optimizers import TerminalValue
    case = cases.make_case(cases.SHAPES[0], "Q")
    P, Q, X = case.policy.numel(), case.critic.numel() // 2, 3
    params = torch.cat([case.policy, case.critic + 1.0, torch.tensor([0.3])])
    normalizer = torch.cat([torch.tensor([10.0]), case.mean, torch.rand(X), case.std])
    sig = dict(trainer="SAC", policy_dims=case.policy_dims, q_dims=case.critic_dims, normalize_observations=True)
    ls = SimpleNamespace(signature=sig, params=params, target_q=case.critic.clone(), normalizer=normalizer)
    tv = TerminalValue.from_sac(ls, weight=0.5)
    assert (tv.kind, tv.action_dim, tv.weight, tv.critic_dims, tv.policy_dims) == ("Q", 1, 0.5, case.critic_dims, case.policy_dims)
    assert torch.equal(tv.policy_params, case.policy) and torch.equal(tv.critic_params, case.critic)
    assert torch.equal(tv.norm_mean, case.mean) and torch.equal(tv.norm_std, case.std)
    assert tv.critic_params.data_ptr() == ls.target_q.data_ptr() and tv.norm_mean.data_ptr() == normalizer.data_ptr() + 4
    online = TerminalValue.from_sac(ls, case.policy_dims, case.critic_dims, target=False)
    assert torch.equal(online.critic_params, case.critic + 1.0) and online.critic_params.data_ptr() == params.data_ptr() + 4 * P
    sig["normalize_observations"] = False
    assert TerminalValue.from_sac(ls).norm_mean is None
    with pytest.raises(ValueError, match="learner_state.params holds"):
        TerminalValue.from_sac(ls, case.policy_dims, [4, 128, 128, 1])
    with pytest.raises(ValueError, match="needs SAC's LearnerState"):
        TerminalValue.from_sac(object())
    with pytest.raises(ValueError, match="PPO"):
        TerminalValue.from_sac(SimpleNamespace(signature=dict(trainer="PPO"), params=params, target_q=None, normalizer=normalizer))
    vcase = cases.make_case(cases.SHAPES[0], "V2")
    vec = torch.cat([torch.tensor([5.0]), vcase.mean, torch.rand(X), vcase.std])
    st = SimpleNamespace(target_critic_params=vcase.critic, state_normalizer_state=SimpleNamespace(mean=vec[1:1 + X], std=vec[1 + 2 * X:]))
    bv = TerminalValue.from_bptt(st, vcase.critic_dims, weight=2.0)
    assert (bv.kind, bv.n_critics, bv.weight) == ("V", 2, 2.0) and bv.critic_params is vcase.critic
    assert torch.equal(bv.norm_std, vcase.std) and bv.norm_std.data_ptr() == vec.data_ptr() + 4 * (1 + 2 * X)


def test_product_path_refuses_cpu_tensors():
    from mbpo import _hip
    case = cases.make_case(cases.SHAPES[0], "V2")
    with pytest.raises((_hip.MbpoHipError, ValueError, TypeError)):
        _tv(case)(cases.make_states(case, 4))


# ------------------------------------------------------------------------------------------------ the restatement on its own
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.shape_id)
@pytest.mark.parametrize("norm", [True, False], ids=["norm", "raw"])
def test_reference_fp32_agrees_with_fp64_and_the_values_spread(shape, kind, norm):
    """What makes the GPU tolerances meaningful: at every parity case the fp32 restatement lies within half the GPU tolerance of the
    fp64 one (so 2e-5 against fp32 and 5e-5 against fp64 can both hold), and the values differ over the rows by at least ten times the
    tolerance (so a kernel that returned a constant, or another row's value, would fail)."""
    case = cases.make_case(shape, kind)
    x = cases.make_states(case, 1000, norm=norm)
    args, kw = case.ref_args(norm)
    v32, v64 = tref.v_hat(x, *args, **kw), tref.v_hat(x.double(), *args, **kw)
    assert v32.dtype == torch.float32 and v64.dtype == torch.float64 and v32.shape == (1000,)
    err = (v32.double() - v64).abs().max().item()
    spread = (v64.max() - v64.min()).item()
    print(f"{cases.shape_id(shape)} {kind} norm={norm}: fp32 vs fp64 {err:.3g}, spread {spread:.3g}")
    assert err <= 0.5 * cases.TOL32
    assert spread >= 10 * cases.TOL64


def test_reference_by_hand():
    """One row of each kind worked through layer by layer in fp64, and the -inf rule."""
    case = cases.make_case(cases.SHAPES[4], "Q")      # relu, two hidden layers
    x = cases.make_states(case, 3).double()
    xn = (x - case.mean.double()) / case.std.double()

    def mlp(flat, dims, h):
        off = 0
        for i in range(len(dims) - 1):
            w = flat[off:off + dims[i] * dims[i + 1]].reshape(dims[i], dims[i + 1]).double(); off += dims[i] * dims[i + 1]
            b = flat[off:off + dims[i + 1]].double(); off += dims[i + 1]
            h = h @ w + b
            if i < len(dims) - 2:
                h = torch.relu(h)
        return h
    a = torch.tanh(mlp(case.policy, case.policy_dims, xn)[:, :1])
    q_in = torch.cat([xn, a], dim=1)
    n = case.critic.numel() // 2
    want = torch.minimum(mlp(case.critic[:n], case.critic_dims, q_in), mlp(case.critic[n:], case.critic_dims, q_in))[:, 0]
    args, kw = case.ref_args()
    assert torch.allclose(tref.v_hat(x, *args, **kw), want, rtol=0, atol=1e-12)
    xb = x.clone()
    xb[1, 2] = float("nan")
    got = tref.bonus(xb, 0.5, *args, **kw)
    assert got[1] == float("-inf") and torch.allclose(got[[0, 2]], 0.5 * want[[0, 2]], rtol=0, atol=1e-12)
