"""The learned reward (MBPO_REWARD_LEARNED) without a device: the C-ABI constant and descriptor field, the argument checks of the
fit / BPTT plans, the host API's wiring (EnsembleDynamics(learn_reward), LearnedReward, EnsembleSystem) and the test restatement's
own consistency (tests/learned_reward_ref.py)."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

from oracle import nets as onets

import learned_reward_ref as lref

ROOT = Path(__file__).resolve().parent.parent
X, U, E = 4, 1, 5


@pytest.fixture(scope="module")
def lib():
    from mbpo import _hip
    return _hip.load()


def test_constant_and_descriptor_field_match_the_header():
    from mbpo import _hip
    h = (ROOT / "include" / "mbpo_hip.h").read_text()
    assert int(re.search(r"#define MBPO_REWARD_LEARNED (\d+)", h).group(1)) == _hip.REWARD_LEARNED == 2
    body = re.search(r"typedef struct mbpo_ens_train_desc \{(.*?)\} mbpo_ens_train_desc;", h, re.S).group(1)
    assert re.search(r"int32_t reward_off;[^\n]*\n\s*$", body), "reward_off must be the last field"
    assert _hip.EnsTrainDesc._fields_[-1] == ("reward_off", C.c_int32)


def _ens_desc(dout, reward_off, X=X, U=U, E=E):
    from mbpo import _hip
    d = _hip.EnsTrainDesc()
    d.x_dim, d.u_dim, d.batch, d.min_std, d.predict_delta = X, U, 64, 1e-3, 1
    m = d.dynamics
    m.params, m.n_nets, m.n_layers, m.activation = 16, E, 4, _hip.ACT_IDS["swish"]
    for i, v in enumerate([X + U, 64, 64, 64, dout]):
        m.dims[i] = v
    m.net_stride = sum(m.dims[i] * m.dims[i + 1] + m.dims[i + 1] for i in range(4))
    d.row_len, d.next_obs_off, d.reward_off = 2 * X + U + 3, X + U + 2, reward_off
    return d


def test_ens_nll_plan_takes_the_reward_head(lib):
    ws = lambda d: lib.mbpo_ens_nll_workspace_floats(C.byref(d))
    assert ws(_ens_desc(2 * X, -1)) > 0
    assert ws(_ens_desc(2 * X + 2, X + U)) > 0
    assert ws(_ens_desc(2 * X + 2, -1)) > 0                 # an analytic-reward fit of a reward-capable ensemble
    assert ws(_ens_desc(2 * X, X + U)) < 0                  # no head to fit
    assert ws(_ens_desc(2 * X + 2, 2 * X + U + 3)) < 0      # outside the row
    # the workspace is the slabs of the parameters: the head adds exactly its output-layer parameters per member and slot
    assert ws(_ens_desc(2 * X + 2, X + U)) == ws(_ens_desc(2 * X + 2, -1))


def _bptt_desc(reward_kind, dout, system="ensemble"):
    from mbpo import _hip
    import test_cpu_bptt_stochastic as tb
    d = tb._desc(system=system, dyn_out=dout)
    d.reward_kind = reward_kind
    return d


def test_bptt_plan_takes_the_learned_reward(lib):
    from mbpo import _hip
    ws = lambda d: lib.mbpo_bptt_workspace_floats(C.byref(d))
    assert ws(_bptt_desc(_hip.REWARD_LEARNED, 2 * X + 2)) > 0
    assert ws(_bptt_desc(_hip.REWARD_QUADRATIC, 2 * X + 2)) > 0      # the analytic rewards ignore the head
    assert ws(_bptt_desc(_hip.REWARD_LEARNED, 2 * X)) < 0
    assert ws(_bptt_desc(_hip.REWARD_LEARNED, 0, system="pendulum")) < 0


def test_model_rollout_refuses_what_it_cannot_run(lib):
    """The argument checks run before any device work (and empty rollouts return after them)."""
    from mbpo import _hip
    d = _hip.RolloutDesc()
    d.x_dim, d.u_dim, d.n_envs, d.n_steps, d.episode_length, d.action_repeat = X, U, 0, 0, 5, 1
    d.row_len = 2 * X + U + 3
    d.actions = 16
    d.system_kind, d.reward_kind = _hip.SYS_ENSEMBLE, _hip.REWARD_LEARNED
    m = d.dynamics
    m.params, m.n_nets, m.n_layers, m.activation = 16, E, 4, _hip.ACT_IDS["swish"]
    for dout, ok in ((2 * X + 2, True), (2 * X, False)):
        for i, v in enumerate([X + U, 64, 64, 64, dout]):
            m.dims[i] = v
        m.net_stride = sum(m.dims[i] * m.dims[i + 1] + m.dims[i + 1] for i in range(4))
        rc = lib.mbpo_model_rollout(C.byref(d), None)
        assert (rc == 0) == ok, (dout, rc)
    d.system_kind = _hip.SYS_PENDULUM
    d.sys_params = 16
    assert lib.mbpo_model_rollout(C.byref(d), None) != 0     # the learned reward needs the ensemble


def test_host_api_wiring():
    from mbpo import _hip
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, LearnedReward, QuadraticReward
    dyn = EnsembleDynamics(X, U, n_members=E, device="cpu", learn_reward=True)
    assert dyn.dims[-1] == 2 * X + 2 and dyn.spec.n_params == onets.n_params(dyn.dims)
    plain = EnsembleDynamics(X, U, n_members=E, device="cpu")
    assert plain.dims[-1] == 2 * X
    with pytest.raises(ValueError):
        LearnedReward(plain)
    rew = LearnedReward(dyn)
    with pytest.raises(ValueError):
        EnsembleSystem(plain, rew)
    with pytest.raises(ValueError):
        EnsembleSystem(EnsembleDynamics(X, U, n_members=E, device="cpu", learn_reward=True), rew)    # another model's head
    system = EnsembleSystem(dyn, rew, mode="ts1")
    sp = system.init_params(3)
    assert sp.reward_params is sp.dynamics_params                 # one object: fit's in-place updates reach both
    spec = system.rollout_spec(sp, torch.device("cpu"))
    assert spec["reward_kind"] == _hip.REWARD_LEARNED and spec["reward_params"] is None
    assert spec["dyn_spec"].dims[-1] == 2 * X + 2
    # the spec cache never takes the repr of the parameters (a device tensor: the repr would copy it to the host)
    class NoRepr:
        def __repr__(self):
            raise AssertionError("repr of the learned reward's parameters")
    assert system.rollout_spec(sp.replace(reward_params=NoRepr()), torch.device("cpu"))["reward_kind"] == _hip.REWARD_LEARNED
    # an analytic reward still works on a reward-capable ensemble
    q = EnsembleSystem(dyn, QuadraticReward(X, U))
    assert q.rollout_spec(q.init_params(0), torch.device("cpu"))["reward_kind"] == _hip.REWARD_QUADRATIC
    with pytest.raises(ValueError):
        plain.fit(plain.init_params(0), torch.zeros(8, 2 * X + U + 3), 1, reward_off=X + U)


def test_differentiable_step_reads_the_reward_head():
    """torch_steps.DifferentiableBuiltin (the wide BPTT path) takes r from y[..., 2X], in every mode, through a stand-in MLP node."""
    from mbpo import _hip, ops
    from mbpo.systems.torch_steps import DifferentiableBuiltin
    g = torch.Generator().manual_seed(0)
    dims = [X + U, 64, 64, 2 * X + 2]
    dp = torch.cat([onets.init_mlp_flat(dims, g) + 0.05 * torch.randn(onets.n_params(dims), generator=g) for _ in range(E)])
    x, u = torch.randn(7, X, generator=g), torch.randn(7, U, generator=g)
    members = torch.randint(0, E, (7,), generator=g, dtype=torch.int32)

    class Node:
        @staticmethod
        def apply(p, xu, spec, *_):
            return onets.ensemble_forward(p, spec.dims, spec.n_nets, xu)
    real = ops.HipMlp
    ops.HipMlp = Node
    try:
        for mode in ("mean", "ts1"):
            spec = dict(system_kind=_hip.SYS_ENSEMBLE, dyn_params=dp, dyn_spec=ops.MlpSpec(dims, "swish", E),
                        ens_mode=_hip.ENS_MEAN if mode == "mean" else _hip.ENS_TS1, ens_predict_delta=True, ens_sample_noise=False,
                        ens_min_std=1e-3, reward_kind=_hip.REWARD_LEARNED, reward_params=None)
            sysd = DifferentiableBuiltin(type("S", (), {"x_dim": X, "u_dim": U})(), spec)
            st = sysd.step(x, u, None, member=members if mode == "ts1" else None)
            ref = lref.TorchLearnedRewardSystem(dp, dims, E, X, U, members=None if mode == "mean" else members[:, None])
            xn, r = ref.step(x, u)
            torch.testing.assert_close(st.x_next, xn, atol=1e-6, rtol=1e-6)
            torch.testing.assert_close(st.reward, r, atol=1e-6, rtol=1e-6)
    finally:
        ops.HipMlp = real


def test_restatement_consistency():
    """The reference system's state equals oracle.systems.EnsembleSystem on the head-cut weights, and its reward is the head."""
    from oracle import systems as osys
    g = torch.Generator().manual_seed(1)
    dims = [X + U, 64, 64, 2 * X + 2]
    dp = torch.cat([onets.init_mlp_flat(dims, g) + 0.05 * torch.randn(onets.n_params(dims), generator=g) for _ in range(E)])
    cut = lref.reward_head_params(dp, dims, E)
    x, u = torch.randn(9, X, generator=g), torch.randn(9, U, generator=g)
    mem = torch.randint(0, E, (9,), generator=g)
    for mode in ("mean", "ts1", "tsinf"):
        a = lref.LearnedRewardEnsembleSystem(dp, dims, E, X, U, mode=mode)
        b = osys.EnsembleSystem(cut, dims[:-1] + [2 * X], E, X, U, mode=mode, reward_fn=lambda x, u: torch.zeros(x.shape[0]))
        xa, ra = a.step(x, u, member_idx=mem, env_index=torch.arange(9))
        xb, _ = b.step(x, u, member_idx=mem, env_index=torch.arange(9))
        assert torch.equal(xa, xb)
        y = onets.ensemble_forward(dp, dims, E, torch.cat([x, u], 1))
        m = {"mean": None, "ts1": mem, "tsinf": torch.arange(9) % E}[mode]
        want = y[..., 2 * X].mean(0) if m is None else y[m, torch.arange(9), 2 * X]
        torch.testing.assert_close(ra, want, atol=1e-6, rtol=1e-6)
    # the fit's reward term is the Gaussian NLL of the head: zero-weight rows of the state part leave only it
    rows = torch.randn(20, 2 * X + U + 3, generator=g)
    idx = torch.randint(0, 20, (E, 8), generator=g)
    g_with, l_with = lref.nll_grads(dp, dims, E, rows, idx, X, U, reward_off=X + U)
    g_wo, l_wo = lref.nll_grads(dp, dims, E, rows, idx, X, U, reward_off=None)
    assert bool((l_with != l_wo).all())
    P = onets.n_params(dims)
    head = torch.zeros(P, dtype=torch.bool)
    last = onets.unflatten(torch.arange(P, dtype=torch.float64), dims)[-1]
    for t in last:
        head[t[..., -2:].reshape(-1).long()] = True
    # without the reward term the head's own weights get no gradient
    assert float(g_wo.reshape(E, P)[:, head].abs().max()) == 0.0
    assert float(g_with.reshape(E, P)[:, head].abs().max()) > 0.0
