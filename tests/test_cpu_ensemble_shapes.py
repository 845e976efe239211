"""Ensembles of any hidden sizes without a device: the model-learning plan sizes a layered path for every shape the fused kernel
does not take (MBPO's 7 x 4 x 200 among them), the storage rule (hidden layers zero-padded to a rollout width up to 256, logical
above), the embed / extract round trip, and init_params unchanged for 64-wide stacks."""
import ctypes as C

import pytest
import torch

X, U = 4, 1


@pytest.fixture(scope="module")
def lib():
    from mbpo import _hip
    return _hip.load()


def _desc(hidden, X=X, U=U, E=7, B=256, dout=None, reward_off=-1):
    from mbpo import _hip
    d = _hip.EnsTrainDesc()
    d.x_dim, d.u_dim, d.batch, d.min_std, d.predict_delta = X, U, B, 1e-3, 1
    dims = [X + U, *hidden, 2 * X if dout is None else dout]
    m = d.dynamics
    m.params, m.n_nets, m.n_layers, m.activation = 16, E, len(dims) - 1, _hip.ACT_IDS["swish"]
    for i, v in enumerate(dims):
        m.dims[i] = v
    m.net_stride = sum(dims[i] * dims[i + 1] + dims[i + 1] for i in range(len(dims) - 1))
    d.row_len, d.next_obs_off, d.reward_off = 2 * X + U + 3, X + U + 2, reward_off
    return d


def fused_lds_bytes(X, U, dout, n_hidden):
    """The fused kernel's LDS plan (ensemble_train.hip, ens_plan): above 160 KiB the layered path runs."""
    up4 = lambda v: (v + 3) & ~3
    ld_xu, ld_h, ld_y = up4(X + U) + 4, 68, up4(dout) + 4
    return 4 * (16 * ld_xu + 3 * 16 * ld_y + (2 * n_hidden + 2) * 16 * ld_h + 16)


def deep_64_case():
    """The shallowest 64-wide stack (at most MBPO_MAX_LAYERS Dense layers) whose fused plan passes 160 KiB, searched over x_dim."""
    for x in range(4, 400):
        for n_hidden in range(1, 8):
            if fused_lds_bytes(x, 2, 2 * x, n_hidden) > 160 * 1024:
                return x, 2, n_hidden
    raise AssertionError("no 64-wide stack passes the LDS plan")


def layered_workspace(X, U, E, B, hidden, dout):
    """Restatement of the layered path's workspace (B <= 1024: no split-k partials)."""
    r4 = lambda n: (n + 3) & ~3
    EB = E * B
    return (r4(EB * (X + U)) + r4(EB * (X + 1)) + sum(2 * r4(EB * h) for h in hidden) + 2 * r4(EB * dout)
            + 2 * r4(EB * max([X + U, *hidden, dout])))


def test_ens_nll_plan_takes_any_hidden_sizes(lib):
    ws = lambda d: int(lib.mbpo_ens_nll_workspace_floats(C.byref(d)))
    # MBPO's model: 7 members of 4 x 200 (was MBPO_ERR_UNSUPPORTED)
    assert ws(_desc((200,) * 4)) == layered_workspace(X, U, 7, 256, (200,) * 4, 2 * X) > 0
    assert ws(_desc((256,) * 4)) == layered_workspace(X, U, 7, 256, (256,) * 4, 2 * X)
    assert ws(_desc((200, 100, 50), E=3, B=37)) == layered_workspace(X, U, 3, 37, (200, 100, 50), 2 * X)
    assert ws(_desc((512, 512), E=2)) > 0
    assert ws(_desc((200,) * 4, dout=2 * X + 2, reward_off=X + U)) == ws(_desc((200,) * 4, dout=2 * X + 2))
    x, u, nh = deep_64_case()
    assert ws(_desc((64,) * nh, X=x, U=u, E=2, B=64)) == layered_workspace(x, u, 2, 64, (64,) * nh, 2 * x)
    # the 64-wide shapes the fused kernel takes keep its plan (slabs of the parameters, not activations)
    assert ws(_desc((64,) * 3)) != layered_workspace(X, U, 7, 256, (64,) * 3, 2 * X)
    # the argument checks hold on the layered path too
    assert ws(_desc((200,) * 4, reward_off=X + U)) < 0                       # no head to fit
    assert ws(_desc((200,) * 4, dout=2 * X + 1)) < 0


@pytest.mark.parametrize("hidden,width", [
    ((64, 64, 64), 64), ((128, 128), 128), ((256,) * 4, 256), ((200,) * 4, 256), ((200, 100), 256), ((100, 30), 128),
    ((32,), 64), ((512, 512), None), ((300, 100), None),
])
def test_storage_rule(hidden, width):
    from mbpo import ops
    from mbpo.systems import EnsembleDynamics
    from mbpo.systems.ensemble_system import kernel_width_for
    assert kernel_width_for(hidden) == width
    dyn = EnsembleDynamics(X, U, n_members=7, hidden_layer_sizes=hidden, device="cpu")
    assert dyn.kernel_width == width
    assert dyn.dims_logical == [X + U, *hidden, 2 * X]
    assert dyn.dims == ops.padded_dims(dyn.dims_logical, width)
    assert list(dyn.spec.dims) == dyn.dims and dyn.spec.n_nets == 7
    if width is not None:
        assert all(h == width for h in dyn.dims[1:-1])


def test_embed_extract_round_trip():
    from oracle import nets as onets
    from mbpo.systems import EnsembleDynamics
    E = 3
    dyn = EnsembleDynamics(X, U, n_members=E, hidden_layer_sizes=(200, 100, 50), device="cpu", learn_reward=True)
    P = onets.n_params(dyn.dims_logical)
    flat = torch.randn(E * P, generator=torch.Generator().manual_seed(0))
    p = dyn.from_logical_params(flat)
    assert p.params.numel() == dyn.spec.total_params
    assert torch.equal(dyn.logical_params(p), flat)
    # the padded network computes the logical one
    xu = torch.randn(11, X + U, generator=torch.Generator().manual_seed(1))
    y_pad = onets.ensemble_forward(p.params, dyn.dims, E, xu)
    y_log = onets.ensemble_forward(flat, dyn.dims_logical, E, xu)
    torch.testing.assert_close(y_pad, y_log, atol=1e-5, rtol=1e-5)
    # exactly the padded entries are zero: the embed of an all-ones logical vector
    ones = dyn.from_logical_params(torch.ones(E * P)).params
    assert int((ones != 0).sum()) == E * P
    # above 256 the parameters are the logical ones
    wide = EnsembleDynamics(X, U, n_members=2, hidden_layer_sizes=(512,), device="cpu")
    f2 = torch.randn(2 * onets.n_params(wide.dims_logical))
    assert torch.equal(wide.logical_params(wide.from_logical_params(f2)), f2)


def test_init_params_unchanged_for_64_wide():
    from mbpo.systems import EnsembleDynamics
    from mbpo.systems.ensemble_system import lecun_uniform_flat
    from mbpo.utils import keys as K
    E, key = 5, 3
    dyn = EnsembleDynamics(X, U, n_members=E, device="cpu")
    gen = torch.Generator().manual_seed(K.PRNGKey(key) % (2 ** 63))
    ref = torch.cat([lecun_uniform_flat([X + U, 64, 64, 64, 2 * X], gen) for _ in range(E)])
    assert torch.equal(dyn.init_params(key).params, ref)


def test_init_params_embeds_the_logical_draw():
    from mbpo.systems import EnsembleDynamics
    from mbpo.systems.ensemble_system import lecun_uniform_flat
    from mbpo.utils import keys as K
    E, key = 7, 4
    dyn = EnsembleDynamics(X, U, n_members=E, hidden_layer_sizes=(200,) * 4, device="cpu")
    p = dyn.init_params(key)
    assert p.params.numel() == dyn.spec.total_params and dyn.dims == [X + U, 256, 256, 256, 256, 2 * X]
    gen = torch.Generator().manual_seed(K.PRNGKey(key) % (2 ** 63))
    ref = torch.cat([lecun_uniform_flat(dyn.dims_logical, gen) for _ in range(E)])
    assert torch.equal(dyn.logical_params(p), ref)
    assert torch.equal(dyn.from_logical_params(ref).params, p.params)
