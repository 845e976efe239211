"""The ensemble's input scaler without a GPU: the fold identity in fp64, padding through the fold, the constant-column rule, the
prepared layout, argument validation of the three entry points (no launches) and the cancellation measurement.

Cancellation ("Input scaler"): the folded layer evaluates sum W'x - sum W'm where the unfolded one evaluates sum W'(x - m).
Measured by test_cancellation_measurement on ens_scaler_ref.cancellation_case (3 members of 4-64-64-64-6, 256 inputs within 3 std of
the mean), max |fp32 folded - fp64 unfolded| over all outputs:
    set a (|mean| <= 3 std in every column):   8.8e-07
    set b (one column at mean = 1000 std):     3.0e-05
(7.6e-07 for set a on another host: the figure depends on the CPU's summation order in the last digit.)
Figure a, taken at run time, times 4 is the tolerance of tests/test_gpu_ens_input_scaler.py's end-to-end comparison."""
import ctypes as C

import pytest
import torch

from oracle import nets as onets

import ens_scaler_ref as ref


def _net_and_scaler(dims, E, seed):
    g = torch.Generator().manual_seed(seed)
    P = onets.n_params(dims)
    params = torch.cat([onets.init_mlp_flat(dims, g, dtype=torch.float64) + 0.02 * torch.randn(P, generator=g, dtype=torch.float64)
                        for _ in range(E)])
    D = dims[0]
    mean = torch.randn(D, generator=g, dtype=torch.float64) * 5
    std = torch.exp(torch.randn(D, generator=g, dtype=torch.float64) * 2)           # stds over orders of magnitude
    xu = mean + std * torch.randn(200, D, generator=g, dtype=torch.float64)
    return params, torch.stack([mean, std]), xu


@pytest.mark.parametrize("dims", [(4, 64, 64, 64, 6), (23, 64, 34)])
def test_fold_identity_fp64(dims):
    E = 3
    params, scaler, xu = _net_and_scaler(dims, E, seed=len(dims))
    folded = ref.folded_net(params, dims, E, scaler, xu)
    unfolded = ref.normalise_then_net64(params, dims, E, scaler, xu)
    rel = float((folded - unfolded).abs().max() / unfolded.abs().max())
    print(f"fold identity {dims}: max |folded - unfolded| / max |unfolded| = {rel:.3e}")
    assert rel <= 1e-12
    # everything outside layer one is copied
    P, n1 = onets.n_params(dims), dims[0] * dims[1] + dims[1]
    f = ref.fold(params, dims, E, scaler).reshape(E, P)
    assert torch.equal(f[:, n1:], params.reshape(E, P)[:, n1:]) and not torch.equal(f[:, :n1], params.reshape(E, P)[:, :n1])


def test_padding_stays_zero_through_the_fold():
    """A 200-wide first layer stored at 256: the 56 padded columns of W_0 and b_0 are +0 before and exactly +0 after, in fp32 and
    fp64, whatever the signs of the means."""
    X, U, H, W = 3, 1, 200, 256
    g = torch.Generator().manual_seed(0)
    w = torch.zeros(X + U, W)
    w[:, :H] = torch.randn(X + U, H, generator=g)
    b = torch.zeros(W)
    b[:H] = torch.randn(H, generator=g)
    tail = torch.randn(W * 8 + 8, generator=g)
    dims = (X + U, W, 8)
    params = torch.cat([w.reshape(-1), b, tail])
    scaler = torch.tensor([[3.0, -7.0, 1e4, -0.0], [0.5, 20.0, 1.0, 3.0]])
    for dt in (torch.float32, torch.float64):
        f = ref.fold(params.to(dt), dims, 1, scaler)
        fw, fb = f[:(X + U) * W].reshape(X + U, W), f[(X + U) * W:(X + U) * W + W]
        zero_bits = torch.zeros((), dtype=dt).view(torch.int64 if dt == torch.float64 else torch.int32)
        for t in (fw[:, H:], fb[H:]):
            assert bool((t.contiguous().view(zero_bits.dtype) == zero_bits).all())         # +0.0, not -0.0
        assert bool((fw[:, :H] != 0).all())


def test_constant_column_gets_std_one():
    g = torch.Generator().manual_seed(1)
    rows = torch.randn(50, 7, generator=g)
    rows[:, 2] = 3.25
    s = ref.stats64(rows, 5)
    assert float(s[1, 2]) == 1.0 and float(s[0, 2]) == 3.25
    assert bool((s[1, [0, 1, 3, 4]] != 1.0).all())
    one = ref.stats64(rows, 5, n=1)                                                     # a single row: std 1 everywhere
    assert torch.equal(one[1], torch.ones(5, dtype=torch.float64)) and torch.equal(one[0], rows[0, :5].double())
    assert ref.stats64(rows, 5, std_floor=10.0)[1].tolist() == [1.0] * 5                # the floor is a parameter


def test_prepared_layout_constants():
    from mbpo import ops
    for X, U in ((3, 1), (17, 6)):
        assert ref.prepared_reward_off(X, U) == ops.prepared_reward_off(X, U) == X + U
        assert ref.prepared_next_obs_off(X, U) == ops.prepared_next_obs_off(X, U) == X + U + 1
        assert ref.prepared_row_len(X, U) == ops.prepared_row_len(X, U) == 2 * X + U + 1
    X, U = 3, 1
    rows = torch.arange(2 * 9, dtype=torch.float32).reshape(2, 9)
    scaler = torch.stack([torch.zeros(4), torch.ones(4)])
    out = ref.prepare(rows, scaler, X, U, reward_off=4, predict_delta=False)
    assert out.shape == (2, 8) and torch.equal(out[:, X + U], rows[:, 4]) and torch.equal(out[:, X + U + 1:], rows[:, 6:9])
    assert torch.equal(ref.prepare(rows, scaler, X, U)[:, X + U], torch.zeros(2))      # no reward column: 0


def test_argument_validation_without_a_device():
    """Every refusal is MBPO_ERR_ARG with a message, before anything is launched (the pointers are never dereferenced)."""
    from mbpo import _hip
    lib = _hip.load()
    ERR_ARG = -1
    p = 1 << 20                                                                         # a non-null, 16-byte aligned "device pointer"
    assert lib.mbpo_ens_scaler_workspace_floats(100000, 5) > 0
    assert lib.mbpo_ens_scaler_workspace_floats(1, 5) == 2 * 2 * 5                     # one workgroup, two passes of fp64 partials
    assert lib.mbpo_ens_scaler_workspace_floats(0, 5) == ERR_ARG
    assert lib.mbpo_ens_scaler_workspace_floats(10, 0) == ERR_ARG
    # the statistics: (rows, n_rows, row_len, idx, n, in_dim, std_floor, scaler, workspace, stream)
    fit = lambda rows=p, n_rows=37, row_len=9, idx=None, n=37, in_dim=4, floor=1e-12, scaler=p + 4096, ws=p + 8192: \
        lib.mbpo_ens_scaler_fit(rows, n_rows, row_len, idx, n, in_dim, floor, scaler, ws, None)
    for bad in (dict(rows=None), dict(scaler=None), dict(ws=None), dict(n=0), dict(floor=-1.0), dict(floor=float("nan")),
                dict(n=38), dict(in_dim=10), dict(ws=p + 8196)):
        assert fit(**bad) == ERR_ARG, bad
        assert lib.mbpo_last_error()
    assert fit(floor=-1.0) == ERR_ARG and b"std_floor" in lib.mbpo_last_error()
    # prepare: (rows, n_rows, row_len, idx, n, x, u, next_obs_off, reward_off, predict_delta, scaler, out, stream)
    prep = lambda rows=p, n_rows=37, row_len=9, idx=None, n=37, x=3, u=1, noff=6, roff=4, scaler=p + 4096, out=p + 8192: \
        lib.mbpo_ens_scaler_prepare(rows, n_rows, row_len, idx, n, x, u, noff, roff, 1, scaler, out, None)
    for bad in (dict(rows=None), dict(scaler=None), dict(out=None), dict(n=0), dict(n=38), dict(noff=7), dict(noff=-1), dict(roff=9),
                dict(x=0), dict(u=-1)):
        assert prep(**bad) == ERR_ARG, bad
    # fold: (params, n_params, n_members, dims0, dims1, scaler, out_params, stream)
    P, E = 4 * 64 + 64 + 64 * 6 + 6, 3
    fold = lambda params=p, n_params=P, E=E, d0=4, d1=64, scaler=p + (1 << 16), out=p + (1 << 17): \
        lib.mbpo_ens_fold_scaler(params, n_params, E, d0, d1, scaler, out, None)
    for bad in (dict(params=None), dict(scaler=None), dict(out=None), dict(E=0), dict(n_params=0), dict(d1=4096),
                dict(out=p), dict(out=p + 4 * (E * P - 1)), dict(out=p - 4 * (E * P - 1))):
        assert fold(**bad) == ERR_ARG, bad
    assert fold(out=p) == ERR_ARG and b"overlaps" in lib.mbpo_last_error()


def test_cancellation_measurement():
    """The figures quoted in this module's docstring and in DESIGN.md: measured, printed, and bounded only by the analysis — the
    layer-one error bound 2^-24 * sum_i |W'_ij| (|x_i| + |m_i|), carried to the output by the network's own sensitivity, which the
    comparison of the two sets isolates: set b exceeds set a, and by no more than the ratio of the two bounds times a margin of 4."""
    fig, bound = {}, {}
    for kind in ("a", "b"):
        params, scaler, xu = ref.cancellation_case(kind)
        fig[kind] = ref.fold_discrepancy(params, ref.CANCEL_DIMS, ref.CANCEL_MEMBERS, scaler, xu)
        d0, d1 = ref.CANCEL_DIMS[0], ref.CANCEL_DIMS[1]
        P = onets.n_params(ref.CANCEL_DIMS)
        w = torch.stack([params[e * P:e * P + d0 * d1].reshape(d0, d1) for e in range(ref.CANCEL_MEMBERS)]).double()
        wf = w / scaler[1].double()[None, :, None]
        mag = xu.double().abs() + scaler[0].double().abs()                              # [N, d0]
        bound[kind] = float(2.0 ** -24 * torch.einsum("ni,eij->enj", mag, wf.abs()).max())
        print(f"cancellation set {kind}: max |fp32 folded - fp64 unfolded| = {fig[kind]:.3e}; layer-one bound {bound[kind]:.3e}")
    assert 0 < fig["a"] < fig["b"]
    assert fig["b"] / fig["a"] <= 4 * bound["b"] / bound["a"]
