"""GPU parity where one workgroup walks MANY tiles: every fused family against its float64 oracle at the very size the kernel runs, on
rows that are all independent draws (tests/many_tiles_cases.py; the replication tests of the per-family modules feed copies of one
tile, so a tile that read what its predecessor left in LDS, registers or a z-store slot would still read correct values there).

Sizes come from the device: tiles > 2 x the launch's cap (a multiple of the compute-unit count), not a multiple of it, ragged last
tile.  Tolerances: those at the head of test_gpu_ppo.py / test_gpu_sac.py / test_gpu_rollout.py / test_gpu_bptt.py against float64
(one PPO case is allowed 4 x the float32 oracle's own gap: many_tiles_cases.PPO_TOL); tests/test_cpu_many_tiles_cases.py pins the
table at 256 compute units.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import many_tiles_cases as mt

pytestmark = pytest.mark.gpu


def _cus(dev) -> int:
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _debug_setter(name):
    from mbpo import _hip
    fn = getattr(_hip.load(), name)
    fn.argtypes = [C.c_int]
    fn.restype = C.c_int
    return fn


# ---------------------------------------------------------------------------------------------------------------------- PPO
@pytest.mark.parametrize("name", list(mt.PPO_CASES))
def test_ppo_many_tiles_against_fp64_oracle(dev, name):
    """Full minibatch_step as in test_ppo_gradients_and_step (gradients, loss terms, AdamW given the device gradient) with more than
    two tiles per gradient slab: k_ppo_fwd_bwd<128,2,false>, the wide <64,4,true>, and the 512-thread <64,2,false> (two slabs per CU)
    with per-sample discounts in the values + GAE launch."""
    from oracle import ppo as oppo
    from test_gpu_ppo import _updater
    from test_gpu_ppo_brax_env import NEQ_KW
    case = mt.PPO_CASES[name]
    cus = _cus(dev)
    B, T = mt.ppo_bt(case, cus)
    assert mt.loops_unevenly(B * T, mt.ppo_cap(case, cus))
    inputs = mt.ppo_inputs(case, cus)
    cfg, st, data, noise, nm, ns = inputs
    g64, terms64 = mt.ppo_oracle(case, inputs, torch.float64)
    up = _updater(dev, cfg, B, T, **(NEQ_KW if case["neq"] else {}))
    up.load_state(st.params.to(dev))
    dd = lambda t: None if t is None else t.to(dev)
    up.minibatch_step(data.to(dev), dd(nm), dd(ns), noise.to(dev))
    torch.cuda.synchronize()
    g = up.grads.cpu()
    err = (g.double() - g64).abs()
    tol = mt.ppo_tol(case)
    print(f"ppo {name}: B={B} T={T} tiles={mt.tiles_of(B * T)} max|dg|={float(err.max()):.3e} "
          f"worst/tol={float((err / (tol['atol'] + tol['rtol'] * g64.abs())).max()):.3f}")
    torch.testing.assert_close(g.double(), g64, **tol)
    np.testing.assert_allclose(up.metrics.cpu().tolist(), [terms64[k] for k in ("total_loss", "policy_loss", "v_loss", "entropy_loss")],
                               rtol=2e-5, atol=1e-5)
    st_new, _, _ = oppo.minibatch_step(cfg, st, data, noise, nm, ns, grad_override=g)
    torch.testing.assert_close(up.params.cpu(), st_new.params, atol=1e-7, rtol=1e-6)
    torch.testing.assert_close(up.adam_m.cpu(), st_new.adam_m, atol=1e-9, rtol=1e-5)
    torch.testing.assert_close(up.adam_v.cpu(), st_new.adam_v, atol=1e-12, rtol=1e-5)
    assert float(up.step_count.cpu()) == 1.0


# ---------------------------------------------------------------------------------------------------------------------- SAC
@pytest.mark.parametrize("B", mt.SAC_BATCHES)
@pytest.mark.parametrize("name", list(mt.SAC_CASES))
def test_sac_many_tiles_against_fp64_oracle(dev, name, B):
    """38 and 70 tiles (two and four full blocks of slab_sum<16> plus a tail of six, the last tile of 8 rows) through the five launch
    variants, each as the three-launch step and as the two-launch step (defined to be bit-equal), against float64."""
    from oracle import sac as osac
    from test_gpu_sac import _updater
    case = mt.SAC_CASES[name]
    inputs = mt.sac_inputs(case, B)
    cfg, st, batch, noise, nm, ns = inputs
    g64, (cl64, ac64, al64) = mt.sac_oracle(inputs, torch.float64)
    d = lambda t: None if t is None else t.to(dev)
    set_lean = _debug_setter("mbpo_debug_set_sac_lean")
    outs = []
    try:
        if case["lean"] >= 0:
            assert set_lean(case["lean"]) == 0
        for two_launch in (False, True):
            up = _updater(dev, cfg, B, two_launch=two_launch)
            up.load_state(st.params.to(dev), st.target_q.to(dev))
            up.sgd_step(batch.to(dev), d(nm), d(ns), *[n.to(dev) for n in noise])
            up.finalize()
            torch.cuda.synchronize()
            outs.append([t.cpu().clone() for t in (up.grads, up.params, up.target_q, up.adam_m, up.adam_v, up.metrics)])
            assert float(up.step_count.cpu()) == 1.0
    finally:
        set_lean(-1)
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    g, params, target_q, adam_m, adam_v, metrics = outs[0]
    P, Q = cfg.P, cfg.Q
    err = (g.double() - g64).abs() / (mt.SAC_TOL["atol"] + mt.SAC_TOL["rtol"] * g64.abs())
    print(f"sac {name} B={B}: worst/tol={float(err.max()):.3f}")
    for gname, sl in (("policy", slice(0, P)), ("critic", slice(P, P + 2 * Q)), ("alpha", slice(P + 2 * Q, None))):
        torch.testing.assert_close(g[sl].double(), g64[sl], msg=lambda m: f"{gname} grad vs fp64 oracle: {m}", **mt.SAC_TOL)
    st_new, met, _ = osac.sgd_step(cfg, st, batch, *noise, nm, ns, grad_override=g)
    np.testing.assert_allclose(metrics.tolist()[:3], [cl64, ac64, al64], rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(metrics.tolist()[3], met["alpha"], rtol=1e-6)
    torch.testing.assert_close(params, st_new.params, atol=1e-7, rtol=1e-6)
    torch.testing.assert_close(target_q, st_new.target_q, atol=1e-7, rtol=1e-6)
    torch.testing.assert_close(adam_m, st_new.adam_m, atol=1e-9, rtol=1e-5)
    torch.testing.assert_close(adam_v, st_new.adam_v, atol=1e-12, rtol=1e-5)


# ------------------------------------------------------------------------------------------------------------------ rollout
def _rollout_hip(dev, case, inp):
    from mbpo import _hip, ops
    X, U, E = case["X"], case["U"], case["E"]
    pdims, ddims, ppar, dpar = inp["pdims"], inp["ddims"], inp["ppar"], inp["dpar"]
    if case.get("pad"):                    # zero-padded to one kernel width, as the trainers do (ops.py "hidden-width padding")
        W = case["pad"]
        ppar, dpar = ops.embed_mlp_params(ppar, pdims, W), ops.embed_mlp_params(dpar, ddims, W, n_nets=E)
        pdims, ddims = ops.padded_dims(pdims, W), ops.padded_dims(ddims, W)
    learned = case.get("reward") == "learned"
    d = lambda t: None if t is None else t.to(dev)
    obs_d, steps_d, done_d = inp["obs0"].to(dev), inp["steps0"].to(dev), inp["done0"].to(dev)
    rows = ops.model_rollout(policy_params=ppar.to(dev), policy_spec=ops.MlpSpec(pdims, "swish", 1), x_dim=X, u_dim=U, obs=obs_d,
                             first_obs=inp["first"].to(dev), steps=steps_d, done=done_d, n_steps=mt.RO_S, episode_length=mt.RO_L,
                             action_repeat=1, reward_params=d(inp["rparams"]), norm_mean=d(inp["nm"]), norm_std=d(inp["ns"]),
                             policy_noise=inp["pnoise"].to(dev), model_noise=d(inp["mnoise"]), member_idx=d(inp["midx"]),
                             system_kind=_hip.SYS_ENSEMBLE, dyn_params=dpar.to(dev), dyn_spec=ops.MlpSpec(ddims, "swish", E),
                             ens_mode={"mean": _hip.ENS_MEAN, "ts1": _hip.ENS_TS1}[case.get("mode", "mean")], ens_predict_delta=True,
                             ens_sample_noise=bool(case.get("sample_noise")), ens_min_std=1e-3,
                             reward_kind=_hip.REWARD_LEARNED if learned else _hip.REWARD_QUADRATIC)
    torch.cuda.synchronize()
    return rows.cpu(), obs_d.cpu(), steps_d.cpu(), done_d.cpu()


@pytest.mark.parametrize("name", list(mt.RO_CASES))
def test_rollout_many_tiles_against_fp64_oracle(dev, name):
    """N = 16 (2 x 4 CUs + 3) + 5 independent environments, S = 3, L = 2: every workgroup of the generic kernels (grid 4 x CUs) takes two
    or three tiles, the lean kernel (grid = CUs, pairs of tiles) four or five pairs; rows, final observations and the exact
    bookkeeping columns against the float64 oracle."""
    case = mt.RO_CASES[name]
    cus = _cus(dev)
    N = mt.ro_n(cus)
    units, cap = mt.ro_units(case, N), mt.ro_cap(case, cus)
    assert units > 2 * cap and units % cap != 0 and N % 16 != 0
    inp = mt.ro_inputs(case, N)
    st_ref, rows_ref = mt.ro_oracle(case, inp, torch.float64)
    set_lean = _debug_setter("mbpo_debug_set_rollout_lean")
    try:
        if case["lean"] >= 0:
            assert set_lean(case["lean"]) == 0
        rows, obs, steps, done = _rollout_hip(dev, case, inp)
    finally:
        set_lean(-1)
    X, U, D = case["X"], case["U"], rows.shape[1]
    err = (rows.double() - rows_ref).abs() / (mt.RO_TOL["atol"] + mt.RO_TOL["rtol"] * rows_ref.abs())
    print(f"rollout {name}: N={N} tiles={mt.tiles_of(N)} worst/tol={float(err.max()):.3f}")
    assert torch.equal(rows[:, X + U + 1].double(), rows_ref[:, X + U + 1])
    assert torch.equal(rows[:, D - 1].double(), rows_ref[:, D - 1])
    assert torch.equal(steps.double(), st_ref.steps) and torch.equal(done.double(), st_ref.done)
    torch.testing.assert_close(rows.double(), rows_ref, **mt.RO_TOL)
    torch.testing.assert_close(obs.double(), st_ref.obs, **mt.RO_TOL)
    if case.get("reward") == "learned":
        assert float(rows[:, X + U].abs().max()) > 1e-3


# --------------------------------------------------------------------------------------------------------------------- BPTT
@pytest.mark.parametrize("name", list(mt.BPTT_CASES))
def test_bptt_many_tiles_against_fp64_oracle(dev, name):
    """n = 16 max(300 | 40, 2 CUs + 3) + 7 | 3 DISTINCT trajectories: every workgroup of k_bptt_actor (one slab per CU) walks two or
    three tiles.  Transitions, lambda-values, losses and the actor gradient against the oracle as in test_bptt_actor_grad_parity; on
    the (4, 1, E = 5) shape also with the member pre-activations recomputed instead of stored — bit-equal, as in
    test_bptt_zstore_equals_recompute."""
    from test_gpu_bptt import _assert_matches_oracle, _run_hip, _set_zstore
    case = mt.BPTT_CASES[name]
    cus = _cus(dev)
    n = mt.bptt_n(case, cus)
    assert mt.loops_unevenly(n, cus)
    X, U, H = case["X"], case["U"], case["H"]
    s = mt.bptt_inputs(case, n)
    cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, tsys, extra = s
    refs = mt.bptt_oracle(case, s)
    g64, aux64 = refs[2], refs[4]
    res = []
    try:
        for mode in case["zstore"]:
            _set_zstore(mode)
            op = _run_hip(dev, cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, case["system"], extra, n)
            g = op.grads.cpu()
            err = (g.double() - g64).abs() / (mt.BPTT_TOL["atol"] + mt.BPTT_TOL["rtol"] * g64.abs())
            print(f"bptt {name} zstore={mode}: n={n} tiles={mt.tiles_of(n)} worst/tol={float(err.max()):.3f} max|g|={float(g64.abs().max()):.3e}")
            _assert_matches_oracle(op, refs, X, U, H, n)
            rows = op.transitions.cpu().reshape(n, H, -1).double()
            torch.testing.assert_close(rows[..., X + U + 2:], aux64["next_observation"], atol=2e-4, rtol=2e-4)
            torch.testing.assert_close(op.lambda_values.cpu().reshape(n, H).double(), aux64["lambda_values"], atol=5e-4, rtol=5e-4)
            res.append((op.grads.clone(), op.metrics.clone(), op.transitions.clone(), op.lambda_values.clone()))
    finally:
        _set_zstore(-1)
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert torch.equal(a, b)


# --------------------------------------------------------------------------------------------------------- ensemble forward
def test_ensemble_forward_many_tiles_generic_and_lean(dev):
    """mbpo_ensemble_mlp_forward at 16 (2 x 8 CUs + 3) + 5 rows: the generic k_ensemble_forward (grid 8 x CUs: two or three tiles per
    workgroup) and k_ens_fwd_lean (2 CUs / E workgroups per member, pairs of tiles) against float64.  The two against each other at
    summation-order tolerance (the module's float32 figure, atol 2e-5 + rtol 2e-5), NOT bit for bit: k_ens_fwd_lean forms the first layer
    as plain FMAs from a register-held weight column (thin_col_request, ens_lean.hip) where the generic kernel runs every layer
    through the MFMA chain (wave_mlp.hpp), so a row's k-sums are not formed by the same arithmetic."""
    from mbpo import ops
    cus = _cus(dev)
    N = mt.ens_n(cus)
    assert mt.loops_unevenly(N, mt.ens_caps(cus)["generic"])
    params, x = mt.ens_inputs(N)
    y64 = mt.ens_oracle(params, x, torch.float64)
    spec = ops.MlpSpec(mt.ENS_CASE["dims"], mt.ENS_CASE["act"], mt.ENS_CASE["E"])
    set_lean = _debug_setter("mbpo_debug_set_ens_lean")
    ys = {}
    try:
        for lean in (0, 1):
            assert set_lean(lean) == 0
            ys[lean] = ops.ensemble_mlp_forward(params.to(dev), spec, x.to(dev)).cpu()
            torch.cuda.synchronize()
    finally:
        set_lean(-1)
    for lean, y in ys.items():
        assert y.shape == y64.shape
        torch.testing.assert_close(y.double(), y64, msg=lambda m: f"ens_lean={lean}: {m}", **mt.ENS_TOL)
    torch.testing.assert_close(ys[0], ys[1], atol=2e-5, rtol=2e-5)
