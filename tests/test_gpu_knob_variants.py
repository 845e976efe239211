"""GPU parity of the kernels that only a documented knob value selects (csrc/knobs.hpp): SAC with two workgroups per
tile (MBPO_SAC_SPLIT=0) and with the reverse-mode actor role at u = 1 (MBPO_SAC_JVP=0), PPO's 1024-thread kernel beyond one tile per
CU (MBPO_PPO_SP2=0), the separate values / GAE / moments launches at shapes the default fuses (MBPO_PPO_VALUES_GAE=0), one launch per
layered GEMM (MBPO_LAYERED_GROUP=0) and philox_permutation without the bucket pre-sort (MBPO_PERM_BUCKETS=0).

The knobs are read once per process, so each VALUE gets one child process (never two at a time, never retried, each under a time
limit; the parent asserts its exit status before the next one starts) that runs two or three shapes and saves gradients, parameters
and metrics.  The parent compares every result with the float64 oracle at the owning module's tolerance (tests/test_gpu_sac.py,
tests/test_gpu_ppo.py; the layered shapes with those modules' layered tolerance) and with the default dispatch on the same inputs at
summation-order tolerance (gradients atol 1e-6 (1 + max|g|) + rtol 1e-4, loss terms atol 1e-6 + rtol 2e-5: those of
test_sac_layered_gemm_tile_variants_agree).  The optimizer step is checked GIVEN the device gradient, as everywhere else.

MBPO_SAC_SPLIT=1 on WIDE networks (x + u or 2u above 16: k_sac_fwd_bwd<64,4,true> on a three-workgroups-per-tile grid) is not launched
here.  From the code it is defined: the kernel takes its role from the run-time A.split, not from a template parameter (sac.hip,
top of k_sac_fwd_bwd), sac_chain_table fills rows 0..2 of the chain table for every kernel, leaving chain slots 2 and 3 idle under
`split`, and tile = blockIdx.x / 3 stays below n_tiles.  The wide kernels keep two workgroups per tile by default because that
measured faster, not because three are unsupported.
"""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import many_tiles_cases as mt

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT_S = 600

_SAC_64 = dict(X=4, U=1, hidden=(64, 64, 64), B=200, normalize=True)
_SAC_U2 = dict(X=4, U=2, hidden=(64, 64, 64), B=200, normalize=False)
_SAC_128 = dict(X=3, U=1, hidden=(128, 128, 128), B=104, normalize=True)
_SAC_ACT = dict(case="sac_thin_rt")      # tests/activation_cases.py: 64 x 3, u = 1, B = 40, policy relu / critics tanh, clear of relu's kink
_SAC_LAYERED = dict(X=4, U=2, hidden=(48, 80), q_hidden=(200, 72, 40), B=100, normalize=True)
_PPO_LAYERED = dict(X=4, U=2, hidden=(48, 80), v_hidden=(200, 72, 40), B=20, T=7, normalize=True, norm_adv=False)
_PPO_REF = dict(X=3, U=1, hidden=(64, 64), B=128, T=40, normalize=True, norm_adv=True)       # the reference's test shape

JOBS = {
    "MBPO_SAC_SPLIT=0": [("sac", _SAC_64), ("sac", _SAC_U2), ("sac", _SAC_128), ("sac", _SAC_ACT)],      # k_sac_fwd_bwd<64,4,false> and <128,2,false>
    "MBPO_SAC_JVP=0": [("sac", _SAC_64), ("sac", _SAC_128), ("sac", _SAC_ACT)],       # reverse-mode dQ/da in the actor role at u = 1
    "MBPO_PPO_SP2=0": [("ppo", dict(name="sp2_neq"))],                                # <64,4,false> with more than two tiles per CU
    "MBPO_PPO_VALUES_GAE=0": [("ppo", _PPO_REF), ("ppo", dict(name="h128_u2"))],      # k_ppo_values<64> / <128> + GAE scan + moments
    "MBPO_LAYERED_GROUP=0": [("sac", _SAC_LAYERED), ("ppo", _PPO_LAYERED)],
    "MBPO_PERM_BUCKETS=0": [("perm", dict(n=16384, seed=11, offset=1 << 33))],
}


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _sac_inputs(item):
    if "case" in item:
        import activation_cases as ac
        return ac.inputs(item["case"])
    from test_gpu_sac import _make
    return _make(item["X"], item["U"], item["hidden"], item["B"], 6, item["normalize"], q_hidden=item.get("q_hidden"), **mt.SAC_CFG)


def _ppo_inputs(item, cus):
    if "name" in item:
        case = mt.PPO_CASES[item["name"]]
        return case, mt.ppo_inputs(case, cus)
    from test_gpu_ppo import _make
    case = dict(item, neq=False)
    return case, _make(item["X"], item["U"], item["hidden"], item["B"], item["T"], 6, item["normalize"], v_hidden=item.get("v_hidden"),
                       normalize_advantage=item["norm_adv"], **mt.PPO_CFG)


def _run_item(dev, kind, item):
    """One shape through whatever kernels this process's knobs select: CPU tensors of what the step left."""
    d = lambda t: None if t is None else t.to(dev)
    if kind == "sac":
        from test_gpu_sac import _updater
        cfg, st, batch, noise, nm, ns = _sac_inputs(item)
        up = _updater(dev, cfg, batch.shape[0], policy_activation=cfg.policy_act, q_activation=cfg.q_act)
        up.load_state(st.params.to(dev), st.target_q.to(dev))
        up.sgd_step(batch.to(dev), d(nm), d(ns), *[n.to(dev) for n in noise])
        up.finalize()
        torch.cuda.synchronize()
        return {k: getattr(up, k).cpu().clone() for k in ("grads", "params", "target_q", "adam_m", "adam_v", "metrics")}
    if kind == "ppo":
        from test_gpu_ppo import _updater
        from test_gpu_ppo_brax_env import NEQ_KW
        case, (cfg, st, data, noise, nm, ns) = _ppo_inputs(item, _cus(dev))
        up = _updater(dev, cfg, data.shape[0], data.shape[1], **(NEQ_KW if case["neq"] else {}))
        up.load_state(st.params.to(dev))
        up.minibatch_step(data.to(dev), d(nm), d(ns), noise.to(dev))
        torch.cuda.synchronize()
        return {k: getattr(up, k).cpu().clone() for k in ("grads", "params", "adam_m", "adam_v", "metrics")}
    from mbpo import ops
    return {"perm": ops.philox_permutation(item["n"], seed=item["seed"], offset=item["offset"]).cpu().clone()}


def _child_main(job, out_path):
    dev = torch.device("cuda", 0)
    torch.save([_run_item(dev, kind, item) for kind, item in JOBS[job]], out_path)


_CHILD = '''
import sys
sys.path.insert(0, "."); sys.path.insert(0, "model-based-policy-optimizers_amd"); sys.path.insert(0, "tests")
import test_gpu_knob_variants as T
T._child_main(sys.argv[1], sys.argv[2])
'''


def _close_to_default(got, dflt, what):
    scale = float(dflt["grads"].abs().max())
    torch.testing.assert_close(got["grads"], dflt["grads"], atol=1e-6 + 1e-6 * scale, rtol=1e-4, msg=lambda m: f"{what} vs default dispatch: {m}")
    torch.testing.assert_close(got["metrics"], dflt["metrics"], atol=1e-6, rtol=2e-5, msg=lambda m: f"{what} metrics vs default: {m}")


def _check_sac(item, got, dflt, what):
    from oracle import sac as osac
    inputs = _sac_inputs(item)
    cfg, st, batch, noise, nm, ns = inputs
    g64, (cl64, ac64, al64) = mt.sac_oracle(inputs, torch.float64)
    g = got["grads"]
    layered = "q_hidden" in item
    P, Q = cfg.P, cfg.Q
    for name, sl in (("policy", slice(0, P)), ("critic", slice(P, P + 2 * Q)), ("alpha", slice(P + 2 * Q, None))):
        if layered:        # test_sac_layered_path_any_widths
            tol = dict(atol=2e-6 + 2e-6 * float(g64[sl].abs().max()), rtol=2e-4)
        else:
            tol = mt.SAC_TOL
        torch.testing.assert_close(g[sl].double(), g64[sl], msg=lambda m: f"{what} {name} grad vs fp64 oracle: {m}", **tol)
    np.testing.assert_allclose(got["metrics"].tolist()[:3], [cl64, ac64, al64], rtol=5e-5 if layered else 2e-5, atol=2e-6)
    st_new, met, _ = osac.sgd_step(cfg, st, batch, *noise, nm, ns, grad_override=g)
    np.testing.assert_allclose(got["metrics"].tolist()[3], met["alpha"], rtol=1e-6)
    torch.testing.assert_close(got["params"], st_new.params, atol=1e-7, rtol=1e-6)
    torch.testing.assert_close(got["target_q"], st_new.target_q, atol=1e-7, rtol=1e-6)
    torch.testing.assert_close(got["adam_m"], st_new.adam_m, atol=1e-9, rtol=1e-5)
    torch.testing.assert_close(got["adam_v"], st_new.adam_v, atol=1e-12, rtol=1e-5)
    _close_to_default(got, dflt, what)


def _check_ppo(item, cus, got, dflt, what):
    from oracle import ppo as oppo
    case, inputs = _ppo_inputs(item, cus)
    cfg, st, data, noise, nm, ns = inputs
    g64, terms64 = mt.ppo_oracle(case, inputs, torch.float64)
    g = got["grads"]
    layered = "v_hidden" in item
    if layered:            # test_ppo_layered_path_any_widths
        tol = dict(atol=2e-6 + 2e-6 * float(g64.abs().max()), rtol=5e-4)
    else:
        tol = mt.ppo_tol(case)
    torch.testing.assert_close(g.double(), g64, msg=lambda m: f"{what} grad vs fp64 oracle: {m}", **tol)
    np.testing.assert_allclose(got["metrics"].tolist(), [terms64[k] for k in ("total_loss", "policy_loss", "v_loss", "entropy_loss")],
                               rtol=5e-5 if layered else 2e-5, atol=1e-5)
    st_new, _, _ = oppo.minibatch_step(cfg, st, data, noise, nm, ns, grad_override=g)
    torch.testing.assert_close(got["params"], st_new.params, atol=1e-7, rtol=1e-6)
    torch.testing.assert_close(got["adam_m"], st_new.adam_m, atol=1e-9, rtol=1e-5)
    torch.testing.assert_close(got["adam_v"], st_new.adam_v, atol=1e-12, rtol=1e-5)
    _close_to_default(got, dflt, what)


@pytest.mark.parametrize("job", list(JOBS))
def test_knob_value_against_oracle_and_default_dispatch(dev, tmp_path, job):
    name, value = job.split("=")
    assert os.environ.get(name) is None, f"{name} is set in this process: its default dispatch is not the default"
    out = tmp_path / "child.pt"
    r = subprocess.run([sys.executable, "-c", _CHILD, job, str(out)], env=dict(os.environ, **{name: value}), capture_output=True, text=True,
                       cwd=str(Path(__file__).resolve().parents[1]), timeout=CHILD_TIMEOUT_S)
    assert r.returncode == 0, r.stderr[-2000:]
    results = torch.load(out, weights_only=True)
    assert len(results) == len(JOBS[job])
    cus = _cus(dev)
    for (kind, item), got in zip(JOBS[job], results):
        what = f"{job} {kind} {item}"
        if kind == "perm":
            from oracle import philox
            ref = philox.philox_permutation(item["seed"], item["offset"], item["n"])
            assert np.array_equal(got["perm"].numpy(), ref), what
            assert torch.equal(got["perm"], _run_item(dev, kind, item)["perm"]), what
            continue
        dflt = _run_item(dev, kind, item)
        if kind == "sac":
            _check_sac(item, got, dflt, what)
        else:
            _check_ppo(item, cus, got, dflt, what)

