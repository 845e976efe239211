"""GPU parity for the arms of PPO's host dispatch (csrc/ppo.hip ppo_variant) that no other case of the suite takes, against the
float64 oracle (oracle/ppo.py), checked the way test_gpu_ppo.py::test_ppo_gradients_and_step checks and to its tolerances:

  values SEPARATE + moments TWO_PASS   T = 1024: the values + GAE launch does not fit its LDS arrays (5 * 1025 > 5120 floats), so
                                       k_ppo_values, the GAE scan and the moments run as separate launches; M = 66 560 > 65 536
                                       (PPO_MOM_FUSED_MAX), so the moments take k_moments_partial / k_moments_final
  values SEPARATE + moments FUSED      the same with B = 8 (M = 8192): k_moments_fused after the same fallback
  values VG with NC = 2 and NC = 4     u = 2 (no k_ppo_vg_lean), one trajectory per workgroup of T + 1 = 21 and 51 rows: two and four
                                       value chains, k_ppo_values_gae<64, 2> and <64, 4> (the suite has NC = 1 and 3)

The float32 oracle's own gap to float64 at these shapes, as a fraction of the module's gradient tolerance (atol 2e-6 + rtol 2e-4),
measured on the CPU: 0.006 (two-pass), 0.008 (fused), 0.070 (NC = 2), 0.047 (NC = 4) — all below a quarter, so the tolerance stays.

The two-pass case draws its inputs with seed 1, not the module's usual 0.  The clipped surrogate is discontinuous in a sample's
gradient where the probability ratio crosses 1 +- clipping_epsilon, and with 66 560 samples some ratio lies within a few float32
roundings of a boundary for most seeds: with seed 0 the nearest is 3.0e-6 (relative) away, the float32 and float64 ORACLES put it on
different sides, and their gradients differ by that one sample's whole contribution (3.3e-5 on an element of 1.3e-2, 7.3 x the
tolerance).  That is a property of the data, not an error of either: of the seeds 0 .. 7 the case takes the one whose nearest ratio
is farthest from a boundary (seed 1: 1.7e-5, against 5e-6 for the summed error bounds of csrc/fast_math.hpp's helpers in the
log-probability), where the two oracles agree to 0.006 of the tolerance.
"""
import numpy as np
import pytest
import torch

from oracle import ppo as oppo
from test_gpu_ppo import _make, _updater

pytestmark = pytest.mark.gpu

CFG = dict(entropy_cost=1e-2, discounting=0.99, reward_scaling=0.5, gae_lambda=0.95, clipping_epsilon=0.3, normalize_advantage=True,
           lr=3e-4, wd=1e-5)


def _check(dev, X, U, B, T, seed):
    cfg, st, data, noise, nm, ns = _make(X, U, (64, 64), B, T, seed, True, **CFG)
    g_ref, _, _, _ = oppo.grads(cfg, st.params, data, noise, nm, ns)
    g_ref64, terms64, _, _ = oppo.grads(cfg, st.params.double(), data.double(), noise.double(), nm.double(), ns.double())
    up = _updater(dev, cfg, B, T)
    up.load_state(st.params.to(dev))
    up.minibatch_step(data.to(dev), nm.to(dev), ns.to(dev), noise.to(dev))
    torch.cuda.synchronize()
    g = up.grads.cpu()
    torch.testing.assert_close(g, g_ref, atol=2e-6, rtol=5e-4)
    torch.testing.assert_close(g.double(), g_ref64, atol=2e-6, rtol=2e-4)
    np.testing.assert_allclose(up.metrics.cpu().tolist(),
                               [terms64["total_loss"], terms64["policy_loss"], terms64["v_loss"], terms64["entropy_loss"]],
                               rtol=2e-5, atol=1e-5)
    st_new, _, _ = oppo.minibatch_step(cfg, st, data, noise, nm, ns, grad_override=g)
    torch.testing.assert_close(up.params.cpu(), st_new.params, atol=1e-7, rtol=1e-6)
    torch.testing.assert_close(up.adam_m.cpu(), st_new.adam_m, atol=1e-9, rtol=1e-5)
    torch.testing.assert_close(up.adam_v.cpu(), st_new.adam_v, atol=1e-12, rtol=1e-5)
    assert float(up.step_count.cpu()) == 1.0


def test_ppo_long_trajectory_two_pass_moments(dev):
    _check(dev, 3, 1, 65, 1024, seed=1)


def test_ppo_long_trajectory_fused_moments(dev):
    _check(dev, 3, 1, 8, 1024, seed=0)


@pytest.mark.parametrize("T", [20, 50])
def test_ppo_values_gae_chain_counts(dev, T):
    _check(dev, 4, 2, 5, T, seed=0)
