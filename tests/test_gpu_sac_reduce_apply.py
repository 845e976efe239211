"""GPU: the optimizer launch of the two-launch SAC step (csrc/sac.hip, k_sac_reduce_apply: slab reduction + unclipped AdamW +
Polyak + undo log in ONE launch) against the three-launch path (k_sac_reduce, k_sac_apply) — BIT FOR BIT, at the edges of that
kernel: the last element (log_alpha) alone in its workgroup, fewer tiles than a load batch, a batch and a tail, the benchmark's
geometry; with the clip check deferred and resolved every step; at a max_grad_norm that never clips and at one that clips some
steps (which is what reads the undo log the kernel writes).

Hidden layers other than 64 / 128 wide run layer by layer and never reach k_sac_reduce_apply, and with 64-wide layers
P + 2 Q = 192 x + 258 u + 322 (mod 64): NP = 1 (mod 256) needs u = 31 (mod 32).  Hence the x = 1, u = 31 case.
"""
import pytest
import torch

from oracle import sac as osac
from test_gpu_sac import _make, _updater

pytestmark = pytest.mark.gpu

STEPS = 6
KEYS = ("params", "adam_m", "adam_v", "target_q", "grads", "metrics", "metrics_accum", "step_count")

#        X, U, policy hidden, critic hidden, B
CASES = {
    "last_element_alone_one_tile": (1, 31, (64, 64), (64, 64), 16),     # NP = 20993 = 82 * 256 + 1
    "three_tiles": (4, 1, (64, 64, 64), (64, 64, 64), 40),
    "thirteen_tiles": (3, 1, (64, 64, 64), (64, 64, 64), 200),          # less than one batch of 16
    "seventeen_tiles": (4, 1, (64, 64, 64), (64, 64, 64), 272),         # a full batch of 16 and a tail of 1
    "benchmark_geometry": (4, 1, (64, 64, 64), (64, 64, 64), 256),
}


def _case(name):
    X, U, ph, qh, B = CASES[name]
    made = _make(X, U, ph, B, 5, True, q_hidden=qh, discounting=0.97, reward_scaling=1.5, lr_policy=1e-3, lr_q=1e-3, lr_alpha=1e-3,
                 wd_q=1e-3)
    return B, made


def _chain(dev, B, made, two_launch, defer, max_norm, steps=STEPS, want_norms=False, poison_step=None):
    """`steps` chained sgd_steps from the same state; returns (updater, state, per-step max group norm of the gradient)."""
    from mbpo import ops
    cfg, st, batch, _, nm, ns = made
    cfg.max_grad_norm = max_norm
    up = _updater(dev, cfg, B, two_launch=two_launch)
    up.load_state(st.params.to(dev), st.target_q.to(dev))
    rng = ops.make_rng(dev, 11)
    norms = []
    for i in range(steps):
        bt = torch.roll(batch, i, 0).to(dev)
        if poison_step == i:
            bt[0, 0] = float("nan")
        up.sgd_step(bt, nm.to(dev), ns.to(dev), seed=3, offset=(7 + i) << 32, rng_dev=rng, defer_clip_check=defer)
        if want_norms:
            g = up.grads
            norms.append(max(float(g[:up.P].norm()), float(g[up.P:up.P + 2 * up.Q].norm()), float(g[-1:].norm())))
    if two_launch:
        # word 0 of the control block counts the speculative steps issued: only k_sac_reduce_apply advances it
        assert int(up._control[0]) == steps, "the two-launch step did not run k_sac_reduce_apply"
    events = up.clip_events()          # (resolves a pending check: finalize)
    up.finalize()
    torch.cuda.synchronize()
    return up, {k: getattr(up, k).detach().clone() for k in KEYS}, events, norms


def _assert_same_bits(a, b, what):
    for k in KEYS:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (what, k)


@pytest.mark.parametrize("name", list(CASES))
def test_two_launch_equals_three_launch_bit_for_bit(dev, name):
    B, made = _case(name)
    up, ref, ev_ref, norms = _chain(dev, B, made, False, False, 1e5, want_norms=True)
    NP = up.P + 2 * up.Q + 1
    if name == "last_element_alone_one_tile":
        assert NP % 256 == 1 and B <= 16, (up.P, up.Q)
    assert ev_ref == 0
    assert float(ref["grads"].abs().sum()) > 0
    med = sorted(norms)[STEPS // 2]
    print(name, "NP", NP, "per-step norms", norms, "threshold", med)
    for max_norm in (1e5, med):
        if max_norm != 1e5:
            _, ref, ev_ref, _ = _chain(dev, B, made, False, False, max_norm)
            print(name, "clip events at the median threshold:", ev_ref)
            assert 0 < ev_ref < STEPS, (ev_ref, norms)
        for defer in (True, False):
            _, two, ev, _ = _chain(dev, B, made, True, defer, max_norm)
            _assert_same_bits(two, ref, (name, max_norm, "deferred" if defer else "resolved every step"))
            assert ev == ev_ref, (name, max_norm, defer, ev, ev_ref)
    assert float(ref["step_count"]) == STEPS


def test_two_launch_step_matches_oracle_with_last_element_alone(dev):
    """One two-launch step where log_alpha sits alone in the launch's last workgroup, against oracle/sac.py GIVEN the device
    gradient — the tolerances of test_gpu_sac.test_sac_gradients_and_step for the state after a step."""
    name = "last_element_alone_one_tile"
    X, U, ph, qh, B = CASES[name]
    cfg, st, batch, noise, nm, ns = _make(X, U, ph, B, 0, True, q_hidden=qh, discounting=0.99, reward_scaling=1.5, lr_policy=3e-4,
                                           lr_q=3e-4, lr_alpha=3e-4, wd_q=1e-3)
    up = _updater(dev, cfg, B, two_launch=True)
    assert (up.P + 2 * up.Q + 1) % 256 == 1
    up.load_state(st.params.to(dev), st.target_q.to(dev))
    up.sgd_step(batch.to(dev), nm.to(dev), ns.to(dev), *[n.to(dev) for n in noise])
    torch.cuda.synchronize()
    assert int(up._control[0]) == 1
    g = up.grads.cpu()
    st_new, met, _ = osac.sgd_step(cfg, st, batch, *noise, nm, ns, grad_override=g)
    assert abs(float(up.metrics[3]) - met["alpha"]) <= 1e-6 * abs(met["alpha"])
    torch.testing.assert_close(up.params.cpu(), st_new.params, atol=1e-7, rtol=1e-6)
    torch.testing.assert_close(up.target_q.cpu(), st_new.target_q, atol=1e-7, rtol=1e-6)
    torch.testing.assert_close(up.adam_m.cpu(), st_new.adam_m, atol=1e-9, rtol=1e-5)
    torch.testing.assert_close(up.adam_v.cpu(), st_new.adam_v, atol=1e-12, rtol=1e-5)
    assert float(up.step_count.cpu()) == 1.0


def test_non_finite_gradient_raises_the_verdict(dev):
    """max_grad_norm = inf makes the quick-check limit overflow to +inf: a NaN gradient must still fail `word < limit` (the kernel
    stores +inf), so that the canonical check runs and the step ends as the three-launch path's does: the same elements are NaN
    and every other element has the same bits (test_gpu_sac.test_mixed_two_and_three_launch_steps_on_one_state's comparison: the
    sign and payload of a NaN that an addition of two NaNs returns follow the operand order hipcc happens to emit)."""
    B, made = _case("benchmark_geometry")
    _, ref, ev_ref, _ = _chain(dev, B, made, False, False, float("inf"), steps=4, poison_step=2)
    _, two, ev, _ = _chain(dev, B, made, True, True, float("inf"), steps=4, poison_step=2)
    assert bool(torch.isnan(ref["params"]).any())
    for k in KEYS:
        a, b = two[k], ref[k]
        assert torch.equal(torch.isnan(a), torch.isnan(b)), k
        assert torch.equal(torch.nan_to_num(a, nan=7.0).view(torch.int32), torch.nan_to_num(b, nan=7.0).view(torch.int32)), k
    assert ev == ev_ref and ev >= 1, (ev, ev_ref)
