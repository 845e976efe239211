"""GPU: k_sac_lean (csrc/sac_lean.hip) against the generic kernel BIT FOR BIT with every operand coming from memory.

The specialised kernel requests its weights ahead of their use and waits for each with a counted s_waitcnt vmcnt(N): the N
requests issued behind the one it needs stay in flight.  A wrong count shows only when a load is slower than the code assumed,
and tests/test_gpu_sac_lean.py runs on parameters, batches and noise that were written a moment earlier and sit in the caches.
Here every launch chain runs behind a pass that overwrites a scratch tensor larger than the last-level cache, so the tile, the
normaliser, the given noise, the weights and the control words all come from HBM.  Shapes: the smallest that reach every load
path — one tile, a ragged last tile, all eight chain waves in layer 0's weight gradient — each with and without the normaliser
(the null-pointer branch changes the request count) and with given and in-kernel noise; and one chain of steps of which some
clip, which runs the kernel's second pass behind the fix-up.
"""
import pytest
import torch

from test_gpu_sac import _make, _updater
from test_gpu_sac_lean import _set_lean, _slab_floats, _state

pytestmark = pytest.mark.gpu

KEYS = ("grads", "metrics", "metrics_accum", "params", "target_q", "adam_m", "adam_v", "step_count")
FLUSH_FLOATS = 96 << 20      # 384 MB: more than the 256 MB last-level cache in front of HBM


@pytest.fixture(autouse=True)
def _restore_default():
    yield
    _set_lean(-1)


@pytest.fixture(scope="module")
def flush(dev):
    scratch = torch.empty(FLUSH_FLOATS, dtype=torch.float32, device=dev)
    count = [0.0]

    def run():
        count[0] += 1.0
        scratch.fill_(count[0])

    yield run
    del scratch


def _run_cold(dev, flush, lean, cfg, st, batches, noise, nm, ns, B, given_noise, defer):
    """One launch chain (a step per batch) on operands that were uploaded BEFORE the flush in front of each step."""
    from mbpo import ops
    _set_lean(1 if lean else 0)
    up = _updater(dev, cfg, B)
    up.load_state(st.params.to(dev), st.target_q.to(dev))
    d = lambda t: None if t is None else t.to(dev)
    bts, nz, nm_d, ns_d = [b.to(dev) for b in batches], [n.to(dev) for n in noise], d(nm), d(ns)
    rng = ops.make_rng(dev, 11)
    for i, bt in enumerate(bts):
        flush()
        if given_noise:
            up.sgd_step(bt, nm_d, ns_d, *nz, defer_clip_check=defer)
        else:
            up.sgd_step(bt, nm_d, ns_d, seed=3, offset=(7 + i) << 32, rng_dev=rng, defer_clip_check=defer)
    up.finalize()
    torch.cuda.synchronize()
    return up, _state(up)


@pytest.mark.parametrize("given_noise", [True, False])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("X,B", [
    (4, 16),      # one tile
    (3, 40),      # ragged: the last tile holds 8 rows
    (6, 32),      # x + 2 = all eight chain waves in layer 0's weight gradient
])
def test_lean_kernel_equals_generic_kernel_on_cold_caches(dev, flush, X, B, normalize, given_noise):
    cfg, st, batch, noise, nm, ns = _make(X, 1, (64, 64, 64), B, 21, normalize, discounting=0.97, reward_scaling=1.5,
                                           lr_policy=3e-4, lr_q=3e-4, lr_alpha=3e-4, wd_q=1e-3)
    up_g, g = _run_cold(dev, flush, False, cfg, st, [batch], noise, nm, ns, B, given_noise, False)
    up_l, l = _run_cold(dev, flush, True, cfg, st, [batch], noise, nm, ns, B, given_noise, False)
    n = _slab_floats(up_g)
    assert torch.equal(g["workspace"][:n], l["workspace"][:n]), "per-tile slabs / loss partials differ"
    assert float(g["grads"].abs().sum()) > 0
    for k in KEYS:
        assert torch.equal(g[k], l[k]), k


def test_lean_kernel_cold_chain_with_clip_fixup(dev, flush):
    """Four chained steps on four different batches, the clip check deferred to the next launch's prologue, at a max_grad_norm
    between the steps' gradient norms: some steps clip, so the specialised kernel runs its second pass (agent-scope log_alpha
    load, scalar-cache invalidation, every request again) on cold caches."""
    X, B, S = 4, 32, 4
    cfg, st, batch, noise, nm, ns = _make(X, 1, (64, 64, 64), S * B, 22, True, discounting=0.95)
    batches = [batch[i * B:(i + 1) * B].contiguous() for i in range(S)]
    noise = [n[:B].contiguous() for n in noise]
    # per-step gradient norms of the unclipped run place the threshold between the second and the third largest
    from mbpo import ops
    _set_lean(1)
    up = _updater(dev, cfg, B)
    up.load_state(st.params.to(dev), st.target_q.to(dev))
    rng = ops.make_rng(dev, 11)
    norms = []
    for i in range(S):
        up.sgd_step(batches[i].to(dev), nm.to(dev), ns.to(dev), seed=3, offset=(7 + i) << 32, rng_dev=rng)
        gr = up.grads
        norms.append(max(float(gr[:up.P].norm()), float(gr[up.P:up.P + 2 * up.Q].norm()), float(gr[-1:].norm())))
    srt = sorted(norms)
    cfg.max_grad_norm = 0.5 * (srt[1] + srt[2])
    up_g, g = _run_cold(dev, flush, False, cfg, st, batches, noise, nm, ns, B, False, True)
    up_l, l = _run_cold(dev, flush, True, cfg, st, batches, noise, nm, ns, B, False, True)
    n = _slab_floats(up_g)
    assert torch.equal(g["workspace"][:n], l["workspace"][:n]), "per-tile slabs / loss partials differ"
    for k in KEYS:
        assert torch.equal(g[k], l[k]), k
    assert up_g.clip_events() == up_l.clip_events()
    assert 0 < up_l.clip_events() < S, (up_l.clip_events(), norms)
