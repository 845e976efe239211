"""CPU checks of the brax-env PPO restatement (tests/ppo_brax_env_ref.py) and of the C-ABI fields that select it."""
import ctypes as C

import numpy as np
import pytest
import torch

import ppo_brax_env_ref as ref
from oracle import ppo as oppo


def _data(X, U, B, T, seed):
    g = torch.Generator().manual_seed(seed)
    cfg = oppo.PpoConfig(x_dim=X, u_dim=U, policy_dims=[X, 32, 32, 2 * U], value_dims=[X, 32, 1], entropy_cost=1e-2, discounting=1.0,
                         reward_scaling=0.5, gae_lambda=0.95)
    st = oppo.init_state(cfg, g, torch.float64)
    D = 2 * X + 2 * U + 4
    data = torch.randn(B, T, D, generator=g, dtype=torch.float64)
    o = X + U
    data[..., X:o] = torch.tanh(data[..., o + 3 + X:o + 3 + X + U])
    data[..., o + 1] = (torch.rand(B, T, generator=g) > 0.1).double()
    data[..., D - 1] = (torch.rand(B, T, generator=g) < 0.15).double()
    noise = torch.randn(B, T, U, generator=g, dtype=torch.float64)
    return cfg, st, data, noise


@pytest.mark.parametrize("norm_adv", [True, False])
def test_zero_continuous_discounting_is_the_plain_loss_at_discount_one(norm_adv):
    """exp(-0 * t) = 1 for every sample: the restated loss equals oracle.ppo.loss at discounting = 1."""
    cfg, st, data, noise = _data(3, 2, 6, 9, 0)
    cfg.normalize_advantage = norm_adv
    neq = ref.Neq(0.0, 0.0, 1.0, 0.1)
    g_ref, terms_ref, vs_ref, _ = oppo.grads(cfg, st.params, data, noise)
    g, terms, vs, _ = ref.grads(cfg, st.params, data, noise, neq=neq)
    torch.testing.assert_close(g, g_ref, atol=1e-12, rtol=1e-10)
    torch.testing.assert_close(vs, vs_ref, atol=1e-12, rtol=1e-10)
    for k in terms_ref:
        assert abs(terms[k] - terms_ref[k]) <= 1e-12 * max(1.0, abs(terms_ref[k])), k


def test_per_sample_discount_changes_the_loss_and_matches_a_hand_value():
    # t = (1 - 0)/2 * a + 1/2 -> a = -0.9: t = 0.05 -> floor to 0.0; a = 0.5: t = 0.75 -> 0.7; a = -1.3: t = -0.15 -> -0.2
    neq = ref.Neq(0.5, 0.0, 1.0, 0.1)
    d = ref.per_sample_discount(np.array([-0.9, 0.5, -1.3]), neq, np.float64)
    np.testing.assert_allclose(d, np.exp(-0.5 * np.array([0.0, 0.7, -0.2])), rtol=1e-12)
    cfg, st, data, noise = _data(3, 1, 4, 7, 1)
    _, terms_plain, _, _ = ref.grads(cfg, st.params, data, noise)
    _, terms_neq, _, _ = ref.grads(cfg, st.params, data, noise, neq=neq)
    assert terms_plain["v_loss"] != terms_neq["v_loss"]


def test_clip_by_global_norm_both_sides_of_the_threshold():
    g = torch.tensor([3.0, 4.0], dtype=torch.float64)            # ||g|| = 5
    assert torch.equal(ref.clip_by_global_norm(g, None), g)
    assert torch.equal(ref.clip_by_global_norm(g, 10.0), g)
    torch.testing.assert_close(ref.clip_by_global_norm(g, 1.0), torch.tensor([0.6, 0.8], dtype=torch.float64), atol=1e-15, rtol=0)
    torch.testing.assert_close(ref.clip_by_global_norm(g, 2.5), torch.tensor([1.5, 2.0], dtype=torch.float64), atol=1e-15, rtol=0)
    # at the threshold optax takes the scaled branch: (g / 5) * 5
    torch.testing.assert_close(ref.clip_by_global_norm(g, 5.0), g, atol=1e-15, rtol=0)
    # the clipped step: AdamW's moments see the clipped gradient
    cfg, st, data, noise = _data(3, 1, 2, 3, 2)
    g_big = torch.full_like(st.params, 10.0)
    new, _, _ = ref.minibatch_step(cfg, st, data, noise, max_grad_norm=1.0, grad_override=g_big)
    n = float(g_big.norm())
    torch.testing.assert_close(new.adam_m, 0.1 * g_big / n, atol=1e-15, rtol=1e-12)
    new, _, _ = ref.minibatch_step(cfg, st, data, noise, max_grad_norm=2 * n, grad_override=g_big)
    torch.testing.assert_close(new.adam_m, 0.1 * g_big, atol=1e-15, rtol=1e-12)


def _ppo_desc(B=512, T=40):
    from mbpo import _hip
    p = _hip.PpoDesc()
    p.x_dim, p.u_dim, p.batch_size, p.unroll_length, p.row_len = 3, 1, B, T, 12
    p.policy_layers, p.value_layers = 3, 3
    for i, v in enumerate([3, 64, 64, 2]):
        p.policy_dims[i] = v
    for i, v in enumerate([3, 64, 64, 1]):
        p.value_dims[i] = v
    return p


def test_c_abi_options_validation_and_workspace():
    """A zero-filled tail is the ppo.py variant; non_equidistant_time without env_dt > 0 is MBPO_ERR_ARG; the options take workspace
    only when on (the per-sample discount array: M floats; the clip norm partials: one per 64 parameters)."""
    from mbpo import _hip
    lib = _hip.load()
    p = _ppo_desc()
    base = lib.mbpo_ppo_workspace_floats(C.byref(p))
    assert base > 0
    p.non_equidistant_time = 1
    assert lib.mbpo_ppo_workspace_floats(C.byref(p)) == -1   # MBPO_ERR_ARG
    assert b"env_dt" in lib.mbpo_last_error()
    p.env_dt = 0.05
    assert lib.mbpo_ppo_workspace_floats(C.byref(p)) == base + 512 * 40
    p.non_equidistant_time, p.env_dt = 0, 0.0
    p.max_grad_norm = 0.5
    npv = (3 * 64 + 64 + 64 * 64 + 64 + 64 * 2 + 2) + (3 * 64 + 64 + 64 * 64 + 64 + 64 + 1)
    assert lib.mbpo_ppo_workspace_floats(C.byref(p)) == base + (((npv + 63) // 64 + 3) & ~3)
    p.max_grad_norm = -1.0                                         # <= 0: no clip
    assert lib.mbpo_ppo_workspace_floats(C.byref(p)) == base


def test_python_validation_without_a_device():
    from mbpo import ops
    kw = dict(x_dim=3, u_dim=1, policy_dims=[3, 64, 64, 2], value_dims=[3, 64, 64, 1], batch_size=8, unroll_length=4, device="cpu")
    with pytest.raises(ValueError, match="env_dt"):
        ops.PpoUpdater(**kw, non_equidistant_time=True, env_dt=0.0)
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError, match="max_grad_norm"):
            ops.PpoUpdater(**kw, max_grad_norm=bad)
