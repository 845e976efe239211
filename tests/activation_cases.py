"""Cases that run the fused kernels under relu and tanh, shared by tests/test_cpu_activation_cases.py (host only) and
tests/test_gpu_activations.py: a table of cases, inputs(name), and an lru_cached oracle(name, dtype).

Every kernel takes its activation from MlpDev.act (csrc/common.hpp act_apply_vec / act_grad_mul_vec / act_grad, the epilogues of
csrc/wave_mlp.hpp and csrc/chain_run.hpp, csrc/layered.hip); the lean kernels refuse anything but swish and the dispatch falls back to
the generic ones.  Where several networks meet in one launch a case gives each its own activation, so a kernel that applied one
network's `act` to another could not pass.  Inputs come from the owning modules' helpers (test_gpu_sac._make, test_gpu_ppo._make,
test_gpu_bptt._setup, test_gpu_ens_model_selection._case_data) at the smallest shapes that reach each kernel variant with at least two
16-row tiles, the last one ragged.

The relu kink.  relu' jumps at 0, so a unit whose pre-activation changes sign between two correct fp32 evaluations moves a gradient by
O(1).  Nothing is left out of a comparison; the INPUTS are chosen so that the reference is clear of the kink.  For every case that
differentiates a relu network the fp32 and the fp64 oracle run under oracle.nets.tap; with G = max |z32 - z64| over every tapped
pre-activation, the case's seed is the first in 0..63 at which every relu pre-activation has |z64| >= 10 G and the two runs agree on
every sign.  KINK records (seed, G, min |z64| over the relu units); test_cpu_activation_cases.py re-derives all three.

Tolerances are the owning modules' (named in TOL below), not figures of the code under test.
"""
from __future__ import annotations

import functools

import torch

from oracle import bptt as obptt
from oracle import ensemble as oens
from oracle import nets as onets

import many_tiles_cases as mt

KINK_FACTOR = 10.0
SEEDS = range(64)

# ------------------------------------------------------------------------------------------------------------------ the table
# Dispatch notes.  No host query names the kernel variant, so each case rests on these lines of the host code (REF_CUS = 256):
#   SAC   csrc/sac.hip:1044 (sac_plan) sends a shape to the layered path by its widths alone (Hp == Hq in {64, 128} stays fused), so
#         these run k_sac_fwd_bwd.  sac_variant: :1226 wide_any = a net with more than 16 inputs or outputs; :1227 split = !wide_any;
#         :1231 jvp = (u == 1) on the register path; :1234 thin = MBPO_SAC_THIN && split && jvp && H == 64 with <= 8 inputs; :1237 lean
#         needs thin and swish.  sac_fwd_bwd_launch: :967 wide -> <64,4,true>; :968 split && thin -> <64,4,false,2,true>; :969 split ->
#         <64,4,false,2>; :972 H = 128, split -> <128,4,false,2> (<128,2,false> at :974 is the MBPO_SAC_SPLIT=0 kernel).
#   PPO   csrc/ppo.hip ppo_variant: :757-759 layered by widths; :764-768 lean / vg_lean need swish (ppo_lean_supports,
#         ppo_vg_lean_supports); :762, :769 sp2 = H 64, narrow ends, tiles > CUs, not lean; :770 wide = H 64 with a wide end; :777, :781
#         values + GAE fused while a trajectory fits (T <= 1023), else the separate values / GAE scan / moments launches.  The loss
#         launch: :1011 wide -> <64,4,true>; :1012 -> <64,4,false>; :1013 sp2 -> <64,2,false>; :1014 -> <128,2,false>.
_SAC = dict(family="sac", normalize=True)
_PPO = dict(family="ppo", normalize=True, v_hidden=None)
_BPTT = dict(family="bptt", E=2, hidden=(64, 64))
CASES = {
    # ---- SAC fused: acts = (policy, q)
    "sac_thin_rt": dict(_SAC, X=4, U=1, hidden=(64, 64, 64), B=40, acts=("relu", "tanh")),      # <64,4,false,2,true>: JVP + thin
    "sac_thin_tr": dict(_SAC, X=4, U=1, hidden=(64, 64, 64), B=40, acts=("tanh", "relu")),      #   (MBPO_SAC_THIN=0: <64,4,false,2>)
    "sac_u2_rt": dict(_SAC, X=4, U=2, hidden=(64, 64), B=40, acts=("relu", "tanh")),            # <64,4,false,2>: reverse-mode actor
    "sac_u2_tr": dict(_SAC, X=4, U=2, hidden=(64, 64), B=40, acts=("tanh", "relu")),
    "sac_wide_rt": dict(_SAC, X=17, U=6, hidden=(64, 64, 64), B=24, acts=("relu", "tanh")),     # <64,4,true>
    "sac_wide_tr": dict(_SAC, X=17, U=6, hidden=(64, 64, 64), B=24, acts=("tanh", "relu")),
    "sac_128_rt": dict(_SAC, X=3, U=1, hidden=(128, 128, 128), B=24, acts=("relu", "tanh")),    # <128,4,false,2>
    "sac_128_tr": dict(_SAC, X=3, U=1, hidden=(128, 128, 128), B=24, acts=("tanh", "relu")),
    # ---- PPO: acts = (policy, value)
    "ppo_64_rt": dict(_PPO, X=3, U=1, hidden=(64, 64), B=8, T=5, acts=("relu", "tanh")),        # k_ppo_values_gae<64> + k_ppo_fwd_bwd<64,4,false>
    "ppo_64_tr": dict(_PPO, X=3, U=1, hidden=(64, 64), B=8, T=5, acts=("tanh", "relu")),
    "ppo_128_rt": dict(_PPO, X=4, U=2, hidden=(128, 128), B=6, T=7, acts=("relu", "tanh")),     # k_ppo_fwd_bwd<128,2,false>
    "ppo_128_tr": dict(_PPO, X=4, U=2, hidden=(128, 128), B=6, T=7, acts=("tanh", "relu")),
    "ppo_wide_rt": dict(_PPO, X=17, U=6, hidden=(64, 64), B=8, T=3, acts=("relu", "tanh"), normalize=False),      # <64,4,true>
    "ppo_wide_tr": dict(_PPO, X=17, U=6, hidden=(64, 64), B=8, T=3, acts=("tanh", "relu"), normalize=False),
    # the layered shape of test_ppo_layered_path_any_widths row 2 (csrc/ppo_layered.hip)
    "ppo_layered_rt": dict(_PPO, X=4, U=2, hidden=(48, 80), v_hidden=(200, 72, 40), B=20, T=7, acts=("relu", "tanh"), norm_adv=False),
    "ppo_layered_tr": dict(_PPO, X=4, U=2, hidden=(48, 80), v_hidden=(200, 72, 40), B=20, T=7, acts=("tanh", "relu"), norm_adv=False),
    # one step past what a workgroup's LDS arrays hold: values, GAE scan and moments as separate launches (k_ppo_values<64>)
    "ppo_t1030_rt": dict(_PPO, X=3, U=1, hidden=(64, 64), B=1, T=1030, acts=("relu", "tanh"), normalize=False),
    # more tiles than CUs at H = 64 with narrow ends: the two-per-CU k_ppo_fwd_bwd<64,2,false>.  B comes from the CU count of the device
    # the test runs on (ppo_sp2_shape; the B below is REF_CUS's, what the host tests use).  524 544 relu units of independent draws never
    # clear the kink (min |z| 7e-9 at seed 0, none of 64 seeds), and the row count cannot shrink, so the minibatch repeats `base` = 7
    # independent trajectories: the CUs + 1 tiles hold only 21 DISTINCT rows, cut differently by every 16-row tile.  The kink condition
    # therefore does not depend on B.
    "ppo_sp2_rt": dict(_PPO, X=3, U=1, hidden=(64, 64), B=(16 * mt.REF_CUS) // 3 + 1, T=3, base=7, acts=("relu", "tanh")),
    # ---- BPTT: acts = (actor, critics, members); the z store and recompute both run on bptt_x4_a
    "bptt_x4_a": dict(_BPTT, X=4, U=1, H=4, n=17, acts=("relu", "tanh", "swish")),
    "bptt_x4_b": dict(_BPTT, X=4, U=1, H=4, n=17, acts=("tanh", "swish", "relu")),
    "bptt_wide": dict(_BPTT, X=17, U=6, H=3, n=16, acts=("swish", "relu", "tanh")),
    # 'ts1' with sampled model noise (test_gpu_bptt_stochastic's system): a member per row and step, explicit member_idx / model_noise
    "bptt_ts1_noise": dict(_BPTT, family="bptt_ts", X=4, U=1, H=4, n=17, acts=("relu", "swish", "tanh")),
    # ---- CriticGrad (k_critic_fwd_bwd): one activation
    "critic_x4_relu": dict(family="critic", X=4, batch=40, hidden=(64, 64), acts=("relu",)),
    "critic_x4_tanh": dict(family="critic", X=4, batch=40, hidden=(64, 64), acts=("tanh",)),
    "critic_x17_relu": dict(family="critic", X=17, batch=40, hidden=(64, 64), acts=("relu",)),
    # ---- HipMlp: forward in mbpo_ensemble_mlp_forward, backward in k_mlp_vjp (fused) / mbpo_mlp_layered_vjp
    "mlp_fused_relu": dict(family="mlp", dims=[3, 64, 64, 2], n=40, acts=("relu",)),
    "mlp_fused_tanh": dict(family="mlp", dims=[3, 64, 64, 2], n=40, acts=("tanh",)),
    "mlp_layered_relu": dict(family="mlp", dims=[3, 128, 128, 2], n=40, acts=("relu",)),
    "mlp_layered_tanh": dict(family="mlp", dims=[3, 128, 128, 2], n=40, acts=("tanh",)),
    # ---- EnsembleNllGrad: k_ens_nll_fwd_bwd (64-wide) and its layered form
    "nll_x4_relu": dict(family="nll", X=4, U=1, E=2, B=40, hidden=(64, 64), acts=("relu",)),
    "nll_x4_tanh": dict(family="nll", X=4, U=1, E=2, B=40, hidden=(64, 64), acts=("tanh",)),
    "nll_x17_relu": dict(family="nll", X=17, U=6, E=2, B=40, hidden=(64, 64), acts=("relu",)),
    "nll_layered_tanh": dict(family="nll", X=4, U=1, E=2, B=40, hidden=(200, 200), acts=("tanh",)),
}
FORWARD_CASES = {
    # mbpo_ensemble_mlp_forward, k_ensemble_forward<64>: k_ens_fwd_lean takes this very shape under swish only
    "ensfwd_relu": dict(family="ensfwd", dims=[5, 64, 64, 64, 8], E=3, N=37, acts=("relu",)),
    "ensfwd_tanh": dict(family="ensfwd", dims=[5, 64, 64, 64, 8], E=3, N=37, acts=("tanh",)),
    "policy_act_relu": dict(family="policy_act", dims=[4, 64, 64, 2], N=37, acts=("relu",)),
    "ens_eval_relu": dict(family="ens_eval", X=4, U=1, E=3, n=70, hidden=(64, 64, 64), acts=("relu",)),      # k_ens_eval
    # terminal values, kind Q: a policy narrower (and wider) than the critics, each with its own activation; acts = (policy, critics)
    "tv_q_narrow_policy": dict(family="tv", X=4, A=1, policy_hidden=(64, 64), critic_hidden=(256, 256), acts=("relu", "tanh")),
    "tv_q_wide_policy": dict(family="tv", X=3, A=2, policy_hidden=(128, 128, 128), critic_hidden=(64, 64, 64), acts=("swish", "relu")),
}
ALL = {**CASES, **FORWARD_CASES}

# Rollouts (forward only) go through test_gpu_rollout._run_rollout_case, which builds the inputs, both oracles and the device run:
# N = 40 (three tiles, the last one ragged), S = 3, episode_length 2, a fifth of the envs entering done.
_RO = dict(N=40, S=3, L=2, AR=1, U=1, system="ensemble", E=3, check64=True)
ROLLOUT_CASES = {
    "ro64_relu_tanh_ts1_noise": dict(_RO, X=4, policy_act="relu", member_act="tanh", mode="ts1", sample_noise=True),   # k_model_rollout64
    "ro64_tanh_relu": dict(_RO, X=4, policy_act="tanh", member_act="relu"),
    "ro64_ppo_env_major": dict(_RO, X=4, policy_act="relu", member_act="tanh", ppo=True, env_major=True, normalize=True),
    "ro128_e2": dict(_RO, X=4, E=2, hidden=(128, 128), policy_act="tanh", member_act="relu"),       # k_model_rollout<128>
    "ro256_e2": dict(_RO, X=4, E=2, hidden=(256, 256), policy_act="relu", member_act="tanh"),       # k_model_rollout<256>
    "ro_pendulum_relu": dict(_RO, X=3, E=0, system="pendulum", policy_act="relu"),
}

# (seed, G, min |z64| over the relu units) of every case that differentiates a relu network — see the module docstring
KINK = {
    "sac_thin_rt": (0, 1.12e-06, 2.17e-05),        # 23 040 relu units
    "sac_thin_tr": (2, 1.88e-06, 2.69e-05),        # 46 080
    "sac_u2_rt": (0, 9.44e-07, 8.24e-05),          # 15 360
    "sac_u2_tr": (0, 8.64e-07, 9.14e-06),          # 30 720
    "sac_wide_rt": (0, 9.47e-07, 6.90e-05),        # 13 824
    "sac_wide_tr": (0, 9.39e-07, 1.95e-05),        # 27 648
    "sac_128_rt": (0, 1.08e-06, 1.10e-04),         # 27 648
    "sac_128_tr": (3, 1.25e-06, 2.71e-05),         # 55 296
    "ppo_64_rt": (0, 1.01e-06, 6.34e-04),          # 5 120
    "ppo_64_tr": (0, 1.81e-06, 3.65e-04),          # 6 144
    "ppo_128_rt": (0, 1.42e-06, 2.51e-04),         # 10 752
    "ppo_128_tr": (0, 1.47e-06, 1.32e-04),         # 12 288
    "ppo_wide_rt": (0, 8.01e-07, 1.82e-04),        # 3 072
    "ppo_wide_tr": (0, 1.07e-06, 3.19e-04),        # 4 096
    "ppo_layered_rt": (1, 1.41e-06, 2.86e-05),     # 17 920
    "ppo_layered_tr": (0, 1.81e-06, 5.08e-05),     # 49 920
    "ppo_t1030_rt": (1, 1.09e-06, 1.55e-05),       # 131 840 (at B = 2, 263 680 units, no seed of the 64 qualifies: rows shrunk to B = 1)
    "ppo_sp2_rt": (0, 6.03e-07, 7.52e-05),         # 524 544, copies of 21 distinct rows
    "bptt_x4_a": (0, 7.72e-07, 8.07e-05),          # 17 408
    "bptt_x4_b": (0, 1.22e-06, 1.38e-05),          # 17 408
    "bptt_wide": (1, 9.44e-07, 1.89e-04),          # 12 288
    "bptt_ts1_noise": (0, 1.29e-06, 5.94e-05),     # 17 408
    "critic_x4_relu": (0, 9.01e-07, 2.04e-04),     # 10 240
    "critic_x17_relu": (0, 7.93e-07, 9.07e-05),    # 10 240
    "mlp_fused_relu": (0, 9.99e-07, 5.83e-05),     # 5 120
    "mlp_layered_relu": (0, 2.31e-06, 2.62e-04),   # 10 240
    "nll_x4_relu": (0, 9.32e-07, 5.32e-04),        # 10 240
    "nll_x17_relu": (0, 6.70e-07, 5.67e-05),       # 10 240
}

# the owning modules' tolerances, by name
TOL = {
    "sac": dict(tol32=dict(atol=2e-6, rtol=2e-4), tol64=mt.SAC_TOL),                       # test_gpu_sac.test_sac_gradients_and_step
    "ppo": dict(tol32=dict(atol=2e-6, rtol=5e-4), tol64=mt.PPO_TOL),                       # test_gpu_ppo.test_ppo_gradients_and_step
    "bptt": dict(tol32=dict(atol=5e-6, rtol=2e-3), tol64=mt.BPTT_TOL),                     # test_gpu_bptt._assert_matches_oracle
    "bptt_ts": dict(tol32=dict(atol=5e-6, rtol=2e-3), tol64=mt.BPTT_TOL),
    "critic": dict(tol32=dict(atol=2e-6, rtol=5e-4), rel64=2e-5),                          # test_gpu_bptt.test_critic_grads_parity
    "mlp": dict(y=dict(atol=2e-5, rtol=2e-5), dx=dict(atol=2e-5, rtol=2e-4), dw=dict(atol=2e-6, rtol=2e-4)),      # test_gpu_bptt_generic
    "nll": dict(tol32=dict(atol=2e-6, rtol=5e-4), rel64=5e-5),                             # test_gpu_ensemble_train
    "ensfwd": dict(tol32=dict(atol=2e-5, rtol=2e-5), tol64=mt.ENS_TOL),                    # test_gpu_rollout.test_ensemble_forward_parity
    "policy_act": dict(tol32=dict(atol=2e-5, rtol=2e-5), tol64=mt.ENS_TOL),
    "ens_eval": dict(tol32=dict(atol=2e-5, rtol=2e-5), tol64=dict(atol=2e-5, rtol=2e-5)),  # test_gpu_ens_model_selection.TOL
    "tv": None,                                                                           # terminal_value_cases.TOL32 / TOL64
}
# relative size of the smallest tolerated error per family: what "differs by at least 100 x the tolerance" is measured against
REL_TOL = {"sac": 1e-4, "ppo": 2e-4, "bptt": 1e-3, "bptt_ts": 1e-3, "critic": 2e-5, "mlp": 2e-4, "nll": 5e-5, "ensfwd": 5e-5, "policy_act": 5e-5,
           "ens_eval": 2e-5, "tv": 5e-5}


def has_relu_backward(name: str) -> bool:
    return name in CASES and "relu" in CASES[name]["acts"]


def seed_of(name: str) -> int:
    return KINK[name][0] if name in KINK else 0


def swapped(acts):
    """Every exchange of two networks' activations (two networks: one; three: the three pairwise swaps and the two rotations); a single
    network takes the other non-swish activation."""
    acts = tuple(acts)
    if len(acts) == 1:
        return [("tanh",) if acts[0] == "relu" else ("relu",)]
    import itertools
    return [p for p in itertools.permutations(acts) if p != acts]


# ---------------------------------------------------------------------------------------------------------------------- inputs
def _net(dims, g, bias=0.02, scale=1.0):
    return onets.init_mlp_flat(dims, g) * scale + bias * torch.randn(onets.n_params(dims), generator=g)


@functools.lru_cache(maxsize=None)
def inputs(name: str, seed=None, acts=None, cus=None):
    """The host tensors of the case, at `seed` (default: the committed one) under `acts` (default: the case's); cus: the compute units
    the PPO two-per-CU case is sized for (default REF_CUS; no other case reads it)."""
    c = ALL[name]
    if cus is not None and name == "ppo_sp2_rt":
        c = dict(c, B=ppo_sp2_shape(cus)[0])
    seed = seed_of(name) if seed is None else seed
    acts = tuple(c["acts"]) if acts is None else tuple(acts)
    fam = c["family"]
    if fam == "sac":
        from test_gpu_sac import _make
        return _make(c["X"], c["U"], c["hidden"], c["B"], seed, c["normalize"], policy_act=acts[0], q_act=acts[1], **mt.SAC_CFG)
    if fam == "ppo":
        from test_gpu_ppo import _make
        B = c.get("base", c["B"])
        cfg, st, data, noise, nm, ns = _make(c["X"], c["U"], c["hidden"], B, c["T"], seed, c["normalize"], v_hidden=c["v_hidden"],
                                              policy_act=acts[0], value_act=acts[1], normalize_advantage=c.get("norm_adv", True), **mt.PPO_CFG)
        if B != c["B"]:
            reps = -(-c["B"] // B)
            data, noise = data.repeat(reps, 1, 1)[:c["B"]].contiguous(), noise.repeat(reps, 1, 1)[:c["B"]].contiguous()
        return cfg, st, data, noise, nm, ns
    if fam == "bptt":
        from test_gpu_bptt import _setup
        return _setup(c["X"], c["U"], c["H"], c["n"], "ensemble", c["E"], seed, hidden=c["hidden"], acts=acts)
    if fam == "bptt_ts":
        from test_gpu_bptt_stochastic import _ts_setup
        return _ts_setup(c["X"], c["U"], c["H"], c["n"], c["E"], seed, hidden=c["hidden"], acts=acts)
    g = torch.Generator().manual_seed(4100 + seed)
    if fam == "critic":
        X, B, R = c["X"], c["batch"], 100
        cfg = obptt.BpttConfig(x_dim=X, u_dim=1, actor_dims=[X, 64, 2], critic_dims=[X, *c["hidden"], 1], critic_act=acts[0])
        cp = torch.cat([_net(cfg.critic_dims, g) for _ in range(2)])
        rows, lam = torch.randn(R, 2 * X + 3, generator=g), torch.randn(R, generator=g) * 3
        idx = torch.randint(0, R, (B,), generator=g, dtype=torch.int32)
        return dict(cfg=cfg, cp=cp, rows=rows, lam=lam, idx=idx, mean=torch.randn(X, generator=g) * 0.2, std=torch.rand(X, generator=g) + 0.6)
    if fam == "mlp":
        dims, n = c["dims"], c["n"]
        return dict(dims=dims, act=acts[0], params=_net(dims, g, 0.05), x=torch.randn(n, dims[0], generator=g),
                    dy=torch.randn(1, n, dims[-1], generator=g), mean=torch.randn(dims[0], generator=g) * 0.3,
                    std=torch.rand(dims[0], generator=g) + 0.5)
    if fam == "nll":
        X, U, E, B, R = c["X"], c["U"], c["E"], c["B"], 100
        dims = [X + U, *c["hidden"], 2 * X]
        params = torch.cat([_net(dims, g) for _ in range(E)])
        rows = torch.randn(R, 2 * X + U + 2, generator=g)
        rows[:, X + U + 2:] = rows[:, :X] + 0.1 * torch.randn(R, X, generator=g)
        return dict(dims=dims, act=acts[0], params=params, rows=rows, idx=torch.randint(0, R, (E, B), generator=g))
    if fam == "ensfwd":
        from test_gpu_rollout import _ens_params
        return dict(act=acts[0], params=_ens_params(c["dims"], c["E"], seed), x=torch.randn(c["N"], c["dims"][0], generator=g))
    if fam == "policy_act":
        dims = c["dims"]
        return dict(act=acts[0], params=_net(dims, g, 0.05), obs=torch.randn(c["N"], dims[0], generator=g),
                    noise=torch.randn(c["N"], dims[-1] // 2, generator=g), mean=torch.randn(dims[0], generator=g) * 0.3,
                    std=torch.rand(dims[0], generator=g) + 0.5)
    if fam == "ens_eval":
        from test_gpu_ens_model_selection import _case_data
        g2, dims, params, rows, R = _case_data(c["X"], c["U"], c["E"], c["hidden"], False, seed)
        idx = torch.randint(0, R, (c["n"],), generator=g2)
        return dict(act=acts[0], dims=dims, params=params, rows=rows, idx=idx)
    if fam == "tv":
        import terminal_value_cases as tvc
        X, A = c["X"], c["A"]
        pdims, cdims = [X, *c["policy_hidden"], 2 * A], [X + A, *c["critic_hidden"], 1]
        critic = torch.cat([tvc._net(cdims, g) for _ in range(2)])
        policy = tvc._net(pdims, g)
        mean, std = torch.randn(X, generator=g), torch.rand(X, generator=g) * 1.5 + 0.5
        x = mean + std * 2.0 * torch.randn(16 * 5 + 1, X, generator=g)
        return dict(acts=acts, pdims=pdims, cdims=cdims, critic=critic, policy=policy, mean=mean, std=std, x=x)
    raise KeyError(fam)


# ---------------------------------------------------------------------------------------------------------------------- oracle
def _run_oracle(name, inp, dtype):
    """dict(main=<the tensor the case is about>, ...) in `dtype`."""
    c = ALL[name]
    fam = c["family"]
    d = lambda t: None if t is None else t.to(dtype)
    if fam == "sac":
        g, (cl, ac, al) = mt.sac_oracle(inp, dtype)
        return dict(main=g, losses=[cl, ac, al])
    if fam == "ppo":
        g, terms = mt.ppo_oracle(dict(neq=False), inp, dtype)
        return dict(main=g, terms=terms)
    if fam == "bptt":
        cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, tsys, extra = inp
        tsys_d = obptt.TorchEnsembleSystem(d(extra["dp"]), extra["dd"], c["E"], c["X"], c["U"], d(extra["tgt"]), d(extra["q"]),
                                           d(extra["r"]), act=extra["act"])
        g, loss, aux = obptt.actor_grads(cfg, tsys_d, d(ap), d(cp), d(x0), d(noise), d(s_mean), d(s_std), d(r_ms[0]), d(r_ms[1]))
        return dict(main=g, loss=loss, aux=aux)
    if fam == "bptt_ts":
        from test_gpu_bptt_stochastic import TsEnsembleSystem
        cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, extra, members, eps = inp
        tsys_d = TsEnsembleSystem(d(extra["dp"]), extra["dd"], c["E"], c["X"], c["U"], d(extra["tgt"]), d(extra["q"]), d(extra["r"]), True,
                                  act=extra["act"]).set_draws(members, d(eps))
        g, loss, aux = obptt.actor_grads(cfg, tsys_d, d(ap), d(cp), d(x0), d(noise), d(s_mean), d(s_std), d(r_ms[0]), d(r_ms[1]))
        assert tsys_d.t == cfg.horizon
        return dict(main=g, loss=loss, aux=aux)
    if fam == "critic":
        i = inp
        rows = i["idx"].long()
        g, loss = obptt.critic_grads(i["cfg"], d(i["cp"]), d(i["rows"][rows, :c["X"]]), d(i["lam"][rows]), d(i["mean"]), d(i["std"]))
        return dict(main=g, loss=loss)
    if fam == "mlp":
        i = inp
        p, x = d(i["params"]).clone().requires_grad_(True), d(i["x"]).clone().requires_grad_(True)
        y = onets.mlp_forward(p, i["dims"], (x - d(i["mean"])) / d(i["std"]), i["act"])
        (y * d(i["dy"][0])).sum().backward()
        return dict(main=p.grad.detach(), dx=x.grad.detach(), y=y.detach())
    if fam == "nll":
        i = inp
        g, losses = oens.nll_grads(d(i["params"]), i["dims"], c["E"], d(i["rows"]), i["idx"], c["X"], c["U"], True, 1e-3, act=i["act"])
        return dict(main=g, losses=losses)
    if fam == "ensfwd":
        return dict(main=onets.ensemble_forward(d(inp["params"]), c["dims"], c["E"], d(inp["x"]), inp["act"]))
    if fam == "policy_act":
        i = inp
        logits = onets.mlp_forward(d(i["params"]), c["dims"], onets.normalize(d(i["obs"]), d(i["mean"]), d(i["std"])), i["act"])
        z = onets.sample_no_postprocessing(logits, d(i["noise"]))
        return dict(main=onets.postprocess(z), mode=onets.mode(logits), raw=z, log_prob=onets.log_prob(logits, z))
    if fam == "ens_eval":
        import ens_select_ref as sref
        i = inp
        return dict(main=sref.eval_metrics(d(i["params"]), i["dims"], c["E"], d(i["rows"]), i["idx"], c["X"], c["U"], True, 1e-3, None,
                                           act=i["act"]))
    if fam == "tv":
        import terminal_value_ref as tref
        i = inp
        return dict(main=tref.v_hat(d(i["x"]), i["critic"], i["cdims"], 2, i["acts"][1], policy=i["policy"], policy_dims=i["pdims"],
                                    policy_act=i["acts"][0], mean=i["mean"], std=i["std"]))
    raise KeyError(fam)


@functools.lru_cache(maxsize=None)
def oracle(name: str, dtype=torch.float32, seed=None, acts=None, cus=None) -> dict:
    """The reference run of the case, computed once per (dtype, seed, acts, cus) and left unchanged."""
    return _run_oracle(name, inputs(name, seed, acts, cus), dtype)


def groups(name: str):
    """Named slices of oracle(name)['main'] that belong to ONE network each (a comparison per network, so that a wrong activation
    in the smaller network cannot hide behind the larger one's gradient)."""
    c = ALL[name]
    if c["family"] == "sac":
        cfg = inputs(name)[0]
        return {"policy": slice(0, cfg.P), "critics": slice(cfg.P, cfg.P + 2 * cfg.Q)}
    if c["family"] == "ppo":
        cfg = inputs(name)[0]
        return {"policy": slice(0, cfg.P), "value": slice(cfg.P, None)}
    return {"all": slice(None)}


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a - b).norm() / b.norm())


# ------------------------------------------------------------------------------------------------------------------- the kink
def kink(name: str, seed=None) -> dict:
    """The fp32 and the fp64 oracle of the case under oracle.nets.tap: G = max |z32 - z64| over every tapped pre-activation, minz =
    min |z64| over the relu ones, flips = relu pre-activations whose sign differs between the runs, units = relu pre-activations."""
    inp = inputs(name, seed)
    return kink_of(lambda dtype: _run_oracle(name, inp, dtype))


def kink_of(run) -> dict:
    """kink() of any oracle run: run(dtype) computes it in fp32 and in fp64."""
    taps = {}
    for dtype in (torch.float32, torch.float64):
        rec = []
        with onets.tap(lambda z, act: rec.append((z.detach().double().reshape(-1), act))):
            run(dtype)
        taps[dtype] = rec
    z32s, z64s = taps[torch.float32], taps[torch.float64]
    assert len(z32s) == len(z64s) and len(z32s) > 0
    G, minz, flips, units = 0.0, float("inf"), 0, 0
    for (z32, a32), (z64, a64) in zip(z32s, z64s):
        assert a32 == a64 and z32.shape == z64.shape
        G = max(G, float((z32 - z64).abs().max()))
        if a64 == "relu":
            minz = min(minz, float(z64.abs().min()))
            flips += int(((z32 > 0) != (z64 > 0)).sum())
            units += z64.numel()
    return dict(G=G, minz=minz, flips=flips, units=units, ok=units > 0 and flips == 0 and minz >= KINK_FACTOR * G)


def find_seed(name: str):
    """(seed, kink record) of the first seed in 0..63 that meets the condition, or (None, None)."""
    for s in SEEDS:
        k = kink(name, s)
        if k["ok"]:
            return s, k
    return None, None


# ------------------------------------------------------------------------------------------------------------- the PPO sp2 case
def ppo_sp2_shape(cus: int):
    """(B, T) of the smallest minibatch the default dispatch gives to k_ppo_fwd_bwd<64, 2> (ppo_variant: sp2 = more tiles than CUs):
    T = 3 and the first B with ceil(3 B / 16) > cus."""
    T = 3
    B = (16 * cus) // T + 1
    assert mt.tiles_of(B * T) == cus + 1
    return B, T
