"""The case table of tests/test_gpu_many_tiles.py and tests/test_cpu_many_tiles_cases.py: shapes at which one workgroup of a fused
kernel walks SEVERAL 16-row tiles, every row an independent random draw, compared with the float64 oracle at the very size the
kernel runs.

Sizing.  Every launch caps its grid (or its gradient slabs) at a multiple of the device's compute units; `cap(cus)` below restates
that multiple per kernel (csrc/ppo.hip ppo_plan, csrc/rollout.hip mbpo_model_rollout / mbpo_ensemble_mlp_forward, csrc/bptt.hip
bptt_plan; fused SAC has no tile loop, its "cap" is the 16-tile block of slab_sum<16>).  rows_beyond(cap) = 16 (2 cap + 3) + 5 gives
2 cap + 4 tiles: more than twice the cap, not a multiple of it (workgroups get two or three tiles), the last tile ragged.

Tolerances are the ones at the head of the per-family GPU modules (test_gpu_ppo.py, test_gpu_sac.py, test_gpu_rollout.py,
test_gpu_bptt.py), against float64: gradients are means over the batch, so their scale does not grow with the row count.
test_cpu_many_tiles_cases.py checks that the float32 oracle alone stays within a quarter of each of them.
"""
import torch

from oracle import nets as onets
from oracle import rollout as oro
from oracle import systems as osys

REF_CUS = 256                  # MI355X; the GPU tests size from the device they run on


def tiles_of(rows: int) -> int:
    return (rows + 15) // 16


def rows_beyond(cap: int, ragged: int = 5) -> int:
    return 16 * (2 * cap + 3) + ragged


def loops_unevenly(rows: int, cap: int) -> bool:
    t = tiles_of(rows)
    return t > 2 * cap and t % cap != 0 and rows % 16 != 0


def distinct_rows(t: torch.Tensor) -> bool:
    t = t.reshape(-1, t.shape[-1])
    return torch.unique(t, dim=0).shape[0] == t.shape[0]


def quarter_gap_ok(got32: torch.Tensor, ref64: torch.Tensor, atol: float, rtol: float):
    """(ok, worst ratio) of |float32 oracle - float64 oracle| against a QUARTER of atol + rtol |ref|."""
    ref64 = ref64.double()
    ratio = ((got32.double() - ref64).abs() / (0.25 * (atol + rtol * ref64.abs()))).max()
    return bool(ratio <= 1.0), float(ratio)


# ---------------------------------------------------------------------------------------------------------------------- PPO
# gradients atol 2e-6 + rtol 2e-4 against float64, loss terms rtol 2e-5 + atol 1e-5 (tests/test_gpu_ppo.py)
# The (4, 2, (128, 128)) case: its value-network gradients reach 6.2 while the policy's are 1e-3, and the float32 ORACLE alone differs
# from the float64 one by 0.421 of that tolerance there (9.3e-7 on an element of 1.0e-3, the same from 1 to 16 host threads).  A kernel
# sums the same terms in another order, so that case is allowed 4 x that gap: 1.7 x the module's tolerance (atol 3.4e-6 + rtol 3.4e-4).
PPO_TOL = dict(atol=2e-6, rtol=2e-4)
PPO_CFG = dict(entropy_cost=1e-2, discounting=0.99, reward_scaling=0.5, gae_lambda=0.95, clipping_epsilon=0.3, lr=3e-4, wd=1e-5)
PPO_CASES = {
    # cap in units of CUs: one slab per CU, two for the 512-thread sp2 launch
    "h128_u2": dict(X=4, U=2, hidden=(128, 128), T=7, cap=1, neq=False, normalize=True, norm_adv=True, tol_scale=1.7),    # k_ppo_fwd_bwd<128,2,false>
    "wide": dict(X=17, U=6, hidden=(64, 64), T=5, cap=1, neq=False, normalize=False, norm_adv=True),       # k_ppo_fwd_bwd<64,4,true>
    "sp2_neq": dict(X=4, U=2, hidden=(64, 64, 64), T=6, cap=2, neq=True, normalize=True, norm_adv=True),   # <64,2,false>, values Q = true
}


def ppo_tol(case):
    k = case.get("tol_scale", 1.0)
    return dict(atol=k * PPO_TOL["atol"], rtol=k * PPO_TOL["rtol"])


def ppo_cap(case, cus):
    return case["cap"] * cus


def ppo_bt(case, cus):
    T, cap = case["T"], ppo_cap(case, cus)
    B = -(-rows_beyond(cap) // T)
    while not loops_unevenly(B * T, cap):
        B += 1
    return B, T


def ppo_inputs(case, cus):
    from test_gpu_ppo import _make
    B, T = ppo_bt(case, cus)
    cfg, st, data, noise, nm, ns = _make(case["X"], case["U"], case["hidden"], B, T, 7, case["normalize"],
                                          normalize_advantage=case["norm_adv"], **PPO_CFG)
    if case["neq"]:
        from test_gpu_ppo_brax_env import _with_switch_times
        data = _with_switch_times(data, case["X"], case["U"], 1)
    return cfg, st, data, noise, nm, ns


def ppo_oracle(case, inputs, dtype):
    from oracle import ppo as oppo
    cfg, st, data, noise, nm, ns = inputs
    c = lambda t: None if t is None else t.to(dtype)
    if case["neq"]:
        import ppo_brax_env_ref as ref
        from test_gpu_ppo_brax_env import NEQ
        g, terms, _, _ = ref.grads(cfg, c(st.params), c(data), c(noise), c(nm), c(ns), neq=NEQ)
    else:
        g, terms, _, _ = oppo.grads(cfg, c(st.params), c(data), c(noise), c(nm), c(ns))
    return g, terms


# ---------------------------------------------------------------------------------------------------------------------- SAC
# gradients atol 2e-6 + rtol 1e-4 against float64, losses rtol 2e-5 + atol 2e-6 (tests/test_gpu_sac.py)
SAC_TOL = dict(atol=2e-6, rtol=1e-4)
SAC_CFG = dict(discounting=0.99, reward_scaling=1.5, lr_policy=3e-4, lr_q=3e-4, lr_alpha=3e-4, wd_q=1e-3)
SAC_BLOCK = 16                                                                       # slab_sum<16>: blocks of 16 tiles, then a tail
SAC_BATCHES = (600, 1112)                                                            # 38 and 70 tiles, the last one of 8 rows
SAC_CASES = {
    # lean: mbpo_debug_set_sac_lean value (-1: leave the default)
    "lean": dict(X=4, U=1, hidden=(64, 64, 64), lean=1, normalize=True),             # k_sac_lean
    "thin": dict(X=4, U=1, hidden=(64, 64, 64), lean=0, normalize=True),             # k_sac_fwd_bwd<64,4,false,2,true>
    "u2": dict(X=4, U=2, hidden=(64, 64, 64), lean=-1, normalize=False),             # k_sac_fwd_bwd<64,4,false,2>
    "wide": dict(X=17, U=6, hidden=(64, 64, 64), lean=-1, normalize=True),           # k_sac_fwd_bwd<64,4,true>
    "h128": dict(X=3, U=1, hidden=(128, 128, 128), lean=-1, normalize=True),         # k_sac_fwd_bwd<128,4,false,2>
}


def sac_inputs(case, B):
    from test_gpu_sac import _make
    return _make(case["X"], case["U"], case["hidden"], B, 3, case["normalize"], **SAC_CFG)


def sac_oracle(inputs, dtype):
    from oracle import sac as osac
    cfg, st, batch, noise, nm, ns = inputs
    c = lambda t: None if t is None else t.to(dtype)
    return osac.grads(cfg, c(st.params), c(st.target_q), c(batch), *[c(n) for n in noise], c(nm), c(ns))


# ------------------------------------------------------------------------------------------------------------------ rollout
# rows atol 2e-4 + rtol 2e-4 for S <= 5 (tests/test_gpu_rollout.py)
RO_TOL = dict(atol=2e-4, rtol=2e-4)
RO_S, RO_L = 3, 2
RO_CASES = {
    # cap in units of CUs: 4 for the generic kernels; the lean kernel takes one workgroup per CU and, from 2 tiles per CU on, PAIRS of
    # tiles (units = ceil(tiles / 2)).  lean: mbpo_debug_set_rollout_lean value
    "generic64": dict(X=4, U=1, E=5, hidden=(64, 64, 64), lean=0, cap=4, normalize=True),               # k_model_rollout64<false,false>
    "lean": dict(X=4, U=1, E=5, hidden=(64, 64, 64), lean=-1, cap=1, pairs=True, normalize=True),       # k_rollout_lean, two tiles in flight
    "wide": dict(X=17, U=6, E=10, hidden=(64, 64, 64), lean=-1, cap=4),                                 # k_model_rollout64<true,false>
    "h128": dict(X=4, U=1, E=3, hidden=(128, 128), lean=-1, cap=4, normalize=True),                     # k_model_rollout<128,false>
    "h256": dict(X=4, U=1, E=2, hidden=(64, 64), dyn_hidden=(200,) * 4, pad=256, lean=-1, cap=4),       # k_model_rollout<256,false>, padded
    "ts1_noise": dict(X=4, U=1, E=5, hidden=(64, 64, 64), lean=0, cap=4, mode="ts1", sample_noise=True),
    "learned": dict(X=4, U=1, E=5, hidden=(64, 64, 64), lean=0, cap=4, reward="learned"),               # k_model_rollout64<false,true>
}


def ro_cap(case, cus):
    return case["cap"] * cus


def ro_units(case, n):
    return (tiles_of(n) + 1) // 2 if case.get("pairs") else tiles_of(n)


def ro_n(cus):
    return rows_beyond(4 * cus)


def ro_inputs(case, N, seed=0):
    """Independent draws for every environment; the networks at their LOGICAL widths (the GPU test pads where case['pad'] says so)."""
    X, U, E, S, L = case["X"], case["U"], case["E"], RO_S, RO_L
    g = torch.Generator().manual_seed(seed)
    learned = case.get("reward") == "learned"
    pdims = [X, *case["hidden"], 2 * U]
    ddims = [X + U, *case.get("dyn_hidden", case["hidden"]), 2 * X + (2 if learned else 0)]
    inp = dict(pdims=pdims, ddims=ddims, N=N)
    inp["ppar"] = onets.init_mlp_flat(pdims, g) + 0.02 * torch.randn(onets.n_params(pdims), generator=g)
    inp["dpar"] = torch.cat([onets.init_mlp_flat(ddims, g) * 0.5 + 0.01 * torch.randn(onets.n_params(ddims), generator=g)
                             for _ in range(E)])
    inp["obs0"], inp["first"] = torch.randn(N, X, generator=g), torch.randn(N, X, generator=g)
    inp["steps0"] = torch.randint(0, L, (N,), generator=g).float()
    inp["done0"] = (torch.rand(N, generator=g) < 0.2).float()
    inp["pnoise"] = torch.randn(S, N, U, generator=g)
    inp["mnoise"] = torch.randn(S, 1, N, X, generator=g) if case.get("sample_noise") else None
    inp["midx"] = torch.randint(0, E, (S, 1, N), generator=g, dtype=torch.int32) if case.get("mode") == "ts1" else None
    inp["nm"] = torch.randn(X, generator=g) * 0.3 if case.get("normalize") else None
    inp["ns"] = torch.rand(X, generator=g) + 0.5 if case.get("normalize") else None
    inp["rparams"] = None if learned else torch.cat([torch.randn(X, generator=g), torch.rand(X, generator=g),
                                                     torch.rand(U, generator=g) * 0.1])
    return inp


def ro_oracle(case, inp, dtype):
    X, U, E = case["X"], case["U"], case["E"]
    c = lambda t: None if t is None else t.to(dtype)
    mode, noise = case.get("mode", "mean"), bool(case.get("sample_noise"))
    if case.get("reward") == "learned":
        import learned_reward_ref as lref
        system = lref.LearnedRewardEnsembleSystem(c(inp["dpar"]), inp["ddims"], E, X, U, mode=mode, predict_delta=True, sample_noise=noise,
                                                  min_std=1e-3)
    else:
        tgt, q, r = c(inp["rparams"][:X]), c(inp["rparams"][X:2 * X]), c(inp["rparams"][2 * X:])
        system = osys.EnsembleSystem(c(inp["dpar"]), inp["ddims"], E, X, U, mode=mode, predict_delta=True, sample_noise=noise, min_std=1e-3,
                                     reward_fn=lambda x, u: osys.quadratic_reward(x, u, tgt, q, r))
    st0 = oro.EnvState(c(inp["obs0"]), c(inp["first"]), c(inp["steps0"]), c(inp["done0"]))
    return oro.rollout(system, c(inp["ppar"]), inp["pdims"], st0, RO_S, RO_L, 1, norm_mean=c(inp["nm"]), norm_std=c(inp["ns"]),
                       policy_noise=c(inp["pnoise"]), model_noise=c(inp["mnoise"]), member_idx=inp["midx"])


# --------------------------------------------------------------------------------------------------------------------- BPTT
# actor gradient atol 5e-6 + rtol 1e-3 against float64, transitions 2e-4, lambda-values 5e-4 (tests/test_gpu_bptt.py)
BPTT_TOL = dict(atol=5e-6, rtol=1e-3)
BPTT_CASES = {
    # one slab per CU (bptt_plan).  min_tiles / ragged: the tile counts the cases were first stated with (16 x 300 + 7, 16 x 40 + 3), kept
    # as a floor; the count actually used is max(min_tiles, 2 CUs + 3), so that every workgroup walks two or three tiles
    "pendulum": dict(X=3, U=1, H=4, system="pendulum", E=0, min_tiles=300, ragged=7, zstore=(-1,)),
    "c2": dict(X=4, U=1, H=5, system="ensemble", E=5, min_tiles=300, ragged=7, zstore=(-1, 0)),       # store and recompute, bit-equal
    "c5": dict(X=17, U=6, H=4, system="ensemble", E=10, min_tiles=40, ragged=3, zstore=(-1,)),        # config 5's shape, short horizon
}


def bptt_n(case, cus):
    return 16 * max(case["min_tiles"], 2 * cus + 3) + case["ragged"]


def bptt_inputs(case, n):
    from test_gpu_bptt import _setup
    return _setup(case["X"], case["U"], case["H"], n, case["system"], case["E"], 5)


def bptt_oracle(case, s):
    from test_gpu_bptt import _oracle
    cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, tsys, extra = s
    return _oracle(cfg, tsys, ap, cp, x0, noise, s_mean, s_std, r_ms, case["system"], extra, case["X"], case["U"], case["E"])


# --------------------------------------------------------------------------------------------------------- ensemble forward
# single forward: atol 5e-5 + rtol 5e-5 against float64 (tests/test_gpu_rollout.py)
ENS_TOL = dict(atol=5e-5, rtol=5e-5)
ENS_CASE = dict(dims=[5, 64, 64, 64, 8], E=5, act="swish")


def ens_caps(cus):
    """generic k_ensemble_forward: 8 workgroups per CU, one tile at a time; k_ens_fwd_lean: 2 CUs / E workgroups per member, one PAIR of
    tiles at a time."""
    return dict(generic=8 * cus, lean=max(1, (2 * cus) // ENS_CASE["E"]))


def ens_n(cus):
    return rows_beyond(8 * cus)


def ens_inputs(N):
    from test_gpu_rollout import _ens_params
    params = _ens_params(ENS_CASE["dims"], ENS_CASE["E"], 2)
    x = torch.randn(N, ENS_CASE["dims"][0], generator=torch.Generator().manual_seed(3))
    return params, x


def ens_oracle(params, x, dtype):
    return onets.ensemble_forward(params.to(dtype), ENS_CASE["dims"], ENS_CASE["E"], x.to(dtype), ENS_CASE["act"])
