"""The case table of tests/test_gpu_scratch_contract.py and tests/test_cpu_scratch_contract.py: one entry per (entry point, dispatch
path) of include/mbpo_hip.h that takes a caller-owned `workspace` (and the outputs-only mbpo_ens_pick_elites), at the smallest shapes
that still cross tiles, slots or a kernel threshold.  Inputs are the owning test modules' (their helpers where they have one, their
generation code with the same seeds where it sits inline in a test).

A case knows three things:
  entries      the C entry points its run calls;
  need(scale)  the workspace size the header states for it, in elements of ws_dtype — a host-side query that needs no device;
               `scale` multiplies the batch / row count at a fixed path (tests/test_cpu_scratch_contract.py: never shrinking);
  run(dev, ws, mem) -> {name: device tensor} of every `out` and `inout` buffer.  `ws` holds at least need() elements; every `out`
               buffer comes from mem.out(name, n, dtype) and every `inout` one from mem.inout(name, initial), so that the caller
               chooses what the kernels find there (zeros, NaN bits, guard bands).
  knob         an optional (mbpo_debug_set_* name, mode) pair that selects the dispatch path; the caller sets it around BOTH need() and
               run() and resets it to -1 (the workspace size may depend on it: the BPTT z store).

Out of scope, by the header's own words: the SAC entry points (mbpo_sac_step: "`workspace` must be zero before the first call"; its
control block is state, not scratch) and the mbpo_p2p_* exchange regions (zero-initialised by mbpo_p2p_alloc, peers write into them).
mbpo_mlp_vjp takes one or two nets per launch; the three-net rows of the table run on mbpo_mlp_layered_vjp, where ops.mlp_vjp
sends them.  mbpo_policy_act has no layer-by-layer path: its second row is the widest policy its kernel takes (256).
"""
from __future__ import annotations

import ctypes as C
import functools
from dataclasses import dataclass
from typing import Callable, Dict, Optional, Tuple

import numpy as np
import torch

REF_CUS = 256      # MI355X; size queries without a device assume it (csrc/api.hip mbpo_num_cus)

# every exported function / descriptor with a `workspace` that this table deliberately leaves out, and why
OUT_OF_SCOPE = {
    "mbpo_sac_desc": "the header states the zero requirement; the control block inside the workspace is state, not scratch",
    "mbpo_p2p_desc": "exchange regions are zero-initialised by mbpo_p2p_alloc and written by peers",
}


@dataclass
class Case:
    id: str
    family: str
    entries: Tuple[str, ...]
    ws_dtype: Optional[str]                 # "float32" | "int32" | None (no workspace: outputs only)
    need: Callable[[int], int]
    run: Callable                           # (dev, ws, mem) -> {name: tensor}
    knob: Optional[Tuple[str, int]] = None
    # `out` elements a kernel legitimately never writes, as explicit flat indices per buffer (the header names them); the poisoned-
    # output check excludes exactly these.  Empty everywhere today.
    unwritten: Optional[Dict[str, list]] = None


CASES: Dict[str, Case] = {}


def _add(case: Case) -> None:
    assert case.id not in CASES, case.id
    CASES[case.id] = case


def _lib():
    from mbpo import _hip
    return _hip, _hip.load()


def _query(n: int, what: str) -> int:
    if n < 0:
        _hip, lib = _lib()
        raise _hip.MbpoHipError(f"{what} failed (rc={n}): {lib.mbpo_last_error().decode('utf-8', 'replace')}")
    return int(n)


def _host_mlp(dims, n_nets: int = 1, act: str = "swish"):
    """An mbpo_mlp_desc for size queries: they never read the parameters."""
    _hip, _ = _lib()
    d = _hip.MlpDesc()
    d.params, d.n_nets, d.n_layers, d.activation = 16, n_nets, len(dims) - 1, _hip.ACT_IDS[act]
    for i, v in enumerate(dims):
        d.dims[i] = int(v)
    d.net_stride = sum(dims[i] * dims[i + 1] + dims[i + 1] for i in range(len(dims) - 1))
    return d


def _np_params(dims) -> int:
    return sum(dims[i] * dims[i + 1] + dims[i + 1] for i in range(len(dims) - 1))


def _stream():
    from mbpo import _hip
    return _hip.current_stream_ptr()


def _p(t):
    return None if t is None else t.data_ptr()


# ====================================================================================================================== PPO
PPO_CFG = dict(entropy_cost=1e-2, discounting=0.99, reward_scaling=0.5, gae_lambda=0.95, clipping_epsilon=0.3, lr=3e-4, wd=1e-5)


def _ppo_bt(c, cus):
    if c.get("many"):
        import many_tiles_cases as mt
        return mt.ppo_bt(mt.PPO_CASES[c["many"]], cus)
    return c["B"], c["T"]


def _ppo_need(c, scale: int = 1) -> int:
    _hip, lib = _lib()
    X, U = c["X"], c["U"]
    B, T = _ppo_bt(c, REF_CUS if not torch.cuda.is_available() else torch.cuda.get_device_properties(0).multi_processor_count)
    pd, vd = [X, *c["hidden"], 2 * U], [X, *c.get("v_hidden", c["hidden"]), 1]
    d = _hip.PpoDesc()
    d.x_dim, d.u_dim, d.policy_layers, d.value_layers = X, U, len(pd) - 1, len(vd) - 1
    for i, v in enumerate(pd):
        d.policy_dims[i] = v
    for i, v in enumerate(vd):
        d.value_dims[i] = v
    d.batch_size, d.unroll_length, d.row_len = B * scale, T, 2 * X + 2 * U + 4
    d.normalize_advantage = 1
    d.max_grad_norm = float(c.get("clip") or 0.0)
    if c.get("neq"):
        d.non_equidistant_time, d.env_dt = 1, 0.1
    return _query(lib.mbpo_ppo_workspace_floats(C.byref(d)), "mbpo_ppo_workspace_floats")


@functools.lru_cache(maxsize=None)
def _ppo_inputs(cid: str, cus: int):
    from test_gpu_ppo import _make
    c = _PPO[cid]
    B, T = _ppo_bt(c, cus)
    cfg, st, data, noise, nm, ns = _make(c["X"], c["U"], c["hidden"], B, T, 7, c.get("normalize", True), v_hidden=c.get("v_hidden"),
                                          normalize_advantage=c.get("norm_adv", True), **PPO_CFG)
    if c.get("neq"):
        from test_gpu_ppo_brax_env import _with_switch_times
        data = _with_switch_times(data, c["X"], c["U"], 1)
    return cfg, st, data, noise, nm, ns, B, T


def _ppo_run(cid, dev, ws, mem):
    from test_gpu_ppo import _updater
    c = _PPO[cid]
    cfg, st, data, noise, nm, ns, B, T = _ppo_inputs(cid, torch.cuda.get_device_properties(dev).multi_processor_count)
    kw = {}
    if c.get("neq"):
        from test_gpu_ppo_brax_env import NEQ_KW
        kw.update(NEQ_KW)
    if c.get("clip"):
        kw["max_grad_norm"] = c["clip"]
    up = _updater(dev, cfg, B, T, **kw)
    assert up.workspace.numel() == _ppo_need(c), "PpoUpdater and the size query disagree"
    up.fused_step = bool(c["fused"])
    # hand in the memory before the first call: workspace, the two pure outputs; the state tensors through the allocator too
    up.workspace = ws
    up.grads, up.metrics = mem.out("grads", up.NPV), mem.out("metrics", 4)
    up.params = mem.inout("params", st.params.to(dev))
    up.adam_m, up.adam_v = mem.inout("adam_m", torch.zeros(up.NPV, device=dev)), mem.inout("adam_v", torch.zeros(up.NPV, device=dev))
    up.step_count, up.metrics_accum = mem.inout("step_count", torch.zeros(1, device=dev)), mem.inout("metrics_accum", torch.zeros(5, device=dev))
    d = up.desc
    d.workspace, d.grads, d.metrics, d.metrics_accum = ws.data_ptr(), up.grads.data_ptr(), up.metrics.data_ptr(), up.metrics_accum.data_ptr()
    d.params, d.adam_m, d.adam_v, d.step_count = up.params.data_ptr(), up.adam_m.data_ptr(), up.adam_v.data_ptr(), up.step_count.data_ptr()
    dd = lambda t: None if t is None else t.to(dev)
    up.minibatch_step(data.to(dev), dd(nm), dd(ns), noise.to(dev))
    torch.cuda.synchronize()
    return dict(grads=up.grads, metrics=up.metrics, params=up.params, adam_m=up.adam_m, adam_v=up.adam_v, step_count=up.step_count,
                metrics_accum=up.metrics_accum)


_STEP, _GA = ("mbpo_ppo_step",), ("mbpo_ppo_grads", "mbpo_ppo_apply")
_PPO = {
    # k_ppo_lean / k_ppo_vg_lean (x = 3, u = 1, 64 x 2 and 64 x 3), one slab per tile; the ragged one ends in a 12-row tile
    "ppo_lean64x2_step": dict(X=3, U=1, hidden=(64, 64), B=128, T=40, fused=1),
    "ppo_lean64x3_ragged": dict(X=3, U=1, hidden=(64, 64, 64), B=20, T=7, fused=0),
    "ppo_lean_off_ragged": dict(X=3, U=1, hidden=(64, 64, 64), B=20, T=7, fused=1, knob=("mbpo_debug_set_ppo_lean", 0)),
    "ppo_generic64_wide": dict(X=17, U=6, hidden=(64, 64), B=8, T=3, fused=1, normalize=False),          # k_ppo_fwd_bwd<64,4,true>
    "ppo_h128": dict(X=4, U=2, hidden=(128, 128), B=24, T=7, fused=0),                                   # k_ppo_fwd_bwd<128,2>
    "ppo_layered": dict(X=4, U=2, hidden=(48, 80), v_hidden=(200, 72, 40), B=20, T=7, fused=1, norm_adv=False),
    "ppo_layered_grads_apply": dict(X=4, U=2, hidden=(48, 80), v_hidden=(200, 72, 40), B=20, T=7, fused=0),
    "ppo_many_slabs": dict(X=17, U=6, hidden=(64, 64), many="wide", fused=1, normalize=False),           # >= 64 slabs: k_ppo_reduce_groups
    "ppo_no_norm_adv": dict(X=4, U=1, hidden=(64, 64, 64), B=16, T=10, fused=1, norm_adv=False),         # the `mom` region unused
    "ppo_long_unroll": dict(X=3, U=1, hidden=(64, 64), B=2, T=1024, fused=1, normalize=False),           # separate values / scan / moments
    "ppo_neq_lean": dict(X=3, U=1, hidden=(64, 64), B=20, T=7, fused=1, neq=True),
    "ppo_neq_layered": dict(X=4, U=2, hidden=(48, 80), v_hidden=(200, 72, 40), B=20, T=7, fused=0, neq=True),   # the `disc` region
    "ppo_neq_long_unroll": dict(X=3, U=1, hidden=(64, 64), B=2, T=1024, fused=0, neq=True, normalize=False),    # `disc`, separate scan
    "ppo_clip_step": dict(X=3, U=1, hidden=(64, 64), B=20, T=7, fused=1, clip=0.05),                     # the `ss_part` region
    "ppo_clip_grads_apply": dict(X=4, U=2, hidden=(128, 128), B=24, T=7, fused=0, clip=0.05),
}
for _cid, _c in _PPO.items():
    _add(Case(_cid, "ppo", _STEP if _c["fused"] else _GA, "float32", functools.partial(_ppo_need, _c), functools.partial(_ppo_run, _cid),
              knob=_c.get("knob")))


# ====================================================================================================================== BPTT
def _bptt_desc(c, n):
    _hip, _ = _lib()
    X, U, H, E = c["X"], c["U"], c["H"], c["E"]
    d = _hip.BpttDesc()
    d.x_dim, d.u_dim, d.horizon, d.n = X, U, H, n
    d.actor_layers = d.critic_layers = 4
    for i, (a, cr) in enumerate(zip([X, 64, 64, 64, 2 * U], [X, 64, 64, 64, 1])):
        d.actor_dims[i], d.critic_dims[i] = a, cr
    d.actor_activation = d.critic_activation = _hip.ACT_IDS["swish"]
    if E:
        d.system_kind, d.reward_kind = _hip.SYS_ENSEMBLE, _hip.REWARD_QUADRATIC
        d.dynamics = _host_mlp([X + U, 64, 64, 64, 2 * X], E)
    else:
        d.system_kind, d.reward_kind = _hip.SYS_PENDULUM, _hip.REWARD_PENDULUM
        d.sys_params = 16
    d.ens_mode = {"mean": _hip.ENS_MEAN, "ts1": _hip.ENS_TS1, "tsinf": _hip.ENS_TSINF}[c.get("mode", "mean")]
    d.ens_sample_noise = int(bool(c.get("noise")))
    return d


def _bptt_need(c, scale: int = 1) -> int:
    _, lib = _lib()
    d = _bptt_desc(c, c["n"] * scale)
    return _query(lib.mbpo_bptt_workspace_floats(C.byref(d)), "mbpo_bptt_workspace_floats")


@functools.lru_cache(maxsize=None)
def _bptt_inputs(cid: str):
    c = _BPTT[cid]
    if c["E"]:
        from test_gpu_bptt_stochastic import _ts_setup
        return _ts_setup(c["X"], c["U"], c["H"], c["n"], c["E"])
    from test_gpu_bptt import _setup
    cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, _, extra = _setup(c["X"], c["U"], c["H"], c["n"], "pendulum", 0, 0)
    return cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, extra, None, None


def bptt_call(op, c, inputs, dev):
    """One mbpo_bptt_actor_grads call of case dict `c` on the ops object `op` (also used by the one-object reuse test)."""
    from mbpo import _hip, ops
    from oracle import nets as onets
    from oracle import systems as osys
    cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, extra, members, eps = inputs
    kw = {}
    if c["E"]:
        mode = c.get("mode", "mean")
        given = c.get("given", True)
        kw.update(system_kind=_hip.SYS_ENSEMBLE, reward_kind=_hip.REWARD_QUADRATIC,
                  reward_params=torch.cat([extra["tgt"], extra["q"], extra["r"]]).to(dev), dyn_params=extra["dp"].to(dev),
                  dyn_spec=ops.MlpSpec(extra["dd"], "swish", extra["dp"].numel() // onets.n_params(extra["dd"])),
                  ens_mode={"mean": _hip.ENS_MEAN, "ts1": _hip.ENS_TS1, "tsinf": _hip.ENS_TSINF}[mode],
                  ens_sample_noise=bool(c.get("noise")), ens_predict_delta=c.get("delta", True),
                  member_idx=members.to(dev).contiguous() if (mode == "ts1" and given) else None,
                  model_noise=eps.to(dev).contiguous() if (c.get("noise") and given) else None)
    else:
        pp = osys.PendulumParams()
        kw.update(system_kind=_hip.SYS_PENDULUM, reward_kind=_hip.REWARD_PENDULUM, reward_params=torch.tensor(pp.reward_vector()).to(dev),
                  sys_params=torch.tensor(pp.sys_vector()).to(dev))
    op(actor_params=ap.to(dev), target_critic_params=cp.to(dev), init_states=x0.to(dev), state_mean=s_mean.to(dev), state_std=s_std.to(dev),
       reward_mean_std=r_ms.to(dev), act_noise=noise.to(dev) if c.get("given", True) else None, offset=3, **kw)
    torch.cuda.synchronize()


def bptt_op(c, cfg, dev):
    from mbpo import ops
    return ops.BpttActorGrad(x_dim=cfg.x_dim, u_dim=cfg.u_dim, horizon=cfg.horizon, actor_dims=cfg.actor_dims, critic_dims=cfg.critic_dims,
                             n=c["n"], device=dev, init_stddev=cfg.init_stddev, discount=cfg.discount, lambda_=cfg.lambda_,
                             ent_coef=cfg.ent_coef, seed=11)


def _bptt_run(cid, dev, ws, mem):
    c = _BPTT[cid]
    inputs = _bptt_inputs(cid)
    op = bptt_op(c, inputs[0], dev)
    op.workspace = ws                     # before the first call: the object then sizes nothing itself
    n, H = c["n"], c["H"]
    op.transitions, op.lambda_values = mem.out("transitions", n * H * op.row_len).view(n * H, op.row_len), mem.out("lambda_values", n * H)
    op.grads, op.metrics = mem.out("grads", op.P), mem.out("metrics", 2)
    bptt_call(op, c, inputs, dev)
    return dict(transitions=op.transitions, lambda_values=op.lambda_values, grads=op.grads, metrics=op.metrics)


_ZS0 = ("mbpo_debug_set_bptt_zstore", 0)
_BPTT = {
    # n = 40: two full tiles and one of 8 rows; n = 24: one and a half.  E = 5 runs two member rounds (4 + 1), E = 3 one.
    "bptt_pendulum": dict(X=3, U=1, H=6, n=24, E=0),
    "bptt_mean_zstore": dict(X=4, U=2, H=6, n=40, E=3),
    "bptt_mean_recompute": dict(X=4, U=2, H=6, n=40, E=3, knob=_ZS0),
    "bptt_ts1_noise_zstore": dict(X=4, U=1, H=6, n=24, E=5, mode="ts1", noise=True),
    "bptt_ts1_noise_recompute": dict(X=4, U=1, H=6, n=24, E=5, mode="ts1", noise=True, delta=False, knob=_ZS0),
    "bptt_tsinf_zstore": dict(X=4, U=2, H=6, n=40, E=3, mode="tsinf", noise=False),
    # members, model noise and actor noise all drawn by the kernel (Philox): the member checkpoints are written by the forward sweep
    "bptt_ts1_philox_zstore": dict(X=4, U=1, H=6, n=40, E=5, mode="ts1", noise=True, given=False),
    "bptt_ts1_philox_recompute": dict(X=4, U=2, H=6, n=24, E=3, mode="ts1", noise=True, given=False, knob=_ZS0),
}
for _cid, _c in _BPTT.items():
    _add(Case(_cid, "bptt", ("mbpo_bptt_actor_grads",), "float32", functools.partial(_bptt_need, _c), functools.partial(_bptt_run, _cid),
              knob=_c.get("knob")))


# ====================================================================================================================== critic
_CRITIC_DIMS = [4, 64, 64, 1]


def _critic_need(batch, scale: int = 1) -> int:
    _, lib = _lib()
    dims = (C.c_int32 * len(_CRITIC_DIMS))(*_CRITIC_DIMS)
    return _query(lib.mbpo_critic_workspace_floats(_CRITIC_DIMS[0], len(_CRITIC_DIMS) - 1, dims, batch * scale), "mbpo_critic_workspace_floats")


@functools.lru_cache(maxsize=None)
def _critic_inputs(batch: int):
    from oracle import nets as onets
    g = torch.Generator().manual_seed(batch)
    X, R, D = _CRITIC_DIMS[0], 96, 2 * _CRITIC_DIMS[0] + 1 + 2
    cp = torch.cat([onets.init_mlp_flat(_CRITIC_DIMS, g) + 0.02 * torch.randn(onets.n_params(_CRITIC_DIMS), generator=g) for _ in range(2)])
    return (cp, torch.randn(R, D, generator=g), torch.randn(R, generator=g), torch.randint(0, R, (batch,), generator=g, dtype=torch.int32),
            torch.randn(X, generator=g) * 0.2, torch.rand(X, generator=g) + 0.6)


def _critic_run(batch, dev, ws, mem):
    from mbpo import ops
    cp, tr, lam, idx, sm, ss = (t.to(dev) for t in _critic_inputs(batch))
    op = ops.CriticGrad(x_dim=_CRITIC_DIMS[0], critic_dims=_CRITIC_DIMS, batch=batch, device=dev)
    assert op.workspace.numel() == _critic_need(batch)
    op.workspace, op.grads, op.metrics = ws, mem.out("grads", 2 * op.C), mem.out("metrics", 1)
    op(cp, tr, lam, idx, sm, ss)
    torch.cuda.synchronize()
    return dict(grads=op.grads, metrics=op.metrics)


for _b in (8, 40):
    _add(Case(f"critic_b{_b}", "critic", ("mbpo_critic_grads",), "float32", functools.partial(_critic_need, _b), functools.partial(_critic_run, _b)))


# ====================================================================================================================== MLP VJPs
def _vjp_dims(c):
    return [c["din"], *c["hidden"], c["dout"]]


def _vjp_need(c, scale: int = 1) -> int:
    _, lib = _lib()
    d = _host_mlp(_vjp_dims(c), c["nets"], c.get("act", "swish"))
    fn = lib.mbpo_mlp_layered_workspace_floats if c["layered"] else lib.mbpo_mlp_vjp_workspace_floats
    return _query(fn(C.byref(d), c["n"] * scale), "mlp workspace query")


@functools.lru_cache(maxsize=None)
def _vjp_inputs(cid: str):
    from oracle import nets as onets
    c = _VJP[cid]
    dims, nets, n = _vjp_dims(c), c["nets"], c["n"]
    g = torch.Generator().manual_seed(len(cid) + n)
    P = onets.n_params(dims)
    params = torch.cat([onets.init_mlp_flat(dims, g) + 0.05 * torch.randn(P, generator=g) for _ in range(nets)])
    return (params, torch.randn(n, dims[0], generator=g), torch.randn(nets, n, dims[-1], generator=g), torch.randn(dims[0], generator=g) * 0.2,
            torch.rand(dims[0], generator=g) + 0.6)


def _vjp_run(cid, dev, ws, mem):
    from mbpo import _hip
    lib = _hip.load()
    c = _VJP[cid]
    dims, nets, n = _vjp_dims(c), c["nets"], c["n"]
    params, x, dy, nm, ns = (t.to(dev) for t in _vjp_inputs(cid))
    d = _hip.mlp_desc(params, dims, c.get("act", "swish"), nets)
    res = {}
    if c.get("y", True):
        res["y"] = mem.out("y", nets * n * dims[-1])
    if c["dx"]:
        res["dx"] = mem.out("dx", nets * n * dims[0])
    if c["dw"]:
        res["dw"] = mem.out("dw", nets * _np_params(dims))
    if c["layered"]:
        _hip.check(lib.mbpo_mlp_layered_vjp(C.byref(d), x.data_ptr(), n, dy.data_ptr(), _p(res.get("y")), _p(res.get("dx")), _p(res.get("dw")),
                                            ws.data_ptr(), _stream()), "mbpo_mlp_layered_vjp")
    else:
        _hip.check(lib.mbpo_mlp_vjp(C.byref(d), x.data_ptr(), n, nm.data_ptr(), ns.data_ptr(), dy.data_ptr(), _p(res.get("y")), _p(res.get("dx")),
                                    _p(res.get("dw")), ws.data_ptr() if c["dw"] else None, _stream()), "mbpo_mlp_vjp")
    torch.cuda.synchronize()
    return res


_VJP = {
    # mbpo_mlp_vjp: n = 33 is two full tiles and a row; the workspace (slabs) is used only with dw
    "vjp_1net_dw_dx": dict(layered=False, din=4, hidden=(64, 64), dout=1, nets=1, n=33, dx=True, dw=True),
    "vjp_2net_dw": dict(layered=False, din=5, hidden=(64, 64, 64), dout=3, nets=2, n=33, dx=False, dw=True, y=False),
    "vjp_2net_dw_dx": dict(layered=False, din=17, hidden=(64, 64), dout=12, nets=2, n=33, dx=True, dw=True),
    # mbpo_mlp_layered_vjp: n = 37 (two 32-row GEMM tiles, the second ragged); 1100 rows split the weight gradients' row range in two
    "layered_48_80": dict(layered=True, din=6, hidden=(48, 80), dout=4, nets=1, n=37, dx=True, dw=True),
    "layered_3net_200_72_40": dict(layered=True, din=5, hidden=(200, 72, 40), dout=3, nets=3, n=37, dx=False, dw=True),
    "layered_3net_dx_only": dict(layered=True, din=5, hidden=(48, 80), dout=3, nets=3, n=37, dx=True, dw=False, y=False),
    "layered_splitk": dict(layered=True, din=6, hidden=(48, 80), dout=4, nets=2, n=1100, dx=True, dw=True),
}
for _cid, _c in _VJP.items():
    _add(Case(_cid, "layered_vjp" if _c["layered"] else "mlp_vjp", ("mbpo_mlp_layered_vjp",) if _c["layered"] else ("mbpo_mlp_vjp",),
              "float32", functools.partial(_vjp_need, _c), functools.partial(_vjp_run, _cid)))


# ====================================================================================================================== AdamW
def _adamw_need(c, scale: int = 1) -> int:
    return 2 * ((c["n"] * scale + 255) // 256) + 4          # the header's formula


def _adamw_run(cid, dev, ws, mem):
    from mbpo import ops
    c = _ADAMW[cid]
    n = c["n"]
    g = torch.Generator().manual_seed(n)
    params, grads, target = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1, torch.randn(n, generator=g)
    if c.get("bad_grad"):
        grads[n // 2] = float("inf")
    opt = ops.AdamW(n, dev, lr=1e-3, weight_decay=1e-2, apply_if_finite=c["aif"])
    assert opt.workspace.numel() == _adamw_need(c)
    opt.workspace, opt.grad_norm = ws, mem.out("grad_norm", 1)
    opt.m, opt.v = mem.inout("m", torch.rand(n, generator=g).to(dev) * 0.01), mem.inout("v", torch.rand(n, generator=g).to(dev) * 0.01)
    opt.count = mem.inout("count", torch.full((1,), 3.0, device=dev))
    p = mem.inout("params", params.to(dev))
    t = mem.inout("target", target.to(dev)) if c["target"] else None
    opt.step(p, grads.to(dev), target=t, tau=0.05, grad_scale=0.5)
    torch.cuda.synchronize()
    res = dict(grad_norm=opt.grad_norm, m=opt.m, v=opt.v, count=opt.count, params=p)
    if t is not None:
        res["target"] = t
    return res


_ADAMW = {
    "adamw_n1": dict(n=1, aif=False, target=False),
    "adamw_n257_finite_target": dict(n=257, aif=True, target=True),            # two partials, the second of one element
    "adamw_n257_skipped": dict(n=257, aif=True, target=True, bad_grad=True),   # a non-finite gradient: the whole update is skipped
    "adamw_n20993": dict(n=20993, aif=False, target=True),                     # 83 partials, a scalar tail behind the 16-byte body
    "adamw_n20993_finite": dict(n=20993, aif=True, target=False),
}
for _cid, _c in _ADAMW.items():
    _add(Case(_cid, "adamw", ("mbpo_adamw_step",), "float32", functools.partial(_adamw_need, _c), functools.partial(_adamw_run, _cid)))


# ====================================================================================================================== ensemble NLL / eval
def _ens_dims(c):
    return [c["X"] + c["U"], *c["hidden"], 2 * c["X"] + (2 if c.get("head") else 0)]


def _ens_need(c, scale: int = 1) -> int:
    _hip, lib = _lib()
    X, U = c["X"], c["U"]
    D = 2 * X + U + 2
    if c["kind"] == "nll":
        d = _hip.EnsTrainDesc()
        d.batch = c["B"] * scale
    else:
        d = _hip.EnsEvalDesc()
        d.n = c["B"] * scale
    d.x_dim, d.u_dim, d.dynamics, d.row_len, d.next_obs_off = X, U, _host_mlp(_ens_dims(c), c["E"]), D, X + U + 2
    d.reward_off = X + U if c.get("fit_reward") else -1
    fn = lib.mbpo_ens_nll_workspace_floats if c["kind"] == "nll" else lib.mbpo_ens_eval_workspace_floats
    return _query(fn(C.byref(d)), "ensemble workspace query")


@functools.lru_cache(maxsize=None)
def ens_inputs(cid: str):
    """tests/test_gpu_ensemble_train.py's generation (its seeds per shape); evaluation shares ONE index list."""
    from oracle import nets as onets
    c = _ENS[cid]
    X, U, E, B = c["X"], c["U"], c["E"], c["B"]
    g = torch.Generator().manual_seed(c["seed"])
    dims = _ens_dims(c)
    P = onets.n_params(dims)
    params = torch.cat([onets.init_mlp_flat(dims, g) + 0.02 * torch.randn(P, generator=g) for _ in range(E)])
    R, D = 500, 2 * X + U + 2
    rows = torch.randn(R, D, generator=g)
    rows[:, X + U + 2:] = rows[:, :X] + 0.1 * torch.randn(R, X, generator=g)
    idx = torch.randint(0, R, (E, B) if c["kind"] == "nll" else (B,), generator=g).to(torch.int32)
    return params, rows, idx


def ens_op(c, dev):
    from mbpo import ops
    cls = ops.EnsembleNllGrad if c["kind"] == "nll" else ops.EnsembleEval
    kw = dict(batch=c["B"]) if c["kind"] == "nll" else {}
    return cls(x_dim=c["X"], u_dim=c["U"], spec=ops.MlpSpec(_ens_dims(c), "swish", c["E"]), device=dev, predict_delta=c.get("delta", True), **kw)


def _ens_run(cid, dev, ws, mem):
    c = _ENS[cid]
    params, rows, idx = (t.to(dev) for t in ens_inputs(cid))
    op = ens_op(c, dev)
    op.workspace = ws                     # before the first call (EnsembleEval keeps a workspace that is large enough)
    if c["kind"] == "nll":
        op.grads, op.metrics = mem.out("grads", op.E * op.n_params), mem.out("metrics", op.E)
    else:
        op.metrics = mem.out("metrics", 2 * op.E).view(2, op.E)
    op(params, rows, idx, reward_off=c["X"] + c["U"] if c.get("fit_reward") else None)
    torch.cuda.synchronize()
    assert op.workspace is ws
    return dict(grads=op.grads, metrics=op.metrics) if c["kind"] == "nll" else dict(metrics=op.metrics)


_ENS = {
    # fused: tests/test_gpu_ensemble_train.py's cases 2, 4 and 5
    "ens_nll_ragged_b70": dict(kind="nll", X=3, U=1, E=3, B=70, hidden=(64, 64, 64), seed=1),
    "ens_nll_x17": dict(kind="nll", X=17, U=6, E=2, B=48, hidden=(64, 64, 64), seed=3),
    "ens_nll_more_tiles_than_slots": dict(kind="nll", X=4, U=1, E=4, B=16 * 150, hidden=(64,), seed=4),
    "ens_nll_head_fitted": dict(kind="nll", X=3, U=1, E=3, B=70, hidden=(64, 64), seed=5, head=True, fit_reward=True),
    "ens_nll_head_unfitted": dict(kind="nll", X=3, U=1, E=3, B=70, hidden=(64, 64), seed=5, head=True),
    # layered
    "ens_nll_layered_reward": dict(kind="nll", X=4, U=1, E=3, B=37, hidden=(200, 100, 50), seed=6, head=True, fit_reward=True),
    "ens_nll_layered_unfitted": dict(kind="nll", X=4, U=1, E=3, B=37, hidden=(200, 100, 50), seed=6, head=True, delta=False),
    "ens_nll_layered_splitk": dict(kind="nll", X=4, U=1, E=2, B=1100, hidden=(48, 80), seed=7),
    "ens_eval_fused": dict(kind="eval", X=3, U=1, E=3, B=70, hidden=(64, 64, 64), seed=1),
    "ens_eval_fused_many_tiles": dict(kind="eval", X=4, U=1, E=4, B=16 * 150 + 5, hidden=(64,), seed=4, head=True, fit_reward=True),
    "ens_eval_fused_unfitted": dict(kind="eval", X=3, U=1, E=3, B=70, hidden=(64, 64), seed=5, head=True),
    "ens_eval_layered_reward": dict(kind="eval", X=4, U=1, E=3, B=37, hidden=(200, 100, 50), seed=6, head=True, fit_reward=True),
    "ens_eval_layered_unfitted": dict(kind="eval", X=4, U=1, E=3, B=300, hidden=(200, 100, 50), seed=6, head=True, delta=False),
}
for _cid, _c in _ENS.items():
    _add(Case(_cid, "ens_" + _c["kind"], ("mbpo_ens_nll_grads",) if _c["kind"] == "nll" else ("mbpo_ens_eval",), "float32",
              functools.partial(_ens_need, _c), functools.partial(_ens_run, _cid)))


# ====================================================================================================================== keep_best / elites
def _select_inputs(E, P):
    g = torch.Generator().manual_seed(E + P)
    params, best = torch.randn(E * P, generator=g), torch.randn(E * P, generator=g)
    score, best_score = torch.rand(E, generator=g), torch.rand(E, generator=g)
    best_score[0] = float("inf")          # a first evaluation
    score[1] = float("nan")               # never an improvement
    return params, best, score, best_score


def _keep_run(E, P, dev, ws, mem):
    from mbpo import ops
    params, best, score, best_score = (t.to(dev) for t in _select_inputs(E, P))
    bp, bs = mem.inout("best_params", best), mem.inout("best_score", best_score)
    st = mem.inout("state", torch.tensor([2, 5], dtype=torch.int32, device=dev))
    ops.ens_keep_best(params, bp, E, score, bs, 0.01, st, workspace=ws)
    torch.cuda.synchronize()
    return dict(best_params=bp, best_score=bs, state=st)


def _elites_run(E, P, k, dev, ws, mem):
    from mbpo import ops
    params, _, score, _ = (t.to(dev) for t in _select_inputs(E, P))
    idx, ep = mem.out("elite_idx", k, torch.int32), mem.out("elite_params", k * P)
    ops.ens_pick_elites(params, E, score, k, elite_idx=idx, elite_params=ep)
    torch.cuda.synchronize()
    return dict(elite_idx=idx, elite_params=ep)


for _E, _P in ((7, 1003), (70, 258)):          # 1003: members not 16-byte aligned against each other; 70 members: two passes of 64 threads
    _add(Case(f"keep_best_e{_E}", "keep_best", ("mbpo_ens_keep_best",), "int32", (lambda s=1, e=_E: e * s), functools.partial(_keep_run, _E, _P)))
    _add(Case(f"pick_elites_e{_E}", "pick_elites", ("mbpo_ens_pick_elites",), None, (lambda s=1: 0), functools.partial(_elites_run, _E, _P, 3)))


# ====================================================================================================================== input scaler fit
def _scaler_need(c, scale: int = 1) -> int:
    _, lib = _lib()
    return _query(lib.mbpo_ens_scaler_workspace_floats(c["n"] * scale, c["in_dim"]), "mbpo_ens_scaler_workspace_floats")


@functools.lru_cache(maxsize=None)
def _scaler_inputs(cid: str):
    c = _SCALER[cid]
    g = torch.Generator().manual_seed(c["n"])
    R = c["n"] if not c["idx"] else max(64, c["n"] // 3)
    rows = torch.randn(R, c["in_dim"] + 3, generator=g) * 2.0 + 0.5
    rows[:, 1] = 0.25                     # a constant column: std below the floor -> exactly 1
    idx = torch.randint(0, R, (c["n"],), generator=g).to(torch.int32) if c["idx"] else None
    return rows, idx


def _scaler_run(cid, dev, ws, mem):
    from mbpo import _hip
    lib = _hip.load()
    c = _SCALER[cid]
    rows, idx = _scaler_inputs(cid)
    rows, idx = rows.to(dev), None if idx is None else idx.to(dev)
    out = mem.out("scaler", 2 * c["in_dim"])
    _hip.check(lib.mbpo_ens_scaler_fit(rows.data_ptr(), rows.shape[0], rows.shape[1], _p(idx), c["n"], c["in_dim"], 1e-12, out.data_ptr(),
                                       ws.data_ptr(), _stream()), "mbpo_ens_scaler_fit")
    torch.cuda.synchronize()
    return dict(scaler=out)


_SCALER = {
    "scaler_n1": dict(n=1, in_dim=5, idx=False),
    "scaler_n777_idx": dict(n=777, in_dim=5, idx=True),
    "scaler_n777": dict(n=777, in_dim=23, idx=False),
    "scaler_n20480_idx": dict(n=20480, in_dim=23, idx=True),
    "scaler_n20480": dict(n=20480, in_dim=5, idx=False),
}
for _cid, _c in _SCALER.items():
    _add(Case(_cid, "scaler", ("mbpo_ens_scaler_fit",), "float32", functools.partial(_scaler_need, _c), functools.partial(_scaler_run, _cid)))


# ====================================================================================================================== running statistics
def _stats_need(X, scale: int = 1) -> int:
    _, lib = _lib()
    return _query(lib.mbpo_running_stats_workspace_floats(X), "mbpo_running_stats_workspace_floats")     # (independent of the row count)


def _stats_run(X, n, fused, dev, ws, mem):
    from mbpo import ops
    g = torch.Generator().manual_seed(X + n)
    rows = (torch.randn(n, X + 4, generator=g) * 1.5 + 0.3).to(dev)
    stats0 = torch.cat([torch.tensor([10.0]), torch.randn(X, generator=g) * 0.1, torch.rand(X, generator=g) * 10, torch.ones(X)])
    stats = mem.inout("stats", stats0.to(dev))
    sums = mem.out("sums", 1 + 2 * X)     # pass 0 writes [0, 1 + X), pass 1 the rest: fully written by either chain
    if fused:
        ops.running_stats_update(rows, 2, X, stats, sums=sums, workspace=ws)
    else:
        ops.running_stats_reduce(rows, 2, X, stats, 0, sums=sums, workspace=ws)
        ops.running_stats_reduce(rows, 2, X, stats, 1, sums=sums, workspace=ws)
        ops.running_stats_apply(stats, sums, X)
    torch.cuda.synchronize()
    return dict(stats=stats, sums=sums)


for _X, _n in ((3, 5), (17, 777), (128, 700)):
    _add(Case(f"stats_update_x{_X}", "stats", ("mbpo_running_stats_update",), "float32", functools.partial(_stats_need, _X),
              functools.partial(_stats_run, _X, _n, True)))
    _add(Case(f"stats_reduce_x{_X}", "stats", ("mbpo_running_stats_reduce",), "float32", functools.partial(_stats_need, _X),
              functools.partial(_stats_run, _X, _n, False)))


# ====================================================================================================================== policy_act
def _act_need(dims, n, scale: int = 1) -> int:
    return n * scale * (dims[0] + dims[-1])          # the header: n * (x_dim + 2 * u_dim)


def _act_run(dims, n, dev, ws, mem):
    from mbpo import _hip
    from oracle import nets as onets
    lib = _hip.load()
    g = torch.Generator().manual_seed(dims[1])
    U = dims[-1] // 2
    params = (onets.init_mlp_flat(dims, g) + 0.02 * torch.randn(onets.n_params(dims), generator=g)).to(dev)
    obs, nm, ns = torch.randn(n, dims[0], generator=g).to(dev), (torch.randn(dims[0], generator=g) * 0.3).to(dev), (torch.rand(dims[0], generator=g) + 0.5).to(dev)
    act, raw, lp = mem.out("action", n * U), mem.out("raw_action", n * U), mem.out("log_prob", n)
    d = _hip.mlp_desc(params, dims, "swish", 1)
    _hip.check(lib.mbpo_policy_act(C.byref(d), obs.data_ptr(), n, nm.data_ptr(), ns.data_ptr(), 0, 0.0, None, 5, 2 << 32, None, 7 * n * U,
                                   act.data_ptr(), raw.data_ptr(), lp.data_ptr(), ws.data_ptr(), _stream()), "mbpo_policy_act")
    torch.cuda.synchronize()
    return dict(action=act, raw_action=raw, log_prob=lp)


for _name, _dims in (("fused64", [3, 64, 64, 6]), ("wide256", [3, 256, 256, 6])):
    _add(Case(f"policy_act_{_name}", "policy_act", ("mbpo_policy_act",), "float32", functools.partial(_act_need, _dims, 33),
              functools.partial(_act_run, _dims, 33)))


# ====================================================================================================================== permutation
def _perm_run(n, dev, ws, mem):
    from mbpo import ops
    out = mem.out("perm", n, torch.int32)
    ops.philox_permutation(n, seed=0xABCDEF, offset=9 << 32, out=out, workspace=ws)
    torch.cuda.synchronize()
    return dict(perm=out)


for _n in (1000, 5000, 20000):                   # one-workgroup LDS sort; bucket sort with the flag word; keys in the workspace + rank count
    _add(Case(f"perm_n{_n}", "perm", ("mbpo_philox_permutation",), "int32", (lambda s=1, n=_n: n * s), functools.partial(_perm_run, _n)))


# ====================================================================================================================== iCEM update
@functools.lru_cache(maxsize=None)
def _icem_inputs(cid: str):
    """tests/test_gpu_icem.py::_check_icem_update's arrays (coarse rewards, so that ties occur), for n_problems problems side by side."""
    c = _ICEM[cid]
    NB, NC, H, U, P = c.get("problems", 1), c["NC"], c["H"], c["U"], c["P"]
    rng = np.random.default_rng(0)
    X = 4
    D = 2 * X + U + 3
    rows = rng.standard_normal((H * NB * NC * P, D)).astype(np.float32)
    rows[:, X + U] = np.round(rows[:, X + U], 1)
    cand = rng.standard_normal((NB * NC, H, U)).astype(np.float32)
    mean, std = rng.standard_normal((NB, H, U)).astype(np.float32), (rng.random((NB, H, U)) + 0.2).astype(np.float32)
    best_seq = rng.standard_normal((NB, H, U)).astype(np.float32)
    best_val = np.where(np.arange(NB) % 2 == 0, -np.inf, 10.0).astype(np.float32)      # taken / kept
    cost = (rng.standard_normal(NB * NC * P) * 0.5).astype(np.float32)
    return tuple(torch.from_numpy(a) for a in (rows, cand, mean, std, best_seq, best_val, cost)) + (D, X)


def _icem_run(cid, dev, ws, mem):
    from mbpo import _hip
    lib = _hip.load()
    c = _ICEM[cid]
    NB, NC, H, U, P, ne, nprev = c.get("problems", 1), c["NC"], c["H"], c["U"], c["P"], c["ne"], c["nprev"]
    rows, cand, mean, std, bseq, bval, cost, D, X = _icem_inputs(cid)
    rows, cand, cost = rows.to(dev), cand.to(dev), cost.to(dev)
    dmean, dstd = mem.inout("mean", mean.to(dev)), mem.inout("std", std.to(dev))
    dbv, dbs = mem.inout("best_value", bval.to(dev)), mem.inout("best_sequence", bseq.to(dev))
    dvals = mem.out("values", NB * NC)
    dprev = mem.out("prev_elites", NB * nprev * H * U) if nprev else None
    st = _stream()
    if c["entry"] == "mbpo_icem_update":
        rc = lib.mbpo_icem_update(rows.data_ptr(), D, X + U, NC, P, H, U, cand.data_ptr(), ne, nprev, 0.3, c.get("use_max", 0), dmean.data_ptr(),
                                  dstd.data_ptr(), dbv.data_ptr(), dbs.data_ptr(), _p(dprev), dvals.data_ptr(), ws.data_ptr(), st)
    elif c["entry"] == "mbpo_icem_update_constrained":
        rc = lib.mbpo_icem_update_constrained(rows.data_ptr(), D, X + U, NC, P, H, U, cand.data_ptr(), ne, nprev, 0.3, c.get("use_max", 0),
                                              cost.data_ptr(), 2.5, 1, dmean.data_ptr(), dstd.data_ptr(), dbv.data_ptr(), dbs.data_ptr(), _p(dprev),
                                              dvals.data_ptr(), ws.data_ptr(), st)
    else:
        rc = lib.mbpo_icem_update_batched(rows.data_ptr(), D, X + U, NB, NC, P, H, U, cand.data_ptr(), ne, nprev, 0.3, c.get("use_max", 0),
                                          cost.data_ptr(), 2.5, 0, dmean.data_ptr(), dstd.data_ptr(), dbv.data_ptr(), dbs.data_ptr(), _p(dprev),
                                          dvals.data_ptr(), ws.data_ptr(), st)
    _hip.check(rc, c["entry"])
    torch.cuda.synchronize()
    res = dict(mean=dmean, std=dstd, best_value=dbv, best_sequence=dbs, values=dvals)
    if dprev is not None:
        res["prev_elites"] = dprev
    return res


def _icem_mode(m):
    return ("mbpo_debug_set_icem_update", m)


_ICEM = {
    # both update kernels (0: global memory, 1: LDS) on tests/test_gpu_icem.py's shapes
    "icem_ref_global": dict(entry="mbpo_icem_update", NC=157, H=12, U=2, ne=20, nprev=6, P=3, knob=_icem_mode(0)),
    "icem_ref_lds": dict(entry="mbpo_icem_update", NC=157, H=12, U=2, ne=20, nprev=6, P=3, knob=_icem_mode(1)),
    "icem_nc1500_global": dict(entry="mbpo_icem_update", NC=1500, H=10, U=2, ne=50, nprev=10, P=2, use_max=1, knob=_icem_mode(0)),
    "icem_nc1500_lds": dict(entry="mbpo_icem_update", NC=1500, H=10, U=2, ne=50, nprev=10, P=2, use_max=1, knob=_icem_mode(1)),
    "icem_all_elites_no_prev": dict(entry="mbpo_icem_update", NC=40, H=6, U=3, ne=40, nprev=0, P=2, knob=_icem_mode(1)),
    "icem_lds69k_default": dict(entry="mbpo_icem_update", NC=300, H=32, U=4, ne=130, nprev=20, P=2),          # past 60 KB: k_icem_update
    "icem_constrained_global": dict(entry="mbpo_icem_update_constrained", NC=100, H=8, U=2, ne=12, nprev=12, P=3, knob=_icem_mode(0)),
    "icem_constrained_lds": dict(entry="mbpo_icem_update_constrained", NC=100, H=8, U=2, ne=12, nprev=12, P=3, knob=_icem_mode(1)),
    # tests/test_gpu_icem_batched.py's NC = 129, H = 10, five problems
    "icem_batched_global": dict(entry="mbpo_icem_update_batched", problems=5, NC=129, H=10, U=1, ne=12, nprev=3, P=2, knob=_icem_mode(0)),
    "icem_batched_lds": dict(entry="mbpo_icem_update_batched", problems=5, NC=129, H=10, U=1, ne=12, nprev=3, P=2, knob=_icem_mode(1)),
}
for _cid, _c in _ICEM.items():
    _add(Case(_cid, "icem", (_c["entry"],), "int32", (lambda s=1, c=_c: c.get("problems", 1) * c["NC"] * s), functools.partial(_icem_run, _cid),
              knob=_c.get("knob")))


# ====================================================================================================================== second-hand scratch
# (A, B): run A on one buffer sized for the larger of the two, then B on the same buffer untouched; B must equal its own control.
SECOND_HAND = [
    ("ppo_lean64x2_step", "ppo_lean64x3_ragged"),
    ("ppo_many_slabs", "ppo_generic64_wide"),
    ("ppo_layered", "ppo_h128"),
    ("ppo_neq_layered", "ppo_clip_step"),
    ("ppo_h128", "ppo_layered_grads_apply"),
    ("bptt_ts1_noise_zstore", "bptt_mean_zstore"),
    ("bptt_mean_zstore", "bptt_ts1_philox_zstore"),
    ("bptt_ts1_philox_zstore", "bptt_pendulum"),
    ("critic_b40", "critic_b8"),
    ("vjp_2net_dw_dx", "vjp_1net_dw_dx"),
    ("layered_splitk", "layered_48_80"),
    ("layered_3net_200_72_40", "layered_splitk"),
    ("adamw_n20993", "adamw_n257_finite_target"),
    ("ens_nll_more_tiles_than_slots", "ens_nll_ragged_b70"),
    ("ens_nll_layered_reward", "ens_nll_head_unfitted"),
    ("ens_nll_x17", "ens_nll_layered_splitk"),
    ("ens_eval_layered_unfitted", "ens_eval_fused"),
    ("ens_eval_fused_many_tiles", "ens_eval_layered_reward"),
    ("keep_best_e70", "keep_best_e7"),
    ("scaler_n20480_idx", "scaler_n777"),
    ("stats_reduce_x128", "stats_update_x17"),
    ("policy_act_wide256", "policy_act_fused64"),
    ("perm_n20000", "perm_n5000"),               # stale keys under the bucket sort's flag word: one redundant full sort, the same result
    ("icem_nc1500_global", "icem_ref_lds"),
    ("icem_batched_lds", "icem_constrained_global"),
]


def covered_entries() -> set:
    return {e for c in CASES.values() for e in c.entries}
