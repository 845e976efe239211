"""SHA-256 of what one launch of every dispatch path of mbpo_model_rollout and mbpo_ensemble_mlp_forward returns, on seeded inputs: a
record to compare two builds of the library bit for bit (run once per library, MBPO_HIP_LIB choosing it), not a test of either.

    MBPO_HIP_LIB=/path/to/libmbpo_hip.so python scripts/rollout_digests.py --out digests.json

Paths: k_model_rollout64 narrow and WIDE, k_model_rollout<128> and <256>, each with the formula, learned and term-table rewards, with and
without the termination box and the start buffer, hallucinated and time-adaptive; k_ensemble_forward<64 | 128 | 256>; k_openloop_pendulum
with and without a start buffer.  The specialised kernels (k_rollout_lean, k_ens_fwd_lean) are switched off so that the generic ones run.
"""
import argparse
import hashlib
import json
import os
import sys
from pathlib import Path

os.environ["MBPO_ROLLOUT_LEAN"] = "0"
os.environ["MBPO_ENS_LEAN"] = "0"
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "model-based-policy-optimizers_amd"))
sys.path.insert(0, str(ROOT / "scripts"))

import torch  # noqa: E402

from bench_kernels import lecun_flat  # noqa: E402

N, S, L, E = 40, 4, 3, 3          # 2.5 tiles, resets inside the launch
HOLD = dict(hold_max_steps=3, hold_min_time=0.05, hold_max_time=0.15, hold_dt=0.05, hold_gamma=0.9, hold_switch_cost=0.1)


def sha(*ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def term_table(X, UE, dev):
    from mbpo.systems.rewards.term_reward import Group, Term, TermRewardParams
    groups = [Group([Term("x", c, "square", 0.5 + 0.1 * c, 0.1 * c) for c in range(X)], weight=-1.0),
              Group([Term("u", d, "abs", 0.2) for d in range(UE)], weight=-0.5, link="sqrt"),
              Group([Term("x_next", 0, "cos", 1.0), Term("x_next", X - 1, "relu", 0.3, -0.1)], weight=0.25, link="tanh")]
    return TermRewardParams(X, UE, 0.05, groups).vector().to(dev)


def start_buffer(X, UE, dev, g):
    from mbpo import ops
    rows = torch.randn(48, 2 * X + UE + 2, generator=g)
    rows[:, :X] *= 0.4
    data, state = torch.zeros(64, rows.shape[1], device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
    ops.replay_insert(data, state, rows.to(dev).contiguous())
    return data, state


def rollout_case(dev, hidden, X, UE, reward, box=False, hal=False, ta=False, ts1=False, seed=0):
    from mbpo import _hip, ops
    g = torch.Generator().manual_seed(1000 + seed)
    A = UE + X if hal else (UE + 1 if ta else UE)
    pdims, ddims = [X, *hidden, 2 * A], [X + UE, *hidden, 2 * X + (2 if reward == "learned" else 0)]
    kw = dict(policy_params=(lecun_flat(pdims, g) * 0.7).to(dev), policy_spec=ops.MlpSpec(pdims, "swish", 1), x_dim=X, u_dim=A,
              system_kind=_hip.SYS_ENSEMBLE, dyn_params=(lecun_flat(ddims, g, E) * 0.5).to(dev), dyn_spec=ops.MlpSpec(ddims, "swish", E),
              ens_mode=_hip.ENS_TS1 if ts1 else _hip.ENS_MEAN, ens_sample_noise=ts1, seed=7 + seed, offset=3)
    if reward == "terms":
        kw.update(reward_kind=_hip.REWARD_TERMS, reward_params=term_table(X, UE, dev))
    elif reward == "learned":
        kw.update(reward_kind=_hip.REWARD_LEARNED, reward_params=None)
    else:
        kw.update(reward_kind=_hip.REWARD_QUADRATIC, reward_params=torch.rand(2 * X + UE, generator=g).to(dev))
    if hal:
        kw.update(halluc_beta=(torch.rand(X, generator=g) + 0.5).to(dev))
    if ta:
        kw.update(HOLD)
    if box:
        data, state = start_buffer(X, UE, dev, g)
        kw.update(term_low=torch.full((X,), -0.8, device=dev), term_high=torch.full((X,), 0.8, device=dev), start_rows=data, start_state=state)
    obs, first = (torch.rand(N, X, generator=g) * 2 - 1).to(dev), (torch.rand(N, X, generator=g) - 0.5).to(dev)
    steps, done = (torch.arange(N) % L).float().to(dev), (torch.rand(N, generator=g) < 0.2).float().to(dev)
    rows = ops.model_rollout(obs=obs, first_obs=first, steps=steps, done=done, n_steps=S, episode_length=L, **kw)
    torch.cuda.synchronize()
    return dict(rows=sha(rows), state=sha(obs, first, steps, done))


def openloop_case(dev, start, seed):
    from mbpo import _hip, ops
    g = torch.Generator().manual_seed(2000 + seed)
    kw = dict(x_dim=3, u_dim=1, actions=(torch.rand(S, N, 1, generator=g) * 2 - 1).to(dev), system_kind=_hip.SYS_PENDULUM,
              sys_params=torch.tensor([8.0, 2.0, 0.05, 9.81, 1.0, 1.0], device=dev), reward_kind=_hip.REWARD_PENDULUM,
              reward_params=torch.tensor([1.0, 0.02, 0.0], device=dev), seed=11, offset=5)
    if start:
        data, state = start_buffer(3, 1, dev, g)
        kw.update(start_rows=data, start_state=state)
    th = torch.rand(N, generator=g) * 6.28
    obs = torch.stack([torch.cos(th), torch.sin(th), torch.randn(N, generator=g)], 1).to(dev)
    first, steps, done = obs.clone(), (torch.arange(N) % L).float().to(dev), torch.zeros(N, device=dev)
    rows = ops.model_rollout(obs=obs, first_obs=first, steps=steps, done=done, n_steps=S, episode_length=L, **kw)
    torch.cuda.synchronize()
    return dict(rows=sha(rows), state=sha(obs, first, steps, done))


def ens_case(dev, H, seed):
    from mbpo import ops
    g = torch.Generator().manual_seed(3000 + seed)
    dims = [5, H, H, 8]
    y = ops.ensemble_mlp_forward((lecun_flat(dims, g, E) * 0.8).to(dev), ops.MlpSpec(dims, "swish", E), torch.randn(N, 5, generator=g).to(dev))
    torch.cuda.synchronize()
    return dict(rows=sha(y))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out, seed = {}, 0
    nets = {"64": ((64, 64), 3, 2), "64wide": ((64, 64), 10, 8), "128": ((128, 128), 3, 2), "256": ((256, 256), 3, 2)}
    for net, (hidden, X, UE) in nets.items():
        for reward in ("formula", "learned", "terms"):
            for form in ("plain", "box_start", "hal", "ta", "ta_box_start", "ts1"):
                if net == "64wide" and form.startswith("ta"):
                    continue      # refused: no k_model_rollout64<WIDE, TA>
                seed += 1
                out[f"rollout_{net}_{reward}_{form}"] = rollout_case(dev, hidden, X, UE, reward, box="box" in form, hal=form == "hal",
                                                                     ta=form.startswith("ta"), ts1=form == "ts1", seed=seed)
    for start in (False, True):
        out[f"openloop_pendulum_{'start' if start else 'plain'}"] = openloop_case(dev, start, int(start))
    for H in (64, 128, 256):
        out[f"ensemble_forward_{H}"] = ens_case(dev, H, H)
    res = dict(library=os.environ.get("MBPO_HIP_LIB", "in-tree"), digests=out)
    txt = json.dumps(res, indent=1, sort_keys=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
