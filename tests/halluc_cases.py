"""Hallucinated-control rollout cases shared by tests/test_cpu_hallucinated.py and tests/test_gpu_hallucinated.py: the inputs, the
reference run of tests/halluc_ref.py (computed once per case and dtype, and left unchanged) and the device run.

Every parity case: N = 40 envs (three 16-row tiles, the last one ragged), episode_length 3 (resets fall inside the launch), initial
steps = env % 3, a few envs entering already done.  Members and policy are lecun-initialised (oracle.nets.init_mlp_flat) with small
non-zero biases, so that the members disagree: the optimistic term beta * sd * eta is two orders above the comparison's tolerance.
"""
from __future__ import annotations

import functools

import torch

from oracle import nets as onets
from oracle import rollout as oro
from oracle import systems as osys

import fresh_start_cases as fc
import fresh_start_ref as fref
import halluc_ref as href
import termination_ref as tref

ATOL = 2e-4            # the project's rollout tolerance (tests/test_gpu_rollout.py: atol = rtol = 2e-4 for S <= 5)
N, L = 40, 3
SEED, OFFSET = 4321, (5 << 32) + 2      # Philox key of the start-buffer draws (case 4)

_C = dict(N=N, L=L, S=4, AR=1, hidden=(64, 64, 64), E=5, ppo=False, env_major=False, normalize=False, reward="quadratic",
          beta="per_dim", term=False, start=False, elites=None, seed=0)
CASES = {
    # 1: k_model_rollout64; input width x + u_env = 5 is no multiple of 4 (the eta columns sit where the input tile's padding was)
    "c1_64_x3_u2": dict(_C, X=3, UE=2),
    # 2: k_model_rollout<128>, action_repeat 2 (eta held, sd recomputed at the inner step)
    "c2_128_x5_ar2": dict(_C, X=5, UE=1, E=3, hidden=(128, 128), AR=2, seed=1),
    # 3: the PPO layout: log_prob over all A dims, raw_action, env-major rows, normaliser on
    "c3_ppo_x4": dict(_C, X=4, UE=1, S=5, ppo=True, env_major=True, normalize=True, seed=2),
    # 4: the three other flags together: learned reward (2x + 2), a termination box, a start buffer
    "c4_lr_term_start": dict(_C, X=3, UE=1, reward="learned", term=True, start=True, beta=1.0, seed=3),
    # 5: a 3-elite subset of 5 members (the kernels see E = 3): the members, in elite order, that mbpo_ens_pick_elites picks
    "c5_elites": dict(_C, X=3, UE=2, elites=(3, 0, 4), seed=4),
}
ELITE_SCORE = (0.2, 0.9, 0.7, 0.1, 0.3)      # members 3, 0, 4 have the lowest score, in that order
TERM_BOX = ([-1.15, -float("inf"), -float("inf")], [1.15, float("inf"), float("inf")])      # case 4: a box on x_0


class _Gather64:
    """oracle.replay.UniformSamplingQueue whose gathered rows are float64 (the same values)."""

    def __init__(self, queue):
        self.queue = queue

    def gather(self, qstate, idx):
        return self.queue.gather(qstate, idx).astype("float64")


def member_params(dims, E, g) -> torch.Tensor:
    return torch.cat([onets.init_mlp_flat(dims, g) + 0.05 * torch.randn(onets.n_params(dims), generator=g) for _ in range(E)])


@functools.lru_cache(maxsize=None)
def build(name: str) -> dict:
    c = CASES[name]
    X, UE, E, S, AR = c["X"], c["UE"], c["E"], c["S"], c["AR"]
    A = UE + X
    g = torch.Generator().manual_seed(1000 + c["seed"])
    pdims = [X, *c["hidden"], 2 * A]
    ddims = [X + UE, *c["hidden"], 2 * X + (2 if c["reward"] == "learned" else 0)]
    ppar = onets.init_mlp_flat(pdims, g) + 0.02 * torch.randn(onets.n_params(pdims), generator=g)
    dpar = member_params(ddims, E, g)
    beta = torch.rand(X, generator=g) * 1.5 + 0.5 if c["beta"] == "per_dim" else torch.full((X,), float(c["beta"]))
    tgt, q, r = torch.randn(X, generator=g), torch.rand(X, generator=g), torch.rand(UE, generator=g) * 0.1
    if c["start"]:      # pendulum-shaped states: the true buffer of tests/fresh_start_cases.py's "pendulum" case
        obs0, first = fc._pendulum_obs(N, g, 2.0), fc._pendulum_obs(N, g, 2.0)
    else:
        obs0, first = torch.randn(N, X, generator=g), torch.randn(N, X, generator=g)
    out = dict(c, A=A, pdims=pdims, ddims=ddims, ppar=ppar, dpar=dpar, beta=beta, rparams=torch.cat([tgt, q, r]),
               obs0=obs0, first=first, steps0=(torch.arange(N) % L).float(), done0=(torch.rand(N, generator=g) < 0.2).float(),
               pnoise=torch.randn(S, N, A, generator=g),
               nm=torch.randn(X, generator=g) * 0.3 if c["normalize"] else None,
               ns=torch.rand(X, generator=g) + 0.5 if c["normalize"] else None)
    return out


def ref_system(name: str, dtype=torch.float32):
    """The restatement of case `name` in `dtype` (case 5: over the elite members, in elite order)."""
    b = build(name)
    X, UE, E = b["X"], b["UE"], b["E"]
    dpar = b["dpar"]
    if b["elites"] is not None:
        P = onets.n_params(b["ddims"])
        dpar = torch.cat([dpar[e * P:(e + 1) * P] for e in b["elites"]])
        E = len(b["elites"])
    tgt, q, r = b["rparams"][:X], b["rparams"][X:2 * X], b["rparams"][2 * X:]
    rfn = lambda x, u: osys.quadratic_reward(x, u, tgt.to(x.dtype), q.to(x.dtype), r.to(x.dtype))
    sysm = href.HallucinatedEnsembleSystem(dpar, b["ddims"], E, X, UE, b["beta"], learned_reward=b["reward"] == "learned", reward_fn=rfn)
    return sysm if dtype == torch.float32 else sysm.double()


@functools.lru_cache(maxsize=None)
def oracle(name: str, dtype=torch.float32) -> dict:
    """The reference run: rows [S*N, D], the final state, the kept-env mask (case 4: envs never within 10 * ATOL of the box) and the
    mean of |beta * sd * eta| over every (env, step, dimension) the run visited."""
    b = build(name)
    c = lambda t: None if t is None else t.to(dtype)
    sysm = ref_system(name, dtype)
    terms = []
    inner_step = sysm.step

    def recording_step(x, a, **kw):
        _, sd, _ = sysm.spread(x, a[:, :sysm.u_env])
        terms.append((sysm.beta.to(x.dtype) * sd * a[:, sysm.u_env:]).abs())
        return inner_step(x, a, **kw)

    sysm.step = recording_step
    run = sysm
    if b["term"]:
        run = tref.TerminatingSystem(sysm, *TERM_BOX)
    st0 = oro.EnvState(c(b["obs0"]), c(b["first"]), c(b["steps0"]), c(b["done0"]))
    kw = dict(action_repeat=b["AR"], norm_mean=c(b["nm"]), norm_std=c(b["ns"]), policy_noise=c(b["pnoise"]), ppo_extras=b["ppo"],
              env_major=b["env_major"])
    if b["start"]:
        queue, qstate = fc.oracle_buffer("pendulum")
        if dtype == torch.float64:      # (fresh_start_ref writes the gathered rows into first_obs: they must come in its dtype)
            queue = _Gather64(queue)
        st, rows, draws = fref.rollout(run, c(b["ppar"]), b["pdims"], st0, b["S"], b["L"], queue=queue, qstate=qstate, seed=SEED,
                                       offset=OFFSET, **kw)
        assert len(draws) > 0
    else:
        st, rows = oro.rollout(run, c(b["ppar"]), b["pdims"], st0, b["S"], b["L"], **kw)
    keep = torch.ones(N, dtype=torch.bool)
    if b["term"]:
        keep = tref.check_oracle_run(run, rows[:, -1], last_of=b["AR"]) if dtype == torch.float32 else ~run.near_mask()
    return dict(rows=rows, state=st, keep=keep, term_mean=float(torch.cat(terms).mean()))


def env_rows(rows: torch.Tensor, name: str) -> torch.Tensor:
    """[N, S, D] whatever the case's row order."""
    b = build(name)
    r = rows.reshape(N, b["S"], -1) if b["env_major"] else rows.reshape(b["S"], N, -1).permute(1, 0, 2)
    return r


def run_device(name: str, dev, **override):
    """Case `name` through ops.model_rollout (case 5: through EnsembleSystem.rollout_spec with elites selected).
    Returns (rows, obs, first_obs, steps, done) as host tensors."""
    from mbpo import _hip, ops
    b = build(name)
    X, A, E = b["X"], b["A"], b["E"]
    d = lambda t: None if t is None else t.to(dev)
    obs, first, steps, done = d(b["obs0"]).clone(), d(b["first"]).clone(), d(b["steps0"]).clone(), d(b["done0"]).clone()
    kw = dict(system_kind=_hip.SYS_ENSEMBLE, dyn_params=d(b["dpar"]), dyn_spec=ops.MlpSpec(b["ddims"], "swish", E), ens_mode=_hip.ENS_MEAN,
              ens_predict_delta=True, reward_kind=_hip.REWARD_LEARNED if b["reward"] == "learned" else _hip.REWARD_QUADRATIC,
              reward_params=None if b["reward"] == "learned" else d(b["rparams"]), halluc_beta=d(b["beta"]))
    if b["elites"] is not None:
        from mbpo.systems import EnsembleDynamics, EnsembleSystem, SystemParams
        from mbpo.systems.rewards.pendulum_reward import QuadraticReward, QuadraticRewardParams
        UE = b["UE"]
        dyn = EnsembleDynamics(X, UE, n_members=E, hidden_layer_sizes=b["hidden"], device=dev)
        dp = dyn.select_elites(dyn.from_logical_params(b["dpar"]), torch.tensor(ELITE_SCORE), len(b["elites"]))
        assert dp.elite_idx.tolist() == list(b["elites"])
        system = EnsembleSystem(dyn, QuadraticReward(X, UE), mode="optimistic", beta=b["beta"])
        rp = b["rparams"]
        rparams = QuadraticRewardParams(target=rp[:X].tolist(), q=rp[X:2 * X].tolist(), r=rp[2 * X:].tolist())
        assert system.action_dim == A and system.u_dim == UE
        kw = system.rollout_spec(SystemParams(dynamics_params=dp, reward_params=rparams, key=0), dev)
        assert kw["dyn_spec"].n_nets == len(b["elites"]) and kw["halluc_beta"] is not None
    if b["term"]:
        kw.update(term_low=torch.tensor(TERM_BOX[0], device=dev), term_high=torch.tensor(TERM_BOX[1], device=dev))
    if b["start"]:
        data, state = fc.device_buffer("pendulum", dev)
        kw.update(start_rows=data, start_state=state, seed=SEED, offset=OFFSET)
    kw.update(override)
    rows = ops.model_rollout(policy_params=d(b["ppar"]), policy_spec=ops.MlpSpec(b["pdims"], "swish", 1), x_dim=X, u_dim=A, obs=obs,
                             first_obs=first, steps=steps, done=done, n_steps=b["S"], episode_length=b["L"], action_repeat=b["AR"],
                             norm_mean=d(b["nm"]), norm_std=d(b["ns"]), ppo_extras=b["ppo"], env_major=b["env_major"],
                             policy_noise=d(b["pnoise"]), **kw)
    torch.cuda.synchronize()
    return rows.cpu(), obs.cpu(), first.cpu(), steps.cpu(), done.cpu()
