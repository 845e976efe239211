"""GPU: the term reward (MBPO_REWARD_TERMS, include/mbpo_hip.h "term rewards") — mbpo_reward_eval against the restatement, the tile
rollouts against oracle/rollout.py in every option the kind runs under, the reward column against mbpo_reward_eval bit for bit, the
non-finite rule, BPTT's gradient against torch autograd, and the trainers / planners on EnsembleSystem(dyn, TermReward).

Tolerances are the project's (tests/test_gpu_rollout.py): one evaluation fp32 against fp64 atol = rtol = 2e-5; rollout rows at S <= 5
atol = rtol = 2e-4.  Every row of every rollout case is compared: the cases' boxes and holds are chosen so that no decision of the
reference run lies near its threshold (asserted on the reference run, before any device result is looked at).
"""
import functools

import numpy as np
import pytest
import torch

from oracle import nets as onets
from oracle import replay as oreplay
from oracle import rollout as oro

import fresh_start_ref as fref
import term_reward_cases as tc
import term_reward_ref as tr
import termination_ref as tref
import time_adaptive_ref as taref

pytestmark = pytest.mark.gpu

EVAL_TOL = 2e-5
ROW_TOL = 2e-4
N, S, E, L = 40, 3, 3, 3            # three tiles, the last one partial; episodes run out inside the launch
INF = float("inf")
BOX = ([-0.7, -INF, -INF, -INF, -0.8], [0.7, INF, INF, INF, 0.8])      # the termination case: a box on x_0 and x_4 of "mixed"
BUF_MAX, BUF_INSERTS, BUF_SAMPLE_POSITION = 37, (20, 20, 10), 5        # the ring of tests/fresh_start_cases.py
START_KEY = (4321, (5 << 32) + 2)
HOLD = taref.Hold(0.05, 0.17, 0.05, 3, gamma=0.97, switch_cost=0.1)    # K = 3


def _table_vec(name, dev):
    rew = tc.make_reward(name)
    return rew.kernel_spec(rew.init_params(0), dev)[1]


# ------------------------------------------------------------------------------------------------ 1. mbpo_reward_eval
@pytest.mark.parametrize("name", sorted(tc.CASES))
def test_reward_eval_against_the_restatement(dev, name):
    from mbpo import _hip, ops
    x, u, xn = tc.eval_inputs(name)
    want = tr.reward(tc.CASES[name], x.double(), u.double(), xn.double())
    got = ops.reward_eval(_hip.REWARD_TERMS, _table_vec(name, dev), x.to(dev), u.to(dev), xn.to(dev)).cpu()
    print(f"{name}: max |eval - fp64| = {float((got.double() - want).abs().max()):.3e}")
    torch.testing.assert_close(got.double(), want, atol=EVAL_TOL, rtol=EVAL_TOL)
    # Reward.__call__ is the same launch; without next-state terms x_next may be left out
    rew = tc.make_reward(name)
    dist, _ = rew(x.to(dev), u.to(dev), rew.init_params(0), xn.to(dev))
    assert torch.equal(dist.mean().cpu(), got) and float(dist.stddev().abs().sum()) == 0
    if not tc.has_next_state_terms(name):
        assert torch.equal(rew(x.to(dev), u.to(dev), rew.init_params(0))[0].mean().cpu(), got)
    # a next state that is not finite reads x
    bad = xn.clone()
    bad[::5, 1] = INF
    bad[2::5, 0] = float("nan")
    got_bad = ops.reward_eval(_hip.REWARD_TERMS, _table_vec(name, dev), x.to(dev), u.to(dev), bad.to(dev)).cpu()
    fixed = torch.where(torch.isfinite(bad).all(dim=1, keepdim=True), bad, x)
    assert torch.equal(got_bad, ops.reward_eval(_hip.REWARD_TERMS, _table_vec(name, dev), x.to(dev), u.to(dev), fixed.to(dev)).cpu())
    assert bool(torch.isfinite(got_bad).all())


def test_reward_eval_quadratic_kind(dev):
    from mbpo import _hip, ops
    x, u, xn = tc.eval_inputs("quadratic")
    want = tr.quadratic(x.double(), u.double(), tc.QUAD_TARGET, tc.QUAD_Q, tc.QUAD_R)
    rp = torch.tensor(tc.QUAD_TARGET + tc.QUAD_Q + tc.QUAD_R, device=dev)
    got = ops.reward_eval(_hip.REWARD_QUADRATIC, rp, x.to(dev), u.to(dev)).cpu()
    torch.testing.assert_close(got.double(), want, atol=EVAL_TOL, rtol=EVAL_TOL)
    terms = ops.reward_eval(_hip.REWARD_TERMS, _table_vec("quadratic", dev), x.to(dev), u.to(dev)).cpu()
    torch.testing.assert_close(terms, got, atol=EVAL_TOL, rtol=EVAL_TOL)
    with pytest.raises(_hip.MbpoHipError):
        ops.reward_eval(_hip.REWARD_PENDULUM, rp, x.to(dev), u.to(dev))


def test_reward_eval_garbage_table_reads_nothing_outside(dev):
    """Counts above the capacities, a z_index of 1e6, negative and NaN ones, ids of 99, a group range past the table: the rows come out
    finite and equal to the restatement with those terms and groups dropped, with NaN guards around the table and around every input
    (a read outside would surface as NaN) and the guards around `out` untouched."""
    from mbpo import _hip, ops
    X, U, bias, groups = tc.MIXED
    x, u, xn = tc.eval_inputs("mixed")
    v = tc.make_reward("mixed").init_params(0).vector()
    T0 = 4 + 64
    v[0], v[1] = 1000.0, 1.0e6                         # counts above the capacities
    v[T0 + 4 * 1 + 0] = 1.0e6                          # term 1 (u_0 square): z_index far outside
    v[T0 + 4 * 3 + 0] = -5.0                           # term 3 (x_0 square under the sqrt): negative z_index
    v[T0 + 4 * 6 + 0] = float("nan")                   # term 6 (x_next_1 under the exp)
    v[T0 + 4 * 8 + 1] = 99.0                           # term 8 (sin): unknown fn
    v[4 + 4 * 5 + 1] = 99.0                            # group 5 (tanh): unknown link
    v[4 + 4 * 9:4 + 4 * 10] = torch.tensor([1.0, 0.0, 1000.0, 1000.0])      # group 9: a range past the table (clamped to nothing)
    v[4 + 4 * 10:4 + 4 * 11] = torch.tensor([0.5, 0.0, 120.0, 1000.0])      # group 10: terms 120 .. 127, all-zero records: 0.5 * 8 * 0 * x_0
    dropped = {1, 3, 6, 8}
    kept, k = [], 0
    for gi, (w, link, terms) in enumerate(groups):
        ts = []
        for t in terms:
            if k not in dropped:
                ts.append(t)
            k += 1
        if gi != 5:
            kept.append((w, link, ts))
    want = tr.reward((X, U, bias, kept), x.double(), u.double(), xn.double())
    G = 64
    nan = lambda *shape: torch.full(shape, float("nan"))
    guard = lambda t: torch.cat([nan(G, *t.shape[1:]), t, nan(G, *t.shape[1:])]).to(dev)
    tab, xg, ug, ng = guard(v), guard(x), guard(u), guard(xn)
    out = torch.full((tc.N_EVAL + 2 * G,), -7.0, device=dev)
    n = tc.N_EVAL
    ops.reward_eval(_hip.REWARD_TERMS, tab[G:G + v.numel()], xg[G:G + n], ug[G:G + n], ng[G:G + n], out=out[G:G + n])
    torch.cuda.synchronize()
    got = out.cpu()
    assert bool((got[:G] == -7.0).all()) and bool((got[G + n:] == -7.0).all())
    assert bool(torch.isfinite(got[G:G + n]).all())
    torch.testing.assert_close(got[G:G + n].double(), want, atol=EVAL_TOL, rtol=EVAL_TOL)


# ------------------------------------------------------------------------------------------------ 2. rollouts against oracle/rollout.py
_R = dict(name="mixed", hidden=(64, 64, 64), mode="mean", noise=False, AR=1, term=False, hal=False, ta=False, seed=0)
ROLLOUTS = {
    "mixed_64_mean": dict(_R),
    "mixed_128_mean": dict(_R, hidden=(128, 128), seed=1),
    "wide_64_mean": dict(_R, name="wide", seed=2),                       # k_model_rollout64<WIDE>: 23 inputs, 34 outputs
    "mixed_64_ts1_noise": dict(_R, mode="ts1", noise=True, seed=3),
    "mixed_128_ts1_noise": dict(_R, hidden=(128, 128), mode="ts1", noise=True, seed=4),
    "mixed_64_ar2": dict(_R, AR=2, seed=5),                              # the copy of the next state that starts the second inner step
    "mixed_128_ar2": dict(_R, hidden=(128, 128), AR=2, mode="ts1", noise=True, seed=6),
    "mixed_64_term_start": dict(_R, term=True, seed=7),                  # a termination box with a start buffer
    "mixed_64_hal": dict(_R, hal=True, seed=8),                          # hallucinated control: the reward sees the hallucinated x'
    "mixed_128_hal": dict(_R, hal=True, hidden=(128, 128), seed=9),
    "mixed_64_ta_k3": dict(_R, ta=True, mode="ts1", noise=True, seed=8),       # (a seed whose hold decisions all lie away from an integer)
    "mixed_128_ta_k3": dict(_R, ta=True, hidden=(128, 128), seed=11),
}


def _buffer_rows(X, U):
    g = torch.Generator().manual_seed(103)
    rows = torch.randn(sum(BUF_INSERTS), 2 * X + U + 2, generator=g)
    rows[:, :X] = 0.4 * torch.randn(rows.shape[0], X, generator=g)
    return rows


@functools.lru_cache(maxsize=None)
def _build(case: str) -> dict:
    c = ROLLOUTS[case]
    table = tc.CASES[c["name"]]
    X, UE = table[0], table[1]
    A = UE + X if c["hal"] else (UE + 1 if c["ta"] else UE)
    inner = HOLD.K if c["ta"] else c["AR"]
    g = torch.Generator().manual_seed(2000 + c["seed"])
    pdims, ddims = [X, *c["hidden"], 2 * A], [X + UE, *c["hidden"], 2 * X]
    ppar = onets.init_mlp_flat(pdims, g) + 0.02 * torch.randn(onets.n_params(pdims), generator=g)
    dpar = torch.cat([onets.init_mlp_flat(ddims, g) * 0.5 + 0.03 * torch.randn(onets.n_params(ddims), generator=g) for _ in range(E)])
    out = dict(c, table=table, X=X, UE=UE, A=A, pdims=pdims, ddims=ddims, ppar=ppar, dpar=dpar,
               obs0=torch.rand(N, X, generator=g) * 2 - 1, first=(torch.rand(N, X, generator=g) * 2 - 1) * 0.5,
               steps0=(torch.arange(N) % L).float(), done0=(torch.rand(N, generator=g) < 0.2).float(),
               pnoise=torch.randn(S, N, A, generator=g),
               mnoise=torch.randn(S, inner, N, X, generator=g) if c["noise"] else None,
               midx=torch.randint(0, E, (S, inner, N), generator=g, dtype=torch.int32) if c["mode"] == "ts1" else None,
               beta=torch.rand(X, generator=g) * 1.5 + 0.5 if c["hal"] else None)
    return out


def _ref_system(b):
    if b["hal"]:
        return tr.TermHallucinatedSystem(b["table"], b["dpar"], b["ddims"], E, b["beta"])
    return tr.TermEnsembleSystem(b["table"], b["dpar"], b["ddims"], E, mode=b["mode"], predict_delta=True, sample_noise=b["noise"], min_std=1e-3)


def _oracle_queue(X, U):
    rows = _buffer_rows(X, U).numpy()
    q = oreplay.UniformSamplingQueue(BUF_MAX, rows.shape[1], 1)
    st, at = q.init(), 0
    for n in BUF_INSERTS:
        st = q.insert(st, rows[at:at + n])
        at += n
    st["sample_position"] = np.int32(BUF_SAMPLE_POSITION)
    return q, st


@functools.lru_cache(maxsize=None)
def _oracle(case: str) -> dict:
    """The reference run in fp32, computed once per case and left unchanged: rows [S*N, D] and the final EnvState."""
    b = _build(case)
    sysm = _ref_system(b)
    st0 = oro.EnvState(b["obs0"], b["first"], b["steps0"], b["done0"])
    if b["ta"]:
        out = taref.rollout(sysm, b["UE"], HOLD, b["ppar"], b["pdims"], st0, S, L, policy_noise=b["pnoise"], model_noise=b["mnoise"],
                            member_idx=b["midx"])
        acts = out["rows"].reshape(S, N, -1)[..., b["X"]:b["X"] + b["A"]]
        assert float(taref.integer_distance(acts, b["UE"], HOLD).min()) >= 2e-3, "a hold decision of the reference run lies near an integer"
        assert set(out["k"].reshape(-1).tolist()) == {1, 2, 3}
        return dict(rows=out["rows"], state=out["state"])
    kw = dict(action_repeat=b["AR"], policy_noise=b["pnoise"], model_noise=b["mnoise"], member_idx=b["midx"])
    if b["term"]:
        run = tref.TerminatingSystem(sysm, *BOX)
        q, qs = _oracle_queue(b["X"], b["UE"])
        st, rows, draws = fref.rollout(run, b["ppar"], b["pdims"], st0, S, L, queue=q, qstate=qs, seed=START_KEY[0], offset=START_KEY[1], **kw)
        assert len(draws) > 0 and not bool(run.near_mask().any()), "an env of the reference run comes within the margin of the box"
        assert int(run.terminated_mask(b["AR"]).sum()) >= 4
        return dict(rows=rows, state=st)
    st, rows = oro.rollout(sysm, b["ppar"], b["pdims"], st0, S, L, **kw)
    return dict(rows=rows, state=st)


def _device_kwargs(b, dev, reward="terms"):
    from mbpo import _hip, ops
    d = lambda t: None if t is None else t.to(dev)
    kw = dict(policy_params=d(b["ppar"]), policy_spec=ops.MlpSpec(b["pdims"], "swish", 1), x_dim=b["X"], u_dim=b["A"],
              system_kind=_hip.SYS_ENSEMBLE, dyn_params=d(b["dpar"]), dyn_spec=ops.MlpSpec(b["ddims"], "swish", E),
              ens_mode={"mean": _hip.ENS_MEAN, "ts1": _hip.ENS_TS1}[b["mode"]], ens_predict_delta=True, ens_sample_noise=b["noise"],
              ens_min_std=1e-3, action_repeat=b["AR"])
    if reward == "terms":
        kw.update(reward_kind=_hip.REWARD_TERMS, reward_params=_table_vec(b["name"], dev))
    else:
        kw.update(reward_kind=_hip.REWARD_QUADRATIC, reward_params=torch.rand(2 * b["X"] + b["UE"], generator=torch.Generator().manual_seed(1)).to(dev))
    if b["hal"]:
        kw.update(halluc_beta=d(b["beta"]))
    if b["ta"]:
        kw.update(hold_max_steps=HOLD.K, hold_min_time=HOLD.t_lo, hold_max_time=HOLD.t_hi, hold_dt=HOLD.dt, hold_gamma=HOLD.gamma,
                  hold_switch_cost=HOLD.switch_cost)
    if b["term"]:
        from mbpo import ops as _ops
        rows = _buffer_rows(b["X"], b["UE"]).to(dev)
        data, state = torch.zeros(BUF_MAX, rows.shape[1], device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
        at = 0
        for n in BUF_INSERTS:
            _ops.replay_insert(data, state, rows[at:at + n].contiguous())
            at += n
        state[1] = BUF_SAMPLE_POSITION
        kw.update(term_low=torch.tensor(BOX[0], device=dev), term_high=torch.tensor(BOX[1], device=dev), start_rows=data, start_state=state,
                  seed=START_KEY[0], offset=START_KEY[1])
    return kw


def _run_device(b, dev, kw, explicit=True, n_steps=S, episode_length=L, **override):
    from mbpo import ops
    d = lambda t: None if t is None else t.to(dev)
    obs, first, steps = d(b["obs0"]).clone(), d(b["first"]).clone(), d(b["steps0"]).clone()
    done = override.pop("done", d(b["done0"])).clone()
    kw = dict(kw)
    if explicit:
        kw.update(policy_noise=d(b["pnoise"]), model_noise=d(b["mnoise"]), member_idx=d(b["midx"]))
    kw.update(override)
    rows = ops.model_rollout(obs=obs, first_obs=first, steps=steps, done=done, n_steps=n_steps, episode_length=episode_length, **kw)
    torch.cuda.synchronize()
    return rows.cpu(), obs.cpu(), first.cpu(), steps.cpu(), done.cpu()


@pytest.mark.parametrize("case", list(ROLLOUTS))
def test_rollout_rows_against_the_oracle(dev, case):
    b, ref = _build(case), _oracle(case)
    X, A = b["X"], b["A"]
    rows, obs, first, steps, done = _run_device(b, dev, _device_kwargs(b, dev))
    want, st = ref["rows"], ref["state"]
    D = rows.shape[1]
    print(f"{case}: max |rows - ref| / (1 + |ref|) = {float(((rows - want).abs() / (1 + want.abs())).max()):.3g}; "
          f"reward column {float((rows[:, X + A] - want[:, X + A]).abs().max()):.3g}")
    assert bool(torch.isfinite(rows).all())
    # integer-valued bookkeeping is exact: discount, truncation, steps, done
    assert torch.equal(rows[:, X + A + 1], want[:, X + A + 1]) and torch.equal(rows[:, D - 1], want[:, D - 1])
    assert torch.equal(steps, st.steps) and torch.equal(done, st.done)
    torch.testing.assert_close(rows, want, atol=ROW_TOL, rtol=ROW_TOL)            # every row, every column
    torch.testing.assert_close(obs, st.obs, atol=ROW_TOL, rtol=ROW_TOL)
    assert int((want[:, X + A + 1] == 0).sum()) > 0                               # resets inside the launch
    assert float(want[:, X + A].abs().min()) > 0 and float(want[:, X + A].std()) > 0.05
    if b["term"]:
        assert torch.equal(first, st.first_obs) and not torch.equal(first, b["first"])
    else:
        assert torch.equal(first, b["first"])


# ------------------------------------------------------------------------------------------------ 3. bits
BITS = ["mixed_64_mean", "mixed_128_mean", "wide_64_mean", "mixed_64_ts1_noise", "mixed_128_ts1_noise", "mixed_64_hal", "mixed_128_hal"]


@pytest.mark.parametrize("case", BITS)
def test_reward_column_is_reward_eval_bit_for_bit(dev, case):
    """Nothing resets (episode_length 2^30) and action_repeat is 1, so a row's next_observation is the step's own next state: the
    reward column equals mbpo_reward_eval on the rows' own (obs, action[:UE], next_obs) columns, for every row.  Philox draws."""
    from mbpo import _hip, ops
    b = _build(case)
    X, A, UE = b["X"], b["A"], b["UE"]
    rows = _run_device(b, dev, _device_kwargs(b, dev), explicit=False, episode_length=2 ** 30, seed=11, offset=(2 << 32) + 1,
                       done=torch.zeros(N, device=dev))[0]
    assert bool((rows[:, X + A + 1] == 1).all())
    r = rows.to(dev)
    want = ops.reward_eval(_hip.REWARD_TERMS, _table_vec(b["name"], dev), r[:, :X].contiguous(), r[:, X:X + UE].contiguous(),
                           r[:, X + A + 2:2 * X + A + 2].contiguous()).cpu()
    assert torch.equal(rows[:, X + A].view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("case", ["mixed_64_mean", "mixed_128_ts1_noise", "mixed_64_ar2", "mixed_64_term_start", "mixed_64_hal", "mixed_64_ta_k3"])
def test_every_other_column_equals_the_quadratic_rewards_run(dev, case):
    """The reward never feeds back into the state: with the same seeds every column but the reward is the QuadraticReward run's, bits."""
    b = _build(case)
    X, A = b["X"], b["A"]
    terms = _run_device(b, dev, _device_kwargs(b, dev))
    quad = _run_device(b, dev, _device_kwargs(b, dev, reward="quadratic"))
    keep = [c for c in range(terms[0].shape[1]) if c != X + A]
    assert torch.equal(terms[0][:, keep], quad[0][:, keep])
    assert not torch.equal(terms[0][:, X + A], quad[0][:, X + A])
    for a, q in zip(terms[1:], quad[1:]):
        assert torch.equal(a, q)


@pytest.mark.parametrize("hidden", [(64, 64, 64), (128, 128)])
def test_from_quadratic_agrees_with_the_quadratic_kind(dev, hidden):
    """At 2e-5, not bits: the quadratic kernel fuses its multiply-adds, the table rounds every product."""
    from mbpo import _hip
    from mbpo.systems import TermReward
    b = dict(_build("mixed_64_mean" if hidden[0] == 64 else "mixed_128_mean"), AR=2)
    X, A = b["X"], b["A"]
    kw = _device_kwargs(b, dev)
    rew = TermReward.from_quadratic(tc.QUAD_TARGET, tc.QUAD_Q, tc.QUAD_R)
    kw.update(reward_params=rew.kernel_spec(rew.init_params(0), dev)[1])
    terms = _run_device(b, dev, kw)[0]
    kw.update(reward_kind=_hip.REWARD_QUADRATIC, reward_params=torch.tensor(tc.QUAD_TARGET + tc.QUAD_Q + tc.QUAD_R, device=dev))
    quad = _run_device(b, dev, kw)[0]
    torch.testing.assert_close(terms[:, X + A], quad[:, X + A], atol=EVAL_TOL, rtol=EVAL_TOL)
    assert float(quad[:, X + A].abs().max()) > 0.1


# ------------------------------------------------------------------------------------------------ 4. the non-finite rule
@pytest.mark.parametrize("hidden", [(64, 64, 64), (128, 128)])
def test_a_diverging_member_leaves_the_reward_finite(dev, hidden):
    """One member's last-layer bias is +inf in 'ts1' with a termination box: the rows that drew it are terminal (discount 0), their
    reward is finite and equals mbpo_reward_eval with x_next = x, bit for bit; all other rows are those of the run without the poison.
    (The divergence the termination's finiteness check exists for; nothing faults.)"""
    from mbpo import _hip, ops
    b = dict(_build("mixed_64_ts1_noise" if hidden[0] == 64 else "mixed_128_ts1_noise"))
    X, A, UE = b["X"], b["A"], b["UE"]
    P = onets.n_params(b["ddims"])
    poisoned = b["dpar"].clone()
    poisoned[1 * P + P - 2 * X + 2] = INF                      # member 1, output bias of mean column 2
    box = dict(term_low=torch.full((X,), -1.0e6, device=dev), term_high=torch.full((X,), 1.0e6, device=dev))
    kw = dict(_device_kwargs(b, dev), **box)
    run = lambda par: _run_device(b, dev, dict(kw, dyn_params=par.to(dev)), n_steps=1, episode_length=2 ** 30,
                                  policy_noise=b["pnoise"][:1].to(dev), model_noise=b["mnoise"][:1].to(dev), member_idx=b["midx"][:1].to(dev))
    clean, bad = run(b["dpar"])[0], run(poisoned)[0]
    hit = b["midx"][0, 0] == 1
    assert 5 <= int(hit.sum()) <= N - 5
    assert bool(torch.isfinite(bad).all())
    assert bool((bad[hit][:, X + A + 1] == 0).all()) and bool((bad[~hit][:, X + A + 1] == 1).all())
    assert torch.equal(bad[~hit], clean[~hit])
    r = bad.to(dev)
    want = ops.reward_eval(_hip.REWARD_TERMS, _table_vec("mixed", dev), r[:, :X].contiguous(), r[:, X:X + UE].contiguous(), None).cpu()
    assert torch.equal(bad[hit][:, X + A].view(torch.int32), want[hit].view(torch.int32))
    assert torch.equal(bad[hit][:, X + A + 2:2 * X + A + 2], b["first"][hit])      # the reset ran: the infinity never left the kernel


# ------------------------------------------------------------------------------------------------ 5. BPTT
def _bptt_setup(hidden):
    import test_gpu_bptt as tb
    X, U, H, n, Em = 17, 6, 8, 16, 10            # tests/test_gpu_bptt.py's quadratic-reward case at x = 17
    cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, _tsys, extra = tb._setup(X, U, H, n, "ensemble", Em, 0, hidden=hidden)
    x0 = x0.clamp(-1.5, 1.5)
    tsys = tr.TorchTermSystem(tc.WIDE, extra["dp"], extra["dd"], Em)
    tsys64 = tr.TorchTermSystem(tc.WIDE, extra["dp"].double(), extra["dd"], Em)
    import oracle.bptt as obptt
    d = lambda t: t.double()
    g_ref, _, aux = obptt.actor_grads(cfg, tsys, ap, cp, x0, noise, s_mean, s_std, r_ms[0], r_ms[1])
    g64, loss64, aux64 = obptt.actor_grads(cfg, tsys64, d(ap), d(cp), d(x0), d(noise), d(s_mean), d(s_std), d(r_ms[0]), d(r_ms[1]))
    return (cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, extra, X, U, H, n, Em), (g_ref, aux, g64, loss64, aux64)


def test_bptt_fused_gradient_against_autograd(dev):
    """Case "wide", 64 x 3 actor: the fused kernel's actor gradient against torch autograd through the restatement, at the tolerances of
    tests/test_gpu_bptt.py's quadratic-reward case (atol 5e-6 + rtol 2e-3 against fp32, rtol 1e-3 against fp64) on its shapes."""
    import test_gpu_bptt as tb
    from mbpo import _hip, ops
    (cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, extra, X, U, H, n, Em), refs = _bptt_setup((64, 64, 64))
    op = ops.BpttActorGrad(x_dim=X, u_dim=U, horizon=H, actor_dims=cfg.actor_dims, critic_dims=cfg.critic_dims, n=n, device=dev,
                           init_stddev=cfg.init_stddev, discount=cfg.discount, lambda_=cfg.lambda_, ent_coef=cfg.ent_coef, seed=0)
    op(actor_params=ap.to(dev), target_critic_params=cp.to(dev), init_states=x0.to(dev), state_mean=s_mean.to(dev), state_std=s_std.to(dev),
       reward_mean_std=r_ms.to(dev), act_noise=noise.to(dev), system_kind=_hip.SYS_ENSEMBLE, reward_kind=_hip.REWARD_TERMS,
       reward_params=_table_vec("wide", dev), dyn_params=extra["dp"].to(dev), dyn_spec=ops.MlpSpec(extra["dd"], "swish", Em))
    torch.cuda.synchronize()
    tb._assert_matches_oracle(op, refs, X, U, H, n)


def test_bptt_wide_path_gradient_against_autograd(dev):
    """The same case at actor (128, 128): the horizon walked on the host, the reward TermReward's own torch form."""
    from mbpo import ops
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, SystemParams
    from mbpo.systems.torch_steps import DifferentiableBuiltin
    (cfg, ap, cp, x0, noise, s_mean, s_std, r_ms, extra, X, U, H, n, Em), refs = _bptt_setup((128, 128))
    g_ref, aux, g64, loss64, aux64 = refs
    dyn = EnsembleDynamics(X, U, n_members=Em, hidden_layer_sizes=(128, 128), device=dev)
    rew = tc.make_reward("wide")
    system = EnsembleSystem(dyn, rew)
    sp = SystemParams(dynamics_params=dyn.from_logical_params(extra["dp"]), reward_params=rew.init_params(0), key=0)
    spec = system.rollout_spec(sp, dev)
    op = ops.BpttActorGradGeneric(x_dim=X, u_dim=U, horizon=H, actor_dims=cfg.actor_dims, critic_dims=cfg.critic_dims, n=n, device=dev,
                                  init_stddev=cfg.init_stddev, discount=cfg.discount, lambda_=cfg.lambda_, ent_coef=cfg.ent_coef)
    op(actor_params=ap.to(dev), target_critic_params=cp.to(dev), init_states=x0.to(dev), state_mean=s_mean.to(dev), state_std=s_std.to(dev),
       reward_mean_std=r_ms.to(dev), system=DifferentiableBuiltin(system, spec), system_params=sp, act_noise=noise.to(dev))
    torch.cuda.synchronize()
    rows = op.transitions.cpu().reshape(n, H, -1)
    torch.testing.assert_close(rows[..., X + U], aux["reward"], atol=5e-4, rtol=5e-4)
    torch.testing.assert_close(rows[..., X + U + 2:], aux["next_observation"], atol=2e-4, rtol=2e-4)
    g = op.grads.cpu()
    torch.testing.assert_close(g, g_ref, atol=5e-6, rtol=2e-3)
    torch.testing.assert_close(g.double(), g64, atol=5e-6, rtol=1e-3)


def test_bptt_refuses_next_state_terms(dev):
    from mbpo.optimizers.policy_optimizers.bptt_optimizer import BPTTOptimizer
    from mbpo.systems import EnsembleDynamics, EnsembleSystem
    system = EnsembleSystem(EnsembleDynamics(5, 2, n_members=3, device=dev), tc.make_reward("mixed"))
    for feats in ((64, 64, 64), (128, 128)):      # fused and wide
        opt = BPTTOptimizer(obs_dim=5, action_dim=2, horizon=4, num_samples_per_gradient_update=8, train_steps=1, actor_features=feats,
                            sampling_buffer_size=256)
        with pytest.raises(ValueError, match="gradient through next-state terms is not built"):
            opt.set_system(system)


# ------------------------------------------------------------------------------------------------ 6. trainers, planners, System.step
X_, U_, E_ = 5, 2, 5
SAC_KW = dict(num_envs=16, batch_size=32, grad_updates_per_step=2, num_env_steps_between_updates=2, episode_length=6,
              normalize_observations=True, max_replay_size=512, min_replay_size=64, discounting=0.95, lr_policy=3e-4, lr_q=3e-4,
              lr_alpha=3e-4)
PPO_KW = dict(num_envs=16, unroll_length=4, batch_size=8, num_minibatches=2, num_updates_per_batch=2, episode_length=8,
              normalize_observations=True, discounting=0.97, lr=3e-4, entropy_cost=1e-2, policy_hidden_layer_sizes=(64, 64),
              critic_hidden_layer_sizes=(64, 64))


def _system(dev, **kw):
    from mbpo.systems import EnsembleDynamics, EnsembleSystem
    return EnsembleSystem(EnsembleDynamics(X_, U_, n_members=E_, device=dev), tc.make_reward("mixed"), **kw)


def _env(dev, rows=256):
    from mbpo.replay import UniformSamplingQueue
    from mbpo.systems.brax_wrapper import BraxWrapper
    from mbpo.types import Transition
    system = _system(dev, mode="ts1", sample_noise=True)
    sp = system.init_params(1)
    dummy = Transition(observation=torch.zeros(X_), action=torch.zeros(U_), reward=torch.zeros(1), discount=torch.zeros(1),
                       next_observation=torch.zeros(X_))
    tb = UniformSamplingQueue(rows, dummy, 1, device=dev)
    data = 0.5 * torch.randn(rows, 2 * X_ + U_ + 2, generator=torch.Generator().manual_seed(0))
    return BraxWrapper(system, sp, tb.insert_rows(tb.init(0), data.to(dev)), tb)


def test_sac_on_a_term_reward_graph_equals_eager(dev):
    from mbpo.optimizers.policy_optimizers.sac.sac import SAC
    Nn, Ss = SAC_KW["num_envs"], SAC_KW["num_env_steps_between_updates"]

    def run(use_graph):
        env = _env(dev)
        t = SAC(environment=env, num_timesteps=64 + Nn * Ss, use_graph=use_graph, **SAC_KW)
        assert t.num_training_steps_per_epoch == 1 and (t.x_dim, t.u_dim) == (X_, U_)
        ts, es, bs = t.init_training_state(7), t.reset_envs(env, 11, Nn), t.replay_buffer.init(13)
        ts, es, bs, _ = t.prefill_replay_buffer(ts, es, bs, 17)
        graphs, metrics = [], []
        for epoch in range(3):      # one training step each: eager (and captured), replayed, replayed
            if use_graph:
                ts, es, bs, m = t.training_epoch(ts, es, bs, 19 + epoch)
                graphs.append(t._graph)
                metrics += list(m.values())
            else:
                t.updater.metrics_accum.zero_()
                t.rekey(19 + epoch)
                ts, es, bs = t.training_step(ts, es, bs)
                metrics += t.updater.metrics_accum.cpu().tolist()
        if use_graph:
            assert graphs[0] is not None and graphs[1] is graphs[0] and graphs[2] is graphs[0]
        assert all(v == v and abs(v) != INF for v in metrics), metrics
        torch.cuda.synchronize()
        out = dict(params=t.updater.params.cpu().clone(), tq=t.updater.target_q.cpu().clone(), obs=es.obs.cpu().clone(),
                   steps=es.info["steps"].cpu().clone(), stats=t._stats_vec.cpu().clone(), rows=t._rollout_rows.cpu().clone(),
                   data=bs.data.cpu().clone(), rng=t._rng.cpu().clone())
        t.close()
        return out

    eager, graph = run(False), run(True)
    for k, v in eager.items():
        assert torch.isfinite(v.float()).all(), k
        assert torch.equal(v, graph[k]), f"graph replay differs from eager in {k}"
    assert float(eager["rows"][:, X_ + U_].abs().max()) > 0


def test_ppo_on_a_term_reward_graph_equals_eager(dev):
    from mbpo.optimizers.policy_optimizers.ppo.ppo import PPO
    per_step = PPO_KW["batch_size"] * PPO_KW["unroll_length"] * PPO_KW["num_minibatches"]

    def run(use_graph):
        env = _env(dev)
        t = PPO(environment=env, num_timesteps=per_step, use_graph=use_graph, **PPO_KW)
        assert t.num_training_steps_per_epoch == 1 and (t.x_dim, t.u_dim) == (X_, U_)
        ts, es = t.init_training_state(5), env.reset([101 + i for i in range(PPO_KW["num_envs"])])
        graphs, metrics = [], []
        for epoch in range(3):
            if use_graph:
                ts, es, m = t.training_epoch(ts, es, 19 + epoch)
                graphs.append(t._graph)
                metrics += list(m.values())
            else:
                t.updater.metrics_accum.zero_()
                t.rekey(19 + epoch)
                ts, es, _ = t.training_step(ts, es)
                metrics += t.updater.metrics_accum.cpu().tolist()
        if use_graph:
            assert graphs[0] is not None and graphs[1] is graphs[0] and graphs[2] is graphs[0]
        assert all(v == v and abs(v) != INF for v in metrics), metrics
        torch.cuda.synchronize()
        u = t.updater
        out = dict(params=u.params.cpu().clone(), m=u.adam_m.cpu().clone(), obs=es.obs.cpu().clone(), stats=t._stats_vec.cpu().clone(),
                   data=t._data.cpu().clone(), rng=t._rng.cpu().clone())
        t.close()
        return out

    eager, graph = run(False), run(True)
    for k, v in eager.items():
        assert torch.isfinite(v.float()).all(), k
        assert torch.equal(v, graph[k]), f"graph replay differs from eager in {k}"


@pytest.mark.parametrize("mode,noise", [("mean", False), ("ts1", True)])
def test_icem_batched_equals_single_calls(dev, mode, noise):
    """iCEM on EnsembleSystem(dyn, TermReward "mixed"), single and batched: each batched problem is its own single call, bit for bit."""
    from mbpo.optimizers import iCemParams, iCemTO
    from mbpo.utils import keys as K
    H, B = 6, 3
    params = iCemParams(num_particles=2, num_samples=126, num_elites=12, num_steps=3, exponent=1.0, alpha=0.1, init_std=0.6)
    opt = iCemTO(horizon=H, action_dim=U_, opt_params=params, key=5)
    opt.set_system(_system(dev, mode=mode, sample_noise=noise))
    g = torch.Generator().manual_seed(3)
    x0 = (torch.randn(B, X_, generator=g) * 0.5).to(dev)
    warm = ((torch.rand(B, H, U_, generator=g) - 0.5) * 1.5).to(dev)
    bst = opt.init(7, batch_size=B).replace(best_sequence=warm.clone())
    bnew = opt.optimize(x0, bst)
    sst = opt.init(7)
    bits = lambda t: t.detach().contiguous().view(torch.int32)
    for i in range(B):
        one = opt.optimize(x0[i], sst.replace(key=bst.key[i], best_sequence=warm[i].clone()))
        assert torch.equal(bits(bnew.best_sequence[i]), bits(one.best_sequence)), f"problem {i}: best_sequence"
        assert torch.equal(bits(bnew.best_reward[i]), bits(one.best_reward)), f"problem {i}: best_reward"
        assert bnew.key[i] == one.key == K.split(bst.key[i], 2)[1]
    assert bool(torch.isfinite(bnew.best_reward).all()) and len(set(float(v) for v in bnew.best_reward)) == B


def test_system_step_reward_against_the_restatement(dev):
    """System.step (one fused launch, 'mean'): the reward is the table on (x, u, the step's own x_next), at 2e-5 against fp64; a single state is
    the batch's row, and Reward.__call__ on the same columns returns the same bits."""
    system = _system(dev)
    sp = system.init_params(3)
    g = torch.Generator().manual_seed(9)
    x, u = (torch.rand(37, X_, generator=g) * 2 - 1), (torch.rand(37, U_, generator=g) * 2 - 1)
    st = system.step(x.to(dev), u.to(dev), sp)
    assert st.x_next.shape == (37, X_) and not torch.equal(st.x_next.cpu(), x)
    want = tr.reward(tc.MIXED, x.double(), u.double(), st.x_next.cpu().double())
    torch.testing.assert_close(st.reward.cpu().double(), want, atol=EVAL_TOL, rtol=EVAL_TOL)
    one = system.step(x[0].to(dev), u[0].to(dev), sp)
    assert torch.equal(one.reward, st.reward[0]) and torch.equal(one.x_next, st.x_next[0])
    dist, _ = system.reward(x.to(dev), u.to(dev), sp.reward_params, st.x_next)
    assert torch.equal(dist.mean(), st.reward)
