"""GPU: warm start of the SAC and PPO learners across run_training / train() calls (not in the reference, whose SAC and PPO optimizers
start every `train` from a fresh initialisation) — the carry is complete, a resumed call never initialises, the retained replay buffer
is continued, the optimizer keeps its trainer and replays or re-captures its graph by the existing address check, and what does not
fit is refused before anything is copied.

Shapes: those of tests/test_gpu_trainer_parity.py (Pendulum and the x = 4, u = 1, E = 5 ensemble; 64 envs, B = 256, G = 4, 5 env steps
per update, a 1500-row ring: the first call's prefill and 4 steps insert 1600 rows, so the ring has wrapped when it is carried over).
Every comparison is BIT FOR BIT: the tree already guarantees eager == graph replay (test_gpu_trainer_parity), so any difference between a
trainer that ran on and one that was resumed from a LearnerState is something the carry left behind."""
import pytest
import torch

from test_gpu_trainer_parity import PPO_KW, SAC_KW, _make_system, _true_buffer

pytestmark = pytest.mark.gpu

N, S = SAC_KW["num_envs"], SAC_KW["num_env_steps_between_updates"]
G = SAC_KW["grad_updates_per_step"]
SAC_STEPS = 4
SAC_TIMESTEPS = 64 + N * S * SAC_STEPS                          # one prefill step (320 rows) + 4 training steps per epoch
PPO_STEPS = 2
PPO_TIMESTEPS = PPO_STEPS * PPO_KW["batch_size"] * PPO_KW["unroll_length"] * PPO_KW["num_minibatches"]
PPO_UPDATES = PPO_KW["num_updates_per_batch"] * PPO_KW["num_minibatches"]       # optimizer steps per training step
LEARNER_FIELDS = ("params", "target_q", "adam_m", "adam_v", "step_count", "normalizer")


def _env(dev, kind, rows=512):
    from mbpo.systems.brax_wrapper import BraxWrapper
    system, sp, _, X, U = _make_system(dev, kind)
    tb, tbs = _true_buffer(dev, X, U, rows)
    return BraxWrapper(system, sp, tbs, tb)


def _sac(dev, kind, use_graph=True, env=None, **kw):
    from mbpo.optimizers.policy_optimizers.sac.sac import SAC
    env = _env(dev, kind) if env is None else env
    tr = SAC(environment=env, num_timesteps=SAC_TIMESTEPS, use_graph=use_graph, **{**SAC_KW, **kw})
    assert tr.num_training_steps_per_epoch * tr.num_evals_after_init == SAC_STEPS and tr.num_prefill_actor_steps == 1
    return tr


def _ppo(dev, kind, use_graph=True, **kw):
    from mbpo.optimizers.policy_optimizers.ppo.ppo import PPO
    tr = PPO(environment=_env(dev, kind, rows=256), num_timesteps=PPO_TIMESTEPS, use_graph=use_graph, **{**PPO_KW, **kw})
    assert tr.num_training_steps_per_epoch == PPO_STEPS
    return tr


def _clone_env_state(es):
    return es.replace(obs=es.obs.clone(), reward=es.reward.clone(), done=es.done.clone(), info={k: v.clone() for k, v in es.info.items()})


def _clone_replay(bs):
    return bs.replace(data=bs.data.clone(), state=bs.state.clone())


def _assert_same_learner(a, b, what):
    for name in LEARNER_FIELDS:
        ta, tb = getattr(a, name), getattr(b, name)
        assert (ta is None) == (tb is None), f"{what}: {name}"
        if ta is not None:
            assert torch.equal(ta, tb), f"{what}: {name} differs"
    assert a.signature == b.signature


def _assert_same_replay(a, b, what):
    assert torch.equal(a.data, b.data), f"{what}: replay data differs"
    assert torch.equal(a.state, b.state), f"{what}: replay device state words differ"
    for name in ("insert_position", "sample_position", "head", "sample_count", "key"):
        assert getattr(a, name) == getattr(b, name), f"{what}: replay host mirror {name}"


# ---------------------------------------------------------------------------------------------------- 1. the carry is complete (SAC)
@pytest.mark.parametrize("kind", ["pendulum", "ensemble"])
def test_sac_carry_is_complete(dev, kind):
    """A runs prefill, epoch(e1), epoch(e2).  B1 runs prefill and epoch(e1) and exports its learner with the buffer; B2, a new trainer,
    loads it, takes clones of B1's env State and runs epoch(e2).  A replayed its graph, B2 ran one eager step and captured its own."""
    e1, e2 = 19, 23
    a = _sac(dev, kind)
    ts, es, bs = a.init_training_state(7), a.reset_envs(a.env, 11, N), a.replay_buffer.init(13)
    ts, es, bs, _ = a.prefill_replay_buffer(ts, es, bs, 17)
    ts, es, bs, _ = a.training_epoch(ts, es, bs, e1)
    graph_a = a._graph
    ts, es, bs, metrics_a = a.training_epoch(ts, es, bs, e2)
    assert a._graph is graph_a and graph_a is not None
    ref = a.export_learner_state(bs)

    b1 = _sac(dev, kind)
    ts1, es1, bs1 = b1.init_training_state(7), b1.reset_envs(b1.env, 11, N), b1.replay_buffer.init(13)
    ts1, es1, bs1, _ = b1.prefill_replay_buffer(ts1, es1, bs1, 17)
    ts1, es1, bs1, _ = b1.training_epoch(ts1, es1, bs1, e1)
    ls = b1.export_learner_state(bs1)
    assert ls.replay is bs1 and ls.replay.data is bs1.data                    # the buffer travels by reference ...
    assert ls.params.data_ptr() != b1.updater.params.data_ptr()               # ... everything else as clones
    assert b1.replay_buffer.size(bs1) == 1500 and bs1.head != 0               # the ring has wrapped

    b2 = _sac(dev, kind)
    ts2 = b2.load_learner_state(ls)
    assert ts2.env_steps == 0
    es2 = _clone_env_state(es1)
    ts2, es2, bs2, metrics_b = b2.training_epoch(ts2, es2, ls.replay, e2)
    torch.cuda.synchronize()
    assert b2._graph is not None
    got = b2.export_learner_state(bs2)
    _assert_same_learner(ref, got, "resumed SAC")
    assert float(got.step_count) == 2 * SAC_STEPS * G
    _assert_same_replay(ref.replay, got.replay, "resumed SAC")
    dev_words = got.replay.state.cpu().tolist()
    assert dev_words[:3] == [got.replay.insert_position, got.replay.sample_position, got.replay.head]
    for name in ("obs", "done"):
        assert torch.equal(getattr(es, name), getattr(es2, name)), name
    for name in ("steps", "first_obs", "truncation"):
        assert torch.equal(es.info[name], es2.info[name]), name
    assert torch.equal(a._rng, b2._rng)
    assert metrics_a == metrics_b
    for t in (a, b1, b2):
        t.close()


# ---------------------------------------------------------------------------------------------------- 2. the same for PPO
def test_ppo_carry_is_complete(dev):
    e1, e2 = 19, 31
    keys = [101 + i for i in range(PPO_KW["num_envs"])]
    a = _ppo(dev, "ensemble")
    ts, es = a.init_training_state(5), a.env.reset(keys)
    ts, es, _ = a.training_epoch(ts, es, e1)
    ts, es, metrics_a = a.training_epoch(ts, es, e2)
    ref = a.export_learner_state()

    b1 = _ppo(dev, "ensemble")
    ts1, es1 = b1.init_training_state(5), b1.env.reset(keys)
    ts1, es1, _ = b1.training_epoch(ts1, es1, e1)
    ls = b1.export_learner_state()
    assert ls.replay is None and ls.target_q is None and ls.params.data_ptr() != b1.updater.params.data_ptr()

    b2 = _ppo(dev, "ensemble")
    ts2 = b2.load_learner_state(ls)
    es2 = _clone_env_state(es1)
    ts2, es2, metrics_b = b2.training_epoch(ts2, es2, e2)
    torch.cuda.synchronize()
    got = b2.export_learner_state()
    _assert_same_learner(ref, got, "resumed PPO")
    assert float(got.step_count) == 2 * PPO_STEPS * PPO_UPDATES
    for name in ("obs", "done"):
        assert torch.equal(getattr(es, name), getattr(es2, name)), name
    for name in ("steps", "first_obs"):
        assert torch.equal(es.info[name], es2.info[name]), name
    assert torch.equal(a._data, b2._data) and torch.equal(a._perm, b2._perm) and torch.equal(a._rng, b2._rng)
    assert metrics_a == metrics_b
    for t in (a, b1, b2):
        t.close()


# ---------------------------------------------------------------------------------------------------- 3. a resumed run never initialises
def _refuse_init(*a, **k):
    raise AssertionError("init_training_state was called in a resumed run_training")


@pytest.fixture(scope="module")
def sac_first_call(dev):
    """One fresh run_training (prefill + one epoch of 4 steps) on the ensemble: (learner state with its buffer, the epoch's metrics).
    Tests that resume from it take `replace(replay=...)` copies; nobody writes to it."""
    tr = _sac(dev, "ensemble", use_graph=False)
    _, metrics = tr.run_training(key=41)
    ls = tr.last_learner_state
    assert float(ls.step_count) == SAC_STEPS * G and ls.replay is not None
    tr.close()
    return ls, metrics


def test_sac_resumed_run_training_never_initialises(dev, sac_first_call, monkeypatch):
    ls = sac_first_call[0].replace(replay=None)
    ends = []
    for _ in range(2):
        tr = _sac(dev, "ensemble")
        monkeypatch.setattr(tr, "init_training_state", _refuse_init)
        policy, metrics = tr.run_training(key=43, learner_state=ls)
        end = tr.last_learner_state
        assert float(end.step_count) == float(ls.step_count) + 1 * SAC_STEPS * G
        assert end.replay is not None and end.params.data_ptr() != tr.updater.params.data_ptr()
        assert torch.equal(policy[1], end.params[:tr.updater.P]) and torch.equal(policy[0].vec, end.normalizer)
        ends.append((end, policy, metrics[-1]["training/critic_loss"]))
        tr.close()
    _assert_same_learner(ends[0][0], ends[1][0], "two resumed runs")
    _assert_same_replay(ends[0][0].replay, ends[1][0].replay, "two resumed runs")
    assert torch.equal(ends[0][1][1], ends[1][1][1]) and ends[0][2] == ends[1][2]
    assert not torch.equal(ends[0][0].params, ls.params)                       # it trained
    assert float(sac_first_call[0].step_count) == SAC_STEPS * G                # and the state it started from is a value: untouched


def test_sac_last_learner_state_is_the_last_one_with_return_best_model(dev, sac_first_call):
    """num_evals = 3: two epochs; whichever evaluation was best, last_learner_state is the END of the call."""
    ls = sac_first_call[0].replace(replay=None)
    tr = _sac(dev, "ensemble", return_best_model=True, num_evals=3, num_eval_envs=8)
    epochs = tr.num_evals_after_init
    tr.run_training(key=47, learner_state=ls)
    end = tr.last_learner_state
    assert epochs == 2 and float(end.step_count) == float(ls.step_count) + epochs * tr.num_training_steps_per_epoch * G
    assert torch.equal(end.params, tr.updater.params) and torch.equal(end.normalizer, tr._stats_vec)
    tr.close()


def test_ppo_resumed_run_training_never_initialises(dev, monkeypatch):
    first = _ppo(dev, "pendulum")
    first.run_training(key=41)
    ls = first.last_learner_state
    first.close()
    assert float(ls.step_count) == PPO_STEPS * PPO_UPDATES
    ends = []
    for _ in range(2):
        tr = _ppo(dev, "pendulum")
        monkeypatch.setattr(tr, "init_training_state", _refuse_init)
        tr.run_training(key=43, learner_state=ls)
        ends.append(tr.last_learner_state)
        assert float(ends[-1].step_count) == float(ls.step_count) + 1 * PPO_STEPS * PPO_UPDATES
        tr.close()
    _assert_same_learner(ends[0], ends[1], "two resumed PPO runs")


# ---------------------------------------------------------------------------------------------------- 4. retained buffer
def _count_get_experience(tr):
    calls = []
    inner = tr.get_experience

    def counted(*a, **k):
        calls.append(1)
        return inner(*a, **k)

    tr.get_experience = counted
    return calls


def test_sac_retained_buffer_is_continued_without_prefill(dev, sac_first_call):
    first, first_metrics = sac_first_call
    carried = _clone_replay(first.replay)
    ls = first.replace(replay=carried)
    # what the size will be: the carried host mirrors moved by this call's inserts, the queue's own integer arithmetic
    tr = _sac(dev, "ensemble", use_graph=False)
    mirror = carried
    for _ in range(SAC_STEPS):
        mirror = tr.replay_buffer.insert_mirror(mirror, N * S)
    calls = _count_get_experience(tr)
    _, metrics = tr.run_training(key=43, learner_state=ls)
    assert metrics[-1]["training/buffer_current_size"] == float(tr.replay_buffer.size(mirror)) == 1500.0
    assert len(calls) == SAC_STEPS                                      # no prefill step ran
    end = tr.last_learner_state.replay
    assert end.data is carried.data and end.state is carried.state      # the same buffer, written in place
    assert (end.insert_position, end.sample_position, end.head) == (mirror.insert_position, mirror.sample_position, mirror.head)
    assert end.state.cpu().tolist()[:3] == [end.insert_position, end.sample_position, end.head]
    assert not torch.equal(end.data, first.replay.data)
    tr.close()

    # without a buffer in the state: a new buffer, prefilled exactly as the first call's was
    tr = _sac(dev, "ensemble", use_graph=False)
    calls = _count_get_experience(tr)
    _, metrics = tr.run_training(key=43, learner_state=first.replace(replay=None))
    assert len(calls) == tr.num_prefill_actor_steps + SAC_STEPS
    assert metrics[-1]["training/buffer_current_size"] == first_metrics[-1]["training/buffer_current_size"]
    fresh = tr.last_learner_state.replay
    assert fresh.data is not first.replay.data
    assert (fresh.insert_position, fresh.sample_position, fresh.head) == \
        (first.replay.insert_position, first.replay.sample_position, first.replay.head)
    tr.close()


def test_sac_retained_buffer_below_min_replay_size_prefills_the_difference(dev):
    """An EMPTY retained buffer needs the fresh call's prefill: ceil((min_replay_size - 0) / num_envs) steps."""
    src = _sac(dev, "pendulum", use_graph=False)
    src.init_training_state(7)
    ls = src.export_learner_state(src.replay_buffer.init(13))
    tr = _sac(dev, "pendulum", use_graph=False)
    calls = _count_get_experience(tr)
    tr.run_training(key=43, learner_state=ls)
    assert len(calls) == tr.num_prefill_actor_steps + SAC_STEPS
    assert tr.last_learner_state.replay.data is ls.replay.data
    src.close()
    tr.close()


# ---------------------------------------------------------------------------------------------------- 5. optimizer level
def _sac_optimizers(dev, n, **kw):
    """n SACOptimizers on ONE system and ONE true buffer (a state moves between optimizer objects of the same architecture)."""
    from mbpo.optimizers import SACOptimizer
    system, sp, _, X, U = _make_system(dev, "ensemble")
    tb, tbs = _true_buffer(dev, X, U, 512)
    opts = [SACOptimizer(system=system, true_buffer=tb, num_timesteps=SAC_TIMESTEPS, use_graph=True, **SAC_KW, **kw) for _ in range(n)]
    state = opts[0].init(key=3, true_buffer_state=tbs).replace(system_params=sp)
    return opts, state


def _fork(opt_state):
    """An optimizer state whose retained buffer is a copy: two optimizers can each continue it."""
    ls = opt_state.learner_state
    return opt_state.replace(learner_state=ls.replace(replay=_clone_replay(ls.replay)))


@pytest.mark.parametrize("model_change", ["none", "in_place", "new_tensor"])
def test_sac_optimizer_kept_trainer_equals_a_rebuilt_one(dev, model_change):
    (kept, rebuilt), state = _sac_optimizers(dev, 2, warm_start=True, retain_replay_buffer=True)
    out1 = kept.train(state)
    s1 = out1.optimizer_state
    assert float(s1.learner_state.step_count) == SAC_STEPS * G and s1.learner_state.replay is not None
    trainer, graph = kept._trainer, kept._trainer._graph
    assert trainer is not None and graph is not None
    dp = s1.system_params.dynamics_params
    if model_change == "in_place":              # what a refit that updates the model in place leaves: the same address, new values
        dp.params.mul_(0.999)
    elif model_change == "new_tensor":          # a refit that returns new tensors
        s1 = s1.replace(system_params=s1.system_params.replace(dynamics_params=dp.replace(params=dp.params.mul(0.999))))
    s1_copy = _fork(s1)
    out2 = kept.train(s1)
    assert kept._trainer is trainer                                     # the trainer was kept ...
    if model_change == "new_tensor":
        assert kept._trainer._graph is not graph                        # ... a new address: captured again
    else:
        assert kept._trainer._graph is graph                            # ... every address as captured: replayed, no re-capture
    ref = rebuilt.train(s1_copy)
    assert rebuilt._trainer is not trainer
    a, b = out2.optimizer_state, ref.optimizer_state
    assert float(a.learner_state.step_count) == 2 * SAC_STEPS * G
    _assert_same_learner(a.learner_state, b.learner_state, "kept trainer vs rebuilt")
    _assert_same_replay(a.learner_state.replay, b.learner_state.replay, "kept trainer vs rebuilt")
    assert torch.equal(a.policy_params[1], b.policy_params[1]) and torch.equal(a.policy_params[0].vec, b.policy_params[0].vec)
    assert a.key == b.key
    for k in ("training/critic_loss", "training/actor_loss", "training/alpha", "training/buffer_current_size", "eval/episode_reward"):
        assert out2.summary[-1][k] == ref.summary[-1][k], k
    assert not torch.equal(a.learner_state.params, out1.optimizer_state.learner_state.params)
    kept.close()
    rebuilt.close()
    assert kept._trainer is None and trainer._graph is None


def test_sac_optimizer_without_retained_buffer_drops_it(dev):
    (opt,), state = _sac_optimizers(dev, 1, warm_start=True)
    out1 = opt.train(state)
    assert out1.optimizer_state.learner_state.replay is None
    out2 = opt.train(out1.optimizer_state)
    assert float(out2.optimizer_state.learner_state.step_count) == 2 * SAC_STEPS * G
    assert out2.summary[-1]["training/buffer_current_size"] == out1.summary[-1]["training/buffer_current_size"]
    opt.close()


def test_sac_optimizer_default_is_a_fresh_learner_per_call(dev):
    from mbpo.optimizers.policy_optimizers.sac.sac import SAC
    (opt,), state = _sac_optimizers(dev, 1)
    made = []

    def recording(**kw):
        made.append(SAC(**kw))
        return made[-1]

    opt.agent_class = recording
    outs = [opt.train(state), opt.train(state)]
    assert opt._trainer is None and len(made) == 2
    for out, tr in zip(outs, made):
        assert out.optimizer_state.learner_state is None
        assert float(tr.updater.step_count) == SAC_STEPS * G            # one call's worth, both times
        assert tr._graph is None                                        # closed
    a, b = (o.optimizer_state for o in outs)
    assert torch.equal(a.policy_params[1], b.policy_params[1]) and torch.equal(a.policy_params[0].vec, b.policy_params[0].vec)
    assert a.key == b.key
    for k in ("training/critic_loss", "training/actor_loss", "training/alpha_loss", "training/alpha", "eval/episode_reward"):
        assert outs[0].summary[-1][k] == outs[1].summary[-1][k], k


def test_ppo_optimizer_warm_start_continues_and_replays(dev):
    from mbpo.optimizers import PPOOptimizer
    system, sp, _, X, U = _make_system(dev, "ensemble")
    tb, tbs = _true_buffer(dev, X, U, 256)
    opt = PPOOptimizer(system=system, true_buffer=tb, num_timesteps=PPO_TIMESTEPS, warm_start=True, **PPO_KW)
    state = opt.init(key=3, true_buffer_state=tbs).replace(system_params=sp)
    out1 = opt.train(state)
    graph = opt._trainer._graph
    assert graph is not None and float(out1.optimizer_state.learner_state.step_count) == PPO_STEPS * PPO_UPDATES
    out2 = opt.train(out1.optimizer_state)
    assert opt._trainer._graph is graph
    assert float(out2.optimizer_state.learner_state.step_count) == 2 * PPO_STEPS * PPO_UPDATES
    # the same call from a second optimizer with a new trainer
    ref = PPOOptimizer(system=system, true_buffer=tb, num_timesteps=PPO_TIMESTEPS, warm_start=True, **PPO_KW).train(out1.optimizer_state)
    _assert_same_learner(out2.optimizer_state.learner_state, ref.optimizer_state.learner_state, "kept PPO trainer vs rebuilt")
    opt.close()


# ---------------------------------------------------------------------------------------------------- 6. refusals
def _flat(tr):
    u = tr.updater
    names = ("params", "target_q", "adam_m", "adam_v", "step_count") if hasattr(u, "target_q") else ("params", "adam_m", "adam_v", "step_count")
    return [getattr(u, n).clone() for n in names] + [tr._stats_vec.clone()], [getattr(u, n) for n in names] + [tr._stats_vec]


def test_refusals_name_the_field_and_copy_nothing(dev):
    wide = _sac(dev, "pendulum")                                         # the default 64 x 3 networks
    wide.init_training_state(7)
    ls3 = wide.export_learner_state()
    narrow = _sac(dev, "pendulum", policy_hidden_layer_sizes=(64, 64), critic_hidden_layer_sizes=(64, 64))
    narrow.init_training_state(9)
    before, live = _flat(narrow)
    with pytest.raises(ValueError, match="policy_dims_logical"):
        narrow.load_learner_state(ls3)
    with pytest.raises(ValueError, match="policy_dims_logical"):
        narrow.run_training(key=1, learner_state=ls3)
    assert all(torch.equal(x, y) for x, y in zip(before, live))
    # a SAC state into PPO
    ppo = _ppo(dev, "pendulum", policy_hidden_layer_sizes=(64, 64, 64), critic_hidden_layer_sizes=(64, 64, 64))
    ppo.init_training_state(5)
    before, live = _flat(ppo)
    with pytest.raises(ValueError, match="trainer"):
        ppo.load_learner_state(ls3)
    assert all(torch.equal(x, y) for x, y in zip(before, live))
    # a retained buffer of another max_replay_size (everything else fits)
    small = _sac(dev, "pendulum", max_replay_size=1000)
    small.init_training_state(9)
    before, live = _flat(small)
    with pytest.raises(ValueError, match="max_replay_size"):
        small.load_learner_state(ls3.replace(replay=wide.replay_buffer.init(0)))
    assert all(torch.equal(x, y) for x, y in zip(before, live))
    small.load_learner_state(ls3)                                        # without the buffer it fits
    assert torch.equal(small.updater.params, ls3.params)
    # a kept trainer is rebound to environments of ITS System and true buffer only
    with pytest.raises(ValueError, match="System"):
        wide.rebind(narrow.env)
    same = wide.env
    wide.rebind(type(same)(same.system, same.init_system_params, same.sample_buffer_state, same.sample_buffer))
    assert wide.env is not same and wide.eval_env is wide.env
    for t in (wide, narrow, ppo, small):
        t.close()


def test_optimizer_refuses_a_state_of_another_architecture(dev):
    from mbpo.optimizers import SACOptimizer
    (opt,), state = _sac_optimizers(dev, 1, warm_start=True)
    out = opt.train(state)
    other = SACOptimizer(system=opt.system, true_buffer=opt.true_buffer, num_timesteps=SAC_TIMESTEPS, warm_start=True,
                         policy_hidden_layer_sizes=(64, 64), **SAC_KW)
    with pytest.raises(ValueError, match="policy_dims_logical"):
        other.train(out.optimizer_state)
    assert other._trainer is None
    opt.close()
