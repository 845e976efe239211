"""Warm start without a GPU: the optimizer-level switches (constructor options, BraxState.learner_state, refusals) and the
LearnerState value — signature comparison and the env-State re-homing of a kept trainer — on CPU tensors."""
import pytest
import torch

from mbpo.optimizers.policy_optimizers.brax_optimizers import BraxState, PPOOptimizer, SACOptimizer
from mbpo.optimizers.policy_optimizers.brax_utils.base import LearnerState, State, rehome_state


def _signature(**kw):
    sig = dict(trainer="SAC", x_dim=3, action_dim=1, policy_dims_logical=[3, 64, 64, 2], policy_dims=[3, 64, 64, 2],
               q_dims_logical=[4, 64, 64, 1], q_dims=[4, 64, 64, 1], normalize_observations=True)
    sig.update(kw)
    return sig


def _learner_state(n=10, **kw):
    return LearnerState(signature=_signature(**kw), params=torch.arange(n, dtype=torch.float32), adam_m=torch.zeros(n),
                        adam_v=torch.zeros(n), step_count=torch.tensor([16.0]), normalizer=torch.zeros(10), target_q=torch.zeros(4))


def test_brax_state_has_no_learner_state_by_default():
    st = BraxState(true_buffer_state=None, system_params=None, key=0)
    assert st.learner_state is None and st.policy_params is None
    assert st.replace(key=1).learner_state is None


def test_constructor_keeps_the_switches_out_of_agent_kwargs():
    opt = SACOptimizer(true_buffer=None, system=None, warm_start=True, retain_replay_buffer=True, num_timesteps=100, num_envs=4)
    assert opt.warm_start and opt.retain_replay_buffer
    assert opt.agent_kwargs == dict(num_timesteps=100, num_envs=4)
    opt = SACOptimizer(true_buffer=None, system=None, num_timesteps=100)
    assert not opt.warm_start and not opt.retain_replay_buffer and opt.agent_kwargs == dict(num_timesteps=100)
    opt = PPOOptimizer(true_buffer=None, system=None, warm_start=True, num_timesteps=100)
    assert opt.warm_start and not opt.retain_replay_buffer and opt.agent_kwargs == dict(num_timesteps=100)
    opt.close()                                 # nothing kept: a no-op


def test_retain_replay_buffer_without_warm_start_is_refused():
    with pytest.raises(ValueError, match="warm_start"):
        SACOptimizer(true_buffer=None, system=None, retain_replay_buffer=True, num_timesteps=100)
    with pytest.raises(ValueError, match="retain_replay_buffer"):
        PPOOptimizer(true_buffer=None, system=None, warm_start=True, retain_replay_buffer=True, num_timesteps=100)


def test_learner_state_signature_comparison():
    ls = _learner_state()
    assert ls.mismatch(_signature()) is None
    ls.check(_signature())
    assert ls.mismatch(_signature(policy_dims_logical=(3, 64, 64, 2))) is None          # a tuple and a list of the same sizes agree
    for field, other in (("trainer", "PPO"), ("x_dim", 4), ("action_dim", 2), ("policy_dims_logical", [3, 64, 64, 64, 2]),
                         ("q_dims", [4, 128, 128, 1]), ("normalize_observations", False)):
        assert ls.mismatch(_signature(**{field: other})) == field
        with pytest.raises(ValueError, match=field):
            ls.check(_signature(**{field: other}))
    # a field only one side has (SAC's q_dims against PPO's value_dims) is a mismatch too, after `trainer`
    ppo = {k: v for k, v in _signature(trainer="PPO").items() if not k.startswith("q_")}
    ppo.update(value_dims_logical=[3, 64, 64, 1], value_dims=[3, 64, 64, 1])
    assert ls.mismatch(ppo) == "trainer"
    assert ls.mismatch(dict(ppo, trainer="SAC")) in ("value_dims_logical", "q_dims_logical")
    # the state is a value: replace() leaves the original alone
    assert ls.replace(replay="buffer").replay == "buffer" and ls.replay is None
    with pytest.raises(ValueError, match="adam_v"):
        ls.replace(adam_v=torch.zeros(3)).check(_signature())


def _state(n, x, fill):
    return State(pipeline_state=None, obs=torch.full((n, x), fill), reward=torch.full((n,), fill), done=torch.zeros(n),
                 system_params=f"params{fill}", info={"steps": torch.full((n,), fill), "truncation": torch.zeros(n),
                                                      "first_obs": torch.full((n, x), fill + 0.5)})


def test_rehome_state_copies_a_fresh_reset_into_the_kept_tensors():
    fresh = _state(4, 3, 2.0)
    assert rehome_state(None, fresh) is fresh
    home = _state(4, 3, 1.0)
    out = rehome_state(home, fresh)
    assert out.obs is home.obs and out.info["first_obs"] is home.info["first_obs"] and out.info["steps"] is home.info["steps"]
    assert torch.equal(out.obs, fresh.obs) and torch.equal(out.info["first_obs"], fresh.info["first_obs"])
    assert torch.equal(out.reward, fresh.reward) and torch.equal(out.info["steps"], fresh.info["steps"])
    assert out.system_params == "params2.0"                        # everything that is no device tensor is the fresh State's
    # another number of envs: the fresh State as it is, the home untouched
    other = _state(5, 3, 7.0)
    assert rehome_state(home, other) is other and torch.equal(home.obs, fresh.obs)
