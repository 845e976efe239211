"""Reference for branched model rollouts (include/mbpo_hip.h, "fresh starts"): a fresh true-buffer start state after every reset.

MBPO's procedure as remembered, unverified against its code (the reference tree's AutoReset returns to the same first_obs every time):

    first_obs[env] is the state the env's next reset goes to.  When the env's step s of a launch ends with done = 1 the reset uses the
    current first_obs[env] (oracle.rollout.env_step, unchanged); immediately after it
        idx            = philox_randint(seed, offset, stream START = 11, element s * N + env, sample_position, insert_position)
        first_obs[env] = data_logical[idx mod max_size][0 .. x)
    An empty range yields sample_position.  One draw per env step whatever action_repeat is.  Everything else about the row —
    discount, truncation, next_observation = the post-reset obs, the termination rules, the reward — is oracle.rollout's.

The rollout itself is oracle.rollout driven ONE env step at a time (explicit policy_noise / model_noise / member_idx sliced per step;
the rows put back into step-major or env-major order); open-loop actions go through oracle.rollout.env_step, which oracle.rollout has
no argument for.  The buffer is oracle.replay.UniformSamplingQueue, which really rolls its array: the product's ring arithmetic
(head, wrap) is checked against it independently.  Every draw is recorded.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

from oracle import philox
from oracle import rollout as oro

STREAM_START = 11          # csrc/common.hpp: MBPO_STREAM_START, the next free id after STREAM_ICEM = 10


@dataclass
class Draws:
    """Every draw of one or more launches: (launch, step, env, logical index), in the order they happened."""
    launch: list = field(default_factory=list)
    step: list = field(default_factory=list)
    env: list = field(default_factory=list)
    idx: list = field(default_factory=list)

    def __len__(self):
        return len(self.idx)

    def of_env(self, env: int):
        return [i for e, i in zip(self.env, self.idx) if e == env]

    def steps_of_env(self, env: int, launch=None):
        return [s for l, s, e in zip(self.launch, self.step, self.env) if e == env and (launch is None or l == launch)]


def draw_indices(seed: int, offset: int, s: int, n_envs: int, envs: np.ndarray, sample_position: int, insert_position: int) -> np.ndarray:
    """The START-stream draw of step s for `envs`."""
    elem = np.uint64(s) * np.uint64(n_envs) + envs.astype(np.uint64)
    return philox.philox_randint(seed, offset, STREAM_START, elem, int(sample_position), int(insert_position))


def rollout(system, policy_params, policy_dims, st: oro.EnvState, n_steps: int, episode_length: int, *, queue, qstate, seed: int,
            offset: int, action_repeat: int = 1, policy_noise=None, model_noise=None, member_idx=None, actions=None,
            ppo_extras: bool = False, env_major: bool = False, norm_mean=None, norm_std=None, draws: Draws | None = None,
            launch: int = 0):
    """One launch of n_steps env steps.  Returns (final EnvState — first_obs updated —, rows [S*N, D], draws)."""
    N, X = st.obs.shape
    draws = Draws() if draws is None else draws
    st = st.clone()
    out = []
    for s in range(n_steps):
        mn = None if model_noise is None else model_noise[s:s + 1]
        mi = None if member_idx is None else member_idx[s:s + 1]
        if actions is None:
            nst, rows = oro.rollout(system, policy_params, policy_dims, st, 1, episode_length, action_repeat, norm_mean=norm_mean,
                                    norm_std=norm_std, policy_noise=policy_noise[s:s + 1], model_noise=mn, member_idx=mi,
                                    ppo_extras=ppo_extras, env_major=False)
        else:
            U = actions.shape[-1]
            nst, reward, trunc = oro.env_step(system, st, actions[s], episode_length, action_repeat, 0, mi, mn)
            rows = torch.cat([st.obs, actions[s], reward[:, None], (1 - nst.done)[:, None], nst.obs, trunc[:, None]], dim=1)
            assert rows.shape[1] == oro.row_len(X, U, False)
        out.append(rows)
        # the reset above consumed first_obs of the envs that came out done: each gets its next start state
        done_envs = np.nonzero(nst.done.numpy() != 0)[0]
        first = nst.first_obs.clone()
        if done_envs.size:
            idx = draw_indices(seed, offset, s, N, done_envs, qstate["sample_position"], qstate["insert_position"])
            first[torch.from_numpy(done_envs)] = torch.from_numpy(queue.gather(qstate, idx)[:, :X].copy())
            for e, i in zip(done_envs.tolist(), idx.tolist()):
                draws.launch.append(launch); draws.step.append(s); draws.env.append(e); draws.idx.append(i)
        st = oro.EnvState(nst.obs, first, nst.steps, nst.done)
    rows = torch.stack(out)                                        # [S, N, D]
    if env_major:
        rows = rows.permute(1, 0, 2)
    return st, rows.reshape(n_steps * N, -1).contiguous(), draws


def chain_of_starts(n_envs: int, n_steps_per_launch, episode_length: int, keys, sample_position: int, insert_position: int,
                    steps0=None):
    """For a rollout that ends episodes by truncation alone (no termination, action_repeat 1): the logical indices every env's resets
    draw, launch after launch, from the bookkeeping rule alone — `keys[l]` = (seed, offset) of launch l.  Returns per env the list of
    drawn indices, in order (what a trainer's recorded draws must be)."""
    steps = np.zeros(n_envs) if steps0 is None else np.asarray(steps0, float).copy()
    done = np.zeros(n_envs)
    chain = [[] for _ in range(n_envs)]
    for (seed, offset), S in zip(keys, n_steps_per_launch):
        for s in range(S):
            steps = np.where(done != 0, 0.0, steps) + 1
            done = (steps >= episode_length).astype(float)
            envs = np.nonzero(done)[0]
            if envs.size:
                for e, i in zip(envs.tolist(), draw_indices(seed, offset, s, n_envs, envs, sample_position, insert_position).tolist()):
                    chain[e].append(i)
    return chain
