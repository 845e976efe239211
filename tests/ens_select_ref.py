"""Ensemble model selection — torch-CPU restatement (test infrastructure) of what mbpo_ens_eval, mbpo_ens_keep_best,
mbpo_ens_pick_elites and EnsembleDynamics.fit(holdout_ratio=) define.  MBPO's procedure (Janner et al. 2019), not the reference's,
which has no learned model: parity unpinned by construction, the definitions are include/mbpo_hip.h's.

    eval      metrics[0][e] = mean_b sum_d [0.5 ((t_d - mu_d) / sigma_d)^2 + log sigma_d]   (oracle.ensemble's loss on ONE index list)
              metrics[1][e] = mean_b sum_d (t_d - mu_d)^2           t = x' - x (predict_delta) or x'; the reward joins both sums
    keep_best improved_e = isfinite(score_e) and score_e < best_score_e * (1 - rel_tol)
    ranking   score ascending, NaN last, ties by lower index (np.argsort(kind="stable"))
    split     perm = Philox permutation(seed, FIT_SITE_HOLDOUT << 32, R); holdout = perm[:n_hold], training = perm[n_hold:]
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from oracle import nets

FIT_SITE_HOLDOUT = 1


def eval_metrics(params: torch.Tensor, dims: Sequence[int], n_members: int, rows: torch.Tensor, idx: torch.Tensor, x_dim: int, u_dim: int,
                 predict_delta: bool = True, min_std: float = 1e-3, reward_off: Optional[int] = None,
                 next_obs_off: Optional[int] = None, act: str = "swish") -> torch.Tensor:
    """[2, E] in the dtype of `params` (pass doubles for the fp64 reference)."""
    P = nets.n_params(dims)
    X = x_dim
    noff = x_dim + u_dim + 2 if next_obs_off is None else next_obs_off
    b = rows[idx.long()]
    t = b[:, noff:noff + X] - (b[:, :X] if predict_delta else 0.0)
    out = []
    for e in range(n_members):
        y = nets.mlp_forward(params[e * P:(e + 1) * P], dims, b[:, :X + u_dim], act)
        mu, sigma = y[:, :X], F.softplus(y[:, X:2 * X]) + min_std
        q = (t - mu) / sigma
        nll = (0.5 * q * q + torch.log(sigma)).sum(dim=1)
        se = ((t - mu) ** 2).sum(dim=1)
        if reward_off is not None:
            r, mu_r, sig_r = b[:, reward_off], y[:, 2 * X], F.softplus(y[:, 2 * X + 1]) + min_std
            qr = (r - mu_r) / sig_r
            nll = nll + 0.5 * qr * qr + torch.log(sig_r)
            se = se + (r - mu_r) ** 2
        out.append(torch.stack([nll.mean(), se.mean()]))
    return torch.stack(out, dim=1)


def keep_best(params: torch.Tensor, best_params: torch.Tensor, score: torch.Tensor, best_score: torch.Tensor, rel_tol: float, state):
    """params / best_params [E, P]; state = [evaluations since an improvement, evaluations].  Returns the new (best_params, best_score,
    state); float32 arithmetic as on the device."""
    score, best_score = score.float(), best_score.float()
    improved = torch.isfinite(score) & (score < best_score * torch.tensor(1.0 - rel_tol, dtype=torch.float32))
    new_params = torch.where(improved[:, None], params, best_params)
    new_score = torch.where(improved, score, best_score)
    return new_params, new_score, [0 if bool(improved.any()) else state[0] + 1, state[1] + 1]


def ranking(score: torch.Tensor) -> list:
    """Member indices in the total order: score ascending, NaN after every number (+inf included), ties by lower index."""
    s = [float(v) for v in score]
    return sorted(range(len(s)), key=lambda e: (math.isnan(s[e]), 0.0 if math.isnan(s[e]) else s[e], e))


def split(seed: int, n_rows: int, holdout_ratio: float, max_holdout: int = 5000):
    """(holdout indices, training indices) of fit(holdout_ratio=) for PRNG key `seed`."""
    from oracle import philox
    perm = np.asarray(philox.philox_permutation(int(seed), FIT_SITE_HOLDOUT << 32, n_rows)).astype(np.int64)
    n_hold = min(int(max_holdout), int(math.floor(holdout_ratio * n_rows)))
    return torch.from_numpy(perm[:n_hold]), torch.from_numpy(perm[n_hold:])
