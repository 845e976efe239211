"""Input scaler of the dynamics ensemble — torch-CPU restatement (test infrastructure, no product imports) of what
mbpo_ens_scaler_fit, mbpo_ens_scaler_prepare and mbpo_ens_fold_scaler define (include/mbpo_hip.h, "N3c").  MBPO's procedure as
remembered, not the reference's, which has no learned model: parity unpinned by construction.

    stats    mean_c = sum_k d_kc / n,  std_c = sqrt(sum_k (d_kc - mean_c)^2 / n)  in fp64, over rows[idx][:, :x+u];
             std_c (rounded to fp32) < std_floor -> 1
    prepare  out[k] = [ (row[:x+u] - mean) * (1 / std) | row[reward_off] or 0 | next_obs - x (predict_delta) or next_obs ]
    fold     W'[i][j] = W[i][j] * (1 / std_i),  b'[j] = b[j] - sum_i W'[i][j] * mean_i   (i ascending), everything else copied
    identity MLP((v - mean) / std; W, b) == MLP(v; W', b')
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from oracle import nets

STD_FLOOR = 1e-12


def prepared_reward_off(x_dim: int, u_dim: int) -> int:
    return x_dim + u_dim


def prepared_next_obs_off(x_dim: int, u_dim: int) -> int:
    return x_dim + u_dim + 1


def prepared_row_len(x_dim: int, u_dim: int) -> int:
    return 2 * x_dim + u_dim + 1


def _select(rows: torch.Tensor, idx: Optional[torch.Tensor], n: Optional[int]) -> torch.Tensor:
    if idx is not None:
        return rows[idx.long()]
    return rows if n is None else rows[:n]


def stats64(rows: torch.Tensor, in_dim: int, idx: Optional[torch.Tensor] = None, n: Optional[int] = None,
            std_floor: float = STD_FLOOR) -> torch.Tensor:
    """[2, in_dim] fp64: mean and population std BEFORE the floor in row 1 where it does not apply; columns whose std, rounded to
    fp32, lies below the floor get exactly 1."""
    d = _select(rows, idx, n)[:, :in_dim].double()
    mean = d.mean(dim=0)
    std = ((d - mean) ** 2).mean(dim=0).sqrt()
    std = torch.where(std.float() < torch.tensor(std_floor, dtype=torch.float32), torch.ones_like(std), std)
    return torch.stack([mean, std])


def prepare(rows: torch.Tensor, scaler: torch.Tensor, x_dim: int, u_dim: int, idx: Optional[torch.Tensor] = None,
            n: Optional[int] = None, next_obs_off: Optional[int] = None, reward_off: Optional[int] = None,
            predict_delta: bool = True) -> torch.Tensor:
    """The prepared matrix in the dtype of `rows` (fp32 rows and scaler: the device's operations, (v - mean) * fl(1 / std))."""
    X, D = x_dim, x_dim + u_dim
    noff = D + 2 if next_obs_off is None else next_obs_off
    b = _select(rows, idx, n)
    scaler = scaler.to(rows.dtype)
    inv = torch.ones((), dtype=rows.dtype) / scaler[1]
    xn = (b[:, :D] - scaler[0]) * inv
    r = b[:, reward_off:reward_off + 1] if reward_off is not None and reward_off >= 0 else torch.zeros(b.shape[0], 1, dtype=rows.dtype)
    t = b[:, noff:noff + X] - b[:, :X] if predict_delta else b[:, noff:noff + X]
    return torch.cat([xn, r, t], dim=1)


def fold(params: torch.Tensor, dims: Sequence[int], n_members: int, scaler: torch.Tensor) -> torch.Tensor:
    """The members' flat parameters ([E * P], layout of `dims`) with the scaler folded into layer one, in the dtype of `params`: fp64
    for the reference, fp32 for the device's operation order (W' rounded as stored, then the products added to the sum, i ascending)."""
    P = nets.n_params(dims)
    d0, d1 = int(dims[0]), int(dims[1])
    scaler = scaler.to(params.dtype)
    inv = torch.ones((), dtype=params.dtype) / scaler[1]
    out = params.clone().reshape(n_members, P)
    for e in range(n_members):
        w = params[e * P:e * P + d0 * d1].reshape(d0, d1) * inv[:, None]
        s = torch.zeros(d1, dtype=params.dtype)
        for i in range(d0):
            s = s + w[i] * scaler[0, i]
        out[e, :d0 * d1] = w.reshape(-1)
        out[e, d0 * d1:d0 * d1 + d1] = params[e * P + d0 * d1:e * P + d0 * d1 + d1] - s
    return out.reshape(-1)


def normalise_then_net64(params: torch.Tensor, dims: Sequence[int], n_members: int, scaler: torch.Tensor, xu: torch.Tensor,
                         act: str = "swish") -> torch.Tensor:
    """[E, N, out] fp64: the UNFOLDED members on (xu - mean) / std."""
    s = scaler.double()
    return nets.ensemble_forward(params.double(), dims, n_members, (xu.double() - s[0]) / s[1], act)


def folded_net(params: torch.Tensor, dims: Sequence[int], n_members: int, scaler: torch.Tensor, xu: torch.Tensor,
               act: str = "swish") -> torch.Tensor:
    """[E, N, out] in the dtype of `params`: the FOLDED members on the raw xu."""
    return nets.ensemble_forward(fold(params, dims, n_members, scaler), dims, n_members, xu.to(params.dtype), act)


# ---- the cancellation measurement (tests/test_cpu_ens_input_scaler.py; its figure for set "a" is the GPU end-to-end tolerance) -----
CANCEL_DIMS = (4, 64, 64, 64, 6)
CANCEL_MEMBERS = 3
CANCEL_N = 256


def cancellation_case(kind: str):
    """(params fp32 [E * P], scaler fp32 [2, 4], raw inputs fp32 [N, 4]) of the measurement.  Set "a": every column has
    |mean| <= 3 std; set "b": the same draw with column 2 at mean = 1000 std.  Inputs are mean + std * U(-3, 3)."""
    g = torch.Generator().manual_seed(1234)
    P = nets.n_params(CANCEL_DIMS)
    params = torch.cat([nets.init_mlp_flat(CANCEL_DIMS, g) + 0.02 * torch.randn(P, generator=g) for _ in range(CANCEL_MEMBERS)])
    std = torch.tensor([1.0, 0.1, 10.0, 2.0])
    mean = torch.tensor([0.5, -0.3, 30.0 if kind == "a" else 10000.0, 0.0])
    z = (torch.rand(CANCEL_N, CANCEL_DIMS[0], generator=g, dtype=torch.float64) * 2 - 1) * 3
    xu = (mean.double() + std.double() * z).float()
    return params, torch.stack([mean, std]), xu


def fold_discrepancy(params: torch.Tensor, dims: Sequence[int], n_members: int, scaler: torch.Tensor, xu: torch.Tensor) -> float:
    """max |fp32 folded members on raw xu - fp64 unfolded members on the normalised xu| over members, rows and outputs."""
    got = folded_net(params.float(), dims, n_members, scaler.float(), xu.float())
    want = normalise_then_net64(params, dims, n_members, scaler, xu)
    return float((got.double() - want).abs().max())
