"""A torch restatement of the seed step of include/mbpo_hip.h "policy priors" (mbpo_icem_seed_candidates): copy, clip, drop, replicate,
mean.  Written from the header's text, on host tensors, with explicit loops over problems and proposals; it shares no code with the kernel
or with iCemTO.  Only copies and a clip happen, so every comparison against it is bit for bit."""
import torch


def gather_proposals(src: torch.Tensor, offset: int, step_stride: int, traj_stride: int, B: int, K: int, H: int, A: int) -> torch.Tensor:
    """p [B, K, H, A]: p(b, k, t, a) = src[offset + t * step_stride + (b * K + k) * traj_stride + a] of the flattened src."""
    flat = src.detach().cpu().reshape(-1)
    p = torch.empty(B, K, H, A, dtype=torch.float32)
    for b in range(B):
        for k in range(K):
            for t in range(H):
                o = offset + t * step_stride + (b * K + k) * traj_stride
                p[b, k, t] = flat[o:o + A]
    return p


def clip(p: torch.Tensor, u_min: torch.Tensor, u_max: torch.Tensor) -> torch.Tensor:
    """fminf(fmaxf(p, u_min[a]), u_max[a]) on finite p (a bound wins where p lies outside, p keeps its bits — -0.0 included — inside)."""
    return torch.minimum(torch.maximum(p, u_min.detach().cpu()), u_max.detach().cpu())


def seed(p: torch.Tensor, u_min: torch.Tensor, u_max: torch.Tensor, NC: int, P: int, actions=None, candidates=None, mean=None):
    """(actions [H, B * NC * P, A], candidates [B, NC, H, A], mean [B, H, A]) after the launch, each None where not given: clones of the
    inputs with the finite proposals written.  A proposal with any non-finite element writes nothing."""
    B, K, H, A = p.shape
    v = clip(p, u_min, u_max)
    finite = torch.isfinite(p).reshape(B, K, H * A).all(dim=-1)
    act = None if actions is None else actions.detach().cpu().clone().reshape(H, B, NC, P, A)
    cand = None if candidates is None else candidates.detach().cpu().clone().reshape(B, NC, H, A)
    mu = None if mean is None else mean.detach().cpu().clone().reshape(B, H, A)
    for b in range(B):
        for k in range(K):
            if not bool(finite[b, k]):
                continue
            if cand is not None:
                cand[b, k] = v[b, k]
                for q in range(P):
                    act[:, b, k, q, :] = v[b, k]
            if mu is not None and k == 0:
                mu[b] = v[b, 0]
    return (None if act is None else act.reshape(H, B * NC * P, A), cand, mu)
