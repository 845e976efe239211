"""CPU reference of SAC on mixed minibatches (MBPO's real_ratio) — test infrastructure, no GPU.

MixedCpuSacLoop is oracle/trainer.py:CpuSacLoop with the sampling step of SAC(real_ratio > 0): every minibatch of B rows starts
with n_real rows of a second, REAL queue (zero-padded to the model row length) and continues with the model queue's rows.  Both
index draws are Philox(seed, (site << 32) + step, stream REPLAY, element j) at the SAME element indices j = 0 .. B*G - 1: the
model draw under SITE_SAMPLE (so a model position gets the index the unmixed step draws there), the real draw under
SITE_SAMPLE_REAL with the real queue's own positions.  Everything after the batch is the parent's SGD loop.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from oracle import philox, replay, sac, trainer as otr

SAC_SITE_SAMPLE_REAL = 3      # must equal sac/sac.py:SITE_SAMPLE_REAL of the package


def mixed_rows(model_queue, model_state, real_queue, real_state, seed: int, offset: int, real_offset: int, n: int, minibatch: int,
               n_real: int):
    """(idx [n] int32, rows [n, D_model] float32) of one mixed sample: what mbpo_replay_sample_mixed computes."""
    j = np.arange(n, dtype=np.uint64)
    is_real = (np.arange(n) % minibatch) < n_real
    idx = np.zeros(n, np.int32)
    rows = np.zeros((n, model_queue.D), np.float32)
    if (~is_real).any():
        midx = philox.philox_randint(seed, offset, philox.STREAM_REPLAY, j[~is_real], int(model_state["sample_position"]),
                                     int(model_state["insert_position"]))
        idx[~is_real] = midx
        rows[~is_real] = model_queue.gather(model_state, midx)
    if is_real.any():
        ridx = philox.philox_randint(seed, real_offset, philox.STREAM_REPLAY, j[is_real], int(real_state["sample_position"]),
                                     int(real_state["insert_position"]))
        idx[is_real] = ridx
        rows[is_real, :real_queue.D] = real_queue.gather(real_state, ridx)       # columns [D_real, D_model) stay 0
    return idx, rows


@dataclass
class MixedCpuSacLoop(otr.CpuSacLoop):
    n_real: int = 0
    real_queue: Optional[replay.UniformSamplingQueue] = None
    real_qstate: Optional[dict] = None

    def __post_init__(self):
        super().__post_init__()
        if not 0 <= self.n_real <= self.batch_size:
            raise ValueError("n_real outside [0, batch_size]")
        if self.n_real > 0 and (self.real_queue is None or self.real_queue.D > self.queue.D):
            raise ValueError("n_real > 0 needs a real queue whose rows fit the model rows")
        self.model_indices_drawn = 0      # how many model indices the sampling steps consumed so far

    def training_step(self, n_sgd: Optional[int] = None):
        U = self.cfg.u_dim
        self.get_experience()
        B, G = self.batch_size, self.grad_updates
        idx, batch = mixed_rows(self.queue, self.qstate, self.real_queue, self.real_qstate, self.seed,
                                (otr.SAC_SITE_SAMPLE << 32) + self.step_index, (SAC_SITE_SAMPLE_REAL << 32) + self.step_index,
                                B * G, B, self.n_real)
        self.model_indices_drawn += (B - self.n_real) * G
        self.last_idx = idx
        self.last_batch = batch
        batch = torch.from_numpy(batch)
        nm, ns = self._norm()
        met = None
        for gi in range(G if n_sgd is None else n_sgd):                        # the parent's SGD loop
            off = ((otr.SAC_SITE_SGD + gi) << 32) + self.step_index
            noise = [otr._normal(self.seed, off, s, (B, U)) for s in (philox.STREAM_SAC_ALPHA, philox.STREAM_SAC_CRITIC, philox.STREAM_SAC_ACTOR)]
            self.state, met, _ = sac.sgd_step(self.cfg, self.state, batch[gi * B:(gi + 1) * B], *noise, nm, ns)
        self.step_index += 1
        return met
