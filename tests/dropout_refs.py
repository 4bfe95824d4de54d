"""Oracles of dropout, shared by tests/test_dropout.py (CPU: the host twin rafiki_amd/ops/dropout.py and the CPU
engine) and tests/test_dropout_gpu.py (the kernel rk_dropout, the engines and the model loops).

Nothing here goes through rafiki_amd.  The draws come from loss_optim_refs.philox4x32_10 (anchored to the published
Random123 vectors by tests/test_flat_optim.py).  A kept element is one fp32 multiply (rounded once more, to
nearest-even, for bf16) and a dropped one is a selected zero, so every kernel comparison against these is bit-exact.
"""
import numpy as np
import torch

import loss_optim_refs as R

_MASK = 0xFFFFFFFF
DROP_STREAM = 0x6472         # site of the feature dropout; FC hidden layer k is DROP_STREAM + 1 + k
SEED = (1 << 32) + 20261     # above 2^32: the key's high word matters


def keep(seed, site, epoch, step, n, p):
    """Bool [n]: element i is kept iff u01(word i % 4 of the Philox block at counter (i // 4, site, step, epoch),
    key (seed low, seed high)) >= p, with u01(w) = (w >> 8) * 2^-24 in fp32."""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    w = R.philox4x32_10((q, int(site) & _MASK, int(step) & _MASK, int(epoch) & _MASK),
                        (int(seed) & _MASK, (int(seed) >> 32) & _MASK)).reshape(-1)[:n]
    u = (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u >= np.float32(p)


def inv_keep(p):
    """1 / (1 - p) with both operations in fp32, as a Python float."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def dropped(x, seed, site, epoch, step, p):
    """The tensor the kernel leaves in place of the contiguous fp32 / bf16 tensor ``x`` (host)."""
    k = torch.from_numpy(keep(seed, site, epoch, step, x.numel(), p)).reshape(x.shape)
    scaled = (x.float() * torch.tensor(inv_keep(p), dtype=torch.float32)).to(x.dtype)
    return torch.where(k, scaled, torch.zeros((), dtype=x.dtype))


def multipliers(seed, site, epoch, step, shape, p, dtype=torch.float64):
    """0 / (1 / (1 - p)) per element of a tensor of ``shape``, for an autograd reference."""
    k = torch.from_numpy(keep(seed, site, epoch, step, int(np.prod(shape)), p)).reshape(tuple(shape))
    return k.to(dtype) * inv_keep(p)


def engine_multipliers(seed, epoch, step, B, feat_dim, hidden, p, feat_p, dtype=torch.float64):
    """{site: multipliers} of a conv net's step: the features [B, feat_dim] at rate ``feat_p`` and hidden layer k
    [B, hidden[k]] (padded widths) at rate ``p``; a rate of 0 leaves its sites out."""
    out = {}
    if feat_p > 0:
        out[DROP_STREAM] = multipliers(seed, DROP_STREAM, epoch, step, (B, feat_dim), feat_p, dtype)
    if p > 0:
        for k, d in enumerate(hidden):
            out[DROP_STREAM + 1 + k] = multipliers(seed, DROP_STREAM + 1 + k, epoch, step, (B, d), p, dtype)
    return out
