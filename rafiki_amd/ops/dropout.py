"""Host twin of the dropout kernel (``rk_dropout``, csrc/kernels/dropout.hip): the same keep decisions in NumPy and
the same select-and-scale in torch, on any device and dtype.  It calls no kernel: the CPU engine trains through it,
and the tests hold the kernel to it.

Element i of a dropped tensor belongs to quad q = i // 4 and uses word i % 4 of the Philox4x32-10 block at counter
(q, site, step, epoch), key (seed low word, seed high word).  It is kept iff u01(word) >= p with u01(w) = (w >> 8) *
2^-24 in fp32, and a kept element is scaled by the fp32 1 / (1 - p); a dropped one is written as zero by selection,
so a dropped inf / NaN becomes 0.  A draw depends on (seed, site, epoch, step, i) alone: nothing is stored between
the forward and the backward pass, and nothing is needed to resume a run.
"""
import numpy as np
import torch

from .augment import _MASK, _philox4x32_10, _u01

DROP_STREAM = 0x6472    # site of the feature dropout; FC hidden layer k drops at site DROP_STREAM + 1 + k


def keep(seed, site, epoch, step, n, p):
    """Bool [n]: which elements of a tensor of ``n`` elements dropped at ``site`` survive step ``step`` of
    ``epoch`` at rate ``p``."""
    n = int(n)
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    full = np.zeros(q.shape, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = _philox4x32_10(q & np.uint64(_MASK), full + np.uint64(int(site) & _MASK), full + np.uint64(int(step) & _MASK),
                       full + np.uint64(int(epoch) & _MASK), seed & _MASK, seed >> 32)
    u = np.stack([_u01(v) for v in w], axis=1).reshape(-1)[:n]
    return u >= np.float32(p)


def inv_keep(p):
    """1 / (1 - p) as the launcher forms it: both operations in fp32."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def multipliers(seed, site, epoch, step, shape, p, dtype=torch.float32, device='cpu'):
    """The 0 / (1 / (1 - p)) multipliers of a tensor of ``shape`` (row-major element order), for an autograd
    reference that multiplies where the kernel selects."""
    n = int(np.prod(shape))
    m = torch.from_numpy(keep(seed, site, epoch, step, n, p)).reshape(tuple(shape))
    return m.to(device=device, dtype=dtype) * inv_keep(p)


def apply(t, seed, site, epoch, step, p):
    """``t`` after dropout at rate ``p``: kept elements scaled (the product in fp32 for the 16-bit dtypes, rounded
    to nearest-even into t's dtype), dropped ones zero.  A new tensor; ``t`` on any device, any float dtype."""
    k = torch.from_numpy(keep(seed, site, epoch, step, t.numel(), p)).reshape(t.shape).to(t.device)
    wide = t if t.dtype in (torch.float32, torch.float64) else t.float()
    scaled = (wide * torch.tensor(inv_keep(p), dtype=wide.dtype, device=t.device)).to(t.dtype)
    return torch.where(k, scaled, torch.zeros((), dtype=t.dtype, device=t.device))
