"""Host twin of the augmenting step prologue (``rk_gather_batch_aug``, csrc/kernels/loss_optim.hip): the same
random-crop and mirror draws in NumPy and the same copy in torch, on any device.  It calls no kernel: the CPU
engine trains through it, and the tests hold the kernel to it.

One Philox4x32-10 block per sample: counter (row low word, row high word, AUG_STREAM, epoch), key (seed low,
seed high) -> dy = randint(w0, 2 * pad + 1) - pad, dx = randint(w1, 2 * pad + 1) - pad, flip = u01(w2) < flip_p,
with u01(w) = (w >> 8) * 2^-24 and randint(w, hi) = min(int(u01(w) * hi), hi - 1), both in fp32.  A draw
depends on (seed, epoch, row) alone: the same image in the same epoch is augmented the same way wherever it
lands in a batch.
"""
import numpy as np
import torch

AUG_STREAM = 0x6175     # Philox stream id of the augmentation draws

_M0, _M1, _W0, _W1, _MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def _philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) over uint64 arrays holding 32-bit counter words."""
    m0, m1, mask, sh = np.uint64(_M0), np.uint64(_M1), np.uint64(_MASK), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ np.uint64(k0), p1 & mask, (p0 >> sh) ^ c3 ^ np.uint64(k1), p0 & mask
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def _u01(w):
    return (w >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def draws(seed, rows, epoch, pad, flip_p, stream_id=AUG_STREAM):
    """(dy, dx, flip) of each dataset row in ``rows`` (any integer array or tensor) at ``epoch``: int32 shifts
    in [-pad, pad] and a bool mirror flag, as NumPy arrays of the shape of ``rows``."""
    if torch.is_tensor(rows):
        rows = rows.detach().cpu().numpy()
    r = np.asarray(rows).astype(np.int64).astype(np.uint64)
    mask = np.uint64(_MASK)
    full = np.full(r.shape, 0, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w0, w1, w2, _ = _philox4x32_10(r & mask, r >> np.uint64(32), full + np.uint64(int(stream_id) & _MASK),
                                   full + np.uint64(int(epoch) & _MASK), seed & _MASK, seed >> 32)
    span = 2 * int(pad) + 1

    def shift(w):
        v = (_u01(w) * np.float32(span)).astype(np.int64)     # the fp32 product, truncated
        return (np.minimum(v, span - 1) - int(pad)).astype(np.int32)
    return shift(w0), shift(w1), _u01(w2) < np.float32(flip_p)


def apply(data, rows, dy, dx, flip):
    """out[b, y, x, :] = data[rows[b], y + dy[b], (flip[b] ? W - 1 - x : x) + dx[b], :] where that pixel lies
    inside the image, zero elsewhere.  ``data`` [N, H, W, C] on any device; the result has its dtype."""
    dev = data.device
    H, W = data.shape[1], data.shape[2]
    rows = torch.as_tensor(rows, dtype=torch.int64, device=dev).reshape(-1)
    dy = torch.as_tensor(np.asarray(dy), dtype=torch.int64, device=dev).reshape(-1, 1)
    dx = torch.as_tensor(np.asarray(dx), dtype=torch.int64, device=dev).reshape(-1, 1)
    flip = torch.as_tensor(np.asarray(flip), dtype=torch.bool, device=dev).reshape(-1, 1)
    y = torch.arange(H, device=dev).unsqueeze(0)
    x = torch.arange(W, device=dev).unsqueeze(0)
    sy = y + dy                                       # [B, H]
    sx = torch.where(flip, W - 1 - x, x) + dx         # [B, W]
    inside = ((sy >= 0) & (sy < H)).unsqueeze(2) & ((sx >= 0) & (sx < W)).unsqueeze(1)
    got = data[rows.view(-1, 1, 1), sy.clamp(0, H - 1).unsqueeze(2), sx.clamp(0, W - 1).unsqueeze(1)]
    return torch.where(inside.unsqueeze(-1), got, torch.zeros((), dtype=data.dtype, device=dev))
