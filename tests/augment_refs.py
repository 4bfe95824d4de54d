"""Oracles of the crop-and-mirror augmentation, shared by tests/test_augment.py (CPU: the host twin
rafiki_amd/ops/augment.py) and tests/test_augment_gpu.py (the prologue kernel rk_gather_batch_aug and the engine).

Nothing here goes through rafiki_amd.  The draws come from loss_optim_refs.philox4x32_10 (anchored to the
published Random123 vectors by tests/test_flat_optim.py); the crop is a plain loop over pixels.  Images are
copied and never computed with, so every comparison against these is bit-exact.
"""
import functools

import numpy as np

import loss_optim_refs as R

_MASK = 0xFFFFFFFF


def draws(seed, rows, epoch, pad, flip_p, stream_id):
    """(dy, dx, flip) per dataset row: one Philox block per row, counter (row low, row high, stream_id, epoch),
    key (seed low, seed high); dy, dx = randint(w0 / w1, 2 pad + 1) - pad, flip = u01(w2) < flip_p, where
    u01(w) = (w >> 8) * 2^-24 and randint(w, hi) = min(int(u01(w) * hi), hi - 1), both in fp32."""
    rows = [int(r) for r in np.asarray(rows).reshape(-1)]
    w = R.philox4x32_10(([r & _MASK for r in rows], [r >> 32 for r in rows], int(stream_id) & _MASK,
                         int(epoch) & _MASK), (int(seed) & _MASK, (int(seed) >> 32) & _MASK))
    u = (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    span = 2 * pad + 1

    def shift(col):
        v = (u[:, col] * np.float32(span)).astype(np.int64)
        return np.minimum(v, span - 1) - pad
    return shift(0), shift(1), u[:, 2] < np.float32(flip_p)


def crop(data, rows, dy, dx, flip):
    """out[b, y, x] = data[rows[b], y + dy[b], (flip[b] ? W - 1 - x : x) + dx[b]] inside the image, else 0."""
    data = np.asarray(data)
    _, H, W, C = data.shape
    out = np.zeros((len(rows), H, W, C), dtype=data.dtype)
    for b, r in enumerate(rows):
        for y in range(H):
            for x in range(W):
                sy, sx = y + int(dy[b]), (W - 1 - x if flip[b] else x) + int(dx[b])
                if 0 <= sy < H and 0 <= sx < W:
                    out[b, y, x] = data[r, sy, sx]
    return out


def clamp_rows(idx, nrows):
    """The prologue's clamp: a row index outside [0, nrows) reads row 0."""
    idx = np.asarray(idx).astype(np.int64).copy()
    idx[(idx < 0) | (idx >= nrows)] = 0
    return idx


# --------------------------------------------------------------------------- the inputs of the kernel test
SEED = (1 << 32) + 20261     # above 2^32: the key's high word matters
STREAM = 0x51ab
NROWS, NSTEPS, H, W = 40, 3, 6, 10
EPOCHS = (None, 0, 5)        # no epoch pointer counts as epoch 0
PAD_FLIP = ((0, 0.0), (0, 1.0), (2, 0.0), (2, 0.5), (5, 0.5))
# channels and dtype per format -> 16-byte vectors per pixel 1, 2, 3
FORMATS = {'bf16c8': ('bfloat16', 8), 'f32c8': ('float32', 8), 'f32c12': ('float32', 12)}


@functools.lru_cache(maxsize=None)
def all_rows_draws(pad, flip_p, epoch):
    return draws(SEED, np.arange(NROWS), 0 if epoch is None else epoch, pad, flip_p, STREAM)
