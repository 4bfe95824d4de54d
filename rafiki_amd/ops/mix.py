"""Host twin of the mixing step prologue (``rk_gather_batch_mix``, csrc/kernels/loss_optim.hip) and the per-epoch
plan of mixup / CutMix.  It calls no kernel: the CPU engine trains through it, and the tests hold the kernel to it.

Output row b of a step is made of two images: the primary a = image of rows[b] and the partner p = image of
rows[(b + 1) % B], each augmented by its own row's draw when the engine augments (``ops/augment.py``).

  blend (mixup):  out = lam * a + (1 - lam) * p per element in fp32, stored in the data's dtype
  box (CutMix):   out[y, x] = p[y, x] for y0 <= y < y1 and x0 <= x < x1 (clamped to the image), a[y, x] elsewhere

One (lam, box) per step, shared by the whole batch as in the published recipes (Zhang et al., ICLR'18; Yun et
al., ICCV'19), drawn on the host per (seed, epoch) — a table next to the learning-rate table of the scheduled
graph, so a replay reads its step's values on the device and a resumed trial redraws the same plan.
"""
import numpy as np
import torch

from . import augment as A

MIX_STREAM = 0x6d6978   # stream constant of the plan's generator
KINDS = ('mixup', 'cutmix')
BLEND, BOX = 1, 2       # the kernel's MIX template values
MODE = {'mixup': BLEND, 'cutmix': BOX}


def plan(seed, epoch, steps, kind, alpha, prob, H, W):
    """(lam [steps] fp32, box [steps, 4] int32 rows (y0, y1, x0, x1), half-open) of one epoch.  With probability
    ``prob`` a step draws lam ~ Beta(alpha, alpha), else lam = 1 and the box is empty.  mixup folds lam to
    max(lam, 1 - lam) (the primary keeps the larger share); cutmix draws a box of area fraction about 1 - lam at
    a uniform centre, clips it to the image and sets lam = 1 - area / (H * W) as fp32 computes it."""
    if kind not in KINDS:
        raise ValueError('kind must be one of {}, got {!r}'.format(KINDS, kind))
    rng = np.random.default_rng([int(seed) & 0xFFFFFFFFFFFFFFFF, MIX_STREAM, int(epoch) & 0xFFFFFFFF])
    lam = np.ones(steps, dtype=np.float32)
    box = np.zeros((steps, 4), dtype=np.int32)
    for s in range(steps):
        # every step consumes the same five draws, mixed or not: step s of a plan does not depend on prob's luck
        # earlier in the epoch
        u, l, cy, cx = rng.random(), rng.beta(alpha, alpha), rng.random(), rng.random()
        if not u < prob:
            continue
        if kind == 'mixup':
            lam[s] = np.float32(max(l, 1.0 - l))
            continue
        r = np.sqrt(1.0 - l)
        bh, bw = int(H * r), int(W * r)
        yc, xc = int(cy * H), int(cx * W)
        y0, y1 = np.clip([yc - bh // 2, yc + (bh + 1) // 2], 0, H)
        x0, x1 = np.clip([xc - bw // 2, xc + (bw + 1) // 2], 0, W)
        box[s] = (y0, y1, x0, x1)
        lam[s] = np.float32(1.0) - np.float32((y1 - y0) * (x1 - x0)) / np.float32(H * W)
    return lam, box


def clamp_box(box, H, W):
    """(y0, y1, x0, x1) clamped into the image, as the kernel clamps a table row."""
    y0, y1, x0, x1 = (int(v) for v in box)
    return min(max(y0, 0), H), min(max(y1, 0), H), min(max(x0, 0), W), min(max(x1, 0), W)


def apply(data, rows, kind, lam, box=None, *, augment=None, seed=0, epoch=0, stream_id=A.AUG_STREAM):
    """The mixed batch of ``rows`` (already clamped to the dataset): ``data`` [N, H, W, C] on any device ->
    [B, H, W, C] in its dtype.  ``augment`` {'pad', 'flip'}: both images are first augmented by their rows' draws
    of (seed, epoch)."""
    dev = data.device
    rows = torch.as_tensor(rows, dtype=torch.int64).reshape(-1).cpu()
    partner = torch.roll(rows, -1)

    def images(r):
        if augment is None:
            return data[r.to(dev)]
        return A.apply(data, r, *A.draws(seed, r, epoch, augment['pad'], augment['flip'], stream_id))
    a, p = images(rows), images(partner)
    if MODE[kind] == BLEND:
        lam = torch.tensor(float(lam), dtype=torch.float32, device=dev)
        return (lam * a.float() + (1.0 - lam) * p.float()).to(data.dtype)
    H, W = data.shape[1], data.shape[2]
    y0, y1, x0, x1 = clamp_box((0, 0, 0, 0) if box is None else box, H, W)
    out = a.clone()
    if y1 > y0 and x1 > x0:
        out[:, y0:y1, x0:x1] = p[:, y0:y1, x0:x1]
    return out
