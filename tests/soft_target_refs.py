"""Oracles of the soft-target loss and of the mixing step prologue, shared by tests/test_soft_target.py (CPU: the
host twin rafiki_amd/ops/mix.py, the engine's reference path) and tests/test_soft_target_gpu.py (the kernels).

Nothing here goes through rafiki_amd.  The loss is fp64 PyTorch; the mixing is a plain loop over pixels of two
already gathered (and, where the case augments, already cropped by augment_refs.crop) image stacks.
"""
import numpy as np
import torch

import loss_optim_refs as R

# (lam, eps) of the loss tests; lam None: no lam pointer (the kernel takes 1)
LAM_EPS = ((1.0, 0.0), (0.0, 0.0), (0.5, 0.0), (0.7311, 0.1), (None, 0.1))
XENT_NCLS = (1, 2, 10, 64, 65, 130)
HEAD_SHAPES = ((256, 512, 16, 10, True), (37, 96, 8, 5, True), (64, 2048, 32, 20, False), (5, 32, 16, 16, True))
BLEND_LAMS = (1.0, 0.0, 0.5, 0.7311)
# fp32 roundings of out = lam * a + (1 - lam) * p as the kernel writes it: 1 - lam, lam * a, (1 - lam) * p and the
# sum, each at most 2^-24 relative to a value no larger than max(|a|, |p|) (lam and 1 - lam lie in [0, 1])
BLEND_K = 4


def f32(v):
    """The fp64 value of v rounded to fp32 (what a float argument or table entry holds)."""
    return float(np.float32(v))


def valid_labels(y, ncls):
    return (y != R.IGNORE) & (y >= 0) & (y < ncls)


def soft_target(ya, yb, ncls, lam, eps):
    """t [B, ncls] fp64 = (1 - eps) * (lam * onehot(ya) + (1 - lam) * onehot(yb)) + eps / ncls; ya, yb valid."""
    one = torch.zeros(len(ya), ncls, dtype=torch.float64).scatter_(1, ya[:, None], 1.0)
    two = torch.zeros(len(yb), ncls, dtype=torch.float64).scatter_(1, yb[:, None], 1.0)
    return (1.0 - eps) * (lam * one + (1.0 - lam) * two) + eps / ncls


def soft_xent_ref(logits, labels, ncls, *, labels2=None, lam=None, eps=0.0, grad_scale):
    """fp64 soft-target cross-entropy of logits[:, :ncls]: dict of loss_rows [B], loss_sum, counted, correct,
    dlogits [B, ncls].  labels2 None: smoothing only (lam is not used); lam None: 1.  A row is valid when labels
    and, if given, labels2 are; an invalid row gives no loss, no count and a zero gradient.  A row is correct
    when the first index of its maximum is the label with the larger share (labels when lam >= 0.5)."""
    x = logits[:, :ncls].double()
    lsm = torch.log_softmax(x, 1)
    ya = labels.long()
    yb = ya if labels2 is None else labels2.long()
    w = 1.0 if labels2 is None or lam is None else f32(lam)
    valid = valid_labels(ya, ncls) & valid_labels(yb, ncls)
    zero = torch.zeros_like(ya)
    t = soft_target(torch.where(valid, ya, zero), torch.where(valid, yb, zero), ncls, w, f32(eps))
    rows = -(t * lsm).sum(1) * valid
    amax = torch.from_numpy(np.argmax(logits[:, :ncls].numpy(), axis=1))
    tgt = ya if w >= 0.5 else yb
    return dict(loss_rows=rows, loss_sum=rows.sum().item(), counted=int(valid.sum()),
                correct=int(((amax == tgt) & valid).sum()), dlogits=(lsm.exp() - t) * valid[:, None] * grad_scale)


def second_labels(labels, ncls, seed, spoil_only_second=False):
    """Partner labels [B] int32: a fixed non-zero rotation of the classes where there are two or more (so every
    mixed row has two different labels), else the label itself.  An invalid label stays invalid.
    spoil_only_second: every third row gets an invalid partner although its own label may be valid."""
    y = labels.long()
    ok = valid_labels(y, ncls)
    gen = torch.Generator().manual_seed(seed)
    rot = torch.randint(1, max(2, ncls), (len(y),), generator=gen)
    y2 = torch.where(ok, (y + rot) % ncls if ncls > 1 else y, y)
    if spoil_only_second:
        bad = torch.tensor([R.IGNORE, -1, ncls])
        y2[::3] = bad[torch.arange(len(y2[::3])) % 3]
    return y2.to(torch.int32)


def clamp_box(box, H, W):
    y0, y1, x0, x1 = (int(v) for v in box)
    return min(max(y0, 0), H), min(max(y1, 0), H), min(max(x0, 0), W), min(max(x1, 0), W)


def box_mix(a, p, box):
    """out[b, y, x] = p[b, y, x] for y0 <= y < y1 and x0 <= x < x1 (as given: NOT clamped here; a pixel loop
    over the image only), a[b, y, x] elsewhere."""
    y0, y1, x0, x1 = (int(v) for v in box)
    out = np.array(a, copy=True)
    _, H, W, _ = out.shape
    for y in range(H):
        for x in range(W):
            if y0 <= y < y1 and x0 <= x < x1:
                out[:, y, x] = p[:, y, x]
    return out


def blend_mix(a, p, lam):
    """fp64 lam * a + (1 - lam) * p with lam the fp32 table value."""
    lam = f32(lam)
    return lam * np.asarray(a, dtype=np.float64) + (1.0 - lam) * np.asarray(p, dtype=np.float64)


def blend_bound(a, p, ref, bf16):
    """Elementwise bound on |kernel - fp64 blend|: BLEND_K fp32 roundings of values no larger than max(|a|, |p|),
    plus, for bf16 storage, half a bf16 ulp of the stored result (at most 2^-8 of its magnitude)."""
    e32 = BLEND_K * 2.0 ** -24 * np.maximum(np.abs(a), np.abs(p)).astype(np.float64)
    if not bf16:
        return e32
    return e32 + 2.0 ** -8 * (np.abs(ref) + e32)


def partner(rows):
    """Row b's partner is row (b + 1) % B of the same batch."""
    return np.roll(np.asarray(rows), -1)


# box cases on the 6 x 10 images of augment_refs: (y0, y1, x0, x1) half-open
BOXES = {'empty': (0, 0, 0, 0), 'pixel': (2, 3, 4, 5), 'corner': (3, 6, 7, 10), 'whole': (0, 6, 0, 10),
         'past': (-3, 4, 6, 25), 'inverted': (4, 2, 5, 1)}
