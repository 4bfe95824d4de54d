"""fp64 references and input sets for the kernels of csrc/kernels/loss_optim.hip and the Philox stream,
shared by tests/test_flat_optim.py (CPU: the references against torch.optim / the published Philox vectors,
and how far a wrong formula moves them) and tests/test_loss_optim_gpu.py (the kernels against them).

Nothing here calls a kernel of this project.  The optimizer formulas take the dtype of their inputs, so the
same function gives the fp64 reference and, where needed, a plain fp32 evaluation.

Error measure everywhere: err(a, ref) = max |a - ref| / max |ref| (max norm, so four wrong elements in four
million are not averaged away).  Tolerance of an fp32 kernel output: 4 * e_ref, e_ref = err of the project's
own fp32 CPU path (or of plain fp32 PyTorch / NumPy) against the same fp64 reference on the same inputs.
"""
import math

import numpy as np
import torch

TOL_FACTOR = 4.0        # kernel error <= TOL_FACTOR * e_ref
SENSITIVITY = 10.0      # a wrong formula must move the reference by >= SENSITIVITY * tolerance
# fixed bounds where plain fp32 PyTorch is exact to rounding but the kernel is not (__expf / __logf, bf16
# stores): the ones tests/test_kernels_gpu.py::test_softmax_xent applies
LOSS_TOL, PROB_TOL, BF16_REL = 1e-4, 1e-5, 1e-2


def err(a, ref):
    a, ref = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    if a.numel() == 0:
        return 0.0
    return ((a - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


# ------------------------------------------------------------------------------------------- Philox
_M0, _M1, _W0, _W1, _MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., SC'11) of counters ctr = (c0, c1, c2, c3) (ints or equal-length integer
    arrays) under key = (k0, k1): uint32 array [..., 4]."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) for c in ctr])
    k0, k1 = int(key[0]) & _MASK, int(key[1]) & _MASK
    m0, m1, mask, sh = np.uint64(_M0), np.uint64(_M1), np.uint64(_MASK), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2          # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ np.uint64(k0), p1 & mask, (p0 >> sh) ^ c3 ^ np.uint64(k1), p0 & mask
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def philox_words(n, seed, stream_id, step=None):
    """The n 32-bit words philox_kernel draws for (seed, stream_id, *step): element 4q + j is word j of counter
    (q low, q high, stream_id, step), key (seed low, seed high); no step tensor counts as step 0."""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    st = 0 if step is None else int(step) & _MASK
    w = philox4x32_10((q & np.uint64(_MASK), q >> np.uint64(32), int(stream_id) & _MASK, st),
                      (int(seed) & _MASK, (int(seed) >> 32) & _MASK))
    return w.reshape(-1)[:n]


def philox_uniform(n, seed, stream_id, step=None):
    """fp32 [0, 1): (x >> 8) * 2^-24, exact in fp32."""
    return (philox_words(n, seed, stream_id, step) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def philox_randint(n, hi, seed, stream_id, step=None):
    u = philox_uniform(n, seed, stream_id, step)
    v = (u * np.float32(hi)).astype(np.int64)     # the fp32 product, truncated
    return np.minimum(v, hi - 1).astype(np.int32)


def philox_normal(n, seed, stream_id, step=None, dtype=np.float64):
    """Box-Muller over word pairs (j, j + 1): radius from the (0, 1] uniform of word j, angle from the [0, 1)
    uniform of word j + 1; element j takes the cosine, j + 1 the sine.  dtype float64: the reference;
    float32: every operation in fp32 (the yardstick for the kernel's error)."""
    w = philox_words(4 * ((n + 3) // 4), seed, stream_id, step) >> np.uint32(8)
    dt = np.dtype(dtype).type
    u1 = (w[0::2].astype(dtype) + dt(1)) * dt(2.0 ** -24)
    u2 = w[1::2].astype(dtype) * dt(2.0 ** -24)
    rad = np.sqrt(dt(-2) * np.log(u1))
    ang = dt(2 * math.pi) * u2
    out = np.empty(w.shape, dtype=dtype)
    out[0::2], out[1::2] = rad * np.cos(ang), rad * np.sin(ang)
    assert out.dtype == np.dtype(dtype)
    return out[:n]


PHILOX_SEEDS = ((1 << 32) + 12345, 0xDEADBEEF12345678)     # both above 2^32: the key's high word matters
PHILOX_STREAMS = (3, 0x9E3779B1)
PHILOX_STEPS = (None, 0, 5)
PHILOX_SIZES = (7, 1024 + 3)


# ------------------------------------------------------------------------------------------- optimizers
def sgd_ref(w, g, mom, *, lr, momentum, wd, nesterov, decay_end, lr_scale=1.0, grad_scale=1.0):
    """One SGD step out of place in the dtype of w: weight decay on [0, decay_end), torch.optim.SGD's momentum
    (buffer = momentum * buffer + g, zero dampening) and Nesterov forms.  mom None: no momentum."""
    wdv = torch.zeros_like(w)
    wdv[:decay_end] = wd
    gg = g * grad_scale + wdv * w
    d = gg
    if mom is not None:
        mom = mom * momentum + gg
        d = gg + momentum * mom if nesterov else mom
    return w - (lr * lr_scale) * d, mom


def adam_ref(w, g, m, v, *, lr, b1, b2, eps, wd, decoupled, t, grad_scale=1.0, drop_c1=False, omb2=None):
    """One Adam (coupled decay: torch.optim.Adam) or AdamW (decoupled) step out of place in the dtype of w, t
    the 1-based step.  drop_c1 / omb2: the wrong formulas of the sensitivity checks (no first-moment bias
    correction; 1 - beta2 as given, e.g. formed from the fp32 beta2)."""
    gg = g * grad_scale
    if not decoupled:
        gg = gg + wd * w
    m = m * b1 + (1.0 - b1) * gg
    v = v * b2 + ((1.0 - b2) if omb2 is None else omb2) * gg * gg
    c1 = 1.0 / (1.0 - b1 ** t) if b1 > 0 and not drop_c1 else 1.0
    c2 = 1.0 / (1.0 - b2 ** t)
    upd = (m * c1) / ((v * c2).sqrt() + eps)
    if decoupled:
        upd = upd + wd * w
    return w - lr * upd, m, v


def fresh_grads(n, steps, seed):
    """steps fp32 gradient vectors, each with exact zeros and 1e-12 among N(0, 1) values."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(steps):
        g = torch.randn(n, generator=gen)
        g[torch.rand(n, generator=gen) < 0.1] = 0.0
        g[torch.rand(n, generator=gen) < 0.1] = 1e-12
        g[0], g[n - 1] = 0.0, 1e-12
        out.append(g)
    return out


def bare_arena(device, w0, decay_end, with_bf16):
    """A FlatParams of exactly w0.numel() elements (build() rounds sizes up to 64; the kernels take any
    multiple of 4): master = w0, decay on [0, decay_end)."""
    from rafiki_amd.engine.flat import FlatParams
    f = FlatParams(torch.device(device), compute_bf16=with_bf16)
    f.master = w0.clone().to(f.device)
    f.grad = torch.zeros_like(f.master)
    f.bf16 = f.master.to(torch.bfloat16) if with_bf16 else None
    f.total, f.decay_end = w0.numel(), int(decay_end)
    return f


SGD_HP = dict(lr=0.1, wd=5e-2)      # a decay this large keeps a 4-element shift of decay_end visible
SGD_MODES = {'plain': dict(momentum=0.0, nesterov=False), 'momentum': dict(momentum=0.9, nesterov=False),
             'nesterov': dict(momentum=0.9, nesterov=True)}
SGD_SCALES = (1.0, 0.25, 0.0, 1.0, 0.25)    # the device LR multiplier of each of the 5 steps
SGD_SIZES = (4, 1028, 4104, 4 * (4096 * 256) + 308)   # the last: past one grid of 4096 blocks x 256 x 4


def sgd_decay_ends(n):
    return sorted({0, 4, n // 2 // 4 * 4, n})


def sgd_inputs(n, seed=11):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=gen), fresh_grads(n, len(SGD_SCALES), seed + 1)


def run_sgd_ref(w0, grads, *, mode, decay_end, scales=SGD_SCALES, grad_scale=1.0, lr=SGD_HP['lr'], wd=SGD_HP['wd'],
                dtype=torch.float64, nesterov=None):
    """(w, mom) after the steps by sgd_ref in dtype."""
    hp = SGD_MODES[mode]
    w = w0.to(dtype)
    mom = torch.zeros_like(w) if hp['momentum'] > 0 else None
    for g, s in zip(grads, scales):
        w, mom = sgd_ref(w, g.to(dtype), mom, lr=lr, momentum=hp['momentum'], wd=wd,
                         nesterov=hp['nesterov'] if nesterov is None else nesterov, decay_end=decay_end,
                         lr_scale=s, grad_scale=grad_scale)
    return w, mom


def run_flat_sgd(device, w0, grads, *, mode, decay_end, scales=SGD_SCALES, with_bf16=False, bump=None,
                 lr=SGD_HP['lr'], wd=SGD_HP['wd'], on_step=None):
    """FlatSGD.step on device (cpu: the project's reference path; cuda: rk_sgd_step) -> (arena, optimizer)."""
    from rafiki_amd.engine.flat import FlatSGD
    hp = SGD_MODES[mode]
    f = bare_arena(device, w0, decay_end, with_bf16)
    opt = FlatSGD(f, lr, momentum=hp['momentum'], weight_decay=wd, nesterov=hp['nesterov'])
    opt.bump = bump
    for i, (g, s) in enumerate(zip(grads, scales)):
        f.grad.copy_(g)
        opt.set_lr_scale(s)
        before = f.master.clone() if on_step is not None else None
        opt.step()
        if on_step is not None:
            on_step(i, s, before, f, opt)
    return f, opt


def adam_arena(device, with_bf16=True, seed=0):
    """An arena in the layout of tests/test_multiseg_gpu.py::_flat, smaller: six parameters of odd sizes,
    every other one decayed, each with its own equalized-LR multiplier."""
    from rafiki_amd.engine.flat import FlatParams, init_const
    f = FlatParams(torch.device(device), compute_bf16=with_bf16)
    for i, n in enumerate((2000, 33, 4096, 517, 20001, 8)):
        f.add('p{}'.format(i), (n,), init_const(0.0), decay=i % 2 == 0, lr_mult=1.0 + 0.37 * i)
    f.build()
    gen = torch.Generator().manual_seed(seed)
    # weights no larger than a few steps of lr: the update, not the start value, carries the error
    f.master.copy_(0.05 * torch.randn(f.total, generator=gen))
    f.sync_bf16()
    return f


ADAM_HP = dict(lr=1e-2, eps=1e-8, wd=1e-2)
ADAM_BETAS = [(b1, b2) for b1 in (0.0, 0.9) for b2 in (0.99, 0.999)]
ADAM_DECAY = {'none': (0.0, False), 'coupled': (ADAM_HP['wd'], False), 'decoupled': (ADAM_HP['wd'], True)}
ADAM_STEPS = 5
# a power of two: g * scale is then exact, so the CPU path fed pre-scaled gradients (it has no grad_scale of
# its own) carries no rounding the kernel does not, and e_ref stays the formula's own
ADAM_GRAD_SCALE = 0.25
SGD_GRAD_SCALE = 0.3
ADAM_LIVE = ['p0', 'p1', 'p4', 'p5']    # p2 and p3 stay out of the live set


def live_segments(f, wd, live):
    """FlatAdam.step's segment list [(a, b, wd, lr_mult)] cut to the live ranges (None: the whole arena)."""
    segs = f.segments(wd)
    if live is not None:
        segs = [(max(a, c), min(b, d), w, mult) for a, b, w, mult in segs for c, d in live if min(b, d) > max(a, c)]
    return segs


def run_adam_ref(f0, grads, *, b1, b2, wd, decoupled, live=None, grad_scale=1.0, lr=ADAM_HP['lr'],
                 eps=ADAM_HP['eps'], dtype=torch.float64, **wrong):
    """(w, m, v) after the steps by adam_ref in dtype, per segment with lr * mult and eps * mult.  f0: an
    arena holding the start weights (not changed)."""
    w = f0.master.detach().cpu().to(dtype).clone()
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    segs = live_segments(f0, wd, live)
    for t, g in enumerate(grads, 1):
        g = g.to(dtype)
        for a, b, swd, mult in segs:
            w[a:b], m[a:b], v[a:b] = adam_ref(w[a:b], g[a:b], m[a:b], v[a:b], lr=lr * mult, b1=b1, b2=b2,
                                              eps=eps * mult, wd=swd, decoupled=decoupled, t=t,
                                              grad_scale=grad_scale, **wrong)
    return w, m, v


def run_flat_adam(f, grads, *, b1, b2, wd, decoupled, live=None, lr=ADAM_HP['lr'], eps=ADAM_HP['eps'],
                  skip_flag=None):
    """FlatAdam.step on f's device (cpu: the project's reference path) -> the optimizer."""
    from rafiki_amd.engine.flat import FlatAdam
    opt = FlatAdam(f, lr, betas=(b1, b2), eps=eps, weight_decay=wd, decoupled=decoupled)
    opt.skip_flag = skip_flag
    for g in grads:
        f.grad.copy_(g)
        opt.step(live=live)
    return opt


def tolerances(got32, ref64):
    """[4 * e_ref] of each output of an fp32 CPU evaluation against the fp64 reference."""
    return [None if r is None else TOL_FACTOR * err(a, r) for a, r in zip(got32, ref64)]


# ------------------------------------------------------------------------------------------- lerp
LERP_T = (0.0, 0.5, 0.99, 1.0)


def lerp_ref(dst, src, t):
    """tf lerp(a=src, b=dst, t) = src + (dst - src) * t, in the dtype of dst."""
    return src + (dst - src) * t


# ------------------------------------------------------------------------------------------- softmax
IGNORE = -100
XENT_B = (1, 3, 5, 301)
XENT_NCLS = (1, 2, 10, 63, 64, 65, 130, 200)


def xent_inputs(B, ncls, padded, seed=0, big=False):
    """logits [B, ld] fp32 (ld = ncls, or ncls + 5 columns of a large sentinel that a broken bound would fold
    into the sums) and int32 labels; with a padded stride every fourth row's label is one of IGNORE, -1 and
    ncls.  big: every row's logits span +-80."""
    gen = torch.Generator().manual_seed(seed * 1000 + B * 7 + ncls)
    ld = ncls + 5 if padded else ncls
    logits = torch.full((B, ld), 30.0)
    logits[:, :ncls] = torch.randn(B, ncls, generator=gen) * 3
    if big:
        logits[:, :ncls] = (torch.rand(B, ncls, generator=gen) * 160 - 80)
        logits[:, 0] = 80.0
        if ncls > 1:
            logits[:, ncls - 1] = -80.0
    labels = torch.randint(0, ncls, (B,), generator=gen, dtype=torch.int32)
    if padded:
        bad = (IGNORE, -1, ncls)
        for i in range(0, B, 4):
            labels[i] = bad[(i // 4) % 3]
    return logits, labels


def xent_ref(logits, labels, ncls, *, grad_scale, scale=1.0, count_ignored=False):
    """fp64 softmax cross-entropy of logits[:, :ncls]: dict of loss_sum, counted, correct (first index of the
    row maximum, NumPy on the host), probs [B, ncls], dlogits [B, ncls].  Rows whose label is IGNORE or outside
    [0, ncls) give no loss, no count and a zero gradient.  count_ignored: the wrong formula of the sensitivity
    check (such rows count, with class 0 standing in)."""
    x = logits[:, :ncls].double()
    lsm = torch.log_softmax(x, 1)
    p = lsm.exp()
    y = labels.long()
    valid = (y != IGNORE) & (y >= 0) & (y < ncls)
    if count_ignored:
        y = torch.where(valid, y, torch.zeros_like(y))
        valid = torch.ones_like(valid)
    yc = torch.where(valid, y, torch.zeros_like(y))
    onehot = torch.zeros_like(p).scatter_(1, yc[:, None], 1.0)
    rows = -lsm.gather(1, yc[:, None])[:, 0]
    amax = torch.from_numpy(np.argmax(logits[:, :ncls].numpy(), axis=1))
    return dict(loss_sum=(rows * valid).sum().item() * scale, counted=int(valid.sum()),
                correct=int(((amax == yc) & valid).sum()), probs=p,
                dlogits=(p - onehot) * valid[:, None] * (grad_scale * scale))


# ------------------------------------------------------------------------------------------- gather
def gather_ref(data, labels, sched, counter, nrows):
    """Rows sched[counter mod nsteps] of data / labels (NumPy), indices outside [0, nrows) reading row 0."""
    idx = np.asarray(sched)[counter % len(sched)].copy()
    idx[(idx < 0) | (idx >= nrows)] = 0
    return np.asarray(data)[idx], np.asarray(labels)[idx]


LR_SCALES = [1.0, 0.25, 0.0, 0.5]     # the scheduled-graph test's per-step LR multipliers
