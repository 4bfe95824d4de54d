"""fp64 formulas, input sets and tolerances for the BatchNorm kernels of csrc/kernels/bn.hip (bf16) and
csrc/kernels/bnf.hip (fp32), shared by tests/test_bn_refs.py (CPU: the formulas against torch autograd, and
how far a wrong formula moves them) and tests/test_bn_gpu.py (the kernels against them).

Nothing here calls a kernel of this project.  Every formula is written out (no autograd) and takes a
``dtype``: float64 gives the reference, float32 the yardstick for the error of fp32 arithmetic.  Activations
are NHWC, [N, H, W, C]; pooling is 2x2, stride 2, floor mode, window order (0,0), (0,1), (1,0), (1,1).

Tolerances (judged per channel, err_c = max over the channel's elements of |got - ref|):
  fp32 output    err_c <= 4 * max(e_ref * max|ref_c|, a_c): a_c is the fp32 yardstick's own error in channel
                 c and e_ref its largest relative error a_c / max|ref_c| over the well-conditioned channels
                 (floored at 2^-23).  A well-conditioned channel is therefore held to 4 * e_ref * max|ref_c|;
                 the two deliberately ill-conditioned ones (CONST: variance 0, sum dz*xhat cancels to 0; OFF:
                 mean = 8 std, E[x^2] - mean^2 cancels) to four times what fp32 itself loses there.  Neither is
                 wider than 4 x the largest relative yardstick error over all channels.
                 Where the output is, or comes from, a sum over pixels, the yardstick is the largest error of
                 ORDERS fp32 summation orders and a_c is not taken below one rounding of every term
                 (sum_floor).  Where the reference itself is only known to some uncertainty (the order a slot
                 table was added in; the fp32 fold of more than 512 partial rows) that is granted on top
                 (bwd_refs, finalize_refs).
  bf16 tensor    |got - ref| <= 2^-8 |ref| + 4 a_c elementwise (one bf16 rounding plus the fp32 yardstick).
"""
import functools
import math

import torch

ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
ACTS = (ACT_NONE, ACT_RELU, ACT_LRELU)
SLOPE = 0.2
NEG_SLOPE = -0.2                              # a non-monotone leaky ReLU: routing on z and on act(z) differ
NEG_SLOPE_SHAPE = (4, 8, 8, 64)               # the cases that also run it (pooled)
GUARD = 2.0 ** -20
TOL_FACTOR = 4.0
SENSITIVITY = 10.0
E_FLOOR = 2.0 ** -23
BF16_ULP = 2.0 ** -8
FROB = 1e-5                                   # the file-level gate of tests/test_f32_gpu.py
HYPER = ((1e-5, 0.1), (1e-3, 0.01))           # (eps, momentum)
# the per-channel parameter set of every case: channel -> what it is
ZERO, BIG, CONST, OFF = 0, 1, 2, 3            # gamma = 0 (beta = 0: z == 0), gamma = -8, y constant, mean = 8 std
CONST_Y, CONST_BETA = 0.5, 0.75

F64, F32 = torch.float64, torch.float32


# ------------------------------------------------------------------------------------------- formulas
def act_f(z, act, slope=SLOPE):
    if act == ACT_RELU:
        return torch.where(z > 0, z, torch.zeros_like(z))
    if act == ACT_LRELU:
        return torch.where(z > 0, z, z * slope)
    return z


def act_d(z, act, slope=SLOPE):
    one = torch.ones_like(z)
    if act == ACT_RELU:
        return torch.where(z > 0, one, torch.zeros_like(z))
    if act == ACT_LRELU:
        return torch.where(z > 0, one, one * slope)
    return one


def windows(x):
    """[N, H, W, C] -> [N, H//2, W//2, C, 4]: the floor-mode 2x2 windows, positions (0,0), (0,1), (1,0), (1,1)."""
    N, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    return x[:, :2 * Ho, :2 * Wo].reshape(N, Ho, 2, Wo, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(N, Ho, Wo, C, 4)


def unwindow(xw, H, W):
    """The inverse of windows(); the last row / column of an odd map, which no window covers, is zero."""
    N, Ho, Wo, C, _ = xw.shape
    full = torch.zeros((N, H, W, C), dtype=xw.dtype, device=xw.device)
    full[:, :2 * Ho, :2 * Wo] = xw.reshape(N, Ho, Wo, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(N, 2 * Ho, 2 * Wo, C)
    return full


def spread(dout, H, W):
    """The pooled-map gradient copied to all four positions of its window."""
    return unwindow(dout.unsqueeze(-1).expand(*dout.shape, 4), H, W)


ORDERS = 6      # fp32 summation orders a sum's yardstick is taken over (the largest error of them, per channel)


def _prod(a, b, dtype, order):
    """a * b for a sum.  An odd fp32 order rounds the exact product once, as a fused multiply-add chain keeps it,
    instead of multiplying two rounded factors."""
    if dtype == F32 and order % 2:
        return (a.to(F64) * b.to(F64)).to(F32)
    return a.to(dtype) * b.to(dtype)


def colsum(v, order=0):
    """Column sums of [P, C].  In fp32 as interleaved sequential chains (the shape of a kernel's per-thread
    accumulators), then one sum over the chains: PyTorch's own pairwise fp32 sum is more accurate than any
    streaming kernel and would make the yardstick too strict by the summation order alone.  ``order`` > 0 permutes
    the rows and varies the chain length (64, 16, 256): one order's error in a channel whose sum nearly cancels
    is a single draw, and a kernel's draw is 4 x above it too often."""
    if v.dtype != F32:
        return v.sum(0)
    P, C = v.shape
    L = (64, 16, 256)[order % 3]
    if order:
        v = v[torch.randperm(P, generator=torch.Generator().manual_seed(order)).to(v.device)]
    pad = -P % L
    if pad:
        v = torch.cat([v, torch.zeros((pad, C), dtype=v.dtype, device=v.device)])
    v = v.reshape(-1, L, C)
    acc = v[:, 0]
    for k in range(1, L):
        acc = acc + v[:, k]
    return acc.sum(0) if acc.shape[0] > 1 else acc[0]


def stats(y, dtype=F64, order=0):
    v = y.to(dtype).reshape(-1, y.shape[-1])
    return colsum(v, order), colsum(_prod(v, v, dtype, order), order)


def finalize(s, q, count, gamma, beta, eps, rm=None, rv=None, momentum=0.1, dtype=F64):
    """-> mean, rstd, scale, shift, rm', rv' (None without running statistics).  rstd from max(var, 0); the
    running variance takes the unbiased estimate, count <= 1 the biased one."""
    s, q = s.to(dtype), q.to(dtype)
    g = torch.ones_like(s) if gamma is None else gamma.to(dtype)
    b = torch.zeros_like(s) if beta is None else beta.to(dtype)
    mean = s / count
    var = (q / count - mean * mean).clamp_min(0)
    rstd = 1 / torch.sqrt(var + eps)
    scale = g * rstd
    shift = b - mean * scale
    if rm is None:
        return mean, rstd, scale, shift, None, None
    unbiased = var * count / (count - 1) if count > 1 else var
    return (mean, rstd, scale, shift, (1 - momentum) * rm.to(dtype) + momentum * mean,
            (1 - momentum) * rv.to(dtype) + momentum * unbiased)


def eval_coeffs(gamma, beta, rm, rv, eps, dtype=F64):
    g = torch.ones_like(rm, dtype=dtype) if gamma is None else gamma.to(dtype)
    b = torch.zeros_like(rm, dtype=dtype) if beta is None else beta.to(dtype)
    scale = g / torch.sqrt(rv.to(dtype) + eps)
    return scale, b - rm.to(dtype) * scale


def fwd(y, scale, shift, pool=False, act=ACT_RELU, slope=SLOPE, dtype=F64):
    a = act_f(y.to(dtype) * scale.to(dtype) + shift.to(dtype), act, slope)
    return windows(a).amax(-1) if pool else a


def route(y, scale, shift, pool=False, act=ACT_RELU, slope=SLOPE, dtype=F64):
    """-> (mask, argmax): dz = mask * (the upstream gradient at / spread over the position).  Without pooling
    mask = act'(z).  With pooling only the first maximum of act(z) in window order keeps act'(z); argmax
    [N, Ho, Wo, C] is its position 0..3."""
    z = y.to(dtype) * scale.to(dtype) + shift.to(dtype)
    if not pool:
        return act_d(z, act, slope), None
    aw = windows(act_f(z, act, slope))
    is_max = aw == aw.amax(-1, keepdim=True)
    first = is_max & (is_max.to(torch.int8).cumsum(-1) == 1)
    mask = unwindow(first.to(dtype) * act_d(windows(z), act, slope), y.shape[1], y.shape[2])
    return mask, first.to(torch.int8).argmax(-1)


def dz_of(dout, y, scale, shift, pool=False, act=ACT_RELU, slope=SLOPE, dtype=F64):
    mask, _ = route(y, scale, shift, pool, act, slope, dtype)
    return mask * (spread(dout.to(dtype), y.shape[1], y.shape[2]) if pool else dout.to(dtype))


def bwd_sums(dout, y, scale, shift, pool=False, act=ACT_RELU, slope=SLOPE, dtype=F64, order=0):
    """-> [2, C]: (sum dz, sum dz * y)."""
    odd = dtype == F32 and order % 2
    dz = dz_of(dout, y, scale, shift, pool, act, slope, F64 if odd else dtype)
    C = y.shape[-1]
    return torch.stack([colsum(dz.to(dtype).reshape(-1, C), order),
                        colsum(_prod(dz, y, dtype, order).reshape(-1, C), order)])


def bwd(dout, y, mean, rstd, scale, shift, gamma, count, pool=False, act=ACT_RELU, slope=SLOPE, dtype=F64, sums=None,
        order=0):
    """-> dy, dgamma, dbeta.  dy = k1 * dz + k2 * y + k3 (the uncovered edge of an odd pooled map has dz = 0).
    ``sums`` [2, C]: use these (sum dz, sum dz * y) instead of forming them (a table some producer filled)."""
    yv = y.to(dtype)
    dz = dz_of(dout, y, scale, shift, pool, act, slope, dtype)
    C = y.shape[-1]
    if sums is None:
        s0, s1 = bwd_sums(dout, y, scale, shift, pool, act, slope, dtype, order)
    else:
        s0, s1 = sums[0].to(dtype), sums[1].to(dtype)
    mean, rstd = mean.to(dtype), rstd.to(dtype)
    g = torch.ones_like(mean) if gamma is None else gamma.to(dtype)
    dgamma = rstd * (s1 - mean * s0)          # sum dz * xhat
    dbeta = s0
    k1 = g * rstd
    k2 = -g * rstd * rstd * dgamma / count
    k3 = -g * rstd * dbeta / count - k2 * mean
    return k1 * dz + k2 * yv + k3, dgamma, dbeta


# ------------------------------------------------------------------------------------------- tables
def _weights(n, shape, seed):
    """n signed fp64 weights per entry that sum to 1: 1/n + 2/n * (zero-mean uniform in [-1, 1])."""
    gen = torch.Generator().manual_seed(seed)
    d = torch.rand((n,) + tuple(shape), generator=gen, dtype=F64) * 2 - 1
    return (1.0 + 2.0 * (d - d.mean(0, keepdim=True))) / n


def split_slots(sums, SL, seed):
    """fp64 per-channel sums [2, C] -> a slot table [SL, 2, C] whose slot sum is the input to 1e-15; every slot of
    a non-zero sum is non-zero and the weights have both signs."""
    sums = sums.to(F64).cpu()
    table = _weights(SL, sums.shape, seed) * sums
    for _ in range(2):
        table[0] += sums - table.sum(0)
    assert bool(((table.sum(0) - sums).abs() <= 1e-15 * sums.abs()).all())
    assert bool((table[:, sums != 0] != 0).all())
    return table


def split_rows(sums, R, seed):
    """The same into an fp32 partial-row table [R, 2, C] -> (table, the fp64 sum of the rounded table): the table
    is the kernel's operand and carries no error against the returned reference."""
    sums = sums.to(F64).cpu()
    table = (_weights(R, sums.shape, seed) * sums).to(F32)
    return table, table.to(F64).sum(0)


# ------------------------------------------------------------------------------------------- ambiguity
def _ambiguity(y, scale, shift, pool, act, slope, guard):
    """-> (sign mask [N,H,W,C], window mask [N,Ho,Wo,C] or None).  A channel with scale == 0 has z == shift in
    every precision and takes no part; neither does a ReLU window whose activations are all exactly 0."""
    yv, sc, sh = y.to(F64), scale.to(F64), shift.to(F64)
    z = yv * sc + sh
    mag = (yv * sc).abs() + sh.abs()
    live = (sc != 0).expand_as(z)
    sign = (z.abs() <= guard * mag) & live if act != ACT_NONE else torch.zeros_like(live)
    if not pool:
        return sign, None
    aw, yw = windows(act_f(z, act, slope)), windows(yv)
    amax = aw.amax(-1, keepdim=True)
    near = ((amax - aw) < guard * windows(mag).amax(-1, keepdim=True)) & windows(live)
    if act == ACT_RELU:
        near &= amax > 0
    inf = torch.full_like(yw, math.inf)
    differ = torch.where(near, yw, inf).amin(-1) != torch.where(near, yw, -inf).amax(-1)
    return sign, (near.sum(-1) >= 2) & differ


def ambiguous(y, scale, shift, pool=False, act=ACT_RELU, slope=SLOPE, guard=GUARD):
    """How many decisions fp32 could take differently from fp64: positions with |z| <= guard * (|y * scale| +
    |shift|) (the sign of z, when the activation looks at it), plus windows whose two largest act(z) are closer
    than the same guard without coming from bit-equal y."""
    n, step = 0, max(1, (1 << 22) // max(1, y[0].numel()))
    for i in range(0, y.shape[0], step):
        sign, win = _ambiguity(y[i:i + step], scale, shift, pool, act, slope, guard)
        n += int(sign.sum()) + (int(win.sum()) if win is not None else 0)
    return n


# ------------------------------------------------------------------------------------------- tolerances
def chan_err(got, ref):
    C = ref.shape[-1]
    return (got.to(F64) - ref.to(F64)).abs().reshape(-1, C).amax(0)


def chan_mag(ref):
    return ref.to(F64).abs().reshape(-1, ref.shape[-1]).amax(0)


def ill_channels(C, device='cpu'):
    ill = torch.zeros(C, dtype=torch.bool, device=device)
    ill[CONST] = ill[OFF] = True
    return ill


def yardstick(ref32, ref64):
    """-> (a_c, e_ref) of an fp32 evaluation (or a list of them: the largest error counts) against the fp64 one:
    the per-channel absolute error and the largest relative error over the well-conditioned channels, floored at
    2^-23."""
    many = ref32 if isinstance(ref32, (list, tuple)) else [ref32]
    a, mag = torch.stack([chan_err(r, ref64) for r in many]).amax(0), chan_mag(ref64)
    good = ~ill_channels(a.numel(), a.device) & (mag > 0)
    e = float((a[good] / mag[good]).max()) if bool(good.any()) else 0.0
    return a, max(e, E_FLOOR)


def tol_f32(ref32, ref64, noise=None, floor=None):
    """Per-channel bound of an fp32 output -> (tol_c, e_ref).  ``noise``: what the reference itself is uncertain by
    in each channel (see bwd_refs), added on top.  ``floor``: a lower bound of a_c (see sum_floor)."""
    a, e = yardstick(ref32, ref64)
    if floor is not None:
        a = torch.maximum(a, floor.to(a.device))
    tol = TOL_FACTOR * torch.maximum(e * chan_mag(ref64), a)
    return (tol if noise is None else tol + noise.to(tol.device)), e


def tol_bf16(ref32, ref64, noise=None):
    """Elementwise bound of a bf16 tensor."""
    a, _ = yardstick(ref32, ref64)
    a = TOL_FACTOR * a if noise is None else TOL_FACTOR * a + noise.to(a.device)
    return BF16_ULP * ref64.abs() + a.to(ref64.device)


# relative to |sum|: the fp64 roundings of <= 7 adds in the kernel's slot order, 7 in the reference's and one
# product (16 * 2^-53 = 1.8e-15), doubled
SLOT_NOISE = 4e-15
ROWS_NOISE = 10 * 2.0 ** -24
# relative to sum_r |row r|: a table of more than 512 partial rows is first folded into groups of <= 32 rows by an
# fp32 pass, four interleaved chains of <= 8 terms each plus two adds: at most 9 roundings of the group's
# absolute sum, whatever the order


def sum_floor(terms):
    """2^-24 * sum |term| per channel of [..., C] terms: one fp32 rounding of every term of a sum.  Any fp32
    evaluation rounds the terms (products, here) before or while it adds them, so no yardstick's error in a
    channel is taken to be below this, however the sampled orders happened to round: in a channel of two terms
    that nearly cancel (2 windows at (2, 2, 2, 2056)) every order gives the same fl(a) + fl(b), and a kernel that
    fuses the multiply into the add rounds differently (measured: 1.017 x the 4 x margin of the sampled orders).
    e_ref is still taken from the sampled orders alone."""
    return 2.0 ** -24 * terms.to(F64).abs().reshape(-1, terms.shape[-1]).sum(0)


def _signs(sums, dsums):
    for a in (1.0, -1.0):
        for b in (1.0, -1.0):
            yield sums + torch.tensor([[a], [b]], dtype=F64, device=sums.device) * dsums


def _noise(f, sums, dsums, ref, ill_only):
    """Per output of f(sums): how far it moves when the two sums move by +-dsums (four sign pairs, per channel)."""
    noise = None
    for p in _signs(sums, dsums):
        moved = [None if r is None else chan_err(a, r) for a, r in zip(f(p), ref)]
        noise = moved if noise is None else [None if m is None else torch.maximum(n, m) for n, m in zip(noise, moved)]
    if ill_only:
        for n in noise:
            if n is not None:
                n[~ill_channels(n.numel(), n.device)] = 0
    return noise


def rows_noise(table):
    """dsums of a partial-row table: the fp64 order of <= 512 rows, or the fp32 fold of more (ROWS_NOISE)."""
    t = table.to(F64)
    return ROWS_NOISE * t.abs().sum(0) if table.shape[0] > 512 else SLOT_NOISE * t.sum(0).abs()


def bwd_refs(dout, y, co, gamma, count, pool, act, slope=SLOPE, sums=None, dsums=None, ill_only=False):
    """-> (ref, r32, noise, floor) of bwd on the fed coefficients co = [mean, rstd, scale, shift]: the fp64 result,
    per output the list of fp32 evaluations (every summation order; one when the sums are given), when the given
    sums are only known to +-dsums how far that moves each output, and when the sums are formed here the
    sum_floor of dgamma and dbeta.  The constant channel makes this matter: its
    sum dz*xhat = rstd * (sum dz*y - mean * sum dz) cancels completely, so fp64 itself gets 1e-16 * rstd * |sum|
    there, not 0, and depends on the order the table was added in.  ``ill_only``: the uncertainty is an fp32 one
    (ROWS_NOISE) and is granted to the two ill-conditioned channels alone."""
    args = (dout, y, co[0], co[1], co[2], co[3], gamma, count, pool, act, slope)
    ref = bwd(*args, dtype=F64, sums=sums)
    orders = range(ORDERS) if sums is None else (0,)
    r32 = tuple(list(x) for x in zip(*[bwd(*args, dtype=F32, sums=sums, order=k) for k in orders]))
    noise, floor = None, None
    if dsums is not None:
        noise = _noise(lambda p: bwd(*args, dtype=F64, sums=p), sums.to(F64), dsums, ref, ill_only)
    if sums is None:
        dz = dz_of(dout, y, co[2], co[3], pool, act, slope, F64)
        f0, f1 = sum_floor(dz), sum_floor(dz * y.to(F64))
        floor = (None, co[1].to(F64).abs() * (f1 + co[0].to(F64).abs() * f0), f0)
    return ref, r32, noise, floor


def finalize_refs(sums, count, gamma, beta, eps, rm, rv, momentum, dsums=None, ill_only=False):
    """-> (ref, r32, noise) of finalize, as bwd_refs."""
    ref = finalize(sums[0], sums[1], count, gamma, beta, eps, rm, rv, momentum, dtype=F64)
    r32 = finalize(sums[0].to(F32), sums[1].to(F32), count, gamma, beta, eps, rm, rv, momentum, dtype=F32)
    noise = None
    if dsums is not None:
        noise = _noise(lambda p: finalize(p[0], p[1], count, gamma, beta, eps, rm, rv, momentum, dtype=F64),
                       sums.to(F64), dsums, ref, ill_only)
    return ref, r32, noise


def stats_refs(y):
    """-> (ref, r32 lists, floors) of (sum, sumsq)."""
    return (stats(y, F64), tuple(list(x) for x in zip(*[stats(y, F32, k) for k in range(ORDERS)])),
            (sum_floor(y), sum_floor(y.to(F64) ** 2)))


def frob(got, ref):
    """Whole-tensor Frobenius error over the well-conditioned channels, relative."""
    good = ~ill_channels(ref.shape[-1], ref.device)
    g, r = got.to(F64)[..., good], ref.to(F64)[..., good]
    return float((g - r).norm() / r.norm().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------- inputs
BF16_SHAPES = ((2, 4, 4, 8), (3, 5, 3, 24), (2, 2, 7, 40), (2, 6, 6, 96), (4, 8, 8, 64), (37, 1, 1, 784),
               (2, 2, 2, 2056))
F32_SHAPES = ((2, 4, 4, 4), (3, 5, 3, 12), (2, 2, 7, 16), (2, 7, 6, 32), (4, 8, 8, 64), (2, 4, 4, 1024),
              (37, 1, 1, 784), (5, 1, 1, 1536), (9, 32, 32, 256))
LARGE = (((17, 32, 32, 512), False), ((33, 32, 32, 512), True))       # bf16, *_acc entries, RELU: (shape, pool)
ROW_COUNTS = (1, 15, 16, 17, 112, 113, 127, 128, 129, 300, 512, 513, 2000)
ROW_CHANNELS = (8, 24, 520)
ROW_SHAPE = (3, 4, 4)                                                  # N, H, W of the row-table cases
ANCHOR_SHAPES = ((3, 5, 3, 8), (2, 2, 7, 8), (2, 4, 4, 8))


def pools_of(shape):
    return (False, True) if shape[1] >= 2 and shape[2] >= 2 else (False,)


def acts_of(shape):
    return ACTS if shape[1] * shape[2] > 1 else (ACT_NONE,)


def _seed(kind, shape):
    return (1 if kind == 'bf16' else 2) * 1000003 + sum(d * 31 ** i for i, d in enumerate(shape))


def _round(t, kind):
    return t.bfloat16().float() if kind == 'bf16' else t


class Case:
    """The inputs of one (kind, shape): y, the per-channel parameters, upstream gradients for both output
    shapes, and the coefficients the kernels after the finalize stage are fed: the fp32 roundings of finalize()
    in fp64.  kind 'bf16': y and dout hold bf16 values, so the reference sees the kernel's operands."""

    def __init__(self, kind, shape, hyper=None, decide=None):
        self.kind, self.shape = kind, tuple(shape)
        N, H, W, C = shape
        self.count = N * H * W
        seed = _seed(kind, shape)
        self.eps, self.momentum = HYPER[seed % 2 if hyper is None else hyper]
        gen = torch.Generator().manual_seed(seed)
        rnd = lambda *s: torch.randn(*s, generator=gen)     # noqa: E731
        uni = lambda *s: torch.rand(*s, generator=gen)      # noqa: E731
        self.gamma = (0.5 + uni(C)) * torch.where(uni(C) < 0.5, -1.0, 1.0)
        self.beta = 0.5 * rnd(C)
        self.gamma[ZERO], self.beta[ZERO], self.gamma[BIG], self.beta[CONST] = 0.0, 0.0, -8.0, CONST_BETA
        self.rm, self.rv = 0.5 * rnd(C), 0.5 + uni(C)
        self.sigma, mu = 0.5 + 1.5 * uni(C), 0.5 * rnd(C)
        mu[OFF] = 8 * self.sigma[OFF]
        self.mu = mu
        self.y = _round(rnd(N, H, W, C) * self.sigma + mu, kind)
        self.y[..., CONST] = CONST_Y
        self.dout = {p: _round(rnd(N, H // 2, W // 2, C) if p else rnd(N, H, W, C), kind) for p in pools_of(shape)}
        self.dgamma0, self.dbeta0 = rnd(C), rnd(C)          # what accumulate=True adds onto
        self.ill = ill_channels(C)
        if decide is None:
            decide = [(p, a, SLOPE) for p in pools_of(shape) for a in acts_of(shape)]
            if self.shape == NEG_SLOPE_SHAPE:
                decide.append((True, ACT_LRELU, NEG_SLOPE))
        self.decide = decide
        self._settle(gen)

    def _coeffs(self):
        s, q = stats(self.y)
        self.sums = torch.stack([s, q])
        self.fin = finalize(s, q, self.count, self.gamma, self.beta, self.eps, self.rm, self.rv, self.momentum)
        self.coeffs = torch.stack([t.to(F32) for t in self.fin[:4]])      # mean, rstd, scale, shift as fed on

    def _settle(self, gen):
        """Redraw the few y that put a decision inside the guard band until none is left (the coefficients move
        with y, hence the loop).  A draw is replaced, never excluded from a comparison."""
        for _ in range(8):
            self._coeffs()
            N = self.shape[0]
            step = max(1, (1 << 22) // max(1, self.y[0].numel()))
            found = 0
            for i in range(0, N, step):
                yv = self.y[i:i + step]
                bad = torch.zeros(yv.shape, dtype=torch.bool)
                for pool, act, slope in self.decide:
                    sign, win = _ambiguity(yv, self.coeffs[2], self.coeffs[3], pool, act, slope, GUARD)
                    bad |= sign
                    if win is not None:
                        bad |= unwindow(win.unsqueeze(-1).expand(*win.shape, 4).to(torch.int8), *yv.shape[1:3]).bool()
                n = int(bad.sum())
                if n:
                    found += n
                    c = bad.nonzero()[:, 3]
                    yv[bad] = _round(torch.randn(n, generator=gen) * self.sigma[c] + self.mu[c], self.kind)
            if not found:
                return
        raise AssertionError('could not settle the inputs of {}'.format(self.shape))


@functools.lru_cache(maxsize=None)
def case(kind, shape, hyper=None):
    return Case(kind, shape, hyper)


@functools.lru_cache(maxsize=None)
def large_case(i):
    shape, pool = LARGE[i]
    return Case('bf16', shape, decide=[(pool, ACT_RELU, SLOPE)])


def row_case(C):
    return case('bf16', ROW_SHAPE + (C,))
