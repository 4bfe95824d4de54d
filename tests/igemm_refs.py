"""fp64 CPU references, input sets and derived tolerances for the bf16 implicit-GEMM family
(csrc/kernels/igemm.hip and the combine kernels it feeds).  Imports nothing from rafiki_amd.

Layouts: activations NHWC, conv weights [Cout][tap][Cin], tap t = 3*kh + kw reads pixel (h + kh - 1, w + kw - 1).
Every product is written as one GEMM  acc[m][n] = sum_k A[m][k] * B[n][k]  in the kernel's own K order
(``operands``), so K-tiles, split-K slabs and "the last product" mean the same thing here as there.  Every
reference also returns S[m][n] = sum_k |A[m][k] * B[n][k]|, the scale of the rounding-error model.

Two input sets with separate roles:

EXACT   small integers (x, dy in [-2, 2], w in {-1, 0, 1}, alpha in {1, 0.5}, bias a multiple of 0.25).  Every
        product and partial sum is an integer below 2^24, so fp32 accumulation is exact in any order and inside
        any MFMA: an fp32 output must equal the reference bit for bit, a bf16 output must equal the reference
        rounded to nearest even, statistics must be equal.  Indexing errors (halo, tap, K tail, tile guard,
        split-K) are exact-arithmetic questions and are answered here.  ``exact_ok`` checks the precondition.
RANDOM  normal draws rounded to bf16 (weights scaled by 1/sqrt(K)), so the reference sees the kernel's operands.
        Tolerances come from the error model, never from a kernel's output:
            fp32 output   |got - ref| <= E32,  E32 = n * 2^-23 * S
                          n = terms of the sum + every further fp32 operation (alpha, bias, leaky slope, slab
                          additions, the accumulate); 2^-23 is twice fp32's unit roundoff, the factor 2 covers
                          an MFMA that aligns and truncates inside its 32-term block
            bf16 output   |got - ref| <= 2^-8 |ref| + (1 + 2^-8) E32   (one rounding to 8 significant bits)
            channel sums  sum over rows of the element tolerances + rows * 2^-23 * sum |term|
        judged element by element and channel by channel.

Decision inputs (ReLU gate, BN mask, 2x2 max-pool routing) are exact: y = k/64 with |k| <= 255, scale = +-2^j,
shift a multiple of 1/64, so y*scale + shift is exact in fp32 with or without contraction and no element has to
be left out of a comparison (``decisions_inexact`` counts the exceptions; it must return 0).
"""
import torch

F64 = torch.float64
U32 = 2.0 ** -23   # twice fp32's unit roundoff
U16 = 2.0 ** -8    # bf16 round-to-nearest: 8 significant bits
BK = 64            # K-tile of the engine: split-K slabs are whole K-tiles
LIM = float(2 ** 24)
TAPS = [(t // 3 - 1, t % 3 - 1) for t in range(9)]
ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2


def cdiv(a, b):
    return (a + b - 1) // b


def bf16r(t):
    """Round to nearest even to bf16, back in fp64 (exact for fp32-representable input)."""
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


def bf16_trunc(t):
    """The wrong rounding: drop the low 16 bits of the fp32 value."""
    bits = t.to(torch.float32).contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32).to(F64)


def f32r(t):
    return t.to(torch.float32).to(F64)


# ------------------------------------------------------------------------------------------- gather
def _pix(N, H, W):
    m = torch.arange(N * H * W)
    return m // (H * W), (m // W) % H, m % W


def cols(x, taps=9, sign=1, up=False, mutant=None):
    """Gathered activation A [pixels][taps * C] of x [N][H][W][C] (fp64), column (t, c) = the pixel tap t reads,
    zero outside the image.  sign = -1 flips the taps (data gradient).  up: x is the input of a 2x nearest
    upscale, rows are pixels of the 2H x 2W output and the gather reads ((h+dy)>>1, (w+dx)>>1).
    mutant: None or one of the wrong formulas of tests/test_igemm_refs.py."""
    N, H, W, C = x.shape
    Ho, Wo = (2 * H, 2 * W) if up else (H, W)
    flat = x.reshape(-1, C)
    n, h, w = _pix(N, Ho, Wo)
    out = torch.zeros(N * Ho * Wo, taps, C, dtype=F64)
    for t in range(taps):
        dy, dx = TAPS[t] if taps == 9 else (0, 0)
        if mutant == 'swap_khkw':
            dy, dx = dx, dy
        dy, dx = sign * dy, sign * dx
        if up:
            if mutant == 'up_gather':       # (h>>1)+dy in place of (h+dy)>>1
                hi, wi = (h >> 1) + dy, (w >> 1) + dx
                ok = (hi >= 0) & (hi < H) & (wi >= 0) & (wi < W)
            else:
                ok = (h + dy >= 0) & (h + dy < Ho) & (w + dx >= 0) & (w + dx < Wo)
                hi, wi = (h + dy) >> 1, (w + dx) >> 1
        else:
            hi, wi = h + dy, w + dx
            rok, cok = (hi >= 0) & (hi < H), (wi >= 0) & (wi < W)
            if mutant == 'wrap_lr':         # no column check: the flat index runs into the neighbouring row
                ok = rok
            elif mutant == 'bottom_next':   # no bottom check: the flat index runs into the next image
                ok = (hi >= 0) & cok
            else:
                ok = rok & cok
        idx = torch.remainder((n * H + hi) * W + wi, flat.shape[0])
        out[:, t, :] = flat[idx] * ok[:, None].to(F64)
    return out.reshape(N * Ho * Wo, taps * C)


def flip_transpose(w):
    """ConvWT: wt[ci][8 - t][co] = w[co][t][ci] for w [Cout][9][Cin]."""
    return w.flip(1).permute(2, 1, 0).contiguous()


def operands(kind, a, b, taps=9, mutant=None):
    """(A [M][K], B [N][K]) of rk_igemm kind 0-6 in the kernel's K order.
    0 conv fwd (x, w)  1 conv dgrad (dy, w)  2 conv wgrad (dy, x)  3 dense (x [M][K], w [N][K])
    4 dense dX (dy [M][No], w [No][Ni])  5 dense dW (dy [M][No], x [M][Ni])  6 upscale + conv fwd (x, w)."""
    if kind == 0:
        return cols(a, taps, 1, mutant=mutant), b.reshape(b.shape[0], -1)
    if kind == 1:   # k = tap * Cout + co;  dx[p][ci] = sum dy[p - d_t][co] * w[co][t][ci]
        return cols(a, taps, 1 if mutant == 'noflip' else -1, mutant=mutant), b.permute(2, 1, 0).reshape(b.shape[2], -1)
    if kind == 2:   # k = pixel
        return a.reshape(-1, a.shape[-1]).t(), cols(b, taps, 1, mutant=mutant).t()
    if kind == 3:
        return a, b
    if kind == 4:
        return a, b.t()
    if kind == 5:
        return a.t(), b.t()
    if kind == 6:
        return cols(a, 9, 1, up=True, mutant=mutant), b.reshape(b.shape[0], -1)
    raise ValueError(kind)


# --------------------------------------------------------------------------------------------- GEMM
def split_ranges(K, splits):
    """K ranges of the split-K slabs: whole K-tiles, ceil(kTiles / splits) per slab (as rk_igemm)."""
    kt = cdiv(K, BK)
    per = cdiv(kt, splits)
    return [(s * per * BK, min(K, (s + 1) * per * BK)) for s in range(splits) if s * per < kt]


def effective_splits(K, splits):
    return len(split_ranges(K, splits))


def gemm(A, B, splits=1, mutant=None):
    """slabs [s][M][N] (slab s = the products of its K range) and S [s][M][N] = sum_k |A*B| over the same range."""
    K = A.shape[1]
    kt = cdiv(K, BK)
    if mutant == 'drop_last_k':
        A = A.clone()
        A[:, K - 1] = 0
    elif mutant == 'drop_last_chunk':       # the last 8-wide chunk of the last tap
        A = A.clone()
        A[:, K - 8:] = 0
    elif mutant == 'drop_last_ktile':       # the last split's last (partial) K-tile
        A = A.clone()
        A[:, (kt - 1) * BK:] = 0
    if mutant == 'acc_bf16':                # the accumulator rounded to bf16 between K-tiles
        acc = torch.zeros(A.shape[0], B.shape[0], dtype=F64)
        for t in range(kt):
            acc = bf16r(acc + A[:, t * BK:(t + 1) * BK] @ B[:, t * BK:(t + 1) * BK].t())
        return acc[None], (A.abs() @ B.abs().t())[None]
    rng = split_ranges(K, splits)
    slabs = torch.stack([A[:, lo:hi] @ B[:, lo:hi].t() for lo, hi in rng])
    S = torch.stack([A[:, lo:hi].abs() @ B[:, lo:hi].abs().t() for lo, hi in rng])
    if mutant == 'ktile_twice':             # the K-tile after a split boundary also counted by the slab before
        lo = rng[1][0]
        slabs[0] += A[:, lo:lo + BK] @ B[:, lo:lo + BK].t()
    return slabs, S


# ---------------------------------------------------------------------------------------- epilogues
def fp32_out(acc, S, K, *, alpha=1.0, bias=None, nslabs=1, prior=None):
    """v = alpha * acc + bias (+ prior for FLAG_ACCUM) and its fp32 error bound E32 = n * 2^-23 * S."""
    v, Sv, n = acc * alpha, S * abs(alpha), K + (alpha != 1.0) + (nslabs - 1)
    if bias is not None:
        v, Sv, n = v + bias, Sv + bias.abs(), n + 1
    if prior is not None:
        v, Sv, n = v + prior, Sv + prior.abs(), n + 1
    return v, n * U32 * Sv


def activate(v, E, act, slope=0.2):
    if act == ACT_RELU:
        return v.clamp_min(0), E
    if act == ACT_LRELU:   # one more fp32 product on the negative side; the map is 1-Lipschitz
        return torch.where(v > 0, v, v * slope), E + U32 * v.abs()
    return v, E


def tol_bf16(ref, E):
    return U16 * ref.abs() + (1 + U16) * E


def stats_ref(v, E, rows=None):
    """FLAG_STATS: (sum v, sum v^2) over the rows `rows` (slice) of the pre-activation values, with tolerances."""
    if rows is not None:
        v, E = v[rows], E[rows]
    r = max(v.shape[0], 1)
    s, q = v.sum(0), (v * v).sum(0)
    ts = E.sum(0) + r * U32 * v.abs().sum(0)
    tq = ((2 * v.abs() + E) * E + U32 * v * v).sum(0) + r * U32 * (v * v).sum(0)
    return torch.stack([s, q]), torch.stack([ts, tq])


def stats_row_sets(M, BM):
    """Row sets of the partial statistics rows: row 2*mt + wm covers rows mt*BM + wm*BM/2 .. + BM/2 (below M)."""
    return [slice(min(M, r * BM // 2), min(M, (r + 1) * BM // 2)) for r in range(cdiv(M, BM) * 2)]


def bnb_mask(y, scale, shift):
    return (y * scale + shift) > 0


def bnp_route(y2, scale, shift, N, H, W, mutant=None):
    """FLAG_BNP: per output element (pooled resolution N x H x W) the first maximal act(y*scale+shift) of the
    2x2 window of y2 [N][2H][2W][C].  Returns (zb > 0 [M][C], yb [M][C])."""
    C = y2.shape[-1]
    win = y2.reshape(N, H, 2, W, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N * H * W, 4, C)
    z = win * scale + shift
    key = win if mutant == 'route_on_y' else z.clamp_min(0)   # route_on_y: the maximum of y, not of act(z)
    best = torch.full_like(key[:, 0], float('-inf'))
    zb, yb = torch.zeros_like(best), torch.zeros_like(best)
    for q in range(4):
        upd = key[:, q] >= best if mutant == 'last_max' else key[:, q] > best
        best = torch.where(upd, key[:, q], best)
        zb = torch.where(upd, z[:, q], zb)
        yb = torch.where(upd, win[:, q], yb)
    return zb > 0, yb


def bn_sums(dz, y):
    """(sum dz, sum dz*y) per channel of the routed / masked values dz (already zero where masked) and the
    tolerance of an fp32 summation of exactly these terms: rows * 2^-23 * sum |term| (+ the product's rounding)."""
    r = dz.shape[0]
    s, q = dz.sum(0), (dz * y).sum(0)
    return torch.stack([s, q]), torch.stack([r * U32 * dz.abs().sum(0), (r + 1) * U32 * (dz * y).abs().sum(0)])


def decisions_inexact(y, scale, shift):
    """Number of elements whose y*scale + shift is not exact in fp32 (must be 0: then every mask and every
    first-maximum tie is reproducible and nothing has to be excluded from a comparison)."""
    z = y * scale + shift
    z32 = y.float() * scale.float() + shift.float()
    return int((z32.to(F64) != z).sum()) + int((f32r(y * scale) != y * scale).sum())


# ------------------------------------------------------------------------------------------- inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(seed, shape, lo, hi):
    return torch.randint(lo, hi + 1, tuple(shape), generator=_gen(seed)).to(F64)


def normal_bf16(seed, shape, scale=1.0):
    return (torch.randn(tuple(shape), generator=_gen(seed)) * scale).to(torch.bfloat16).to(F64)


def draw(mode, seed, shape, K=None):
    """An activation-like operand (K None) or a weight-like one (scaled by 1/sqrt(K) on RANDOM)."""
    if mode == 'exact':
        return ints(seed, shape, -2, 2) if K is None else ints(seed, shape, -1, 1)
    return normal_bf16(seed, shape, 1.0 if K is None else K ** -0.5)


def draw_bias(mode, seed, n, big=False):
    """EXACT: multiples of 0.25; big puts +-300 on a few channels, so stored values above 256 need a real bf16
    rounding (ties included: 300 + k/4 ... sits between bf16 neighbours 2 apart)."""
    if mode == 'exact':
        b = ints(seed, (n,), -8, 8) * 0.25
        if big:
            b[1::7] = 300.0
            b[2::7] = -300.25
            b[5::7] = 301.0    # integers around 301 are ties of the 2-wide bf16 grid above 256
    else:
        b = f32r(torch.randn(n, generator=_gen(seed)).to(F64))
    return b


def draw_decision(seed, shape):
    """y = k/64, |k| <= 255 (8 significant bits: a bf16 value)."""
    return ints(seed, shape, -255, 255) / 64.0


def draw_scale_shift(seed, C):
    """scale = +-2^j (every third channel negative), shift a multiple of 1/64 with |shift| <= 1."""
    j = ints(seed, (C,), -1, 1)
    scale = torch.pow(torch.tensor(2.0, dtype=F64), j)
    scale[1::3] *= -1
    return scale, ints(seed + 1, (C,), -64, 64) / 64.0


def draw_pool_y(seed, N, H, W, C, scale):
    """y [N][2H][2W][C] for FLAG_BNP with tied maxima (every 3rd window: all four equal; every 7th: elements 1 and
    2 equal) and all-nonpositive windows (every 5th: |y| >= 2 against the sign of scale, so z <= 0)."""
    y = draw_decision(seed, (N, 2 * H, 2 * W, C))
    win = y.reshape(N, H, 2, W, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N * H * W, 4, C).clone()
    m = torch.arange(N * H * W)
    win[m % 3 == 0] = win[m % 3 == 0][:, :1]
    t = m % 7 == 1
    win[t, 2] = win[t, 1]
    neg = m % 5 == 2
    win[neg] = -scale.sign() * (2.0 + win[neg].abs() / 4.0).clamp_max(255.0 / 64.0)
    win = (win * 64).round() / 64
    return win.reshape(N, H, W, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, 2 * H, 2 * W, C).contiguous()


def exact_ok(S, v=None, granule=1.0):
    """EXACT precondition: S (and sum_m v^2 per channel, in units of granule^2) below 2^24."""
    ok = bool((S < LIM).all())
    if v is not None:
        ok = ok and bool(((v * v).sum(0) / (granule * granule) < LIM).all()) and bool((v.abs().sum(0) / granule < LIM).all())
    return ok


# ------------------------------------------------------------------------------------------- shapes
# Smallest shapes that reach each edge, (N, H, W, Cin, Cout); K-tile counts are for the 3x3 forward conv:
#   (3,4,4,8,72)     M = 48 under one tile, partial N, 2 K-tiles with an 8-wide tail, fewer tiles than ring stages
#   (2,16,16,16,136) 4 M-tiles, partial second N-tile, 3 K-tiles      (1,8,8,32,64) 5 K-tiles, the last one half
#   (2,8,8,64,64)    9 K-tiles, exact      (3,6,6,24,40), (1,12,20,8,8) reciprocal pixel / channel decode
#   (5,2,2,64,64)    every pixel on a border
CONV_SHAPES = [(3, 4, 4, 8, 72), (2, 16, 16, 16, 136), (1, 8, 8, 32, 64), (2, 8, 8, 64, 64), (3, 6, 6, 24, 40),
               (1, 12, 20, 8, 8), (5, 2, 2, 64, 64)]
TAP1_SHAPES = [(2, 8, 8, 64, 64), (3, 4, 4, 8, 72)]
# the data gradient needs a power-of-two Cout (its launcher refuses the others): the shapes with Cin and Cout
# swapped give it the partial N-tiles the forward shapes have
DGRAD_EXTRA = [(3, 4, 4, 72, 8), (2, 16, 16, 136, 16)]
UP_SHAPES = [(2, 2, 2, 16, 24), (3, 3, 5, 24, 40)]          # at the input resolution
DENSE_SHAPES = [(37, 64, 16), (200, 520, 96), (130, 72, 132)]   # (M, K, N)
SWEEP = ([(k, s, 9) for k in (0, 1, 2) for s in CONV_SHAPES] + [(k, s, 1) for k in (0, 1, 2) for s in TAP1_SHAPES]
         + [(1, s, 9) for s in DGRAD_EXTRA] + [(6, s, 9) for s in UP_SHAPES]
         + [(k, s, 1) for k in (3, 4, 5) for s in DENSE_SHAPES])
EPI_SHAPES = [(2, 8, 8, 64, 128), (3, 4, 4, 8, 72)]          # full tiles of every shape (M = N = 128); guarded ones


def problem(kind, shape, taps, mode):
    """The two operands of rk_igemm kind 0-6 at `shape` ((N,H,W,Cin,Cout) or dense (M,K,N)), drawn from the input
    set `mode`; ``operands(kind, a, b, taps)`` gives their GEMM view."""
    seed = 1000 * kind + 7 * sum(shape) + taps
    if kind in (0, 6):
        Nb, H, W, Ci, Co = shape
        return draw(mode, seed, (Nb, H, W, Ci)), draw(mode, seed + 1, (Co, taps, Ci), K=taps * Ci)
    if kind == 1:
        Nb, H, W, Ci, Co = shape
        return draw(mode, seed, (Nb, H, W, Co)), draw(mode, seed + 1, (Co, taps, Ci), K=taps * Co)
    if kind == 2:
        Nb, H, W, Ci, Co = shape
        return draw(mode, seed, (Nb, H, W, Co)), draw(mode, seed + 1, (Nb, H, W, Ci))
    M, K, N = shape
    if kind == 3:
        return draw(mode, seed, (M, K)), draw(mode, seed + 1, (N, K), K=K)
    if kind == 4:
        return draw(mode, seed, (M, N)), draw(mode, seed + 1, (N, K), K=N)
    return draw(mode, seed, (M, N)), draw(mode, seed + 1, (M, K))
