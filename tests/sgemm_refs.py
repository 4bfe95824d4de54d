"""fp64 CPU references, input sets and derived tolerances for the fp32 implicit-GEMM family
(csrc/kernels/sgemm.hip + sgemm_core.h: rk_sgemm, rk_sgemm_g, rk_sgemm_grp; the combine kernel rk_sreduce_epi;
the dense wrappers around the pre-split x6p GEMM).  Imports nothing from rafiki_amd; what applies unchanged
comes from igemm_refs (the 3x3 gather, the decision draws, the statistics and BN-backward references).

Every operation is one GEMM  acc[m][n] = sum_k A[m][k] * B[n][k]  in the kernel's K order (``view``), with
S[m][n] = sum_k |A[m][k] * B[n][k]| alongside.  The K-tile is 32; split-K slab s covers the K-tiles
[s * ktPer, (s + 1) * ktPer), ktPer = ceil(ceil(K / 32) / splits), and a slab past the last K-tile is zero.

Input sets
  EXACT       igemm_refs' integers: activations in [-2, 2], weights in {-1, 0, 1}, bias multiples of 0.25, alpha in
              {1, 0.5}.  Every partial sum is an integer below 2^24: both K loops must return the reference bit
              for bit (the X6 pieces of a small integer are (x, 0, 0)).
  EXACT-WIDE  for the X6 pieces, still exact in fp32:
              'wide_a'  the A-side raw operand holds odd integers of 18 significant bits (2^17 <= |x| < 2^18) on a
                        sparse subset, the other operand is in {-1, 0, 1};  'wide_b' the roles swapped.
                        Round-to-nearest residuals are signed, so two bf16 pieces already carry 17 bits
                        (|x - hi| <= 2^8 fits the 8 bits of mid whenever it is odd): 18 bits is the smallest
                        width at which lo is nonzero, ``pieces_used`` checks that it is.
              'wide_mm' both operands are 256 s + t, s, t in [-3, 3] (neither zero) on a sparse subset: hi and mid
                        on both sides, lo zero - this is what reaches the mid*mid term.
              The density keeps S < 2^24 (``exact_ok``); the dropped terms mid*lo, lo*mid, lo*lo are exactly zero
              (on wide_a / wide_b the narrow side is (x, 0, 0); on wide_mm lo is zero), every piece product is an
              integer below 2^24, so both loops must again return the reference bit for bit.
  RANDOM      full-mantissa fp32 normal draws (weights scaled by 1 / sqrt(K)).

RANDOM tolerances
  hard, f32 loop   |got - ref| <= n * 2^-23 * S, n = K + every further fp32 operation (igemm_refs.fp32_out).
  hard, X6 loop    (the comment at the top of sgemm.hip) x = hi + mid + lo with each piece the bf16 rounding of the
                   remaining residual: |mid| <= 2^-9 |x| (1 + 2^-9), |lo| <= 2^-18 |x| (1 + ...), and the three
                   pieces hold 8 + 1 + 8 + 1 + 8 = 26 bits, so x is represented exactly (fp32 has 24).  Of the nine
                   piece products the loop keeps six; the dropped ones are bounded by
                       |mid*lo| + |lo*mid| + |lo*lo| <= (2 * 2^-27 + 2^-36) |x y| < 2^-25 |x y|,
                   i.e. the product error is below 2^-25 S per output.  The six kept terms go through six MFMAs per
                   16-deep chunk, each adding its piece products to the same fp32 accumulator: 6 K additions whose
                   magnitudes sum to at most (1 + 2 * 2^-8 + 3 * 2^-16) S < 1.008 S.  With 2^-23 per addition
                   (igemm_refs' rule: twice the unit roundoff, covering the alignment inside an MFMA block)
                       |got - ref| <= (6 * 1.008 * K + 1 + extra) * 2^-23 * S,   ``n_x6(K) = ceil(6.05 K) + 1``.
  yardstick        the hard bound is a worst case (about 100x too loose to notice a missing X6 term at K = 132), so
                   every RANDOM result is also held to the same GEMM accumulated in plain fp32 on the CPU, one k at
                   a time in ascending order (a rank-1 update per k), then through the same epilogue in fp32
                   (``epilogue32``): per output row and per output column
                       rms(got - ref) <= 4 * rms(yardstick - ref)
                   (rows and columns with fewer than 16 elements that carry an error, e.g. behind a ReLU, are
                   judged together as one population: see ``rms_ratio``).
"""
import math

import torch

import igemm_refs as R
from igemm_refs import (ACT_LRELU, ACT_NONE, ACT_RELU, F64, U32, TAPS, bn_sums, bnb_mask, bnp_route, cdiv, cols,  # noqa: F401
                        decisions_inexact, draw_bias, draw_decision, draw_pool_y, draw_scale_shift, exact_ok, f32r,
                        flip_transpose, ints, stats_ref)

BK = 32
YARD = 4.0
MODES = ('exact', 'wide_a', 'wide_b', 'wide_mm', 'random')
EXACT_MODES = MODES[:4]
S2_TAPS = [(t // 4 - 1, t % 4 - 1) for t in range(16)]


# --------------------------------------------------------------------------------------- split-bf16 pieces
def bf16r(t):
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


def split3(x):
    """(hi, mid, lo) of the X6 loop in fp64, from torch's bf16 rounding (x must be fp32-representable)."""
    hi = bf16r(x)
    mid = bf16r(x - hi)
    lo = bf16r(x - hi - mid)
    return hi, mid, lo


X6_TERMS = ('hh', 'hm', 'mh', 'hl', 'lh', 'mm')


def x6_gemm(A, B, drop=None):
    """The six-term product of the X6 loop in fp64 (``drop``: one of X6_TERMS left out)."""
    pa, pb = dict(zip('hml', split3(A))), dict(zip('hml', split3(B)))
    out = torch.zeros(A.shape[0], B.shape[0], dtype=F64)
    for t in X6_TERMS:
        if t != drop:
            out += pa[t[0]] @ pb[t[1]].t()
    return out


def pieces_used(t):
    """Fractions of the nonzero elements whose mid / lo piece is nonzero."""
    _, mid, lo = split3(t)
    nz = max(int((t != 0).sum()), 1)
    return int((mid != 0).sum()) / nz, int((lo != 0).sum()) / nz


# ------------------------------------------------------------------------------------------- gathers
def gcols(x, Ho, Wo, stride, taps, mutant=None):
    """Table-driven gather (rk_sgemm_g): rows = pixels (b, i, j) of the Ho x Wo grid, column (t, c) = x at
    (stride*i + dy_t, stride*j + dx_t), zero outside the H x W input."""
    N, H, W, C = x.shape
    flat = x.reshape(-1, C)
    n, i, j = R._pix(N, Ho, Wo)
    out = torch.zeros(N * Ho * Wo, len(taps), C, dtype=F64)
    for t, (dy, dx) in enumerate(taps):
        if mutant == 'swap_khkw':
            dy, dx = dx, dy
        hi, wi = stride * i + dy, stride * j + dx
        rok, cok = (hi >= 0) & (hi < H), (wi >= 0) & (wi < W)
        ok = rok if mutant == 'wrap_lr' else ((hi >= 0) & cok) if mutant == 'bottom_next' else rok & cok
        idx = torch.remainder((n * H + hi) * W + wi, flat.shape[0])
        out[:, t, :] = flat[idx] * ok[:, None].to(F64)
    return out.reshape(N * Ho * Wo, len(taps) * C)


def par_d(r, u):
    return (0 if u == 0 else 2) if r == 0 else (1 if u == 0 else -1)


def s2t_taps(g):
    """Parity group g = 2 ry + rx of the adjoint: tap t4 = 2u + v reads source offset (r - d) / 2."""
    ry, rx = g >> 1, g & 1
    return [((ry - par_d(ry, t4 >> 1)) >> 1, (rx - par_d(rx, t4 & 1)) >> 1) for t4 in range(4)]


def s2t_weights(Wt, g):
    """B_g [Ci][4 * Co] of parity group g from W [Co][16][Ci]: column (t4, co) = W[co][tap(g, t4)][ci]."""
    ry, rx = g >> 1, g & 1
    tap = [4 * (par_d(ry, t4 >> 1) + 1) + par_d(rx, t4 & 1) + 1 for t4 in range(4)]
    return Wt[:, tap, :].permute(2, 1, 0).reshape(Wt.shape[2], -1)


def s2t_rows(Nb, h, w, g, mutant=None):
    """os == 2: row (b, i, j) of group g lands on pixel (2i + oy, 2j + ox) of the 2h x 2w map."""
    oy, ox = g >> 1, g & 1
    if mutant == 'parity_pixel':
        oy, ox = ox, oy
    b, i, j = R._pix(Nb, h, w)
    return (b * 2 * h + 2 * i + oy) * (2 * w) + 2 * j + ox


def view(name, a, b, taps=9, mutant=None):
    """[(A [M][K], B [N][K])] per group, in the kernel's K order.
    conv (x, w [Co][taps][Ci]) | dgrad (dy, w) | wgrad (dy, x) | dense (x [M][K], w [N][K]) |
    dx (dy [M][No], w [No][Ni]) | dw (dy [M][No], x [M][Ni]) | s2 (x, W [Co][16][Ci]) | s2t (z, W) |
    s2w (g, x) | conv_grp (x [G or 1][..], w [G][Co][taps][Ci]) | dense_grp (x [G or 1][M][K], w [G][N][K])."""
    kind = {'conv': 0, 'dgrad': 1, 'wgrad': 2, 'dense': 3, 'dx': 4, 'dw': 5}.get(name)
    if kind is not None:
        return [R.operands(kind, a, b, taps, mutant=mutant)]
    if name == 's2':
        Nb, H, W, _ = a.shape
        return [(gcols(a, H // 2, W // 2, 2, S2_TAPS, mutant), b.reshape(b.shape[0], -1))]
    if name == 's2t':
        Nb, h, w, _ = a.shape
        return [(gcols(a, h, w, 1, s2t_taps(0 if mutant == 'tap_table' else g), mutant), s2t_weights(b, g))
                for g in range(4)]
    if name == 's2w':
        Nb, H, W, _ = b.shape
        return [(a.reshape(-1, a.shape[-1]).t(), gcols(b, H // 2, W // 2, 2, S2_TAPS, mutant).t())]
    G = b.shape[0]
    inner = 'conv' if name == 'conv_grp' else 'dense'
    return [view(inner, a[g if a.shape[0] > 1 else 0], b[g], taps, mutant)[0] for g in range(G)]


# --------------------------------------------------------------------------------------------- GEMM
def split_ranges(K, splits):
    """K range of every slab (rk_sgemm: whole 32-deep K-tiles, ceil(kTiles / splits) each); empty ones are (K, K)."""
    kt = cdiv(K, BK)
    per = cdiv(kt, splits)
    return [(min(K, s * per * BK), min(K, (s + 1) * per * BK)) for s in range(splits)]


def gemm(A, B, splits=1, mutant=None):
    """slabs [s][M][N] and S [s][M][N] over each slab's K range."""
    K = A.shape[1]
    kt = cdiv(K, BK)
    if mutant in ('drop_last_k', 'drop_last_chunk', 'drop_last_ktile'):
        A = A.clone()
        A[:, {'drop_last_k': K - 1, 'drop_last_chunk': K - 4, 'drop_last_ktile': (kt - 1) * BK}[mutant]:] = 0
    rng = split_ranges(K, splits)
    slabs = torch.stack([A[:, lo:hi] @ B[:, lo:hi].t() for lo, hi in rng])
    S = torch.stack([A[:, lo:hi].abs() @ B[:, lo:hi].abs().t() for lo, hi in rng])
    if mutant in ('ktile_twice', 'ktile_split_drop'):   # the K-tile after the first split boundary
        lo = rng[1][0]
        slabs[0 if mutant == 'ktile_twice' else 1] += (1 if mutant == 'ktile_twice' else -1) * (
            A[:, lo:lo + BK] @ B[:, lo:lo + BK].t())
    return slabs, S


def yardstick(A, B):
    """The same GEMM in plain fp32 on the CPU: ascending k, one rank-1 update per k."""
    A32, B32 = A.to(torch.float32), B.to(torch.float32)
    acc = torch.zeros(A.shape[0], B.shape[0], dtype=torch.float32)
    for k in range(A.shape[1]):
        acc += A32[:, k, None] * B32[None, :, k]
    return acc.to(F64)


MIN_LIVE = 16


def rms_ratio(got, ref, yard, info=None):
    """Worst over rows and columns of rms(got - ref) / rms(yardstick - ref).  A ratio of two rms estimates needs
    samples: a row (column) with fewer than MIN_LIVE elements on which either error is nonzero - a ReLU or a gate
    leaves some with one or two - is not judged alone (one element's yardstick error is as often 1/10 of its
    typical size as not); those rows (columns) are judged together as one population.  No element is left out.
    info (a dict): receives rows / cols judged alone and rows_pooled / cols_pooled."""
    e, y = (got - ref) ** 2, (yard - ref) ** 2
    live = (e > 0) | (y > 0)
    worst = 0.0
    for d, what in ((1, 'rows'), (0, 'cols')):
        few = live.sum(d) < MIN_LIVE
        num, den = e.sum(d), y.sum(d)
        if info is not None:
            info[what], info[what + '_pooled'] = int((~few).sum()), int(few.sum())
        num = torch.cat([num[~few], num[few].sum()[None]])
        den = torch.cat([den[~few], den[few].sum()[None]])
        if bool(((den == 0) & (num > 0)).any()):
            return float('inf')
        ok = den > 0
        if bool(ok.any()):
            worst = max(worst, float((num[ok] / den[ok]).sqrt().max()))
    return worst


def n_x6(K):
    return int(math.ceil(6.05 * K)) + 1


def n_terms(K, x6):
    return n_x6(K) if x6 else K


# ---------------------------------------------------------------------------------------- epilogues
def epilogue(acc, S, n, *, alpha=1.0, bias=None, stats=False, act=ACT_NONE, slope=0.2, gate=None, bnb=None,
             bnp=None, prior=None, mutant=None, exact=False):
    """s_epilogue in its own order: alpha, bias, statistics (pre-activation), ReLU / leaky, gate, BNB, BNP,
    accumulate.  n = fp32 operations of the accumulator (``n_terms``).  bnb = (y [M][N], scale, shift);
    bnp = (y2 [Nb][2H][2W][N], scale, shift, Nb, H, W).  Returns dict(out, tol[, sums, sums_tol])."""
    v, Sv, n = acc * alpha, S * abs(alpha), n + (alpha != 1.0)
    if bias is not None:
        v, Sv, n = v + bias, Sv + bias.abs(), n + 1
    E = n * U32 * Sv
    res = {}
    if stats and mutant != 'stats_after_act':
        res['sums'], res['sums_tol'] = stats_ref(v, E)
    if act == ACT_RELU:
        v = v.clamp_min(0)
    elif act == ACT_LRELU:   # the fp32 slope; on the exact sets the one product is rounded as the kernel rounds it
        neg = v * float(torch.tensor(slope, dtype=torch.float32))
        v, E = torch.where(v > 0, v, f32r(neg) if exact else neg), E + U32 * v.abs()
    if stats and mutant == 'stats_after_act':
        res['sums'], res['sums_tol'] = stats_ref(v, E)
    if gate is not None:
        m = ((gate >= 0) if mutant == 'gate_ge0' else (gate > 0)).to(F64)
        v, E = v * m, E * m
    if bnb is not None:
        y, scale, shift = bnb
        m = bnb_mask(y, scale, shift).to(F64)
        dz = v if mutant == 'bnb_unmasked' else v * m
        res['sums'], t = bn_sums(dz, y)
        res['sums_tol'] = t + torch.stack([(E * m).sum(0), (E * m * y.abs()).sum(0)])
        v, E = v * m, E * m
    if bnp is not None:
        y2, scale, shift, Nb, H, W = bnp
        pos, yb = bnp_route(y2, scale, shift, Nb, H, W, mutant={'bnp_last_max': 'last_max',
                                                                'bnp_route_on_y': 'route_on_y'}.get(mutant))
        m = pos.to(F64)
        res['sums'], t = bn_sums(v * m, yb)
        res['sums_tol'] = t + torch.stack([(E * m).sum(0), (E * m * yb.abs()).sum(0)])
    if prior is not None:
        E = E + U32 * (v.abs() + prior.abs())
        v = v + prior
    res['out'], res['tol'] = v, E
    return res


def epilogue32(acc, *, alpha=1.0, bias=None, act=ACT_NONE, slope=0.2, gate=None, prior=None):
    """The yardstick's epilogue: the same steps on an fp32 accumulator, every one rounded to fp32 (a bias of the
    accumulator's size costs a rounding as large as the accumulation's own error)."""
    v = f32r(acc * alpha)
    if bias is not None:
        v = f32r(v + bias)
    if act == ACT_RELU:
        v = v.clamp_min(0)
    elif act == ACT_LRELU:
        v = torch.where(v > 0, v, f32r(v * float(torch.tensor(slope, dtype=torch.float32))))
    if gate is not None:
        v = v * (gate > 0).to(F64)
    if prior is not None:
        v = f32r(v + prior)
    return v


def reduce_epi(slabs, Ss, n, **kw):
    """rk_sreduce_epi / rk_reduce_slabs on the slabs: the slab sum (one more fp32 addition per slab) through
    ``epilogue`` (alpha, bias, activation, gate)."""
    return epilogue(slabs.sum(0), Ss.sum(0), n + slabs.shape[0] - 1, **kw)


# ------------------------------------------------------------------------------------------- inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _sparse(seed, shape, keep):
    return (torch.rand(tuple(shape), generator=_gen(seed)) < keep).to(F64)


def wide18(seed, shape, keep):
    """Odd integers with 2^17 <= |x| < 2^18 on a fraction ``keep`` of the elements, zero elsewhere."""
    mag = 2 * torch.randint(2 ** 16, 2 ** 17, tuple(shape), generator=_gen(seed)) + 1
    sign = 2 * torch.randint(0, 2, tuple(shape), generator=_gen(seed + 1)) - 1
    return (mag * sign).to(F64) * _sparse(seed + 2, shape, keep)


def wide_mm(seed, shape, keep):
    s, t = (ints(seed + i, shape, 1, 3) * (2 * ints(seed + 5 + i, shape, 0, 1) - 1) for i in (0, 1))
    return (256 * s + t) * _sparse(seed + 2, shape, keep)


def draw_gate(seed, shape):
    """A ReLU gate: igemm_refs' decision draw with every 5th element exactly zero (the mask is gate > 0)."""
    g = draw_decision(seed, shape).reshape(-1).clone()
    g[::5] = 0.0
    return g.reshape(tuple(shape))


def normal_f32(seed, shape, scale=1.0):
    return (torch.randn(tuple(shape), generator=_gen(seed)) * scale).to(torch.float32).to(F64)


def draw_pair(mode, seed, sa, sb, K):
    """(activation-like a of shape sa, weight-like b of shape sb) for a reduction of length K."""
    if mode == 'exact':
        return ints(seed, sa, -2, 2), ints(seed + 10, sb, -1, 1)
    if mode == 'wide_a':    # <= 2^18 * 40 expected per output: far below 2^24 / 2^18 = 64 products at +-4 sigma
        return wide18(seed, sa, min(1.0, 24.0 / K)), ints(seed + 10, sb, -1, 1)
    if mode == 'wide_b':
        return ints(seed, sa, -1, 1), wide18(seed + 10, sb, min(1.0, 24.0 / K))
    if mode == 'wide_mm':   # products <= 771^2 < 2^20: 16 per output allowed, K * keep^2 = 4 expected
        keep = min(1.0, (4.0 / K) ** 0.5)
        return wide_mm(seed, sa, keep), wide_mm(seed + 10, sb, keep)
    return normal_f32(seed, sa), normal_f32(seed + 10, sb, K ** -0.5)


def problem(name, shape, taps, mode):
    """Raw operands (a, b) of ``view(name, ...)`` at ``shape``: conv kinds (Nb, H, W, Cin, Cout) with H x W the
    full-resolution map, dense kinds (M, N, K) of the GEMM, grouped ones with G = 3 (``shared``: one input)."""
    shared = name.endswith('_shared')
    name = name.replace('_shared', '')
    seed = 7 * sum(shape) + taps + 1000 * sorted(NAMES).index(name)
    if name in ('dense', 'dx', 'dw', 'dense_grp'):
        M, N, K = shape
        sa, sb = {'dense': ((M, K), (N, K)), 'dx': ((M, K), (K, N)), 'dw': ((K, M), (K, N)),
                  'dense_grp': ((1 if shared else 3, M, K), (3, N, K))}[name]
        return draw_pair(mode, seed, sa, sb, K)
    Nb, H, W, Ci, Co = shape
    pix = Nb * H * W
    if name == 'conv':
        return draw_pair(mode, seed, (Nb, H, W, Ci), (Co, taps, Ci), taps * Ci)
    if name == 'conv_grp':
        return draw_pair(mode, seed, (1 if shared else 3, Nb, H, W, Ci), (3, Co, taps, Ci), taps * Ci)
    if name == 'dgrad':
        return draw_pair(mode, seed, (Nb, H, W, Co), (Co, taps, Ci), taps * Co)
    if name == 'wgrad':
        return draw_pair(mode, seed, (Nb, H, W, Co), (Nb, H, W, Ci), pix)
    if name == 's2':
        return draw_pair(mode, seed, (Nb, H, W, Ci), (Co, 16, Ci), 16 * Ci)
    if name == 's2t':    # z at half resolution, W [Co][16][Ci]
        return draw_pair(mode, seed, (Nb, H // 2, W // 2, Co), (Co, 16, Ci), 4 * Co)
    if name == 's2w':
        return draw_pair(mode, seed, (Nb, H // 2, W // 2, Co), (Nb, H, W, Ci), pix // 4)
    raise ValueError(name)


NAMES = ('conv', 'dgrad', 'wgrad', 'dense', 'dx', 'dw', 's2', 's2t', 's2w', 'conv_grp', 'dense_grp')

# ------------------------------------------------------------------------------------------- shapes
# dense (M, N, K): (264, 132, 132) two tiles each way even at 256x128, the last partial in M and N, 4 K-tiles and
# a 4-wide tail (a 3-stage ring wraps);  (37, 20, 36) under one tile, fewer K-tiles than ring stages;  K = 32.
DENSE_SHAPES = [(264, 132, 132), (37, 20, 36), (72, 40, 32)]
# the weight gradient reduces over rows (K-outer operands: M, N in multiples of 4, any K): K = 37 is a 5-row tail
DW_SHAPES = [(264, 132, 132), (36, 20, 37), (72, 40, 32)]
# conv (Nb, H, W, Cin, Cout): C % 32 == 0 with reciprocal / shift pixel decode, the general gather (a K-tile
# straddles taps, reciprocal channel decode), every pixel on a border
CONV_SHAPES = [((8, 6, 6, 32, 132), 9), ((5, 8, 8, 32, 72), 9), ((3, 6, 6, 12, 40), 9), ((1, 12, 20, 8, 8), 9),
               ((5, 2, 2, 64, 64), 9), ((5, 8, 8, 32, 72), 1), ((3, 6, 6, 12, 40), 1)]
S2_SHAPES = [(2, 8, 8, 32, 64), (1, 12, 12, 24, 40)]
GRP_CONV = [((2, 6, 6, 12, 40), 9), ((1, 4, 4, 32, 72), 1)]
GRP_DENSE = [(37, 20, 36), (136, 72, 132)]
SWEEP = ([('conv', s, t) for s, t in CONV_SHAPES] + [('wgrad', s, t) for s, t in CONV_SHAPES]
         + [(k, s, 1) for k in ('dense', 'dx') for s in DENSE_SHAPES] + [('dw', s, 1) for s in DW_SHAPES]
         + [(k, s, 16) for k in ('s2', 's2t', 's2w') for s in S2_SHAPES]
         + [(k, s, t) for k in ('conv_grp', 'conv_grp_shared') for s, t in GRP_CONV]
         + [(k, s, 1) for k in ('dense_grp', 'dense_grp_shared') for s in GRP_DENSE])
# the dense layer (batch 256, 2048 -> 512), the smallest at which the pre-split dense candidates are offered, as the
# (M, N, K) of its three GEMMs: forward x [256][2048] . w [512][2048]^T, data gradient dy [256][512] . w [512][2048],
# weight gradient dy [256][512]^T . x [256][2048]
BIG_LAYER = {'dense': (256, 512, 2048), 'dx': (256, 2048, 512), 'dw': (512, 2048, 256)}
