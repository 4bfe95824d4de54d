"""fp64 CPU references, input sets, derived tolerances and the judge for the fused Winograd family
(csrc/kernels/winograd.hip, winograd4.hip, wino_wt.h: rk_wino_conv_grp, rk_wino2s_conv_grp, rk_wino4_conv_grp,
rk_wino_wgrad, rk_wino4_wgrad, rk_wino_weights, rk_wino4_weights, rk_wino4b_weights).  Imports nothing from
rafiki_amd; the epilogue references (bias, ReLU, statistics, BNB, BNP), the decision draws and the yardstick gate
come from sgemm_refs / igemm_refs unchanged.

The algorithm.  MO = 2 is F(2x2,3x3) (points 0, 1, -1, inf), MO = 4 is F(4x4,3x3) (Lavin & Gray's points 0, 1,
-1, 2, -2, inf); A = MO + 2, P = A * A positions, position q = a * A + b.  The literal tables BT, AT, G below are
the kernels' bt6 / at6 / g6 and bt4 / at4 / w_transform written as matrices.
  transform_weights   U[q][row][col] = (G g G^T)[a][b] of g = w[co][ky][kx][ci]: rows co, columns ci for the
                      forward set; for the data-gradient set rows ci, columns co and g flipped (tap t -> 8 - t)
  fused_conv          y = A^T [sum_c U_c (.) (B^T d_c B)] A per MO x MO output tile, d the A x A window at
                      (MO ty - 1, MO tx - 1), zero outside the image.  It takes any U.
  fused_wgrad         dW = G^T [sum_t (A dY_t A^T) (.) (B^T d_t B)] G, one slab per split: split s owns the
                      tiles [s tps, (s + 1) tps), tps = ceil(ceil(T / splits) / 8) * 8 (tiles in (n, ty, tx) order)
  normalise-on-load   d = relu(x * scale + shift) on in-image elements, zero outside
Every function takes ``absval``: the same algorithm on |x|, |U|, |G|, |B|, |A| (|x * scale| + |shift| under
normalise-on-load, no ReLU).  That is S, the scale of the error model.

Hard tolerance of a RANDOM result: n * 2^-23 * S per element (2^-23 is twice fp32's unit roundoff, igemm_refs'
rule).  n = terms of the MFMA sum + the fp32 roundings on the longest path through the transforms, counted from
the kernels' code, each stage applied once per axis (FMA contraction only removes roundings):
  bt6   t0 = 4 d0 - 5 d2 + d4: one product (4 d0 is exact), two additions           3 per axis, 6
  at6   o3 = (m1 - m2) + 8 (m3 - m4) + m5: difference, addition, addition (8 x exact)  3 per axis, 6
  bt4   one addition per axis                                                           2
  at4   o0 = m0 + m1 + m2                                                           2 per axis, 4
  g6    u3 = g0 / 24 + g1 / 12 + g2 / 6: the rounded constant, product, two additions  4 per axis, 8
  w_transform  0.5 (g0 + g1 + g2): two additions (the halving is exact)                2 per axis, 4
  a6 (weight gradient, A dY)  m3 = (y0 + 4 y2) + (2 y1 + 8 y3)                          2 per axis, 4
  gt6 (G^T)  g0 = x0 / 4 - (x1 + x2) / 6 + (x3 + x4) / 24: sum, constant, product, two additions  5 per axis, 10
  F(2x2) weight gradient: A dY one addition per axis (2), G^T x0 + 0.5 (x1 + x2) two per axis (4)
so  N_FWD = {2: C + 6, 4: C + 12} (+ 1 with a bias, + 2 with normalise-on-load: the fma and nothing else, counted
as product and sum),  N_WGRAD = {2: T + 8, 4: T + 20} (+ 1 accumulating, + 2 with normalise-on-load),
N_WEIGHTS = {2: 4, 4: 8}.  These counts are derived, not measured.

Statistics.  The epilogues sum v and v * v (BNB / BNP: dz and dz * y) in fp32 per lane over 4 tiles (4 MO^2
elements), add four lanes by shuffles and only then add to the fp64 slots.  Against the fp64 reference the bound
is igemm_refs.stats_ref's (sgemm_refs.epilogue).  Against the output the same launch wrote (``own_sums``) only the
epilogue's own arithmetic counts: (4 MO^2 + 2) additions and, for the second sum, one product, i.e.
    |sum - sum(out)| <= (4 MO^2 + 2) 2^-23 sum |v|,   |sumsq - sum(out^2)| <= (4 MO^2 + 3) 2^-23 sum v^2
and on the exact sets a sum must be equal wherever its fp32 partial sums (16 MO^2 terms) stay below 2^24
(``sums_exact``: the sum of v on every sweep shape, the sum of v^2 on F(2x2) only: F(4x4)'s exact values reach 3e4
and their squares leave fp32's integers), else it is held to the bound.

Input sets
  exact     integer x in [-2, 2] and an integer-valued U in {-1, 0, 1} on a sparse subset (``draw_u``: at most
            about 24 nonzeros per output and position), handed to the kernel directly, blocked variants through
            ``blocked_index`` (winograd4.hip's w4b_index).  ``exact_ok`` asserts S < 2^24 for every element: every
            intermediate is then an integer fp32 holds, and the output must be right to the bit.
  exact_w   F(2x2) only: weights that are multiples of 4.  G has only 1 and 1/2, so G g G^T is an integer and
            the whole path from w is exact.  F(4x4)'s G has 1/6 and 1/24, which fp32 does not hold: no such set,
            and for the same reason (G^T) the F(4x4) weight gradient has no exact set either; F(2x2)'s has.
  yardstick the same algorithm in plain fp32 torch on the CPU: the transforms as fp32 einsums, the sum over input
            channels (weight gradient: over tiles) one term at a time in ascending order, sgemm_refs.yardstick's
            rule.  (An fp32 BLAS sums in blocks; at C = 512 that is 2.4x more accurate than plain fp32.)
  random    normal x, w / sqrt(9 C); U = G g G^T in fp64 rounded to fp32, so the reference sees the kernel's
            operand and the fused kernel is judged apart from the weight transform.
  BNB / BNP gates are sgemm_refs' decision draws (y = k / 64, scale +-2^j, shift a multiple of 1/64):
  ``decisions_inexact`` must be 0, nothing is left out of a comparison.
"""
import torch

import sgemm_refs as G_
from igemm_refs import F64, U32, LIM, cdiv, f32r, ints  # noqa: F401
from sgemm_refs import YARD, rms_ratio

F32 = torch.float32
RELU, BIAS, STATS, LRELU, BNB, BNP, POOL = 1, 2, 4, 8, 512, 1024, 2048
POOLED = BIAS | RELU | POOL
KC = 8
PRO_MAXC = 512

BT6 = [[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
       [0, 4, 0, -5, 0, 1]]
AT6 = [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]]
G6 = [[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6],
      [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]]
BT4 = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
AT4 = [[1, 1, 1, 0], [0, 1, -1, -1]]
G4 = [[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]]
MATS = {2: tuple(torch.tensor(m, dtype=F64) for m in (BT4, AT4, G4)),
        4: tuple(torch.tensor(m, dtype=F64) for m in (BT6, AT6, G6))}
N_TRANSFORMS_FWD = {2: 6, 4: 12}
N_TRANSFORMS_WGRAD = {2: 8, 4: 20}
N_WEIGHTS = {2: 4, 4: 8}


def mats(MO, absval=False, dtype=F64):
    m = MATS[MO]
    return tuple((t.abs() if absval else t).to(dtype) for t in m)


def n_fwd(MO, C, bias=False, pro=False):
    return C + N_TRANSFORMS_FWD[MO] + int(bias) + 2 * int(pro)


def n_wgrad(MO, tiles, pro=False, prior=False):
    return tiles + N_TRANSFORMS_WGRAD[MO] + 2 * int(pro) + int(prior)


# ---------------------------------------------------------------------------------------- weights
def transform_weights(w, MO, dgrad=False, absval=False, mutant=None, dtype=F64):
    """w [Co][9][Ci] -> U [P][Co][Ci], or the data-gradient set [P][Ci][Co] of the flipped filters."""
    Co, _, Ci = w.shape
    Gm = mats(MO, absval, dtype)[2]
    g = (w.abs() if absval else w).to(dtype).reshape(Co, 3, 3, Ci)
    if dgrad:
        if mutant != 'noflip':
            g = g.flip(1, 2)
        g = g.permute(3, 1, 2, 0)
    U = torch.einsum('ay,rykc,bk->abrc', Gm, g, Gm)
    return U.reshape(-1, U.shape[2], U.shape[3]).contiguous()


def blocked_index(rows, cols):
    """Flat offset of element (pos, r, c) of a [36][rows][cols] set in the blocked layout (w4b_index):
    [rows / 32 rounded up][cols / 8][36][32][8], column swizzled by row bits 2-3."""
    pos, r, c = torch.meshgrid(torch.arange(36), torch.arange(rows), torch.arange(cols), indexing='ij')
    return ((((r >> 5) * (cols >> 3) + (c >> 3)) * 36 + pos) * 32 + (r & 31)) * 8 + ((c & 7) ^ ((((r & 31) >> 2) & 3) << 1))


def blocked_numel(rows, cols):
    return 36 * cdiv(rows, 32) * 32 * cols


def to_blocked(U):
    """The blocked image (flat, zero in the rows padded up to 32) of U [36][rows][cols]."""
    _, rows, cols = U.shape
    out = torch.zeros(blocked_numel(rows, cols), dtype=U.dtype)
    out[blocked_index(rows, cols).reshape(-1)] = U.reshape(-1)
    return out


# --------------------------------------------------------------------------------------- fused conv
def normalise(x, pro, absval=False, dtype=F64):
    if pro is None:
        return x.abs() if absval else x
    scale, shift = (t.to(dtype) for t in pro)
    if absval:
        return (x * scale).abs() + shift.abs()
    return (x * scale + shift).clamp_min(0)


def windows(x, MO, pro=None, absval=False, mutant=None):
    """d [Nb][H/MO][W/MO][A][A][C]: the A x A window of every tile, zero outside the image."""
    Nb, H, W, C = x.shape
    A = MO + 2
    xn = normalise(x, pro, absval, x.dtype)
    xp = torch.zeros(Nb, H + 2, W + 2, C, dtype=x.dtype)
    if mutant == 'pad_relu_shift':       # the padding normalised like an element: relu(0 * scale + shift)
        xp += pro[1].to(x.dtype).clamp_min(0)
    xp[:, 1:-1, 1:-1] = xn
    if mutant == 'border_neighbour':     # the row above a middle image: the previous image's last row, not zero
        m = Nb // 2
        xp[m, 0, 1:-1] = xn[m - 1, H - 1]
    return torch.stack([torch.stack([xp[:, a:a + H:MO, b:b + W:MO] for b in range(A)], 3) for a in range(A)], 3)


def fused_conv(x, U, MO, *, pro=None, absval=False, mutant=None, tile_block=64):
    """y [Nb][H][W][N] of x [Nb][H][W][C] and U [P][N][C], in x's dtype (fp64: the reference; fp32: the yardstick).
    mutant: one of the wrong kernels of tests/test_wino_refs.py."""
    Nb, H, W, C = x.shape
    A = MO + 2
    dtype = x.dtype
    N = U.shape[1]
    BT, AT, _ = mats(MO, absval, dtype)
    U = (U.abs() if absval else U).to(dtype).reshape(A, A, N, C)
    d = windows(x, MO, pro, absval, mutant)
    V = torch.einsum('ia,ntxabc,jb->ntxijc', BT, d, BT)
    if mutant == 'drop_last_chunk':
        V = V.clone()
        V[..., C - KC:] = 0
    if dtype == F64:
        M = torch.einsum('ntxijc,ijkc->ntxijk', V, U)
    else:   # the yardstick: plain fp32, one input channel at a time in ascending order (as sgemm_refs.yardstick;
        M = torch.zeros(V.shape[:5] + (N,), dtype=dtype)    # a BLAS sums in blocks, which is better than plain)
        for c in range(C):
            M += V[..., c, None] * U[..., c]
    if mutant == 'double_chunk':         # the two-stage loop's tail: with an odd chunk count the last one runs twice
        M = M + torch.einsum('ntxijc,ijkc->ntxijk', V[..., C - KC:], U[..., C - KC:])
    Y = torch.einsum('pi,ntxijk,qj->ntxpqk', AT, M, AT)
    if mutant in ('at_coeff', 'at_slight'):   # A^T[MO - 1][3] (8 in at6) halved, or off by 2^-16 of itself, at
        AT2 = AT.clone()                      # in-tile position (MO - 1, 1) only
        AT2[MO - 1, 3] *= 0.5 if mutant == 'at_coeff' else 1 - 2.0 ** -16
        Y2 = torch.einsum('pi,ntxijk,qj->ntxpqk', AT2, M, AT)
        Y = Y.clone()
        Y[:, :, :, MO - 1, 1] = Y2[:, :, :, MO - 1, 1]
    if mutant == 'drop_tile_block':      # the last, partial block of ``tile_block`` tiles never written
        T = Nb * (H // MO) * (W // MO)
        flat = Y.reshape(T, MO, MO, N).clone()
        flat[T // tile_block * tile_block:] = 0
        Y = flat.reshape(Y.shape)
    if mutant == 'skip_channel':         # channel N - 1 of a partial 16-channel block left unwritten
        Y = Y.clone()
        Y[..., N - 1] = 0
    return Y.permute(0, 1, 3, 2, 4, 5).reshape(Nb, H, W, N)


def pool2(v):
    """2x2 max-pool of v [Nb][H][W][N] -> [Nb][H/2][W/2][N]."""
    Nb, H, W, N = v.shape
    return v.reshape(Nb, H // 2, 2, W // 2, 2, N).amax((2, 4))


def pooled(acc, S, n, bias, mutant=None):
    """WF_POOL: max over each 2x2 window of relu(acc + bias).  The maximum is 1-Lipschitz in every argument: the
    window's largest element tolerance bounds the error."""
    v = (acc + bias).clamp_min(0)
    E = (n + 1) * U32 * (S + bias.abs())
    if mutant == 'pool_shift':           # the window one column to the right of where it belongs
        v = torch.roll(v, -1, 2)
    return pool2(v), pool2(E)


def own_sums(out, MO, *, second=None):
    """(sum out, sum out * second) per channel of the output a launch wrote (second None: out itself), with the
    accuracy the epilogue's fp32 partial sums allow."""
    o = out.reshape(-1, out.shape[-1])
    s2 = o if second is None else second.reshape(o.shape)
    n = 4 * MO * MO + 2
    return (torch.stack([o.sum(0), (o * s2).sum(0)]),
            torch.stack([n * U32 * o.abs().sum(0), (n + 1) * U32 * (o * s2).abs().sum(0)]))


# ---------------------------------------------------------------------------------- weight gradient
def wgrad_splits(tiles, splits):
    """[(first tile, end tile)] per split, or None where the launcher refuses (a split without tiles)."""
    tps = cdiv(cdiv(tiles, splits), KC) * KC
    if cdiv(tiles, tps) != splits:
        return None
    return [(s * tps, min((s + 1) * tps, tiles)) for s in range(splits)]


def fused_wgrad(dy, x, MO, splits=1, *, pro=None, absval=False, mutant=None):
    """slabs [splits][Co][9][Ci] of dy [Nb][H][W][Co], x [Nb][H][W][Ci], and the tile count of every split."""
    Nb, H, W, Co = dy.shape
    Ci = x.shape[-1]
    dtype = x.dtype
    BT, AT, Gm = mats(MO, absval, dtype)
    d = windows(x, MO, pro, absval, mutant).reshape(-1, MO + 2, MO + 2, Ci)
    dyt = (dy.abs() if absval else dy).reshape(Nb, H // MO, MO, W // MO, MO, Co).permute(0, 1, 3, 2, 4, 5)
    dyt = dyt.reshape(-1, MO, MO, Co)
    V = torch.einsum('ia,tabc,jb->tijc', BT, d, BT)
    Md = torch.einsum('pi,tpqk,qj->tijk', AT, dyt, AT)      # A dY A^T, A = (A^T)^T
    rng = wgrad_splits(V.shape[0], splits)
    if mutant == 'split_short':          # the first split stops one chunk of 8 tiles early
        rng = [(rng[0][0], max(rng[0][0], rng[0][1] - KC))] + rng[1:]
    slabs = []
    for lo, hi in rng:
        if dtype == F64:
            dU = torch.einsum('tijk,tijc->ijkc', Md[lo:hi], V[lo:hi])
        else:   # the yardstick: one tile at a time in ascending order
            dU = torch.zeros(Md.shape[1:] + (Ci,), dtype=dtype)
            for t in range(lo, hi):
                dU += Md[t, :, :, :, None] * V[t, :, :, None, :]
        slabs.append(torch.einsum('iy,ijkc,jx->kyxc', Gm, dU, Gm).reshape(Co, 9, Ci))
    return torch.stack(slabs), [hi - lo for lo, hi in rng]


# -------------------------------------------------------------------------------------------- judge
WORST, YWORST = {}, {}


def _by_position(t, MO):
    """[Nb][H][W][N] -> [MO * MO][the rest]: one row per in-tile position (oy % MO, ox % MO)."""
    Nb, H, W, N = t.shape
    return t.reshape(Nb, H // MO, MO, W // MO, MO, N).permute(2, 4, 0, 1, 3, 5).reshape(MO * MO, -1)


def _rows_ratio(got, ref, yard):
    """sgemm_refs.rms_ratio over the rows of [rows][samples] alone (only the rows mean something here: a column
    would be one pixel across channels).  Rows go eight at a time, so the columns hold fewer than MIN_LIVE elements
    and rms_ratio judges them together as one population; the rows that a ReLU or a gate leaves fewer than
    MIN_LIVE elements with an error are judged together as one population, rms_ratio's own rule, as one long row;
    where even together they have fewer than MIN_LIVE, their elements are judged with everything else, as part of
    the whole tensor.  No element is left out."""
    live = (((got - ref) != 0) | ((yard - ref) != 0)).sum(1)
    few = live < G_.MIN_LIVE
    pooled = few if int(live[few].sum()) >= G_.MIN_LIVE else torch.ones_like(few)
    sets = [[t[pooled].reshape(1, -1) for t in (got, ref, yard)]] if bool(few.any()) else []
    full = [t[~few] for t in (got, ref, yard)]
    sets += [[t[i:i + 8] for t in full] for i in range(0, full[0].shape[0], 8)]
    return max(rms_ratio(*v) for v in sets)


def yard_ratio(got, ref, yard, layout, MO):
    """Worst rms(got - ref) / rms(yardstick - ref) per output channel and per in-tile position of a conv output
    [Nb][H][W][N], per output channel and per tap of a weight gradient [Co][9][Ci]."""
    if layout == 'wgrad':
        Co = got.shape[0]
        views = [[t.reshape(Co, -1) for t in (got, ref, yard)],
                 [t.permute(1, 0, 2).reshape(9, -1) for t in (got, ref, yard)]]
    else:
        N = got.shape[-1]
        views = [[t.reshape(-1, N).t() for t in (got, ref, yard)]]
        if MO > 1:
            views.append([_by_position(t, MO) for t in (got, ref, yard)])
    return max(_rows_ratio(*v) for v in views)


def judge(tag, got, ref, tol, mode, yard=None, what='', layout='conv', MO=1):
    """Exact sets: got == ref everywhere.  RANDOM: |got - ref| <= tol element by element and, with a yardstick,
    rms(got - ref) <= YARD * rms(yardstick - ref) per channel and per in-tile position (``yard_ratio``).
    Records the worst error / tolerance and the worst yardstick ratio per tag."""
    got = got.to('cpu', F64)
    assert got.shape == ref.shape, (tag, what, got.shape, ref.shape)
    nan = torch.isnan(got)
    assert not bool(nan.any()), '{} {}: {} NaN in the output (unwritten, or an over-read operand); first at {}'.format(
        tag, what, int(nan.sum()), tuple(int(v) for v in nan.nonzero()[0]))
    err = (got - ref).abs()
    if mode != 'random':
        bad = err != 0
    else:
        bad = err > tol
        ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), (err > 0).to(F64) * 1e30)
        WORST[tag] = max(WORST.get(tag, 0.0), float(ratio.max()) if ratio.numel() else 0.0)
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError('{} {} [{}]: {} of {} elements off; first at {}: got {!r} ref {!r} tol {!r}'.format(
            tag, what, mode, int(bad.sum()), bad.numel(), i, float(got[i]), float(ref[i]),
            float(tol[i]) if mode == 'random' else 0.0))
    if mode == 'random' and yard is not None:
        r = yard_ratio(got, ref, yard, layout, MO)
        YWORST[tag] = max(YWORST.get(tag, 0.0), r)
        assert r <= YARD, '{} {}: rms error {:.2f}x the fp32 yardstick (gate {})'.format(tag, what, r, YARD)


def sums_exact(v, MO, second=None, unit=1.0):
    """Whether the fp32 partial sums of v and of v * second (second None: v itself; ``unit``: the granule of the
    products) are exact on an exact set, 16 MO^2 elements each (4 tiles per lane, four lanes): (first sum, second
    sum).  The fp64 slots add the partial sums exactly."""
    n, a = 16 * MO * MO, float(v.abs().max())
    b = float((v * (v if second is None else second)).abs().max()) / unit
    return n * a < LIM, n * b < LIM


def judge_sums(tag, got, ref, tol, mode, v, MO, what='', second=None, unit=1.0):
    """The two rows of a statistic [2][N]: equal where ``sums_exact`` says the epilogue's sums are exact, else
    within tol."""
    for i, ok in enumerate(sums_exact(v, MO, second, unit)):
        judge(tag, got[i], ref[i], tol[i], mode if ok else 'random', what='{} sum {}'.format(what, i))


def frobenius(a, b):
    """The older Winograd tests' one number: relative Frobenius error over the whole tensor."""
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


OLD_GATE = {2: 1e-5, 4: 3e-5}


# ------------------------------------------------------------------------------------------- inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def draw_u(seed, MO, N, C):
    """Integer-valued U [P][N][C] in {-1, 0, 1}, about min(C, 24) nonzeros per output and position."""
    P = (MO + 2) ** 2
    keep = (torch.rand((P, N, C), generator=_gen(seed + 1)) < min(1.0, 24.0 / C)).to(F64)
    return ints(seed, (P, N, C), -1, 1) * keep


def draw_x(mode, seed, shape):
    if mode == 'random':
        return G_.normal_f32(seed, shape)
    return ints(seed, shape, -2, 2)


def draw_w(mode, seed, Co, Ci):
    """w [Co][9][Ci]: random w / sqrt(9 C); exact_w multiples of 4."""
    if mode == 'exact_w':
        return 4.0 * ints(seed, (Co, 9, Ci), -2, 2)
    return G_.normal_f32(seed, (Co, 9, Ci), (9 * Ci) ** -0.5)


def draw_bias(mode, seed, n):
    return G_.normal_f32(seed, (n,)) if mode == 'random' else ints(seed, (n,), -3, 3)


def draw_pro(mode, seed, C):
    """(scale, shift) of normalise-on-load: scale of both signs, shift positive and negative.  Exact sets: scale
    +-1 / +-2 and integer shift, so x * scale + shift is an integer with or without contraction."""
    if mode == 'random':
        scale = G_.normal_f32(seed, (C,)) + 0.25
        shift = G_.normal_f32(seed + 1, (C,), 0.5)
    else:
        scale = (2.0 ** ints(seed, (C,), 0, 1)) * (2 * ints(seed + 2, (C,), 0, 1) - 1)
        shift = ints(seed + 1, (C,), -2, 2)
    scale[0], shift[0] = scale[0].abs(), shift[0].abs() + 1       # both signs in every draw, C >= 8
    scale[1], shift[1] = -scale[1].abs(), -shift[1].abs() - 1
    scale[2], shift[2] = -scale[2].abs(), shift[2].abs() + 1
    return scale, shift


def exact_ok(S, units=1.0):
    """The exact sets' precondition: the absolute-value companion below 2^24 for every element (in ``units``)."""
    return bool((S / units < LIM).all())


def conv_problem(mode, MO, shape, pro=False, salt=0):
    """(x, U [P][N][C], pro or None) of the fused conv at shape (Nb, H, W, C, N); ``salt``: another draw (the
    groups of a grouped launch)."""
    Nb, H, W, C, N = shape
    seed = 31 * sum(shape) + 1000 * MO + (500 if pro else 0) + 77 * salt
    x = draw_x(mode, seed, (Nb, H, W, C))
    if mode == 'random':
        U = f32r(transform_weights(draw_w(mode, seed + 10, N, C), MO))
    else:
        U = draw_u(seed + 10, MO, N, C)
    return x, U, (draw_pro(mode, seed + 20, C) if pro else None)


def wgrad_problem(mode, MO, shape):
    """(dy [Nb][H][W][Co], x [Nb][H][W][Ci]) at shape (Nb, H, W, Ci, Co)."""
    Nb, H, W, Ci, Co = shape
    seed = 37 * sum(shape) + 1000 * MO
    return draw_x(mode, seed, (Nb, H, W, Co)), draw_x(mode, seed + 10, (Nb, H, W, Ci))


# ------------------------------------------------------------------------------------------- shapes
# F(4x4) (Nb, H, W, C, N); F(2x2) runs the same with H, W halved, so the tile counts are the same:
#   (3, 4, 12, 24, 40)   9 tiles: below one tile block, no multiple of 8 (the weight gradient's chunk tail); a middle
#                        image with neighbours on both sides; H != W, 3 tiles per row; C = 24: three chunks, odd
#                        for the two-stage and warp-specialised loops; N = 40: partial 16-, 32- and 64-channel blocks;
#                        weight gradient Co = 40 against variant 1's 64-row block, Ci = 24
#   (1, 12, 20, 8, 8)    15 tiles under a 16-tile block, 5 tiles per row (W = 20), one chunk, N = 8, Ci = 8
#   (5, 12, 20, 8, 72)   75 tiles: blocks of 16, 32 and 64 tiles all full at least once with a remainder (11);
#                        N = 72: three 32-channel blocks, the last partial; 2 and 4 splits end on a short split
#   (2, 4, 4, 512, 32)   C = 512 = W4_PRO_MAXC once, on a 4x4 map: 64 chunks, every window on all four borders
#   (3, 8, 8, 16, 40)    12 tiles, two chunks, a middle image, partial channel blocks
SHAPES4 = [(3, 4, 12, 24, 40), (1, 12, 20, 8, 8), (5, 12, 20, 8, 72), (2, 4, 4, 512, 32), (3, 8, 8, 16, 40)]


def shapes(MO):
    return SHAPES4 if MO == 4 else [(s[0], s[1] // 2, s[2] // 2, s[3], s[4]) for s in SHAPES4]


# the forward entry points: (entry, variant) -> (MO, tiles per block, channels per block, blocked weights,
# two-stage / warp-specialised K loop)
FWD = {
    ('rk_wino_conv_grp', 0): (2, 64, 32, False, False), ('rk_wino_conv_grp', 1): (2, 64, 64, False, True),
    ('rk_wino2s_conv_grp', 0): (2, 32, 32, False, False), ('rk_wino2s_conv_grp', 1): (2, 16, 32, False, False),
    ('rk_wino2s_conv_grp', 2): (2, 64, 32, False, False), ('rk_wino2s_conv_grp', 3): (2, 64, 32, False, True),
    ('rk_wino4_conv_grp', 0): (4, 64, 32, False, False), ('rk_wino4_conv_grp', 1): (4, 32, 32, False, False),
    ('rk_wino4_conv_grp', 2): (4, 32, 32, False, True), ('rk_wino4_conv_grp', 3): (4, 64, 32, True, False),
    ('rk_wino4_conv_grp', 4): (4, 32, 32, True, False), ('rk_wino4_conv_grp', 5): (4, 32, 32, True, True),
}
PRO_VARIANTS = (3, 4, 5)
# flag combinations with a compile-time instantiation in launch_gfwd, then what falls to FL = -1 (rk_wino_conv_grp
# reads its flags at run time throughout)
FLAG_SETS = [0, STATS, BIAS | RELU, BNB, BNP, POOLED, BIAS, RELU, BIAS | STATS, RELU | STATS, BIAS | RELU | STATS]


def expected_status(entry, variant, shape, *, flags=0, groups=1, bias=False, stats=False, gate=False, pro=False,
                    splits=1, accumulate=False):
    """What the launcher must answer, from the argument checks of rk_wino_conv_grp, gfwd_dispatch + launch_gfwd,
    rk_wino_wgrad and rk_wino4_wgrad in their own order: 0, RK_EBADARG (-1) or RK_EUNSUPPORTED (-2).
    shape (Nb, H, W, C, N) for the forward entries, (Nb, H, W, Ci, Co) for the weight gradients."""
    Nb, H, W, C, N = shape
    if entry in ('rk_wino_wgrad', 'rk_wino4_wgrad'):
        MO = 2 if entry == 'rk_wino_wgrad' else 4
        if Nb <= 0 or H <= 0 or W <= 0 or H % MO or W % MO or C <= 0 or N <= 0 or splits <= 0:
            return -1
        if splits > 1 and accumulate:
            return -1
        if MO == 4:
            if variant < 0 or variant > 2:
                return -1
            if pro and variant == 2:
                return -2
        tiles = Nb * (H // MO) * (W // MO)
        if tiles >= 1 << 22:
            return -2
        if 4 * Nb * H * W * max(C, N) >= 0x7fffffff:
            return -2
        return 0 if wgrad_splits(tiles, splits) is not None else -1
    if entry == 'rk_wino_conv_grp':
        if variant not in (0, 1):
            return -1
        if flags & POOL:
            return -2
        MO, blocked = 2, False
    else:
        if (entry, variant) not in FWD or (pro and (entry != 'rk_wino4_conv_grp' or variant not in PRO_VARIANTS)):
            return -2 if pro else -1
        MO, blocked = FWD[(entry, variant)][0], FWD[(entry, variant)][3]
    if Nb <= 0 or H <= 0 or W <= 0 or H % MO or W % MO or C <= 0 or C % KC or N <= 0 or groups <= 0:
        return -1
    if flags & (STATS | BNB | BNP) and not stats:
        return -1
    if flags & (BNB | BNP) and not (gate and bias):
        return -1
    if flags & BIAS and not bias:
        return -1
    if groups > 1 and flags & (STATS | BNB | BNP):
        return -2
    if entry != 'rk_wino_conv_grp':
        if flags & POOL and (flags != POOLED or pro or H & 1 or W & 1):
            return -2
        if pro and (groups > 1 or flags & ~STATS or C > PRO_MAXC):
            return -2
    tiles = Nb * (H // MO) * (W // MO)
    if tiles >= 1 << 30:
        return -1
    P = (MO + 2) ** 2
    ybytes = 4 * Nb * (H // 2) * (W // 2) * N if flags & POOL else 4 * Nb * H * W * N
    ubytes = 4 * P * (cdiv(N, 32) * 32 if blocked else N) * C
    if max(4 * Nb * H * W * C, ubytes, 4 * ybytes if flags & BNP else ybytes) >= 0x7fffffff:
        return -2
    return 0


def decode(t, d):
    """The weight-gradient kernels' tile decode, (int)((t + 0.5f) * (1.0f / d)), in numpy float32."""
    import numpy as np
    inv = np.float32(1.0) / np.float32(d)
    return ((t.astype(np.float32) + np.float32(0.5)) * inv).astype(np.int64)
