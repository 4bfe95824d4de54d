"""fp64 CPU references, input sets, derived tolerances and expected statuses for the pre-split X6 GEMM
(csrc/kernels/x6p.hip: rk_x6p_gemm, rk_x6p_split, rk_x6p_split_t) and the pre-transformed half of
csrc/kernels/winograd4.hip (rk_wino4_pt_input, rk_wino4_pt_transform, rk_wino4_pt_output, rk_wino4_pt_conv_out,
rk_x6p_w4_input, rk_x6p_w4_wgrad_transform, rk_x6p_w4_weights).  Imports nothing from rafiki_amd; the matrices, the
windows, normalise-on-load, the weight transform, the judge and the draws come from wino_refs, the bf16 pieces, the
six-term product, the epilogues, the decision draws and the yardstick gate from sgemm_refs, unchanged.

One function per stage, in the layouts the kernels use.  Position q = a * 6 + b, tiles in (n, ty, tx) order,
T = Nb * H/4 * W/4:
  v_of        V = B^T d B of every 6x6 window (zero outside the image, normalise-on-load inside)   [36][T][C]
  m_of        M = A dY A^T of every 4x4 patch                                                      [36][T][Co]
  planes      (hi, mid, lo) of sgemm_refs.split3 stacked in front of the last two dimensions       [...][3][rows][cols]
  planes_t    the K-inner transposes of the weight-gradient operands                               [36][3][C][T]
  gemm_planes rk_x6p_gemm read from flat plane buffers through lda / ldb, plane and group strides (a group stride
              of 0 broadcasts), one result per split-K slab and group: the six kept terms, and S = sum |a| |b|.
              Slab s covers the K-tiles [s ktPer, (s + 1) ktPer), ktPer = ceil((K / kt) / splits), kt 32 or 64.
              ``c_index`` places the results in C (ldc, group-major or row-interleaved [M][G][N], slab stride).
  conv_out    A^T (sum of slabs Y') A per tile, read position-major [36][T][N] or tile-major [T][36][N] at any slab
              stride, then sgemm_refs.epilogue (bias, statistics before the activation, ReLU, leaky ReLU, BNB, BNP)
  wgrad_out   dW = G^T (sum of slabs dU) G (+ prior)                                                [Co][9][Ci]
Every function takes ``absval`` (the same algorithm on absolute values: S, the scale of the error model) and
``mutant`` (the wrong kernels of tests/test_pt_refs.py).

Hard tolerance of a RANDOM result: n * 2^-23 * S per element, wino_refs' rule, n counted from the kernels' code
(each transform once per axis; FMA contraction only removes roundings; the split into three bf16 planes holds 26
bits and is exact):
  bt6  3 per axis (6)     a6  2 per axis (4)     at6  3 per axis (6)     gt6  5 per axis (10)     g6  4 per axis (8)
  each further slab added, a bias, an accumulation onto a prior, the leaky-ReLU product   + 1 each
  normalise-on-load (the fma, counted as product and sum)                                 + 2
  the plane GEMM   sgemm_refs.n_x6(K) = ceil(6.05 K) + 1 (six MFMA terms per k, the three dropped products)
  end to end       the stage counts summed: conv 6 + n_x6(C) + 6 (+ slabs - 1, + 1 bias, + 2 normalise-on-load);
                   weight gradient 4 + 6 + n_x6(T) + 10 (+ slabs - 1, + 1 accumulating); on fp32 operands the GEMM
                   term is K (one fp32 product sum per k; the X6 loop of sgemm n_x6(K)).
These counts are derived, not measured.

Statistics of rk_wino4_pt_conv_out.  A thread sums the 16 elements of its tile (v, v * v; BNB / BNP dz, dz * y) in
fp32, the block adds its TPB <= 4 tile lanes through LDS in fp32, one fp64 atomic per block and channel follows.
Against the fp64 reference the bound is igemm_refs.stats_ref's / bn_sums' (sgemm_refs.epilogue).  Against the output
the same launch wrote (``own_sums``) only that arithmetic counts: 16 + 4 additions and, for the second sum, one
product:  |sum - sum(out)| <= 20 * 2^-23 sum |v|,  |sumsq - sum(out^2)| <= 21 * 2^-23 sum v^2.  On the exact sets a
sum is equal wherever its fp32 partial sums (64 terms at most) stay below 2^24 (``sums_exact``).

Input sets
  exact   integer x, dy in [-2, 2], Y' and dU integer; U in {-1, 0, 1} sparse (wino_refs.draw_u); every transform
          intermediate, plane, partial sum and output is an integer below 2^24 (asserted through S): bit for bit.
  wide    the exact set with odd 18-bit integers (sgemm_refs.wide18's magnitudes) at one element per window and
          axis residue (x: row % 4 == c % 4, column % 4 == (c / 4) % 4; dy: patch position (c % 3, (c / 3) % 3)), so
          a transformed value is at most 25 (16) wide elements' worth, below 2^24, and has 18 or more significant
          bits: hi, mid and lo of the producers are all live (``pieces_used``).  The GEMM uses sgemm_refs' wide_a /
          wide_b / wide_mm unchanged.
  random  full-mantissa normals, weights / sqrt(9 C).
"""
import torch

import sgemm_refs as G
import wino_refs as R
from igemm_refs import F64, LIM, U32, cdiv, f32r, ints  # noqa: F401
from sgemm_refs import X6_TERMS, YARD, n_x6, pieces_used, rms_ratio, split3, x6_gemm  # noqa: F401
from wino_refs import (BIAS, BNB, BNP, FLAG_SETS, LRELU, POOL, RELU, STATS, exact_ok, judge, mats, normalise,  # noqa: F401
                       transform_weights, windows, yard_ratio)

F32 = torch.float32
OK, EBADARG, EUNSUPPORTED = 0, -1, -2
N_BT6, N_A6, N_AT6, N_GT6, N_G6, N_PRO = 6, 4, 6, 10, 8, 2
LDS_MAX = 163840
# rk_x6p_gemm's tiles: (BM, BN, warp-specialised)
TILES = ((128, 128, 0), (128, 64, 0), (64, 128, 0), (64, 64, 0), (64, 64, 0), (128, 64, 0), (64, 128, 0),
         (256, 128, 0), (128, 256, 0), (128, 128, 1), (128, 64, 1), (64, 128, 1), (64, 64, 1))
# (Nb, H, W) of every transform stage: non-square, images straddling a 32-tile and a 4-tile block
SPATIAL = [(3, 4, 12), (16, 4, 8), (2, 8, 16), (5, 8, 4)]
CHANNELS = (4, 8, 12, 40)


def tiles(Nb, H, W):
    return Nb * (H // 4) * (W // 4)


# ------------------------------------------------------------------------------------- transforms
def v_of(x, pro=None, absval=False, mutant=None):
    """V [36][T][C] of x [Nb][H][W][C]."""
    Nb, H, W, C = x.shape
    if mutant == 'hw_swap':              # the tile decode with H and W exchanged: the same memory as [Nb][W][H][C]
        x, H, W = x.reshape(Nb, W, H, C), W, H
    BT = mats(4, absval, x.dtype)[0]
    d = windows(x, 4, pro, absval, 'pad_relu_shift' if mutant == 'pad_relu_shift' else None)
    V = torch.einsum('ia,ntxabc,jb->ijntxc', BT, d, BT)
    if mutant == 'q_swap':
        V = V.transpose(0, 1)
    if mutant == 'tile_order':
        V = V.transpose(3, 4)
    return V.reshape(36, -1, C).contiguous()


def m_of(dy, absval=False, mutant=None):
    """M [36][T][Co] of dy [Nb][H][W][Co]."""
    Nb, H, W, Co = dy.shape
    if mutant == 'hw_swap':
        dy, H, W = dy.reshape(Nb, W, H, Co), W, H
    AT = mats(4, absval, dy.dtype)[1]
    p = (dy.abs() if absval else dy).reshape(Nb, H // 4, 4, W // 4, 4, Co)
    M = torch.einsum('pi,nypxqk,qj->ijnyxk', AT, p, AT)
    if mutant == 'q_swap':
        M = M.transpose(0, 1)
    if mutant == 'tile_order':
        M = M.transpose(3, 4)
    return M.reshape(36, -1, Co).contiguous()


def planes(t, mutant=None):
    """[...][3][rows][cols] of t [...][rows][cols]."""
    h, m, l = split3(t)
    return torch.stack((h, l, m) if mutant == 'plane_order' else (h, m, l), -3)


def planes_t(t, mutant=None):
    """[36][3][C][T] of t [36][T][C]."""
    return planes(t.transpose(-1, -2).contiguous(), mutant)


def unplanes(p):
    return p.sum(-3)


def tol_of(n, S):
    return n * U32 * S


# ------------------------------------------------------------------------------------- plane GEMM
def gemm_layout(M, N, K, groups=1, *, lda=None, ldb=None, ldc=None, bcast_a=False, bcast_b=False, interleave=False,
                splits=1, guard=2):
    """Every stride of one rk_x6p_gemm launch and the sizes of its three buffers (elements).  Group-major outputs
    are ``guard`` rows apart, row-interleaved ones ([M][G][N]) 4 columns, split-K slabs 2 ldc further apart."""
    lda, ldb = lda or K, ldb or K
    L = dict(M=M, N=N, K=K, groups=groups, lda=lda, ldb=ldb, psA=M * lda, psB=N * ldb, splits=splits)
    L['gsA'], L['gsB'] = (0 if bcast_a else 3 * L['psA']), (0 if bcast_b else 3 * L['psB'])
    L['sizeA'] = L['gsA'] * (groups - 1) + 3 * L['psA']
    L['sizeB'] = L['gsB'] * (groups - 1) + 3 * L['psB']
    if interleave:
        L['gsC'] = N + 4
        L['ldc'] = max(ldc or 0, groups * L['gsC'])
        one = M * L['ldc']
    else:
        L['ldc'] = ldc or N
        L['gsC'] = (M + guard) * L['ldc']
        one = groups * L['gsC']
    L['slabStride'] = one + 2 * L['ldc'] if splits > 1 else 0
    L['sizeC'] = (splits - 1) * L['slabStride'] + one + (guard * L['ldc'] if interleave else 0)
    L['bytesA'], L['bytesB'] = 2 * L['sizeA'], 2 * L['sizeB']
    return L


def pack_planes(t, ld, fill=float('nan')):
    """Flat plane buffer [G][3][rows][ld] of t [G][rows][K] (the columns past K hold ``fill``)."""
    Gn, rows, K = t.shape
    buf = torch.full((Gn, 3, rows, ld), fill, dtype=F64)
    buf[..., :K] = planes(t)
    return buf.reshape(-1)


def _take(flat, rows, K, ld, ps, gs, groups):
    return torch.as_strided(flat, (groups, 3, rows, K), (gs, ps, ld, 1))


def slab_ranges(K, kt, splits):
    """[(k0, k1)] of every slab, or None where the launcher refuses the split count (a split without a K-tile)."""
    nk = K // kt
    per = cdiv(nk, splits)
    if cdiv(nk, per) != splits:
        return None
    return [(s * per * kt, min(K, (s + 1) * per * kt)) for s in range(splits)]


def gemm_planes(A, B, L, kt=32, *, drop=None, absval=False, mutant=None):
    """acc [splits][groups][M][N] (and S) of flat plane buffers A, B under layout L (``gemm_layout``).
    drop: one of X6_TERMS left out."""
    M, N, K, Gn = L['M'], L['N'], L['K'], L['groups']
    pa = _take(A, M, K, L['lda'], L['psA'], L['gsA'], Gn)
    pb = _take(B, N, K, L['ldb'], L['psB'], L['gsB'], Gn)
    if mutant == 'stale_stage' and K // kt >= 2:     # the last K-tile read from the stage the one before it left
        pa = pa.clone()
        pa[..., K - kt:] = pa[..., K - 2 * kt:K - kt]
    rng = slab_ranges(K, kt, L['splits'])
    acc = torch.zeros(len(rng), Gn, M, N, dtype=F64)
    S = torch.zeros_like(acc)
    ix = dict(h=0, m=1, l=2)
    for s, (k0, k1) in enumerate(rng):
        a, b = pa[..., k0:k1], pb[..., k0:k1]
        for t in X6_TERMS:
            if t != drop:
                acc[s] += a[:, ix[t[0]]] @ b[:, ix[t[1]]].transpose(-1, -2)
        S[s] = a.abs().sum(1) @ b.abs().sum(1).transpose(-1, -2)
    return (S if absval else acc), S


def c_index(L):
    """Flat offsets [splits][groups][M][N] of the output elements in C."""
    s, g, m, n = torch.meshgrid(*(torch.arange(v) for v in (L['splits'], L['groups'], L['M'], L['N'])), indexing='ij')
    return s * L['slabStride'] + g * L['gsC'] + m * L['ldc'] + n


def place_c(vals, L, prior=None, mutant=None):
    """The flat C a launch must leave: ``vals`` [splits][groups][M][N] at ``c_index``, everything else NaN (the
    prior's values where it accumulates)."""
    buf = torch.full((L['sizeC'],), float('nan'), dtype=F64)
    idx = c_index(L)
    if mutant == 'row_spill':            # row M of a group (zeros: the rows past M are read as zeros) written too
        buf[(idx[:, :, -1] + L['ldc']).reshape(-1)] = 0.0
    buf[idx.reshape(-1)] = (vals if prior is None or mutant == 'no_accumulate' else vals + prior).reshape(-1)
    return buf


def guards_ok(flat, idx):
    """Everything outside ``idx`` is still NaN."""
    keep = torch.ones(flat.numel(), dtype=torch.bool)
    keep[idx.reshape(-1)] = False
    return bool(torch.isnan(flat[keep]).all())


def judge_mat(tag, got, ref, tol, mode, yard=None, what=''):
    """wino_refs.judge element by element; the yardstick per output row and per output column
    (sgemm_refs.rms_ratio)."""
    judge(tag, got, ref, tol, mode, None, what)
    if mode == 'random' and yard is not None:
        r = rms_ratio(got.to('cpu', F64), ref, yard)
        R.YWORST[tag] = max(R.YWORST.get(tag, 0.0), r)
        assert r <= YARD, '{} {}: rms error {:.2f}x the fp32 yardstick (gate {})'.format(tag, what, r, YARD)


def judge_planes(tag, got, ref, tol, mode, what=''):
    """got [...][3][rows][cols] (fp64 of the bf16 planes) of the value ref.  Exact sets: the planes are split3 of
    the reference.  RANDOM: the planes are the canonical split of their own sum, and the sum is within tol."""
    got = got.to('cpu', F64)
    nan = torch.isnan(got)
    assert not bool(nan.any()), '{} {}: {} NaN planes; first at {}'.format(
        tag, what, int(nan.sum()), tuple(int(v) for v in nan.nonzero()[0]))
    v = unplanes(got)
    want = planes(ref if mode != 'random' else v)
    bad = got != want
    if bool(bad.any()):
        i = tuple(int(t) for t in bad.nonzero()[0])
        raise AssertionError('{} {} [{}]: {} plane elements are not the split of {}; first at {}: got {!r} want {!r}'
                             .format(tag, what, mode, int(bad.sum()), 'the reference' if mode != 'random' else 'their sum',
                                     i, float(got[i]), float(want[i])))
    judge(tag, v, ref, tol, mode, None, what)


# --------------------------------------------------------------------------------- output transforms
def _slabs(flat, shape, strides, nslab, slab, mutant, dense):
    k = nslab - 1 if mutant == 'last_slab_dropped' and nslab > 1 else nslab
    step = dense if mutant == 'slab_stride' else slab
    return torch.as_strided(flat, (k,) + shape, (step,) + strides).sum(0)


def conv_out(yt, Nb, H, W, N, flags=0, *, bias=None, gate=None, nslab=1, slab=0, tmajor=0, slope=0.0, n_in=0,
             S_in=None, mutant=None, exact=False):
    """rk_wino4_pt_conv_out of the flat Y' buffer: dict(out [Nb][H][W][N], tol, acc, S[, sums, sums_tol]).
    bias: [N], or (scale, shift) with BNB / BNP; gate: y [T * 16][N] (BNB) or y2 [Nb][2H][2W][N] (BNP).
    n_in / S_in: the roundings the values of Y' already carry and their absolute-value companion (a flat buffer
    like yt; default |yt|)."""
    T = tiles(Nb, H, W)
    if mutant == 'tmajor':
        tmajor = 1 - tmajor
    strides = (N, 36 * N, 1) if tmajor else (T * N, N, 1)
    AT, ATa = mats(4, False)[1], mats(4, True)[1]
    Sf = torch.nan_to_num(yt.abs() if S_in is None else S_in)
    res = []
    for flat, A_, mu in ((torch.nan_to_num(yt) if mutant else yt, AT, mutant), (Sf, ATa, None)):
        y = _slabs(flat, (36, T, N), strides, nslab, slab, mu, 36 * T * N).reshape(6, 6, Nb, H // 4, W // 4, N)
        if mu == 'q_swap':
            y = y.transpose(0, 1)
        if mu == 'tile_order':
            y = y.reshape(6, 6, Nb, W // 4, H // 4, N).transpose(3, 4)
        o = torch.einsum('pi,ijnyxk,qj->nypxqk', A_, y, A_).reshape(Nb, H, W, N)
        res.append(o)
    acc, S = res
    kw = dict(exact=exact)
    if flags & BIAS:
        kw['bias'] = bias
    if flags & RELU:
        kw['act'] = G.ACT_RELU
    if flags & LRELU:
        kw['act'], kw['slope'] = G.ACT_LRELU, slope
    if flags & STATS:
        kw['stats'] = True
        if mutant == 'stats_after_act':
            kw['mutant'] = mutant
    if flags & BNB:
        kw['bnb'] = (gate, bias[0], bias[1])
    if flags & BNP:
        kw['bnp'] = (gate, bias[0], bias[1], Nb, H, W)
        if mutant in ('bnp_last_max', 'bnp_route_on_y'):
            kw['mutant'] = mutant
    r = G.epilogue(acc.reshape(-1, N), S.reshape(-1, N), n_in + N_AT6 + nslab - 1, **kw)
    r['out'], r['tol'] = r['out'].reshape(Nb, H, W, N), r['tol'].reshape(Nb, H, W, N)
    r['acc'], r['S'] = acc, S
    return r


def wgrad_out(du, Co, Ci, *, nslab=1, slab=0, accumulate=False, prior=None, absval=False, mutant=None):
    """dW [Co][9][Ci] of the flat dU buffer (nslab slabs of [36][Co][Ci], ``slab`` floats apart)."""
    Gm = mats(4, absval)[2]
    flat = du.abs() if absval else du
    if mutant or absval:
        flat = torch.nan_to_num(flat)
    u = _slabs(flat, (36, Co, Ci), (Co * Ci, Ci, 1), nslab, slab, mutant, 36 * Co * Ci).reshape(6, 6, Co, Ci)
    if mutant == 'q_swap':
        u = u.transpose(0, 1)
    dw = torch.einsum('iy,ijkc,jx->kyxc', Gm, u, Gm).reshape(Co, 9, Ci)
    if accumulate and mutant != 'no_accumulate':
        dw = dw + (prior.abs() if absval else prior)
    return dw


def n_wgrad_out(nslab=1, accumulate=False, n_in=0):
    return n_in + N_GT6 + nslab - 1 + int(accumulate)


def n_conv_e2e(C, planes_=True, slabs=1, bias=False, pro=False, x6=True):
    return N_BT6 + (n_x6(C) if planes_ or x6 else C) + N_AT6 + slabs - 1 + int(bias) + N_PRO * int(pro)


def n_wgrad_e2e(T, planes_=True, slabs=1, accumulate=False, pro=False, x6=True):
    return N_A6 + N_BT6 + (n_x6(T) if planes_ or x6 else T) + N_GT6 + slabs - 1 + int(accumulate) + N_PRO * int(pro)


# ------------------------------------------------------------------------------------- statistics
N_OWN = 16 + 4


def own_sums(out, second=None):
    """(sum out, sum out * second) per channel of the output a launch wrote and what rk_wino4_pt_conv_out's own
    reduction may lose (16 elements per thread, 4 lanes through LDS, in fp32)."""
    o = out.reshape(-1, out.shape[-1])
    s2 = o if second is None else second.reshape(o.shape)
    return (torch.stack([o.sum(0), (o * s2).sum(0)]),
            torch.stack([N_OWN * U32 * o.abs().sum(0), (N_OWN + 1) * U32 * (o * s2).abs().sum(0)]))


def sums_exact(v, second=None, unit=1.0):
    """Whether the fp32 partial sums (64 terms: 16 per thread, 4 lanes) of v and of v * second are exact."""
    a = float(v.abs().max())
    b = float((v * (v if second is None else second)).abs().max()) / unit
    return 64 * a < LIM, 64 * b < LIM


def judge_sums(tag, got, ref, tol, mode, v, what='', second=None, unit=1.0):
    for i, ok in enumerate(sums_exact(v, second, unit)):
        judge(tag, got[i], ref[i], tol[i], mode if ok else 'random', what='{} sum {}'.format(what, i))


# ------------------------------------------------------------------------------------------- inputs
def _wide_mag(seed, shape):
    g = torch.Generator().manual_seed(seed)
    mag = 2 * torch.randint(2 ** 16, 2 ** 17, tuple(shape), generator=g) + 1
    return (mag * (2 * torch.randint(0, 2, tuple(shape), generator=g) - 1)).to(F64)


def draw_x(mode, seed, shape):
    """x [Nb][H][W][C]; 'wide': an odd 18-bit integer at (row % 4, column % 4) == (c % 4, (c / 4) % 4)."""
    if mode != 'wide':
        return R.draw_x(mode, seed, shape)
    Nb, H, W, C = shape
    x = ints(seed, shape, -2, 2)
    h, w, c = torch.meshgrid(torch.arange(H), torch.arange(W), torch.arange(C), indexing='ij')
    at = (h % 4 == c % 4) & (w % 4 == (c // 4) % 4)
    return torch.where(at, _wide_mag(seed + 1, shape), x)


def draw_dy(mode, seed, shape):
    """dy [Nb][H][W][Co]; 'wide': an odd 18-bit integer at patch position (c % 3, (c / 3) % 3) (A's coefficients
    there are at most 4 per axis)."""
    if mode != 'wide':
        return R.draw_x(mode, seed, shape)
    Nb, H, W, C = shape
    dy = ints(seed, shape, -2, 2)
    h, w, c = torch.meshgrid(torch.arange(H), torch.arange(W), torch.arange(C), indexing='ij')
    at = (h % 4 == c % 3) & (w % 4 == (c // 3) % 3)
    return torch.where(at, _wide_mag(seed + 1, shape), dy)


def draw_mat(mode, seed, shape, scale=1.0):
    """A plain matrix for the splitters: integers, 18-bit odd integers (every element), or normals."""
    if mode == 'exact':
        return ints(seed, shape, -200, 200)
    if mode == 'wide':
        return _wide_mag(seed, shape)
    return G.normal_f32(seed, shape, scale)


def draw_yt(mode, seed, n):
    """n values of a synthetic Y' (or dU): integers in [-2, 2], or normals."""
    return ints(seed, (n,), -2, 2) if mode != 'random' else G.normal_f32(seed, (n,))


def with_slabs(vals, nslab, slab, seed, mode):
    """A flat buffer of nslab slabs ``slab`` apart with NaN between them: the first slab is ``vals``, every further
    one its own draw of the same size (mode 'zero': zeros)."""
    n = vals.numel()
    buf = torch.full(((nslab - 1) * slab + n,), float('nan'), dtype=F64)
    buf[:n] = vals.reshape(-1)
    for k in range(1, nslab):
        buf[k * slab:k * slab + n] = 0.0 if mode == 'zero' else draw_yt(mode, seed + k, n)
    return buf


# --------------------------------------------------------------------------------- expected statuses
def _spatial_bad(Nb, H, W):
    return Nb <= 0 or H <= 0 or W <= 0 or H % 4 != 0 or W % 4 != 0


def expected_status(entry, **a):
    """What the launcher must answer, transcribed from its argument checks in their order: 0, RK_EBADARG (-1) or
    RK_EUNSUPPORTED (-2)."""
    g = a.get
    lim = 1 << 31
    if entry == 'rk_x6p_gemm':
        tile, nst, M, N, K, groups, splits = a['tile'], g('nst', 2), a['M'], a['N'], a['K'], g('groups', 1), g('splits', 1)
        lda, ldb, ldc = g('lda', K), g('ldb', K), g('ldc', N)
        psA, psB = g('psA', M * lda), g('psB', N * ldb)
        gsA, gsB, gsC = g('gsA', 3 * psA), g('gsB', 3 * psB), g('gsC', M * ldc)
        flags, slab = g('flags', 0), g('slabStride', 0)
        bytesA, bytesB = g('bytesA', 2 * (gsA * (groups - 1) + 3 * psA)), g('bytesB', 2 * (gsB * (groups - 1) + 3 * psB))
        if M <= 0 or N <= 0 or K <= 0 or groups <= 0 or nst not in (2, 3) or tile < 0 or (tile & 15) > 12 \
                or tile >= 32 or splits <= 0:
            return EBADARG
        if splits > 1 and (flags & 1 or slab < groups * gsC or slab < M * ldc):
            return EBADARG
        kt = 64 if tile >> 4 else 32
        tile &= 15
        if K % kt or lda % 8 or ldb % 8 or lda < K or ldb < K:
            return EUNSUPPORTED
        if psA < M * lda or psB < N * ldb or bytesA <= 0 or bytesB <= 0:
            return EBADARG
        if M * ldc * 4 >= lim or ldc < N:
            return EUNSUPPORTED
        if (2 * psA + M * lda) * 2 >= lim or (2 * psB + N * ldb) * 2 >= lim:
            return EUNSUPPORTED
        if groups > 1 and ((gsA and gsA < 3 * psA) or (gsB and gsB < 3 * psB)
                           or (gsC < M * ldc and (gsC < N or ldc < groups * gsC))):
            return EBADARG
        if 2 * (gsA * (groups - 1) + 3 * psA) > bytesA or 2 * (gsB * (groups - 1) + 3 * psB) > bytesB:
            return EBADARG
        if slab_ranges(K, kt, splits) is None:
            return EBADARG
        BM, BN, _ = TILES[tile]
        if cdiv(M, BM) * cdiv(N, BN) * groups * splits >= lim:
            return EUNSUPPORTED
        return OK if nst * 3 * (BM + BN) * 2 * kt <= LDS_MAX else EUNSUPPORTED
    if entry == 'rk_x6p_split':
        rows, cols = a['rows'], a['cols']
        lds, ldd = g('lds', cols), g('ldd', cols)
        return EBADARG if rows <= 0 or cols <= 0 or lds < cols or ldd < cols or g('ps', rows * ldd) < rows * ldd else OK
    if entry == 'rk_x6p_split_t':
        rows, cols = a['rows'], a['cols']
        lds, ldd = g('lds', cols), a['ldd']
        ps = g('ps', cols * ldd)
        return EBADARG if rows <= 0 or cols <= 0 or lds < cols or ldd < rows or ldd & 3 or ps & 3 or ps < cols * ldd else OK
    if entry == 'rk_x6p_w4_weights':
        Co, Ci = a['Co'], a['Ci']
        if Co <= 0 or Ci <= 0 or not (g('u', True) or g('ut', True)):
            return EBADARG
        return EUNSUPPORTED if 108 * Co * Ci >= lim else OK
    if entry in ('rk_wino4_pt_input', 'rk_x6p_w4_input'):
        Nb, H, W, C = a['Nb'], a['H'], a['W'], a['C']
        if _spatial_bad(Nb, H, W) or C <= 0:
            return EBADARG
        if C & 3:
            return EUNSUPPORTED
        T = tiles(Nb, H, W)
        if entry == 'rk_wino4_pt_input':
            return EUNSUPPORTED if 36 * T * C >= lim else OK
        return EUNSUPPORTED if 108 * T * C >= lim or Nb * H * W * C >= lim else OK
    if entry in ('rk_wino4_pt_transform', 'rk_x6p_w4_wgrad_transform'):
        Nb, H, W, Co, Ci = a['Nb'], a['H'], a['W'], a['Co'], a['Ci']
        if _spatial_bad(Nb, H, W) or Co <= 0 or Ci <= 0:
            return EBADARG
        if Co & 3 or Ci & 3:
            return EUNSUPPORTED
        T, f = tiles(Nb, H, W), 36 if entry == 'rk_wino4_pt_transform' else 108
        if f * T * Co >= lim or f * T * Ci >= lim:
            return EUNSUPPORTED
        if f == 108 and Nb * H * W * max(Co, Ci) >= lim:
            return EUNSUPPORTED
        return OK
    if entry == 'rk_wino4_pt_output':
        Co, Ci, nslab = a['Co'], a['Ci'], g('nslab', 1)
        if Co <= 0 or Ci <= 0 or nslab <= 0 or (nslab > 1 and g('slab', 0) < 36 * Co * Ci):
            return EBADARG
        return EUNSUPPORTED if Ci & 3 or 36 * Co * Ci >= lim else OK
    if entry == 'rk_wino4_pt_conv_out':
        Nb, H, W, N, flags, nslab = a['Nb'], a['H'], a['W'], a['N'], g('flags', 0), g('nslab', 1)
        if _spatial_bad(Nb, H, W) or N <= 0 or nslab <= 0:
            return EBADARG
        if flags & LRELU and flags & (RELU | STATS | BNB | BNP):
            return EBADARG
        if flags & (STATS | BNB | BNP) and not g('stats', False):
            return EBADARG
        if flags & (BNB | BNP) and not (g('gate', False) and g('bias', False)):
            return EBADARG
        if flags & BIAS and not g('bias', False):
            return EBADARG
        T = tiles(Nb, H, W)
        if T * N >= lim:
            return EUNSUPPORTED
        if nslab > 1 and g('slab', 0) < 36 * T * N:
            return EBADARG
        return OK
    raise ValueError(entry)


def wgrad_form(Nb, H, W, Co, Ci):
    """Which kernels rk_x6p_w4_wgrad_transform takes: the LDS-staged w4pt_planesT_kernel or the fallback pair."""
    return 'staged' if tiles(Nb, H, W) % 32 == 0 and Co % 8 == 0 and Ci % 8 == 0 else 'fallback'


def conv_out_form(N, vw=2):
    """Which kernel rk_wino4_pt_conv_out takes under RAFIKI_PT_OUT_VW = vw."""
    return 'vector{}'.format(vw) if N % vw == 0 else 'scalar'


# ------------------------------------------------------------------------------------ GEMM sweep
def gemm_shapes(tile):
    """(M, N) of the sweep for one tile: one row, one under / over the tile, more than one block each way."""
    BM, BN, _ = TILES[tile & 15]
    big = (257, 130) if BM == 256 else (130, 257) if BN == 256 else (BM + 33, 2 * BN - 7)
    return [(1, 8), (BM - 1, BN + 1), big]


K_TILES = (1, 2, 3, 5)


def gemm_problem(mode, M, N, K, groups=3):
    """(a [groups][M][K], b [groups][N][K]) fp32-representable operands."""
    a, b = G.draw_pair(mode, 11 * M + 7 * N + K, (groups, M, K), (groups, N, K), K)
    return a, b
