"""Every bf16 implicit-GEMM candidate of csrc/kernels/igemm.hip, and the combine kernels it feeds, against the
fp64 references of tests/igemm_refs.py (anchored and shown to bite in tests/test_igemm_refs.py).

Each item runs on both input sets of igemm_refs: EXACT (integer operands: the output must EQUAL the reference,
bf16 outputs its round-to-nearest-even) and RANDOM (bf16 normals: element-by-element and channel-by-channel
tolerances from the error model, n * 2^-23 * S and one bf16 rounding).  Every output is prefilled with NaN, sits
in a buffer with a canary-filled pad (ldc = N + 8, 8 rows below) that must come back untouched, and dense operands
have NaN-filled pads (lda, ldb wider than the row).  A launcher refusal is predicted by ``expected_status`` and
asserted with its status, never skipped.  No element is excluded from a comparison.  Every figure is kept; the
worst error / tolerance per entry point on RANDOM is printed at the end (pytest -s).
"""
import re
import types

import pytest
import torch

import igemm_refs as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
NAN = float('nan')
CANARY = 77.0
MODES = ('exact', 'random')
RELU, BIAS, STATS, GATE, ACCUM, LRELU, SATOM, BNB, BNP = 1, 2, 4, 8, 16, 32, 256, 512, 1024
KS = 4
BM_OF = (128, 128, 64, 64, 64)
# tile shapes 0-3 x every staging form, the wave-K-split tile x its two rings, and codes the launcher refuses
STAGINGS = (0, 16, 64, 32, 128)
ALL_TILES = [t | v for t in range(4) for v in STAGINGS] + [KS | 64, KS | 32, KS, KS | 16, KS | 128, 5]
VALID_TILES = ALL_TILES[:22]
EPI_TILES = [3, 0 | 16, 2 | 64, 1 | 32, 3 | 128, KS | 64, KS | 32]
WORST = {}
COUNT = {'ran': 0, 'refused': 0}


@pytest.fixture(scope='module')
def F():
    from rafiki_amd.ops import _lib, functional
    _lib.lib()  # loud failure if the native library is missing
    yield functional
    for entry in sorted(WORST):
        print('WORST {:28s} err / tol {:.3f}'.format(entry, WORST[entry]))
    print('launches checked {ran}, refusals asserted {refused}'.format(**COUNT))


@pytest.fixture(autouse=True)
def _stop_after_a_fault():
    """A kernel fault is sticky: end the session at the first one instead of launching on a faulted device."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:
        pytest.exit('GPU fault: {}'.format(exc), returncode=3)


# ------------------------------------------------------------------------------------------ helpers
def _status(fn):
    """0 if the launch went through, else the status the launcher refused it with."""
    from rafiki_amd.ops._lib import KernelError
    try:
        fn()
    except KernelError as e:
        return int(re.search(r'status (-?\d+)', str(e)).group(1))
    return 0


def _dev(t, dtype=BF16, ld=None):
    """Device copy of a 2-D (or NHWC) fp64 tensor; ld: row stride in elements, the pad filled with NaN."""
    if ld is None:
        return t.to(DEV, dtype).contiguous()
    buf = torch.full((t.shape[0], ld), NAN, dtype=dtype, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV, dtype)
    return buf


def _out_buf(rows, N, ldc, dtype, slabs=1, prior=None):
    buf = torch.full((slabs, rows + 8, ldc), CANARY, dtype=dtype, device=DEV)
    buf[:, :rows, :N] = NAN if prior is None else prior.to(DEV, dtype)
    return buf


def _read_out(buf, rows, N):
    host = buf.to('cpu', F64)
    assert bool((host[:, rows:, :] == CANARY).all()) and bool((host[:, :rows, N:] == CANARY).all()), \
        'wrote outside out[M][N]'
    body = host[:, :rows, :N]
    assert not bool(torch.isnan(body).any()), 'left {} elements unwritten'.format(int(torch.isnan(body).sum()))
    return body


def _check(entry, got, ref, tol, mode, what=''):
    """EXACT: got == ref everywhere.  RANDOM: |got - ref| <= tol element by element (tol 0 means equal)."""
    got = got.to('cpu', F64) if got.is_cuda or got.dtype != F64 else got
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert not bool(torch.isnan(got).any()), '{} {}: NaN in the output'.format(entry, what)
    err = (got - ref).abs()
    if mode == 'exact':
        bad = err != 0
    else:
        bad = err > tol
        ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), (err > 0).to(F64) * 1e30)
        WORST[entry] = max(WORST.get(entry, 0.0), float(ratio.max()) if ratio.numel() else 0.0)
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError('{} {} [{}]: {} of {} elements off; first at {}: got {!r} ref {!r} tol {!r}'.format(
            entry, what, mode, int(bad.sum()), bad.numel(), i, float(got[i]), float(ref[i]),
            float(tol[i]) if mode != 'exact' else 0.0))


def _pow2(v):
    return v > 0 and not (v & (v - 1))


# -------------------------------------------------------------------------------------------- cases
class Case:
    """One rk_igemm problem: fp64 operands, their GEMM view (A, B in the kernel's K order) and launch geometry."""
    _cache = {}

    @classmethod
    def get(cls, kind, shape, taps, mode):
        key = (kind, tuple(shape), taps, mode)
        if key not in cls._cache:
            cls._cache[key] = cls(kind, shape, taps, mode)
        return cls._cache[key]

    def __init__(self, kind, shape, taps, mode):
        self.kind, self.shape, self.taps, self.mode = kind, shape, taps, mode
        a, b = R.problem(kind, shape, taps, mode)
        self.H = self.W = 1
        self.C, self.Cb = 8, 1
        if kind in (0, 1, 2, 6):
            Nb, H, W, Ci, Co = shape
            self.H, self.W = (2 * H, 2 * W) if kind == 6 else (H, W)
            pix = Nb * self.H * self.W
            if kind in (0, 6):
                self.M, self.N, self.K, self.C, self.lda, self.ldb = pix, Co, taps * Ci, Ci, Ci, taps * Ci
            elif kind == 1:
                self.M, self.N, self.K, self.C, self.Cb = pix, Ci, taps * Co, Co, Co
                self.lda, self.ldb = Co, taps * Ci
            else:
                self.M, self.N, self.K, self.C, self.lda, self.ldb = Co, taps * Ci, pix, Ci, Co, 0
            self.a_dev, self.b_dev = _dev(a), _dev(b.reshape(b.shape[0], -1) if kind != 2 else b)
        else:
            M, K, N = shape
            if kind == 3:
                self.M, self.N, self.K = M, N, K
            elif kind == 4:
                self.M, self.N, self.K = M, K, N
            else:
                self.M, self.N, self.K = N, K, M
            self.lda, self.ldb = a.shape[1] + 8, b.shape[1] + 16
            self.a_dev, self.b_dev = _dev(a, ld=self.lda), _dev(b, ld=self.ldb)
        self.A, self.B = R.operands(kind, a, b, taps)
        assert self.A.shape == (self.M, self.K) and self.B.shape == (self.N, self.K)
        self.kt = R.cdiv(self.K, R.BK)
        self._g = {}

    def gemm(self, splits=1):
        if splits not in self._g:
            slabs, S = R.gemm(self.A, self.B, splits)
            if self.mode == 'exact':
                assert R.exact_ok(S.sum(0)), 'EXACT precondition: S >= 2^24'
            self._g[splits] = (slabs, S)
        return self._g[splits]

    @property
    def nonpow2(self):
        return self.kind in (0, 1, 2, 6) and not (_pow2(self.C) and _pow2(self.H) and _pow2(self.W))


def expected_status(c, epi, tile, flags=0, splits=1):
    """What rk_igemm must answer: 0, RK_EBADARG (-1) or RK_EUNSUPPORTED (-2).  Conv extents that are no power
    of two fall back silently to the register-staged forms (tile &= 15|16): those launches are still checked."""
    conv = c.kind in (0, 1, 2, 6)
    if c.N % 4 or (c.kind not in (2, 5) and c.K % 8):
        return -2
    if conv and (c.C % 8 or c.C < 8):
        return -2
    if c.nonpow2:
        tile &= 31
    if epi == 0 and splits != 1:
        return -1
    if flags & BNP and (epi != 0 or not (_pow2(c.H) and _pow2(c.W)) or not flags & SATOM):
        return -2
    if c.kind == 1 and not _pow2(c.Cb):
        return -2
    if c.kind in (2, 5) and epi != 1:
        return -1
    if c.kind == 6:
        if epi != 0:
            return -1
        tile &= 31
    if tile & 15 > 4:
        return -1
    if tile & 15 == KS:
        if tile & 128 or not tile & (32 | 64):
            return -2
        if flags & STATS and not flags & SATOM:
            return -2
    return 0


def launch(F, c, epi, tile, *, flags=0, alpha=1.0, slope=0.2, splits=1, bias=None, stats=None, gate=None,
           prior=None, ldc=None):
    """One rk_igemm launch into a canaried buffer.  Returns (status, out [slabs][M][N] fp64 on the host)."""
    ldc = c.N + 8 if ldc is None else ldc
    buf = _out_buf(c.M, c.N, ldc, F32 if epi else BF16, splits, prior)
    st = _status(lambda: F.igemm(c.kind, epi, c.a_dev, c.b_dev, buf, c.M, c.N, c.K, c.lda, c.ldb, ldc, bias=bias,
                                 stats=stats, gate=gate, H=c.H, W=c.W, C=c.C, taps=c.taps, Cb=c.Cb, splits=splits,
                                 slab_stride=(c.M + 8) * ldc, flags=flags, alpha=alpha, slope=slope, tile=tile))
    if st != 0:
        host = buf.to('cpu', F64)
        assert bool(((host == CANARY) | torch.isnan(host)).all()), 'a refused launch wrote something'
        return st, None
    return 0, _read_out(buf, c.M, c.N)


SWEEP, DENSE_SHAPES = R.SWEEP, R.DENSE_SHAPES


# ------------------------------------------------------------------- rk_igemm: every kind x tile x staging
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('kind,shape,taps', SWEEP, ids=lambda v: '-'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_igemm_every_tile_and_staging(F, kind, shape, taps, mode):
    """Kinds 0-6, both epilogues, tile shapes 0-3 x staging {0, 16, 64, 32, 128} and the wave-K-split tile x
    {64, 32}: bf16 plain epilogue, and fp32 slabs (alpha = 0.5, two K splits where there are two K-tiles) judged
    slab by slab.  Every combination is either checked or refused with the predicted status."""
    c = Case.get(kind, shape, taps, mode)
    entry = 'rk_igemm kind {}'.format(kind)
    for tile in ALL_TILES:
        for epi in (0, 1):
            splits = 1 if epi == 0 else min(2, c.kt)
            alpha = 1.0 if epi == 0 else 0.5
            want = expected_status(c, epi, tile, 0, splits)
            st, got = launch(F, c, epi, tile, alpha=alpha, splits=splits)
            assert st == want, 'kind {} epi {} tile {}: status {} (expected {})'.format(kind, epi, tile, st, want)
            if st != 0:
                COUNT['refused'] += 1
                continue
            COUNT['ran'] += 1
            slabs, S = c.gemm(splits)
            rng = R.split_ranges(c.K, splits)
            for s in range(len(rng)):
                v, E = R.fp32_out(slabs[s], S[s], rng[s][1] - rng[s][0], alpha=alpha)
                ref, tol = (v, E) if epi else (R.bf16r(v) if mode == 'exact' else v, R.tol_bf16(v, E))
                _check(entry, got[s], ref, tol, mode, 'epi {} tile {} slab {}'.format(epi, tile, s))


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('kind,shape', [(2, (3, 6, 6, 24, 40)), (2, (5, 2, 2, 64, 64)), (2, (2, 16, 16, 16, 136)),
                                        (5, (37, 64, 16)), (5, (200, 520, 96)), (5, (130, 72, 132))])
def test_igemm_wgrad_splits_and_accumulate(F, kind, shape, mode):
    """Kinds 2 and 5 with K (pixels / rows) no multiple of 8: 1, 2 and 3 splits with uneven K-tile counts, slab
    by slab, and FLAG_ACCUM onto a nonzero buffer."""
    c = Case.get(kind, shape, 9 if kind == 2 else 1, mode)
    # K = 108, 20, 37, 130 are no multiples of 8; (2,16,16,16,136) has 8 K-tiles: 3 + 3 + 2 over three splits
    entry = 'rk_igemm kind {}'.format(kind)
    for tile in (3, 0 | 16, 1 | 64, 2 | 32, 3 | 128, KS | 64, KS | 32):
        for splits in (1, 2, 3):
            s_eff = R.effective_splits(c.K, splits)
            st, got = launch(F, c, 1, tile, splits=s_eff)
            want = expected_status(c, 1, tile, 0, s_eff)
            assert st == want, (tile, splits, st, want)
            if st != 0:
                COUNT['refused'] += 1
                continue
            COUNT['ran'] += 1
            slabs, S = c.gemm(s_eff)
            rng = R.split_ranges(c.K, s_eff)
            for s in range(s_eff):
                v, E = R.fp32_out(slabs[s], S[s], rng[s][1] - rng[s][0])
                _check(entry, got[s], v, E, mode, 'tile {} splits {} slab {}'.format(tile, s_eff, s))
        if expected_status(c, 1, tile) != 0:
            continue
        prior = R.draw(mode, 99, (c.M, c.N)) * 3
        st, got = launch(F, c, 1, tile, flags=ACCUM, alpha=0.5, prior=prior)
        assert st == 0
        slabs, S = c.gemm(1)
        v, E = R.fp32_out(slabs[0], S[0], c.K, alpha=0.5, prior=prior)
        _check(entry, got[0], v, E, mode, 'tile {} FLAG_ACCUM'.format(tile))
        COUNT['ran'] += 1


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', DENSE_SHAPES)
def test_igemm_dense_epilogues(F, shape, mode):
    """Dense forward with alpha != 1, bias (+-300 channels on EXACT: real bf16 roundings, ties included) and
    ReLU / leaky ReLU; fp32 output with alpha and bias; dX with a ReLU gate.  lda, ldb, ldc wider than the row."""
    c = Case.get(3, shape, 1, mode)
    slabs, S = c.gemm(1)
    bias = R.draw_bias(mode, 5, c.N, big=True)
    bias_dev = bias.to(DEV, F32)
    for tile in EPI_TILES:
        for act, fl in ((R.ACT_NONE, BIAS), (R.ACT_RELU, BIAS | RELU), (R.ACT_LRELU, BIAS | LRELU)):
            st, got = launch(F, c, 0, tile, flags=fl, alpha=0.5, slope=0.25, bias=bias_dev)
            assert st == 0
            v, E = R.fp32_out(slabs[0], S[0], c.K, alpha=0.5, bias=bias)
            v, E = R.activate(v, E, act, 0.25)
            _check('rk_igemm kind 3', got[0], R.bf16r(v) if mode == 'exact' else v, R.tol_bf16(v, E), mode,
                   'tile {} flags {}'.format(tile, fl))
            COUNT['ran'] += 1
        st, got = launch(F, c, 1, tile, flags=BIAS, alpha=0.5, bias=bias_dev)
        assert st == 0
        v, E = R.fp32_out(slabs[0], S[0], c.K, alpha=0.5, bias=bias)
        _check('rk_igemm kind 3', got[0], v, E, mode, 'tile {} fp32 bias'.format(tile))
    # dX = dy @ w with the ReLU-backward gate (gate > 0), the gate strided as the output
    d = Case.get(4, shape, 1, mode)
    gate = R.draw_decision(6, (d.M, d.N))
    gate_dev = _dev(gate, ld=d.N + 8)
    for tile in EPI_TILES:
        st, got = launch(F, d, 0, tile, flags=GATE, gate=gate_dev)
        want = expected_status(d, 0, tile, GATE)
        assert st == want
        if st != 0:
            COUNT['refused'] += 1
            continue
        ds, dS = d.gemm(1)
        v, E = R.fp32_out(ds[0], dS[0], d.K)
        m = (gate > 0).to(F64)
        _check('rk_igemm kind 4', got[0], (R.bf16r(v) if mode == 'exact' else v) * m, R.tol_bf16(v, E) * m, mode,
               'tile {} gate'.format(tile))
        COUNT['ran'] += 1
    # linear_dx itself (the tile picked by the heuristic), on views whose row strides are wider than the row
    buf = _out_buf(d.M, d.N, d.N + 8, BF16)
    st = _status(lambda: F.linear_dx(d.a_dev[:, :d.K], d.b_dev[:, :d.N], gate=gate_dev[:, :d.N],
                                     out=buf[0, :d.M, :d.N]))
    assert st == expected_status(d, 0, 0, GATE)
    if st == 0:
        ds, dS = d.gemm(1)
        v, E = R.fp32_out(ds[0], dS[0], d.K)
        m = (gate > 0).to(F64)
        _check('linear_dx', _read_out(buf, d.M, d.N)[0], (R.bf16r(v) if mode == 'exact' else v) * m,
               R.tol_bf16(v, E) * m, mode)


# ---------------------------------------------------------------------- every specialised tile epilogue
def _stats_check(entry, F, c, tile, got_stats, v, E, mode, what):
    """Partial statistics rows [rows][2][N], row set by row set."""
    rows = F.stats_rows(c.M, c.N, tile)
    sets = R.stats_row_sets(c.M, BM_OF[tile & 15])
    assert rows == len(sets) and got_stats.shape[0] == rows
    for r, sl in enumerate(sets):
        ref, tol = R.stats_ref(v, E, sl)
        _check(entry, got_stats[r], ref, tol, mode, '{} stats row {}'.format(what, r))


def _epilogue_sets(c, mode):
    """(name, flags, kwargs) of the nine specialised flag sets and two that fall to the runtime-flag copy."""
    N = c.N
    bias = R.draw_bias(mode, 11, N, big=True)
    sbias = R.ints(12, (N,), -3, 3) if mode == 'exact' else R.draw_bias(mode, 12, N)   # with statistics: integers
    return [('none', 0, {}), ('STATS', STATS, {}), ('STATS|SATOM', STATS | SATOM, {}), ('GATE', GATE, {}),
            ('BIAS', BIAS, {'bias': bias}), ('BIAS|RELU', BIAS | RELU, {'bias': bias}),
            ('BIAS|LRELU', BIAS | LRELU, {'bias': bias}), ('BNB|SATOM', BNB | SATOM, {}),
            ('BNP|SATOM', BNP | SATOM, {}), ('BIAS|RELU|STATS', BIAS | RELU | STATS, {'bias': sbias}),
            ('GATE|BIAS', GATE | BIAS, {'bias': bias})]


def _run_epilogue(F, entry, c, tile, name, flags, bias, mode, launcher):
    """Reference of one flag set of tile_epi and the comparison.  launcher(flags, bias_dev, stats_dev, gate_dev)
    -> (status, out [M][N] fp64); gate tensors are drawn here, strided like the output (ldc = N + 8)."""
    M, N = c.M, c.N
    slabs, S = c.gemm(1)
    alpha = 1.0 if flags & (STATS | BNB | BNP) else 0.5
    Nb = M // (c.H * c.W)
    ldc = N + 8
    scale, shift = R.draw_scale_shift(21, N)
    gate = gate_dev = None
    if flags & (GATE | BNB):
        gate = R.draw_decision(22, (M, N))
        gate_dev = _dev(gate, ld=ldc)
    elif flags & BNP:
        gate = R.draw_pool_y(23, Nb, c.H, c.W, N, scale)
        gate_dev = _dev(gate.reshape(-1, N), ld=ldc)
    if flags & (BNB | BNP):
        assert R.decisions_inexact(gate, scale, shift) == 0     # nothing has to be excluded
        bias_dev = torch.cat([scale, shift]).to(DEV, F32)
    else:
        bias_dev = None if bias is None else bias.to(DEV, F32)
    v, E = R.fp32_out(slabs[0], S[0], c.K, alpha=alpha, bias=bias if flags & BIAS else None)
    if mode == 'exact' and flags & STATS:
        assert R.exact_ok(S[0], v)
    masks = (0, F.bn_slots(N) - 1) if flags & SATOM else (0,)
    for slmask in masks:
        stats_dev = None
        if flags & SATOM:
            stats_dev = torch.zeros((slmask + 1, 2, N), dtype=F64, device=DEV)
        elif flags & STATS:
            stats_dev = torch.full((F.stats_rows(M, N, tile), 2, N), NAN, dtype=F32, device=DEV)
        st, got = launcher(flags | (slmask << 12), bias_dev, stats_dev, gate_dev)
        if st != 0:
            return st
        what = '{} tile {} slots {}'.format(name, tile, slmask + 1)
        o, Eo = R.activate(v, E, R.ACT_RELU if flags & RELU else R.ACT_LRELU if flags & LRELU else 0, 0.25)
        if flags & GATE:
            m = (gate > 0).to(F64)
        elif flags & BNB:
            m = R.bnb_mask(gate, scale, shift).to(F64)
        else:
            m = torch.ones_like(o)
        _check(entry, got, (R.bf16r(o) if mode == 'exact' else o) * m, R.tol_bf16(o, Eo) * m, mode, what)
        if flags & STATS and flags & SATOM:
            ref, tol = R.stats_ref(v, E)
            _check(entry, stats_dev.sum(0), ref, tol, mode, what + ' fp64 slots')
        elif flags & STATS:
            _stats_check(entry, F, c, tile, stats_dev.to('cpu', F64), v, E, mode, what)
        if flags & (BNB | BNP):
            # the sums are over the bf16 values as stored: (a) the stored values themselves, summed in fp64,
            # with the tolerance of an fp32 summation alone; (b) the pure reference with the element tolerances
            if flags & BNB:
                route, yb = m, gate
            else:
                pos, yb = R.bnp_route(gate, scale, shift, Nb, c.H, c.W)
                route = pos.to(F64)
            sums = stats_dev.sum(0).to('cpu')
            ref, tol = R.bn_sums(got * route, yb)
            if mode == 'exact':   # every partial sum of dz * y is a multiple of 1/64 (1/128 at alpha 0.5) below 2^24
                assert bool(((got * route * yb).abs().sum(0) * 128 < R.LIM).all())
            _check(entry, sums, ref, tol, mode, what + ' sums of the stored values')
            ref2, tol2 = R.bn_sums(R.bf16r(o) * route if mode == 'exact' else o * route, yb)
            et = R.tol_bf16(o, Eo) * route
            _check(entry, sums, ref2, tol2 + torch.stack([et.sum(0), (et * yb.abs()).sum(0)]), mode, what + ' sums')
    return 0


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', R.EPI_SHAPES, ids=['full', 'guarded'])
def test_igemm_every_specialised_epilogue(F, shape, mode):
    """The nine flag sets tile_epilogue specialises and two that take the runtime-flag copy (BIAS|RELU|STATS,
    GATE|BIAS), on full tiles of every shape (M = N = 128) and on guarded partial tiles (M = 48, N = 72), through
    every tile shape x staging form and both wave-K-split forms (which refuse partial-row statistics: asserted).
    Partial-row statistics row set by row set; SATOM slot tables with (flags >> 12) & 15 at 0 and at the
    bn_slots value."""
    c = Case.get(0, shape, 9, mode)
    for name, flags, kw in _epilogue_sets(c, mode):
        for tile in VALID_TILES:
            def launcher(fl, bias_dev, stats_dev, gate_dev):
                st, got = launch(F, c, 0, tile, flags=fl, alpha=1.0 if fl & (STATS | BNB | BNP) else 0.5, slope=0.25,
                                 bias=bias_dev, stats=stats_dev, gate=gate_dev)
                return st, None if got is None else got[0]
            st = _run_epilogue(F, 'rk_igemm epilogue ' + name, c, tile, name, flags, kw.get('bias'), mode, launcher)
            assert st == expected_status(c, 0, tile, flags), (name, tile, st)
            COUNT['ran' if st == 0 else 'refused'] += 1


@pytest.mark.parametrize('mode', MODES)
def test_igemm_dgrad_gate_and_bnb(F, mode):
    """The data gradient (kind 1: flipped gather, tap-major K-outer weights) with its two epilogues."""
    c = Case.get(1, (2, 8, 8, 64, 64), 9, mode)
    for name, flags in (('GATE', GATE), ('BNB|SATOM', BNB | SATOM)):
        for tile in EPI_TILES:
            def launcher(fl, bias_dev, stats_dev, gate_dev):
                st, got = launch(F, c, 0, tile, flags=fl, alpha=1.0 if fl & BNB else 0.5, bias=bias_dev,
                                 stats=stats_dev, gate=gate_dev)
                return st, None if got is None else got[0]
            assert _run_epilogue(F, 'rk_igemm kind 1 ' + name, c, tile, name, flags, None, mode, launcher) == 0
            COUNT['ran'] += 1


# ------------------------------------------------------------------------------------------- rk_hconv
HCONV_SHAPES = [(8, 4, 4), (2, 8, 8), (2, 16, 16), (2, 8, 32)]


class HCase:
    """Operands of one halo-tiled conv: M pixels, Cch gathered channels, N output channels."""
    _cache = {}

    @classmethod
    def get(cls, *key):
        if key not in cls._cache:
            cls._cache[key] = cls(*key)
        return cls._cache[key]

    def __init__(self, dgrad, nhw, Cch, N, mode):
        Nb, H, W = nhw
        self.H, self.W, self.C, self.N, self.M, self.K = H, W, Cch, N, Nb * H * W, 9 * Cch
        seed = 5000 + 100 * dgrad + Nb * H * W + Cch + N
        a = R.draw(mode, seed, (Nb, H, W, Cch))
        if dgrad:   # w [Cch = Cout][9][N = Cin]
            w = R.draw(mode, seed + 1, (Cch, 9, N), K=9 * Cch)
            self.ldb = 9 * N
        else:
            w = R.draw(mode, seed + 1, (N, 9, Cch), K=9 * Cch)
            self.ldb = 9 * Cch
        self.A, self.B = R.operands(1 if dgrad else 0, a, w)
        self.a_dev, self.b_dev = _dev(a), _dev(w.reshape(w.shape[0], -1))
        self.slabs, self.S = R.gemm(self.A, self.B)
        self.mode = mode
        if mode == 'exact':
            assert R.exact_ok(self.S[0])
        self.kind = 0

    def gemm(self, splits=1):
        return self.slabs, self.S


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dgrad', [0, 1])
@pytest.mark.parametrize('Cch', [64, 128])
@pytest.mark.parametrize('nhw', HCONV_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_hconv(F, nhw, Cch, dgrad, mode):
    """rk_hconv forward and data gradient: W in {4, 8, 16, 32}, both bn_bit values, grid 0 and a persistent grid
    smaller than the item count, C 64 and 128, two or more images (an item's halo meets another item of the
    same image and an image edge), flags STATS (partial rows), BIAS|RELU, GATE, BNB|SATOM, BNP|SATOM."""
    Nb, H, W = nhw
    entry = 'rk_hconv dgrad' if dgrad else 'rk_hconv fwd'
    bm = 64 if W == 8 else 128
    for bn_bit in (0, 1):
        N = 256 if bn_bit else 128
        c = HCase.get(dgrad, nhw, Cch, N, mode)
        items = (c.M // bm) * (N // (128 if bn_bit else 64))
        assert items >= 2
        for grid in (0, max(1, items // 2) if items < 6 else 3):
            for name, flags, kw in _epilogue_sets(c, mode):
                if name not in ('STATS', 'BIAS|RELU', 'GATE', 'BNB|SATOM', 'BNP|SATOM'):
                    continue

                def launcher(fl, bias_dev, stats_dev, gate_dev):
                    buf = _out_buf(c.M, N, N, BF16)
                    # the halo kernels take no ldc: gates are read with the row stride N
                    g = None if gate_dev is None else gate_dev[:, :N].contiguous()
                    st = _status(lambda: F.hconv(dgrad, c.a_dev, c.b_dev, buf, c.M, N, c.K, c.ldb, H, W, Cch,
                                                 bias=bias_dev, stats=stats_dev, gate=g, flags=fl,
                                                 alpha=1.0 if fl & (STATS | BNB | BNP) else 0.5, slope=0.25,
                                                 bn_bit=bn_bit, grid=grid))
                    return st, (_read_out(buf, c.M, N)[0] if st == 0 else None)
                what = '{} bn_bit {} grid {}'.format(name, bn_bit, grid)
                if flags == STATS:
                    st = _hconv_stats(F, entry, c, bm, flags, mode, launcher, what)
                else:
                    st = _run_epilogue(F, entry, c, 3, what, flags, kw.get('bias'), mode, launcher)
                assert st == 0, what
                COUNT['ran'] += 1


def _hconv_stats(F, entry, c, bm, flags, mode, launcher, what):
    stats_dev = torch.full((c.M // bm * 2, 2, c.N), NAN, dtype=F32, device=DEV)
    st, got = launcher(flags, None, stats_dev, None)
    if st != 0:
        return st
    v, E = R.fp32_out(c.slabs[0], c.S[0], c.K)
    if mode == 'exact':
        assert R.exact_ok(c.S[0], v)
    _check(entry, got, R.bf16r(v) if mode == 'exact' else v, R.tol_bf16(v, E), mode, what)
    got_stats = stats_dev.to('cpu', F64)
    for r, sl in enumerate(R.stats_row_sets(c.M, bm)):
        ref, tol = R.stats_ref(v, E, sl)
        _check(entry, got_stats[r], ref, tol, mode, '{} stats row {}'.format(what, r))
    return 0


def test_hconv_refusals(F):
    """Outside the covered shapes rk_hconv answers RK_EUNSUPPORTED (a wrong ldb: RK_EBADARG) and writes nothing."""
    def status(Nb, H, W, Cch, N, ldb=None, bn_bit=0):
        x = torch.zeros(Nb, H, W, Cch, dtype=BF16, device=DEV)
        w = torch.zeros(N, 9 * Cch, dtype=BF16, device=DEV)
        buf = _out_buf(Nb * H * W, N, N, BF16)
        st = _status(lambda: F.hconv(0, x, w, buf, Nb * H * W, N, 9 * Cch, 9 * Cch if ldb is None else ldb, H, W,
                                     Cch, bn_bit=bn_bit))
        host = buf.to('cpu', F64)
        assert st == 0 or bool(((host == CANARY) | torch.isnan(host)).all())
        return st
    assert status(2, 8, 8, 64, 64) == 0
    assert status(2, 6, 6, 64, 64) == -2       # W outside {4, 8, 16, 32}
    assert status(2, 12, 8, 64, 64) == -2      # H no power of two
    assert status(2, 2, 16, 64, 64) == -2      # H * W below one item
    assert status(3, 4, 4, 64, 64) == -2       # 4x4: whole items of 8 images
    assert status(8, 8, 4, 64, 64) == -2       # W = 4 needs H = 4
    assert status(2, 8, 8, 32, 64) == -2       # C below 64
    assert status(2, 8, 8, 192, 64) == -2      # C no power of two
    assert status(2, 8, 8, 64, 96) == -2       # N no multiple of BN
    assert status(2, 8, 8, 64, 64, bn_bit=1) == -2
    assert status(2, 8, 8, 64, 64, ldb=640) == -1


# ------------------------------------------------------------------------- rk_hconv_wgrad + rk_reduce_slabs
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('nhw,Ci,Co', [((8, 4, 4), 64, 64), ((2, 8, 8), 64, 128), ((5, 8, 8), 64, 64),
                                       ((2, 16, 16), 128, 64), ((2, 8, 32), 64, 64)],
                         ids=lambda s: 'x'.join(map(str, s)) if isinstance(s, tuple) else str(s))
def test_hconv_wgrad_and_reduce(F, nhw, Ci, Co, mode):
    """rk_hconv_wgrad slab by slab (slab s = the pixel items s*per .. (s+1)*per; surplus slabs exactly zero) for
    S = 1, an uneven split and S above the item count; then rk_reduce_slabs, plain and accumulating."""
    Nb, H, W = nhw
    c = Case.get(2, (Nb, H, W, Ci, Co), 9, mode)
    P = 64 if W == 8 else 128
    items = c.K // P
    for S_ in sorted({1, 2 if items % 2 else 3, items + 2}):
        slab = torch.full((S_, Co, 9 * Ci), NAN, dtype=F32, device=DEV)
        F.hconv_wgrad(c.a_dev, c.b_dev, slab, S_)
        got = slab.to('cpu', F64)
        per = R.cdiv(items, S_)
        refs, tols = [], []
        for s in range(S_):
            lo, hi = min(c.K, s * per * P), min(c.K, (s + 1) * per * P)
            v = c.A[:, lo:hi] @ c.B[:, lo:hi].t()
            E = (hi - lo) * R.U32 * (c.A[:, lo:hi].abs() @ c.B[:, lo:hi].abs().t())
            if lo == hi:
                assert bool((got[s] == 0).all()), 'surplus slab {} of {} is not zero'.format(s, S_)
            _check('rk_hconv_wgrad', got[s], v, E, mode, 'S {} slab {}'.format(S_, s))
            refs.append(R.f32r(v) if mode == 'exact' else got[s])
            tols.append(E)
        # the reduction is judged on the slabs it was given (fp32 values, summed here in fp64)
        tot = torch.stack(refs).sum(0)
        tol = (S_ - 1) * R.U32 * torch.stack(refs).abs().sum(0)
        out = torch.full((Co, 9 * Ci), NAN, dtype=F32, device=DEV)
        F.reduce_slabs(slab, out)
        _check('rk_reduce_slabs', out, tot, tol, mode, 'S {}'.format(S_))
        prior = R.draw(mode, 77, (Co, 9 * Ci)) * 5
        out = prior.to(DEV, F32)
        F.reduce_slabs(slab, out, accumulate=True)
        _check('rk_reduce_slabs', out, tot + prior, tol + R.U32 * (tot.abs() + prior.abs()), mode,
               'S {} accumulate'.format(S_))
        COUNT['ran'] += 3


def test_hconv_wgrad_refusals(F):
    def status(Nb, H, W, Ci, Co, S_=1):
        dy = torch.zeros(Nb, H, W, Co, dtype=BF16, device=DEV)
        x = torch.zeros(Nb, H, W, Ci, dtype=BF16, device=DEV)
        slab = torch.zeros(max(S_, 1), Co, 9 * Ci, dtype=F32, device=DEV)
        return _status(lambda: F.hconv_wgrad(dy, x, slab, S_))
    assert status(2, 8, 8, 64, 64) == 0
    assert status(2, 6, 6, 64, 64) == -2
    assert status(3, 4, 4, 64, 64) == -2
    assert status(2, 8, 8, 32, 64) == -2
    assert status(2, 8, 8, 64, 72) == -2
    assert status(2, 8, 8, 64, 64, S_=0) == -2


# --------------------------------------------------------------- rk_slab_epi and rk_reduce_slabs_epi
def _slabs(mode, seed, S_, M, N):
    """Slabs built in fp64 and rounded to fp32: a fault is the combine kernel's, not a GEMM's."""
    if mode == 'exact':
        return R.ints(seed, (S_, M, N), -40, 40)
    return R.f32r(torch.randn((S_, M, N), generator=torch.Generator().manual_seed(seed)).to(F64))


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('M,N,S_', [(48, 8, 1), (300, 64, 3), (70, 256, 2), (600, 1024, 2)])
def test_slab_epi_modes(F, M, N, S_, mode):
    """rk_slab_epi modes 0-3 (plain, forward statistics, BN-backward mask and sums, ReLU gate).  M = 600 at
    N = 1024 makes the capped statistics grid walk its rows twice."""
    slabs = _slabs(mode, 31 + M, S_, M, N)
    dev = slabs.to(DEV, F32)
    v = slabs.sum(0)
    E = (S_ - 1) * R.U32 * slabs.abs().sum(0)
    scale, shift = R.draw_scale_shift(32, N)
    y = R.draw_decision(33, (M, N))
    assert R.decisions_inexact(y, scale, shift) == 0
    y_dev = _dev(y)
    for md in (0, 1, 2, 3):
        out = torch.full((M + 8, N), CANARY, dtype=BF16, device=DEV)
        out[:M] = NAN
        acc = torch.zeros((F.bn_slots(N), 2, N), dtype=F64, device=DEV) if md in (1, 2) else None
        F.slab_epi(dev, S_, M, N, out, mode=md, gate=y_dev if md >= 2 else None,
                   scale=scale.to(DEV, F32) if md == 2 else None, shift=shift.to(DEV, F32) if md == 2 else None,
                   acc=acc)
        got = _read_out(out[None, :, :], M, N)[0]
        m = (y > 0).to(F64) if md == 3 else R.bnb_mask(y, scale, shift).to(F64) if md == 2 else torch.ones_like(v)
        entry = 'rk_slab_epi mode {}'.format(md)
        _check(entry, got, (R.bf16r(v) if mode == 'exact' else v) * m, R.tol_bf16(v, E) * m, mode)
        if md == 1:
            if mode == 'exact':
                assert R.exact_ok(slabs.abs().sum(0), v)
            ref, tol = R.stats_ref(v, E)
            _check(entry, acc.sum(0), ref, tol, mode, 'statistics')
        if md == 2:
            # as FLAG_BNB: the sums are over the bf16 values as stored
            ref, tol = R.bn_sums(got * m, y)
            _check(entry, acc.sum(0), ref, tol, mode, 'sums of the stored values')
        COUNT['ran'] += 1


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('M,N,S_', [(37, 16, 2), (130, 132, 5), (200, 96, 1)])
def test_reduce_slabs_epi(F, M, N, S_, mode):
    """rk_reduce_slabs_epi: bf16 and fp32 output, each activation, alpha, bias, strided output."""
    from rafiki_amd.ops import _lib
    slabs = _slabs(mode, 41 + M, S_, M, N)
    dev = slabs.to(DEV, F32)
    bias = R.draw_bias(mode, 42, N, big=True)
    bias_dev = bias.to(DEV, F32)
    ldc = N + 8
    for f32_out in (False, True):
        for act in (0, 1, 2):
            for alpha, b in ((1.0, None), (0.5, bias)):
                buf = _out_buf(M, N, ldc, F32 if f32_out else BF16)
                _lib.call('rk_reduce_slabs_epi', dev.data_ptr(), S_, M, N, None if b is None else bias_dev.data_ptr(),
                          act, 0.25, alpha, None if f32_out else buf.data_ptr(), buf.data_ptr() if f32_out else None,
                          ldc, F._s())
                got = _read_out(buf, M, N)[0]
                v, E = R.fp32_out(slabs.sum(0), slabs.abs().sum(0), 0, alpha=alpha, bias=b, nslabs=S_)
                v, E = R.activate(v, E, act, 0.25)
                ref, tol = (v, E) if f32_out else (R.bf16r(v) if mode == 'exact' else v, R.tol_bf16(v, E))
                _check('rk_reduce_slabs_epi', got, ref, tol, mode, 'f32 {} act {} alpha {}'.format(f32_out, act, alpha))
                COUNT['ran'] += 1


# ----------------------------------------------------------------------------------------- rk_conv_wt
def test_conv_wt_bit_equal(F):
    """ConvWT: several layers in one launch, Cin / Cout no multiples of 64 included, bit-equal to the flipped
    transpose; the gaps between the layers' copies stay untouched."""
    layers = [(64, 64), (72, 24), (128, 8), (40, 136), (256, 64)]   # (Cout, Cin)
    ws = [R.normal_bf16(50 + i, (co, 9, ci)) for i, (co, ci) in enumerate(layers)]
    sizes = [(w.numel() + 63) // 64 * 64 for w in ws]
    arena = torch.zeros(sum(sizes) + 64, dtype=BF16, device=DEV)
    views, off = [], 0
    for w, n in zip(ws, sizes):
        v = arena[off:off + w.numel()].view(w.shape[0], -1)
        v.copy_(w.reshape(w.shape[0], -1).to(DEV, BF16))
        views.append(v)
        off += n
    wt = F.ConvWT(arena, views)
    wt.buf.fill_(CANARY)
    wt.refresh()
    covered = torch.zeros(wt.buf.numel(), dtype=torch.bool)
    for l, w in enumerate(ws):
        ref = R.flip_transpose(w).reshape(w.shape[2], -1)
        got = wt.view(l).to('cpu', F64)
        assert torch.equal(got, ref), 'layer {}'.format(l)
        o = wt._views[l][0]
        covered[o:o + w.numel()] = True
    assert bool((wt.buf.to('cpu', F64)[~covered] == CANARY).all())


# --------------------------------------------------------------------------- every offered candidate
CAND_SHAPES = [(8, 4, 4, 64, 64), (2, 16, 16, 64, 128), (3, 6, 6, 24, 40)]


@pytest.fixture
def capture(F, monkeypatch):
    """functional._tuned captures (candidates, run) and answers with the first candidate."""
    seen = {}

    def tuned(key, candidates, run):
        seen['c'], seen['run'] = list(candidates), run
        return candidates[0]
    monkeypatch.setattr(F, '_tuned', tuned)
    return seen


def _nslabs(cfg):
    return cfg[2] if cfg[0] == 'k' else 1


def _each_candidate(seen, nonpow2, before, check):
    """Run every captured candidate once.  The wave-K-split tile is offered at extents that are no power of
    two, where the launcher refuses it (the tuner skips a refused candidate): asserted as that refusal."""
    ran = 0
    assert len(seen['c']) >= 1
    for cfg in seen['c']:
        before()
        st = _status(lambda: seen['run'](cfg))
        if st != 0:
            assert st == -2 and nonpow2 and isinstance(cfg[0], int) and cfg[0] & 15 == KS, (cfg, st)
            COUNT['refused'] += 1
            continue
        check(cfg)
        ran += 1
        COUNT['ran'] += 1
    assert ran >= 1
    return ran


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', CAND_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_candidates_conv_fwd(F, capture, shape, mode):
    """conv_fwd: no statistics, partial-row statistics, fp64-slot statistics, bias + activation: every offered
    candidate (tile x staging, wave-K-split, halo-tiled, split-K + rk_slab_epi) against the reference."""
    Nb, H, W, Ci, Co = shape
    c = Case.get(0, shape, 9, mode)
    slabs, S = c.gemm(1)
    x, w = c.a_dev, c.b_dev
    out = torch.empty((Nb, H, W, Co), dtype=BF16, device=DEV)
    v, E = R.fp32_out(slabs[0], S[0], c.K)
    if mode == 'exact':
        assert R.exact_ok(S[0], v)
    ref = R.bf16r(v) if mode == 'exact' else v

    def tol_of(cfg):   # a split-K candidate ('k', tile, S) adds its slabs in fp32
        return R.tol_bf16(v, R.fp32_out(slabs[0], S[0], c.K, nslabs=_nslabs(cfg))[1])

    def fill():
        out.fill_(NAN)
    # plain
    F.conv_fwd(x, w, out=out)
    _each_candidate(capture, c.nonpow2, fill,
                    lambda cfg: _check('conv_fwd', out.reshape(-1, Co), ref, tol_of(cfg), mode, str(cfg)))
    # partial-row statistics
    _, st_view = F.conv_fwd(x, w, out=out, want_stats=True)
    rows_buf = st_view._base if st_view._base is not None else st_view

    def fill_rows():
        out.fill_(NAN)
        rows_buf.fill_(NAN)

    def check_rows(cfg):
        _check('conv_fwd', out.reshape(-1, Co), ref, tol_of(cfg), mode, str(cfg))
        bm = F._cfg_bm(cfg, W)
        got = rows_buf.to('cpu', F64)
        for r, sl in enumerate(R.stats_row_sets(c.M, bm)):
            sref, stol = R.stats_ref(v, E, sl)
            _check('conv_fwd', got[r], sref, stol, mode, '{} stats row {}'.format(cfg, r))
    _each_candidate(capture, c.nonpow2, fill_rows, check_rows)
    # fp64 slots
    acc = F.bn_acc_buffer(Co, DEV)
    F.conv_fwd(x, w, out=out, stats_acc=acc)

    def fill_acc():
        out.fill_(NAN)
        acc.zero_()

    def check_acc(cfg):
        _check('conv_fwd', out.reshape(-1, Co), ref, tol_of(cfg), mode, str(cfg))
        sref, stol = R.stats_ref(v, R.fp32_out(slabs[0], S[0], c.K, nslabs=_nslabs(cfg))[1])
        _check('conv_fwd', acc.sum(0), sref, stol, mode, '{} slots'.format(cfg))
    _each_candidate(capture, c.nonpow2, fill_acc, check_acc)
    # bias + leaky ReLU
    bias = R.draw_bias(mode, 61, Co, big=True)
    F.conv_fwd(x, w, out=out, bias=bias.to(DEV, F32), act=F.ACT_LRELU, slope=0.25)
    vb, Eb = R.fp32_out(slabs[0], S[0], c.K, bias=bias)
    vb, Eb = R.activate(vb, Eb, R.ACT_LRELU, 0.25)
    _each_candidate(capture, c.nonpow2, fill,
                    lambda cfg: _check('conv_fwd', out.reshape(-1, Co), R.bf16r(vb) if mode == 'exact' else vb,
                                       R.tol_bf16(vb, Eb), mode, 'bias+lrelu {}'.format(cfg)))


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', [(8, 2, 2, 64, 64), (2, 8, 8, 64, 128), (3, 3, 3, 24, 40)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_candidates_conv_up(F, capture, shape, mode):
    """conv_up (kind 6) at input resolutions whose outputs are the candidate shapes."""
    Nb, H, W, Ci, Co = shape
    c = Case.get(6, shape, 9, mode)
    slabs, S = c.gemm(1)
    bias = R.draw_bias(mode, 62, Co, big=True)
    out = torch.empty((Nb, 2 * H, 2 * W, Co), dtype=BF16, device=DEV)
    F.conv_up(c.a_dev, c.b_dev, out=out, bias=bias.to(DEV, F32), act=F.ACT_RELU)
    v, E = R.fp32_out(slabs[0], S[0], c.K, bias=bias)
    v, E = R.activate(v, E, R.ACT_RELU)
    _each_candidate(capture, c.nonpow2, lambda: out.fill_(NAN),
                    lambda cfg: _check('conv_up', out.reshape(-1, Co), R.bf16r(v) if mode == 'exact' else v,
                                       R.tol_bf16(v, E), mode, str(cfg)))


def _dgrad_modes(F, c, mode, call, M, N, Nb, H, W, capture, entry, pool_ok):
    """plain, gate, BNB and (power-of-two geometry) BNP through every candidate of a data-gradient entry point."""
    slabs, S = c.gemm(1)
    v = slabs[0]
    ref = R.bf16r(v) if mode == 'exact' else v

    def tol_of(cfg):
        return R.tol_bf16(v, R.fp32_out(slabs[0], S[0], c.K, nslabs=_nslabs(cfg))[1])
    out = torch.empty((Nb, H, W, N), dtype=BF16, device=DEV)
    scale, shift = R.draw_scale_shift(71, N)
    coeffs = torch.stack([torch.zeros(N, dtype=F64), torch.ones(N, dtype=F64), scale, shift]).to(DEV, F32)
    y = R.draw_decision(72, (M, N))
    assert R.decisions_inexact(y, scale, shift) == 0
    y_dev = _dev(y).view(Nb, H, W, N)
    acc = F.bn_acc_buffer(N, DEV)

    def fill():
        out.fill_(NAN)
        acc.zero_()
    call(out=out)
    _each_candidate(capture, c.nonpow2, fill, lambda cfg: _check(entry, out.reshape(-1, N), ref, tol_of(cfg), mode, str(cfg)))
    call(out=out, gate=y_dev)
    g = (y > 0).to(F64)
    _each_candidate(capture, c.nonpow2, fill,
                    lambda cfg: _check(entry, out.reshape(-1, N), ref * g, tol_of(cfg) * g, mode, 'gate {}'.format(cfg)))
    call(out=out, bn_y=y_dev, bn_coeffs=coeffs, bn_acc=acc)
    m = R.bnb_mask(y, scale, shift).to(F64)

    def check_bnb(cfg):
        got = out.reshape(-1, N).to('cpu', F64)
        _check(entry, got, ref * m, tol_of(cfg) * m, mode, 'bnb {}'.format(cfg))
        sref, stol = R.bn_sums(got * m, y)
        _check(entry, acc.sum(0), sref, stol, mode, 'bnb sums of the stored values {}'.format(cfg))
    _each_candidate(capture, c.nonpow2, fill, check_bnb)
    if not pool_ok:
        return
    y2 = R.draw_pool_y(73, Nb, H, W, N, scale)
    assert R.decisions_inexact(y2, scale, shift) == 0
    pos, yb = R.bnp_route(y2, scale, shift, Nb, H, W)
    call(out=out, bn_pool_y=_dev(y2), bn_coeffs=coeffs, bn_acc=acc)

    def check_bnp(cfg):
        got = out.reshape(-1, N).to('cpu', F64)
        _check(entry, got, ref, tol_of(cfg), mode, 'bnp {}'.format(cfg))
        sref, stol = R.bn_sums(got * pos.to(F64), yb)
        _check(entry, acc.sum(0), sref, stol, mode, 'bnp sums of the stored values {}'.format(cfg))
    _each_candidate(capture, c.nonpow2, fill, check_bnp)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', [(8, 4, 4, 64, 64), (2, 16, 16, 128, 64), (3, 6, 6, 40, 8)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_candidates_conv_dgrad(F, capture, shape, mode):
    """conv_dgrad (kind 1, halo-tiled data gradient, split-K + rk_slab_epi modes 0 / 2 / 3): plain, gate, BNB."""
    Nb, H, W, Ci, Co = shape
    c = Case.get(1, shape, 9, mode)
    _dgrad_modes(F, c, mode, lambda **kw: F.conv_dgrad(c.a_dev, c.b_dev, **kw), c.M, Ci, Nb, H, W, capture,
                 'conv_dgrad', False)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', CAND_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_candidates_conv_dgrad_t(F, capture, shape, mode):
    """conv_dgrad_t on ConvWT's flipped transpose: plain, gate, BNB, BNP through every forward candidate."""
    Nb, H, W, Ci, Co = shape
    seed = 8000 + sum(shape)
    dy = R.draw(mode, seed, (Nb, H, W, Co))
    w = R.draw(mode, seed + 1, (Co, 9, Ci), K=9 * Co)
    arena = w.reshape(Co, -1).to(DEV, BF16).contiguous()
    wt = F.ConvWT(arena.view(-1), [arena])
    wt.refresh()
    assert torch.equal(wt.view(0).to('cpu', F64), R.flip_transpose(w).reshape(Ci, -1))

    A, B = R.operands(0, dy, R.flip_transpose(w))   # the forward conv of dy on wt, in that K order
    slabs, S = R.gemm(A, B)
    if mode == 'exact':
        assert R.exact_ok(S[0])
    T = types.SimpleNamespace(kind=0, K=9 * Co, M=Nb * H * W, nonpow2=not (_pow2(Co) and _pow2(H) and _pow2(W)),
                              gemm=lambda splits=1: (slabs, S))
    dy_dev = _dev(dy)
    _dgrad_modes(F, T, mode, lambda **kw: F.conv_dgrad_t(dy_dev, wt.view(0), **kw), T.M, Ci, Nb, H, W, capture,
                 'conv_dgrad_t', _pow2(H) and _pow2(W))


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', CAND_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_candidates_conv_wgrad(F, capture, shape, mode):
    """conv_wgrad: every (tile, splits) candidate and the halo-tiled weight gradient + rk_reduce_slabs."""
    Nb, H, W, Ci, Co = shape
    c = Case.get(2, shape, 9, mode)
    slabs, S = c.gemm(1)
    out = torch.empty((Co, 9 * Ci), dtype=F32, device=DEV)
    F.conv_wgrad(c.a_dev, c.b_dev, out=out)

    def check(cfg):
        s = cfg[1]
        v, E = R.fp32_out(slabs[0], S[0], c.K, nslabs=s)
        _check('conv_wgrad', out, v, E, mode, str(cfg))
    _each_candidate(capture, c.nonpow2, lambda: out.fill_(NAN), check)


@pytest.mark.parametrize('mode', MODES)
def test_candidates_linear(F, capture, mode):
    """linear at a small-M shape where split-K + rk_reduce_slabs_epi is offered: bf16 bias + ReLU, fp32 plain."""
    c = Case.get(3, (37, 1024, 16), 1, mode)
    slabs, S = c.gemm(1)
    x, w = c.a_dev[:, :c.K], c.b_dev[:, :c.K]     # row strides wider than the row
    bias = R.draw_bias(mode, 81, c.N, big=True)
    out = torch.empty((c.M, c.N), dtype=BF16, device=DEV)
    F.linear(x, w, bias.to(DEV, F32), act=F.ACT_RELU, out=out, alpha=0.5)
    assert len(capture['c']) > 1

    def check(cfg):
        v, E = R.fp32_out(slabs[0], S[0], c.K, alpha=0.5, bias=bias, nslabs=cfg[1])
        v, E = R.activate(v, E, R.ACT_RELU)
        _check('linear', out, R.bf16r(v) if mode == 'exact' else v, R.tol_bf16(v, E), mode, str(cfg))
    _each_candidate(capture, False, lambda: out.fill_(NAN), check)
    out32 = torch.empty((c.M, c.N), dtype=F32, device=DEV)
    F.linear(x, w, out=out32)

    def check32(cfg):
        v, E = R.fp32_out(slabs[0], S[0], c.K, nslabs=cfg[1])
        _check('linear', out32, v, E, mode, 'fp32 {}'.format(cfg))
    _each_candidate(capture, False, lambda: out32.fill_(NAN), check32)
