"""Every tile, ring depth and K loop of the fp32 implicit-GEMM family (csrc/kernels/sgemm.hip: rk_sgemm,
rk_sgemm_g, rk_sgemm_grp), the combine kernels and every candidate the wrappers of ops/f32.py offer, against the
fp64 references of tests/sgemm_refs.py (anchored and shown to bite in tests/test_sgemm_refs.py).

Input sets (sgemm_refs): EXACT and the three EXACT-WIDE sets must come back bit for bit on both K loops; RANDOM is
held element by element to the hard tolerance n * 2^-23 * S and, per output row and column, to 4x the error of a
plain fp32 accumulation on the CPU (the yardstick).  Every output buffer is NaN-prefilled with ldc = N + 4 and two
rows below that must still be NaN afterwards; every operand is a view 64 floats inside a larger NaN-filled storage
(dense operands with lda, ldb wider than the row), so an unmasked over-read shows as a NaN in the output.  Every
launch runs once; a launcher refusal is predicted by ``expected_status`` and asserted, never skipped.  The worst
error / tolerance and the worst yardstick ratio per entry point and K loop are printed at the end (pytest -s)
with the number of launches checked and refusals asserted.
"""
import re

import pytest
import torch

import sgemm_refs as G

pytestmark = pytest.mark.gpu

DEV = 'cuda'
F64, F32 = torch.float64, torch.float32
NAN = float('nan')
X6 = 16
RELU, BIAS, STATS, GATE, ACCUM, LRELU, BNB, BNP = 1, 2, 4, 8, 16, 32, 512, 1024
TILES = list(range(11))
BAD_TILES = [11, 15, 27, 31, 32, -1]
EPI_TILES = (0, 3, 5, 10)
PAD = 64
WORST, YWORST, POOLED = {}, {}, {}
COUNT = {'ran': 0, 'refused': 0}
IDS = lambda v: '-'.join(map(str, v)) if isinstance(v, tuple) else str(v)   # noqa: E731


@pytest.fixture(scope='module')
def S():
    from rafiki_amd.ops import _lib, f32
    _lib.lib()   # loud failure if the native library is missing
    yield f32
    Prob._cache.clear()
    for tag in sorted(WORST):
        pl = POOLED.get(tag, [0, 0, 0, 0])
        print('WORST {:34s} err / hard tol {:.4f}   yardstick ratio {:.3f}   rows alone {} pooled {}   cols alone {} '
              'pooled {}'.format(tag, WORST[tag], YWORST.get(tag, 0.0), *pl))
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
    from rafiki_amd.ops._lib import KernelError
    try:
        fn()
    except KernelError as e:
        return int(re.search(r'status (-?\d+)', str(e)).group(1))
    return 0


def _arena(t, ld=None, dtype=F32):
    """Device copy of t (rows = every leading dim, row stride ld) as a view PAD floats inside a NaN-filled
    storage that also runs PAD floats past it."""
    cols = t.shape[-1]
    rows = t.numel() // cols
    ld = ld or cols
    buf = torch.full((2 * PAD + rows * ld,), NAN, dtype=dtype, device=DEV)
    v = buf[PAD:PAD + rows * ld].view(rows, ld)
    v[:, :cols] = t.reshape(rows, cols).to(DEV, dtype)
    return v if ld != cols else v.view(t.shape)


def _out_buf(rows, N, ldc, slabs=1, prior=None):
    buf = torch.full((slabs, rows + 2, ldc), NAN, dtype=F32, device=DEV)
    if prior is not None:
        buf[:, :rows, :N] = prior.to(DEV, F32)
    return buf


def _read_out(buf, rows, N):
    host = buf.to('cpu', F64)
    assert bool(torch.isnan(host[:, rows:, :]).all()) and bool(torch.isnan(host[:, :rows, N:]).all()), \
        'wrote outside out[M][N]'
    body = host[:, :rows, :N]
    assert not bool(torch.isnan(body).any()), '{} NaN in the output (unwritten, or an over-read operand)'.format(
        int(torch.isnan(body).sum()))
    return body


def judge(tag, got, ref, tol, mode, yard=None, what=''):
    """Exact sets: got == ref everywhere.  RANDOM: |got - ref| <= tol element by element and, with a yardstick,
    rms(got - ref) <= 4 rms(yardstick - ref) per row and per column."""
    got = got.to('cpu', F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert not bool(torch.isnan(got).any()), '{} {}: NaN in the output'.format(tag, what)
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
        info = {}
        r = G.rms_ratio(got, ref, yard, info)
        YWORST[tag] = max(YWORST.get(tag, 0.0), r)
        # never everything pooled: rows or columns (one of them has the samples) are judged one by one
        assert info['rows'] + info['cols'] > 0, '{} {}: every row and column pooled {}'.format(tag, what, info)
        pl = POOLED.setdefault(tag, [0, 0, 0, 0])
        for i, k in enumerate(('rows', 'rows_pooled', 'cols', 'cols_pooled')):
            pl[i] += info[k]
        assert r <= G.YARD, '{} {}: rms error {:.2f}x the fp32 yardstick (gate {})'.format(tag, what, r, G.YARD)


# -------------------------------------------------------------------------------------------- cases
class Prob:
    """One problem of the family on the device: raw operands in NaN arenas, the GEMM view per group, the launch."""
    _cache = {}

    @classmethod
    def get(cls, name, shape, taps, mode):
        key = (name, tuple(shape), taps, mode)
        if key not in cls._cache:
            cls._cache[key] = cls(name, shape, taps, mode)
        return cls._cache[key]

    def __init__(self, full, shape, taps, mode):
        from rafiki_amd.ops import f32 as S
        self.full, self.shape, self.taps, self.mode = full, shape, taps, mode
        self.name = name = full.replace('_shared', '')
        self.shared = full.endswith('_shared')
        a, b = G.problem(full, shape, taps, mode)
        self.a, self.b = a, b
        self.views = G.view(name, a, b, taps)
        self.M, self.K = self.views[0][0].shape
        self.N = self.views[0][1].shape[0]
        self.groups = len(self.views)
        self.rows = self.M * self.groups
        self.ldc = self.N + 4
        self.entry = {'s2': 'rk_sgemm_g', 's2t': 'rk_sgemm_g', 's2w': 'rk_sgemm_g', 'conv_grp': 'rk_sgemm_grp',
                      'dense_grp': 'rk_sgemm_grp'}.get(name, 'rk_sgemm')
        self.kind = {'conv': 0, 'wgrad': 2, 'dense': 3, 'dx': 4, 'dw': 5, 's2': 6, 's2t': 6, 's2w': 7, 'conv_grp': 0,
                     'dense_grp': 3}[name]
        self.tag = '{} kind {}'.format(self.entry, self.kind)
        self.geo = {}
        self.big = False
        if name in ('dense', 'dx', 'dw'):
            self.lda, self.ldb = a.shape[1] + 4, b.shape[1] + 8
            self.A, self.B = _arena(a, self.lda), _arena(b, self.ldb)
        elif name == 'dense_grp':     # padded rows: gstrideA = M * lda, gstrideB = N * ldb
            self.lda, self.ldb = self.K + 4, self.K + 8
            self.A, self.B = _arena(a, self.lda), _arena(b, self.ldb)
        elif name in ('conv', 'conv_grp'):
            Nb, H, W, Ci, Co = shape
            self.lda, self.ldb = Ci, self.K + 8
            self.A, self.B = _arena(a), _arena(b.reshape(-1, self.K), self.ldb)
            self.geo = dict(H=H, W=W, C=Ci, taps=taps)
            self.big = name == 'conv' and Ci % 32 == 0
        elif name == 'wgrad':
            Nb, H, W, Ci, Co = shape
            self.lda, self.ldb = Co, Ci
            self.A, self.B = _arena(a), _arena(b)
            self.geo = dict(H=H, W=W, C=Ci, taps=taps)
            self.big = True
        else:
            Nb, H, W, Ci, Co = shape
            s2 = (H, W, Ci, H // 2, W // 2, 2, 16, [S._S2_TPY], [S._S2_TPX])
            if name == 's2':
                self.lda, self.ldb, self.g_geo, self.g_kw = Ci, self.K, s2, {}
                self.A, self.B = _arena(a), _arena(b.reshape(Co, -1))
            elif name == 's2w':
                self.lda, self.ldb, self.g_geo, self.g_kw = Co, Ci, s2, {}
                self.A, self.B = _arena(a), _arena(b)
            else:
                self.lda, self.ldb = Co, self.K
                self.g_geo = (H // 2, W // 2, Co, H // 2, W // 2, 1, 4, S._S2T_TPY, S._S2T_TPX)
                self.g_kw = dict(groups=4, oyx=S._S2T_OYX, os_=2, gstride_b=Ci * self.K)
                self.A = _arena(a)
                self.B = _arena(torch.stack([G.s2t_weights(b, g) for g in range(4)]))
        self._ref, self._yard = {}, {}

    def assemble(self, outs):
        """Per-group [M][N] results -> the output's rows (parity groups scattered to their pixels, groups stacked)."""
        if self.name == 's2t':
            Nb, h, w, _ = self.a.shape
            full = torch.zeros(self.rows, self.N, dtype=F64)
            for g in range(4):
                full[G.s2t_rows(Nb, h, w, g)] = outs[g]
            return full
        return torch.cat(outs)

    def ref(self, splits=1):
        """(slabs [s][rows][N], S [s][rows][N]) with the exact-set precondition asserted before any launch."""
        if splits not in self._ref:
            per = [G.gemm(A, B, splits) for A, B in self.views]
            slabs = torch.stack([self.assemble([p[0][s] for p in per]) for s in range(splits)])
            Ss = torch.stack([self.assemble([p[1][s] for p in per]) for s in range(splits)])
            if self.mode != 'random':
                assert G.exact_ok(Ss.sum(0)), 'exact-set precondition: S >= 2^24'
            self._ref[splits] = (slabs, Ss)
        return self._ref[splits]

    def yard(self, lo=0, hi=None):
        hi = self.K if hi is None else hi
        if (lo, hi) not in self._yard:
            self._yard[(lo, hi)] = self.assemble([G.yardstick(A[:, lo:hi], B[:, lo:hi]) for A, B in self.views])
        return self._yard[(lo, hi)]

    def expected_status(self, tile, nst, flags=0, splits=1):
        """What the launcher must answer: 0, RK_EBADARG (-1) or RK_EUNSUPPORTED (-2)."""
        t = tile & 15
        if tile < 0 or t > 10 or tile > 26 or nst not in (2, 3):
            return -1
        if self.entry != 'rk_sgemm':
            if 4 <= t <= 7 or (splits > 1 and flags):
                return -1
        else:
            if splits > 1 and flags & ~ACCUM:
                return -1
            if 4 <= t <= 7 and not self.big:
                return -2
        if nst == 3 and t in (5, 6, 8, 9, 10):    # 3-stage rings are built for the 4-wave tiles only
            return -2
        return 0

    def launch(self, S, tile, nst=2, *, splits=1, flags=0, alpha=1.0, slope=0.2, bias=None, stats=None, gate=None,
               prior=None):
        """One launch into a NaN-prefilled padded buffer.  Returns (status, out [slabs][rows][N] fp64 on the host)."""
        buf = _out_buf(self.rows, self.N, self.ldc, splits, prior)
        ss = (self.rows + 2) * self.ldc
        common = dict(tile=tile, nst=nst, splits=splits, slab_stride=ss, bias=bias, flags=flags, alpha=alpha, slope=slope)
        if self.entry == 'rk_sgemm':
            fn = lambda: S.sgemm(self.kind, self.A, self.B, buf, self.M, self.N, self.K, self.lda, self.ldb,  # noqa: E731
                                 self.ldc, stats=stats, gate=gate, **self.geo, **common)
        elif self.entry == 'rk_sgemm_g':
            fn = lambda: S.sgemm_g(self.kind, self.A, self.B, buf, self.M, self.N, self.K, self.lda, self.ldb,  # noqa: E731
                                   self.ldc, *self.g_geo, **self.g_kw, **common)
        else:
            gsa = 0 if self.shared else (self.M * self.lda if self.name == 'dense_grp' else self.A[0].numel())
            fn = lambda: S.sgemm_grp(self.kind, self.A, self.B, buf, self.M, self.N, self.K, self.lda, self.ldb,  # noqa: E731
                                     self.ldc, self.groups, gsa, self.N * self.ldb, self.M * self.ldc,
                                     0 if bias is None else self.N, **self.geo, **common)
        st = _status(fn)
        if st != 0:
            assert bool(torch.isnan(buf).all() if prior is None else True), 'a refused launch wrote something'
            COUNT['refused'] += 1
            return st, None
        COUNT['ran'] += 1
        return 0, _read_out(buf, self.rows, self.N)


def loop_tag(p, tile):
    return '{} {}'.format(p.tag, 'X6' if tile & X6 else 'f32')


# ------------------------------------------------------------- 1. every kind x tile x K loop x ring depth
@pytest.mark.parametrize('name,shape,taps', G.SWEEP, ids=IDS)
def test_sgemm_every_tile_loop_and_ring(S, name, shape, taps):
    """Tile codes 0-10 x {f32, X6} x ring depth {2, 3} on EXACT, the three EXACT-WIDE sets and RANDOM; the codes
    the launcher refuses (11-15, above 26, tiles 4-7 where they are not built, 3-stage rings off the 4-wave tiles)
    answer with the predicted status.  The 64x64 tiles put 15 blocks on the (264, 132) and (288, 132) outputs
    and 18 on the grouped (136, 72) x 3: above 8 and no multiple of 8, so the XCD remap deals unequal ranges
    (kinds 6 and 7 get there in the split-K test: 12 and 18 blocks)."""
    for mode in G.MODES:
        p = Prob.get(name, shape, taps, mode)
        slabs, Ss = p.ref(1)
        yard = p.yard() if mode == 'random' else None
        for tile in [t + x for t in TILES for x in (0, X6)] + (BAD_TILES if mode == 'exact' else []):
            for nst in (2, 3):
                want = p.expected_status(tile, nst)
                st, got = p.launch(S, tile, nst)
                assert st == want, '{} tile {} nst {}: status {} (expected {})'.format(p.tag, tile, nst, st, want)
                if st != 0:
                    continue
                tol = G.n_terms(p.K, tile & X6) * G.U32 * Ss[0]
                judge(loop_tag(p, tile), got[0], slabs[0], tol, mode, yard, 'tile {} nst {}'.format(tile, nst))


def test_sgemm_ring_depth_4_is_refused(S):
    p = Prob.get('dense', (37, 20, 36), 1, 'exact')
    for nst in (1, 4):
        assert p.launch(S, 0, nst)[0] == -1


# ------------------------------------------------------------------ the launchers' refusal lines, each once
def test_sgemm_refusals(S, monkeypatch):
    d = Prob.get('dense', (37, 20, 36), 1, 'exact')
    c = Prob.get('conv', (3, 6, 6, 12, 40), 9, 'exact')
    buf = _out_buf(64, 64, 68)
    stats = torch.zeros(1, 2, 64, dtype=F64, device=DEV)

    def sg(kind, want, *, A=d.A, B=d.B, M=36, N=20, K=36, lda=40, ldb=44, ldc=68, **kw):
        st = _status(lambda: S.sgemm(kind, A, B, buf, M, N, K, lda, ldb, ldc, **kw))
        assert st == want, (kind, kw, st, want)
        COUNT['refused'] += 1
    conv = dict(A=c.A, B=c.B, M=108, N=40, K=108, lda=12, ldb=116, H=6, W=6, C=12, taps=9)
    sg(3, -1, M=0), sg(3, -1, N=0), sg(3, -1, K=0), sg(3, -1, splits=0), sg(3, -1, nst=4), sg(3, -1, tile=-1)
    sg(3, -1, tile=11), sg(3, -1, tile=27), sg(3, -1, taps=3)
    sg(3, -2, K=34), sg(3, -2, lda=42), sg(4, -2, K=34), sg(0, -2, **dict(conv, K=106))
    sg(3, -2, ldb=42), sg(0, -2, **dict(conv, ldb=118))
    sg(4, -2, N=18), sg(4, -2, ldb=42), sg(5, -2, N=18), sg(2, -2, **dict(conv, M=40, N=106, lda=40, ldb=12))
    sg(5, -2, M=34), sg(5, -2, lda=42), sg(2, -2, **dict(conv, M=38, N=108, lda=40, ldb=12))
    sg(0, -2, **dict(conv, C=6)), sg(0, -2, **dict(conv, C=0)), sg(0, -2, **dict(conv, H=0)), sg(2, -2, **dict(conv, M=40, N=108, lda=40, ldb=12, W=0))
    for fl in (BIAS, RELU, LRELU, GATE, STATS, BNB, BNP):
        sg(3, -1, splits=2, flags=fl, slab_stride=64 * 68, stats=stats)
    # reciprocal pixel decode: exact below 2^22 only (refused before anything is launched)
    sg(0, -2, **dict(conv, M=(1 << 22) - 40, H=6, W=6)), sg(2, -2, **dict(conv, M=40, N=108, lda=40, ldb=12, K=1 << 22))
    sg(0, -2, **dict(conv, flags=BNP, gate=c.A, bias=c.A, stats=stats))           # BNP: power-of-two maps
    pw = dict(conv, H=4, W=4)
    sg(0, -2, **dict(pw, flags=BNP, bias=c.A, stats=stats)), sg(0, -2, **dict(pw, flags=BNP, gate=c.A, stats=stats))
    sg(0, -2, **dict(pw, flags=BNP, gate=c.A, bias=c.A))
    sg(3, -1, flags=STATS), sg(3, -1, flags=BNB)
    sg(1, -1), sg(6, -1), sg(9, -1)
    for t in (4, 5, 6, 7):      # the 256-wide tiles exist for kind 0 with C % 32 == 0 and kind 2
        sg(3, -2, tile=t), sg(4, -2, tile=t + X6), sg(5, -2, tile=t), sg(0, -2, **dict(conv, tile=t))
    monkeypatch.setattr(S, '_nbytes', lambda t: 0)
    sg(3, -2)
    monkeypatch.setattr(S, '_nbytes', lambda t: 1 << 31)
    sg(3, -2)
    monkeypatch.undo()
    assert bool(torch.isnan(buf).all()), 'a refused launch wrote something'


def test_sgemm_g_and_grp_refusals(S, monkeypatch):
    p = Prob.get('s2', (1, 12, 12, 24, 40), 16, 'exact')
    w = Prob.get('s2w', (1, 12, 12, 24, 40), 16, 'exact')
    buf = _out_buf(64, 400, 404)

    def g(want, kind=6, q=p, **kw):
        a = dict(M=q.M, N=q.N, K=q.K, lda=q.lda, ldb=q.ldb, ldc=q.N, H=12, W=12, C=24, Ho=6, Wo=6, stride=2, ntaps=16,
                 tpy=[S._S2_TPY], tpx=[S._S2_TPX])
        a.update({k: kw.pop(k) for k in list(kw) if k in a})
        st = _status(lambda: S.sgemm_g(kind, q.A, q.B, buf, *a.values(), **kw))
        assert st == want, (kind, kw, st, want)
        COUNT['refused'] += 1
    g(-1, kind=5), g(-1, kind=0), g(-1, M=0), g(-1, splits=0), g(-1, nst=1), g(-1, tile=-1), g(-1, tile=11), g(-1, tile=27)
    for t in (4, 5, 6, 7):
        g(-1, tile=t), g(-1, tile=t + X6)
    g(-1, ntaps=0), g(-1, ntaps=17), g(-1, groups=0), g(-1, groups=5), g(-1, stride=3), g(-1, os_=3)
    g(-1, kind=7, q=w, groups=2, tpy=[S._S2_TPY] * 2, tpx=[S._S2_TPX] * 2)
    g(-2, C=6), g(-2, H=0), g(-2, Wo=0)
    g(-1, K=p.K - 24), g(-1, kind=7, q=w, N=w.N - 24)
    g(-2, lda=26), g(-2, ldb=p.K + 2), g(-2, kind=7, q=w, M=38), g(-2, kind=7, q=w, lda=42)
    for fl in (BIAS, RELU, LRELU):
        g(-1, splits=2, flags=fl, slab_stride=64 * 404)
    for fl in (GATE, STATS, BNB, BNP):
        g(-2, flags=fl)
    g(-2, M=1 << 22), g(-2, kind=7, q=w, K=1 << 22)
    monkeypatch.setattr(S, '_nbytes', lambda t: 0)
    g(-2)
    monkeypatch.undo()

    d = Prob.get('dense_grp', (37, 20, 36), 1, 'exact')
    c = Prob.get('conv_grp', (2, 6, 6, 12, 40), 9, 'exact')

    def grp(want, kind=3, q=d, gs=None, **kw):
        a = dict(M=q.M, N=q.N, K=q.K, lda=q.lda, ldb=q.ldb, ldc=q.N, groups=3, gstride_a=q.M * q.K if q is d else 72 * 12,
                 gstride_b=q.N * q.K, gstride_o=q.M * q.N, gstride_bias=0)
        a.update({k: kw.pop(k) for k in list(kw) if k in a})
        st = _status(lambda: S.sgemm_grp(kind, q.A, q.B, buf, *a.values(), **dict(q.geo, **kw)))
        assert st == want, (kind, kw, st, want)
        COUNT['refused'] += 1
    grp(-1, kind=2), grp(-1, kind=4), grp(-1, M=0), grp(-1, splits=0), grp(-1, nst=4), grp(-1, tile=11), grp(-1, tile=27)
    for t in (4, 5, 6, 7):
        grp(-1, tile=t), grp(-1, kind=0, q=c, tile=t + X6)
    grp(-1, groups=0), grp(-1, gstride_a=-1), grp(-1, gstride_b=-1), grp(-1, gstride_o=-1), grp(-1, gstride_bias=-1)
    grp(-1, taps=2), grp(-2, K=34), grp(-2, lda=38), grp(-2, ldb=38)
    grp(-2, kind=0, q=c, C=6), grp(-2, kind=0, q=c, H=0)
    for fl in (STATS, GATE, ACCUM, BNB, BNP):
        grp(-2, flags=fl)
    for fl in (BIAS, RELU, LRELU):
        grp(-1, splits=2, flags=fl, slab_stride=64 * 404)
    grp(-2, kind=0, q=c, M=1 << 22)
    monkeypatch.setattr(S, '_nbytes', lambda t: 1 << 31)
    grp(-2)
    monkeypatch.undo()
    assert bool(torch.isnan(buf).all()), 'a refused launch wrote something'


# ------------------------------------------------------------------------------------- 2. epilogues
def _epi_sweep(S, p, cases, rows_geo=None):
    """cases: (what, flags, reference kwargs, launch kwargs built by ``dev(kw)``).  Tiles 0, 3, 5, 10 x both loops."""
    slabs, Ss = p.ref(1)
    mode = p.mode
    for what, flags, kw, dev in cases:
        for tile in [t + x for t in EPI_TILES for x in (0, X6)]:
            want = p.expected_status(tile, 2, flags)
            dkw = dev()
            st, got = p.launch(S, tile, 2, flags=flags, **dkw)
            assert st == want, (p.tag, what, tile, st, want)
            if st != 0:
                continue
            n = G.n_terms(p.K, tile & X6)
            r = G.epilogue(slabs[0], Ss[0], n, exact=mode != 'random', **kw)
            ykw = {k: v for k, v in kw.items() if k not in ('stats', 'bnb', 'bnp')}
            yard = G.epilogue32(p.yard(), **ykw) if mode == 'random' else None
            if 'bnb' in kw and yard is not None:
                yard = yard * G.bnb_mask(*kw['bnb']).to(F64)
            judge(loop_tag(p, tile), got[0], r['out'], r['tol'], mode, yard, '{} tile {}'.format(what, tile))
            if 'sums' in r:
                sums = dkw['stats'].to('cpu').sum(0)
                judge(loop_tag(p, tile) + ' sums', sums, r['sums'], r['sums_tol'], mode, None,
                      '{} tile {} statistics'.format(what, tile))


@pytest.mark.parametrize('mode', ('exact', 'random'))
def test_sgemm_conv_epilogues(S, mode):
    """What conv_fwd and conv_dgrad form: bias, ReLU, leaky 0.2, statistics (slot masks 0 and 3, the slot sum is
    judged), the ReLU gate, BNB, BNP (power-of-two maps, tied maxima)."""
    shape = (5, 8, 8, 32, 72)
    Nb, H, W, Ci, Co = shape
    p = Prob.get('conv', shape, 9, mode)
    bias = G.draw_bias(mode, 5, Co)
    bias_d = _arena(bias)
    gate = G.draw_gate(6, (p.M, Co))
    gate_d = _arena(gate, p.ldc)
    scale, shift = G.draw_scale_shift(7, Co)
    y = G.draw_decision(8, (p.M, Co))
    y2 = G.draw_pool_y(9, Nb, H, W, Co, scale)
    assert G.decisions_inexact(y, scale, shift) == 0 and G.decisions_inexact(y2, scale, shift) == 0
    ss_d = _arena(torch.cat([scale, shift]))
    y_d, y2_d = _arena(y, p.ldc), _arena(y2.reshape(-1, Co), p.ldc)

    def st(slots):
        return lambda: dict(stats=torch.zeros(slots, 2, Co, dtype=F64, device=DEV))
    cases = [
        ('bias', BIAS, dict(bias=bias), lambda: dict(bias=bias_d)),
        ('relu', RELU, dict(act=G.ACT_RELU), dict),
        ('bias+relu', BIAS | RELU, dict(bias=bias, act=G.ACT_RELU), lambda: dict(bias=bias_d)),
        ('bias+leaky', BIAS | LRELU, dict(bias=bias, act=G.ACT_LRELU, slope=0.2), lambda: dict(bias=bias_d, slope=0.2)),
        ('stats slots 1', STATS, dict(stats=True), st(1)),
        ('stats slots 4 + bias + relu', STATS | BIAS | RELU, dict(stats=True, bias=bias, act=G.ACT_RELU),
         lambda: dict(bias=bias_d, **st(4)())),
        ('stats + leaky', STATS | LRELU, dict(stats=True, act=G.ACT_LRELU, slope=0.2), lambda: dict(slope=0.2, **st(4)())),
        ('gate', GATE, dict(gate=gate), lambda: dict(gate=gate_d)),
        ('BNB slots 1', BNB, dict(bnb=(y, scale, shift)), lambda: dict(gate=y_d, bias=ss_d, **st(1)())),
        ('BNB slots 4', BNB, dict(bnb=(y, scale, shift)), lambda: dict(gate=y_d, bias=ss_d, **st(4)())),
        ('BNP slots 4', BNP, dict(bnp=(y2, scale, shift, Nb, H, W)), lambda: dict(gate=y2_d, bias=ss_d, **st(4)())),
    ]
    _epi_sweep(S, p, cases)


@pytest.mark.parametrize('mode', ('exact', 'random'))
def test_sgemm_dense_and_wgrad_epilogues(S, mode):
    """linear (alpha != 1, bias, activations), linear_dx (gate), linear_dw and conv_wgrad (accumulate onto a prior)."""
    p = Prob.get('dense', (264, 132, 132), 1, mode)
    bias = G.draw_bias(mode, 15, p.N)
    bias_d = _arena(bias)
    cases = [('alpha', 0, dict(alpha=0.5), lambda: dict(alpha=0.5)),
             ('alpha+bias+relu', BIAS | RELU, dict(alpha=0.5, bias=bias, act=G.ACT_RELU), lambda: dict(alpha=0.5, bias=bias_d)),
             ('bias+leaky', BIAS | LRELU, dict(bias=bias, act=G.ACT_LRELU, slope=0.2), lambda: dict(bias=bias_d, slope=0.2)),
             ('leaky', LRELU, dict(act=G.ACT_LRELU, slope=0.2), lambda: dict(slope=0.2))]
    _epi_sweep(S, p, cases)
    d = Prob.get('dx', (264, 132, 132), 1, mode)
    gate = G.draw_gate(16, (d.M, d.N))
    gate_d = _arena(gate, d.ldc)
    _epi_sweep(S, d, [('gate', GATE, dict(gate=gate), lambda: dict(gate=gate_d))])
    for q in (Prob.get('dw', (264, 132, 132), 1, mode), Prob.get('wgrad', (5, 8, 8, 32, 72), 9, mode)):
        prior = G.ints(17, (q.M, q.N), -6, 6) if mode == 'exact' else G.normal_f32(17, (q.M, q.N))
        _epi_sweep(S, q, [('accumulate', ACCUM, dict(prior=prior), lambda: dict(prior=prior))])


@pytest.mark.parametrize('mode', ('exact', 'random'))
def test_sgemm_g_and_grp_epilogues(S, mode):
    """The resampling convs with bias + leaky 0.2 (the parity groups share one bias), the grouped launches with a
    bias per group + ReLU."""
    for name in ('s2', 's2t'):
        p = Prob.get(name, (2, 8, 8, 32, 64), 16, mode)
        bias = G.draw_bias(mode, 25, p.N)
        bias_d = _arena(bias)
        _epi_sweep(S, p, [('bias+leaky', BIAS | LRELU, dict(bias=bias, act=G.ACT_LRELU, slope=0.2),
                           lambda: dict(bias=bias_d, slope=0.2)),
                          ('alpha+relu', RELU, dict(alpha=0.5, act=G.ACT_RELU), lambda: dict(alpha=0.5))])
    for full, shape, taps in (('dense_grp', (136, 72, 132), 1), ('conv_grp_shared', (2, 6, 6, 12, 40), 9)):
        p = Prob.get(full, shape, taps, mode)
        bias = torch.stack([G.draw_bias(mode, 30 + g, p.N) for g in range(3)])
        rows = bias.repeat_interleave(p.M, 0)            # group g's rows take bias[g]
        bias_d = _arena(bias)
        _epi_sweep(S, p, [('group bias + relu', BIAS | RELU, dict(bias=rows, act=G.ACT_RELU), lambda: dict(bias=bias_d)),
                          ('group bias + leaky', BIAS | LRELU, dict(bias=rows, act=G.ACT_LRELU, slope=0.2),
                           lambda: dict(bias=bias_d, slope=0.2))])


# -------------------------------------------------------------------------------------- 3. split-K
SPLIT_CASES = [('dense', (264, 132, 132), 1), ('dx', (264, 132, 132), 1), ('dw', (36, 20, 37), 1),
               ('conv', (3, 6, 6, 12, 40), 9), ('conv', (8, 6, 6, 32, 132), 9), ('wgrad', (3, 6, 6, 12, 40), 9),
               ('s2', (1, 12, 12, 24, 40), 16), ('s2t', (2, 8, 8, 32, 64), 16), ('s2w', (2, 8, 8, 32, 64), 16),
               ('s2w', (1, 12, 12, 24, 40), 16),
               ('dense_grp', (136, 72, 132), 1), ('conv_grp_shared', (2, 6, 6, 12, 40), 9)]


@pytest.mark.parametrize('mode', ('exact', 'wide_a', 'random'))
@pytest.mark.parametrize('name,shape,taps', SPLIT_CASES, ids=IDS)
def test_sgemm_split_k_slabs_and_combines(S, name, shape, taps, mode):
    """Splits 2, 3 and one count above the number of K-tiles (the empty splits write zero slabs), every slab
    against its own K range; then rk_reduce_slabs and rk_sreduce_epi (bias, each activation, alpha, gate, a bias
    per row block) on the slabs the kernel wrote."""
    p = Prob.get(name, shape, taps, mode)
    kt = G.cdiv(p.K, G.BK)
    for splits in (2, 3, kt + 3):
        rng = G.split_ranges(p.K, splits)
        slabs, Ss = p.ref(splits)
        for tile, nst in ((0, 2), (3, 3), (1 + X6, 3), (10 + X6, 2), (5, 2)):
            want = p.expected_status(tile, nst, 0, splits)
            st, got = p.launch(S, tile, nst, splits=splits)
            assert st == want, (p.tag, tile, nst, splits, st, want)
            if st != 0:
                continue
            for s, (lo, hi) in enumerate(rng):
                what = 'tile {} nst {} splits {} slab {}'.format(tile, nst, splits, s)
                if lo == hi:
                    assert bool((got[s] == 0).all()), what + ': an empty split must write zeros'
                    continue
                tol = G.n_terms(hi - lo, tile & X6) * G.U32 * Ss[s]
                judge(loop_tag(p, tile) + ' slab', got[s], slabs[s], tol, mode,
                      p.yard(lo, hi) if mode == 'random' else None, what)
    # the combines, on the slabs of one launch (3 splits, tile 3)
    splits = 3
    slabs, Ss = p.ref(splits)
    st, got = p.launch(S, 3, 2, splits=splits)
    assert st == 0
    slab_d = got.to(DEV, F32).contiguous()
    M, N = p.rows, p.N
    exact = mode != 'random'
    n = G.n_terms(p.K, False)
    prior = G.ints(41, (M, N), -5, 5)
    for acc, scale in ((False, 1.0), (True, 1.0), (False, 0.5)):
        out = torch.full((M, N), NAN, device=DEV) if not acc else prior.to(DEV, F32)
        S.reduce_slabs(slab_d, out, accumulate=acc, scale=scale)
        r = G.reduce_epi(slabs, Ss, n, alpha=scale, prior=prior if acc else None)
        judge('rk_reduce_slabs', out, r['out'], r['tol'], mode, None, 'accumulate {} scale {}'.format(acc, scale))
        COUNT['ran'] += 1
    bias = _bias(mode, 42, N)
    gate = G.draw_gate(43, (M, N))
    G3 = 3 if M % 3 == 0 else 1
    brows = torch.stack([_bias(mode, 44 + g, N) for g in range(G3)])
    for what, kw, dkw in (
            ('plain', {}, {}),
            ('bias', dict(bias=bias), dict(bias=_arena(bias))),
            ('bias+relu', dict(bias=bias, act=G.ACT_RELU), dict(bias=_arena(bias), act=G.ACT_RELU)),
            ('bias+leaky', dict(bias=bias, act=G.ACT_LRELU, slope=0.2), dict(bias=_arena(bias), act=G.ACT_LRELU, slope=0.2)),
            ('alpha', dict(alpha=0.5), dict(alpha=0.5)),
            ('gate', dict(gate=gate), dict(gate=_arena(gate, N + 4))),
            ('bias_rows', dict(bias=brows.repeat_interleave(M // G3, 0)), dict(bias=_arena(brows), bias_rows=M // G3))):
        buf = _out_buf(M, N, N + 4)
        S.sreduce_epi(slab_d, M, N, buf[0, :M, :N], **dkw)
        r = G.reduce_epi(slabs, Ss, n, exact=exact, **kw)
        yard = G.epilogue32(p.yard(), **kw) if mode == 'random' else None
        judge('rk_sreduce_epi', _read_out(buf, M, N)[0], r['out'], r['tol'], mode, yard, what)
        COUNT['ran'] += 1


# -------------------------------------------------------------- 4. every offered candidate of every wrapper
def _grab(S, monkeypatch):
    seen = {}

    def grab(key, cands, run, protect=()):
        seen['cands'], seen['run'] = list(cands), run
        return cands[0]
    monkeypatch.setattr(S, '_pick', grab)
    return seen


def _run_candidates(S, seen, tag, out, ref, Ss, K, mode, yard, *, stats=None, sums=None, prior=None,
                    twice=False, ran=None):
    """Every candidate with cfg[0] >= 0 and every pre-split dense one (XPD_CFGS), each launched once (``twice``:
    and once more straight after, no sync between), against ref: exact sets bit for bit, RANDOM hard + yardstick."""
    prior_d = None if prior is None else prior.to(DEV, F32)
    for cfg in seen['cands']:
        xpd = cfg[0] == S.XP_DENSE
        if cfg[0] < 0 and not xpd:
            continue
        x6 = xpd or bool(cfg[0] & X6)
        ltag = '{} {}'.format(tag, 'x6p' if xpd else 'X6' if x6 else 'f32')
        if prior is None:
            out.fill_(NAN)
        else:
            out.copy_(prior.to(DEV, F32))
        if stats is not None:
            stats.zero_()
        seen['run'](cfg)
        results = [out.clone()]
        if twice:   # straight after, same buffer, no sync; the refill is a kernel on the same stream
            if prior is not None:
                out.copy_(prior_d)
            else:
                out.fill_(NAN)
            seen['run'](cfg)
            results.append(out)
        torch.cuda.synchronize()
        r = ref(G.n_terms(K, x6) + (cfg[2] - 1 if cfg[2] > 1 else 0))
        for i, got in enumerate(results):
            judge(ltag, got.reshape(r['out'].shape), r['out'], r['tol'], mode, yard, 'cfg {} launch {}'.format(cfg, i + 1))
        if sums is not None:
            judge(ltag + ' sums', stats.to('cpu').sum(0), r['sums'], r['sums_tol'], mode, None,
                  'cfg {} statistics'.format(cfg))
        COUNT['ran'] += len(results)
        if ran is not None:
            ran.append(cfg)
    assert any(c[0] >= 0 for c in seen['cands'])


def _ref(p, **kw):
    """n -> the reference through the epilogue, for a candidate whose accumulator takes n fp32 operations."""
    slabs, Ss = p.ref(1)
    return (lambda n: G.epilogue(slabs[0], Ss[0], n, exact=p.mode != 'random', **kw)), Ss[0]


def _bias(mode, seed, n):
    """igemm_refs' bias; on the wide sets (sums of 2^20 and more) whole numbers, so that the sum stays exact."""
    b = G.draw_bias('random' if mode == 'random' else 'exact', seed, n)
    return b * 4 if mode.startswith('wide') else b


CAND_MODES = ('exact', 'wide_a', 'wide_mm', 'random')


@pytest.mark.parametrize('mode', CAND_MODES)
@pytest.mark.parametrize('shape,taps', [((8, 6, 6, 32, 132), 9), ((3, 6, 6, 12, 40), 9), ((5, 8, 8, 32, 72), 1)], ids=IDS)
def test_conv_wrapper_candidates(S, monkeypatch, shape, taps, mode):
    """conv_fwd (plain; bias + ReLU with statistics), conv_dgrad (plain, BNB), conv_wgrad (plain, accumulate)."""
    seen = _grab(S, monkeypatch)
    Nb, H, W, Ci, Co = shape
    p = Prob.get('conv', shape, taps, mode)
    yard = p.yard() if mode == 'random' else None
    w2 = p.B[:, :p.K].contiguous()
    out = torch.empty((Nb, H, W, Co), device=DEV)
    S.conv_fwd(p.A, w2, taps=taps, out=out)
    r, Ss = _ref(p)
    _run_candidates(S, seen, 'conv_fwd', out, r, Ss, p.K, mode, yard)
    sums_exact = mode in ('exact', 'random')   # v^2 and v * y of the wide sets' 2^20 sums are no fp32 numbers
    if sums_exact:
        stats = torch.zeros(S.bn_slots(Co), 2, Co, dtype=F64, device=DEV)
        S.conv_fwd(p.A, w2, taps=taps, out=out, stats_acc=stats)
        r, Ss = _ref(p, stats=True)
        _run_candidates(S, seen, 'conv_fwd stats', out, r, Ss, p.K, mode, yard, stats=stats, sums=True)
    # data gradient = the same forward conv on (dy, wt): plain and into a BN + ReLU layer
    out = torch.empty((Nb, H, W, Co), device=DEV)
    S.conv_dgrad(p.A, w2, taps=taps, out=out)
    r, Ss = _ref(p)
    _run_candidates(S, seen, 'conv_dgrad', out, r, Ss, p.K, mode, yard)
    if sums_exact:
        scale, shift = G.draw_scale_shift(51, Co)
        y = G.draw_decision(52, (p.M, Co))
        assert G.decisions_inexact(y, scale, shift) == 0
        coeffs = _arena(torch.stack([scale, shift, scale, shift]))
        stats = torch.zeros(S.bn_slots(Co), 2, Co, dtype=F64, device=DEV)
        S.conv_dgrad(p.A, w2, taps=taps, out=out, bnb=(_arena(y.reshape(Nb, H, W, Co)), coeffs, stats))
        r, Ss = _ref(p, bnb=(y, scale, shift))
        _run_candidates(S, seen, 'conv_dgrad BNB', out, r, Ss, p.K, mode,
                        None if yard is None else yard * G.bnb_mask(y, scale, shift).to(F64), stats=stats, sums=True)
    q = Prob.get('wgrad', shape, taps, mode)
    yq = q.yard() if mode == 'random' else None
    out = torch.empty((q.M, q.N), device=DEV)
    S.conv_wgrad(q.A, q.B, taps=taps, out=out)
    r, Ss = _ref(q)
    _run_candidates(S, seen, 'conv_wgrad', out, r, Ss, q.K, mode, yq)
    prior = G.ints(53, (q.M, q.N), -6, 6)
    out.copy_(prior.to(DEV, F32))
    S.conv_wgrad(q.A, q.B, taps=taps, out=out, accumulate=True)
    r, Ss = _ref(q, prior=prior)
    _run_candidates(S, seen, 'conv_wgrad accumulate', out, r, Ss, q.K, mode, None if yq is None else G.epilogue32(yq, prior=prior),
                    prior=prior)


def _dense_wrappers(S, monkeypatch, shapes, mode, twice=False):
    """shapes: the (M, N, K) of the GEMM of each of 'dense', 'dx', 'dw'."""
    seen = _grab(S, monkeypatch)
    ran = {}
    M, N, K = shapes['dense']
    p = Prob.get('dense', shapes['dense'], 1, mode)
    A, B = _arena(p.a), _arena(p.b)          # the wrappers' pre-split path takes contiguous operands
    yard = p.yard() if mode == 'random' else None
    bias = _bias(mode, 61, N)
    out = torch.empty((M, N), device=DEV)
    S.linear(A, B, _arena(bias), act=S.ACT_RELU, out=out)
    r, Ss = _ref(p, bias=bias, act=G.ACT_RELU)
    yb = None if yard is None else G.epilogue32(yard, bias=bias, act=G.ACT_RELU)
    _run_candidates(S, seen, 'linear', out, r, Ss, K, mode, yb, twice=twice, ran=ran.setdefault('linear', []))
    M, N, K = shapes['dx']
    out = torch.empty((M, N), device=DEV)
    d = Prob.get('dx', shapes['dx'], 1, mode)
    A, B = _arena(d.a), _arena(d.b)
    gate = G.draw_gate(62, (M, N))
    S.linear_dx(A, B, gate=_arena(gate), out=out)
    r, Ss = _ref(d, gate=gate)
    yd = None if mode != 'random' else G.epilogue32(d.yard(), gate=gate)
    _run_candidates(S, seen, 'linear_dx', out, r, Ss, K, mode, yd, twice=twice, ran=ran.setdefault('linear_dx', []))
    M, N, K = shapes['dw']
    out = torch.empty((M, N), device=DEV)
    w = Prob.get('dw', shapes['dw'], 1, mode)
    A, B = _arena(w.a), _arena(w.b)
    yw = w.yard() if mode == 'random' else None
    S.linear_dw(A, B, out=out)
    r, Ss = _ref(w)
    _run_candidates(S, seen, 'linear_dw', out, r, Ss, K, mode, yw, twice=twice, ran=ran.setdefault('linear_dw', []))
    prior = G.ints(63, (M, N), -6, 6)
    out.copy_(prior.to(DEV, F32))
    S.linear_dw(A, B, out=out, accumulate=True)
    r, Ss = _ref(w, prior=prior)
    _run_candidates(S, seen, 'linear_dw accumulate', out, r, Ss, K, mode, None if yw is None else G.epilogue32(yw, prior=prior),
                    prior=prior, twice=twice)
    return ran


@pytest.mark.parametrize('mode', CAND_MODES)
@pytest.mark.parametrize('shape', [(264, 132, 132), (72, 40, 32)], ids=IDS)
def test_dense_wrapper_candidates(S, monkeypatch, shape, mode):
    """linear (bias + ReLU), linear_dx (gated), linear_dw (plain, accumulate) at the sweep's shapes."""
    _dense_wrappers(S, monkeypatch, dict.fromkeys(('dense', 'dx', 'dw'), shape), mode)


@pytest.mark.parametrize('mode', ('exact', 'random'))
def test_dense_wrapper_candidates_at_the_presplit_threshold(S, monkeypatch, mode):
    """The dense layer (batch, in, out) = (256, 2048, 512), the smallest at which the pre-split dense candidates
    (XPD_CFGS) are offered, with its operands as the layer has them: linear on x [256][2048], w [512][2048]
    (GEMM 256 x 512, K = 2048), linear_dx on dy [256][512], w (256 x 2048, K = 512), linear_dw on dy, x
    (512 x 2048, K = 256).  Every candidate is launched twice back to back into the same buffer (refilled on the
    stream in between, no sync), as a tuning sweep does, and both results are judged: per element on EXACT, by the
    hard tolerance and the yardstick on RANDOM."""
    ran = _dense_wrappers(S, monkeypatch, G.BIG_LAYER, mode, twice=True)
    for name, cfgs in ran.items():
        xpd = [c for c in cfgs if c[0] == S.XP_DENSE]
        assert not S.USE_X6P or len(xpd) == len(S.XPD_CFGS), (name, len(xpd))
        print('{} [{}]: {} candidates run twice ({} pre-split): {}'.format(name, mode, len(cfgs), len(xpd), cfgs))


@pytest.mark.parametrize('mode', CAND_MODES)
def test_resampling_and_grouped_wrapper_candidates(S, monkeypatch, mode):
    """s2_conv, s2t_conv (its weights regrouped on the device), s2_wgrad, conv_fwd_grp, linear_grp."""
    seen = _grab(S, monkeypatch)
    for shape in G.S2_SHAPES:
        Nb, H, W, Ci, Co = shape
        p = Prob.get('s2', shape, 16, mode)
        bias = _bias(mode, 71, Co)
        out = torch.empty((Nb, H // 2, W // 2, Co), device=DEV)
        S.s2_conv(p.A, p.B, bias=_arena(bias), act=S.ACT_LRELU, slope=0.2, out=out)
        r, Ss = _ref(p, bias=bias, act=G.ACT_LRELU, slope=0.2)
        yard = G.epilogue32(p.yard(), bias=bias, act=G.ACT_LRELU, slope=0.2) if mode == 'random' else None
        _run_candidates(S, seen, 's2_conv', out, r, Ss, p.K, mode, yard)
        t = Prob.get('s2t', shape, 16, mode)
        out = torch.empty((Nb, H, W, Ci), device=DEV)
        S.s2t_conv(t.A, _arena(t.b.reshape(Co, -1)), out=out)
        r, Ss = _ref(t)
        _run_candidates(S, seen, 's2t_conv', out, r, Ss, t.K, mode, t.yard() if mode == 'random' else None)
        w = Prob.get('s2w', shape, 16, mode)
        out = torch.empty((w.M, w.N), device=DEV)
        S.s2_wgrad(w.B, w.A, out=out)
        r, Ss = _ref(w)
        _run_candidates(S, seen, 's2_wgrad', out, r, Ss, w.K, mode, w.yard() if mode == 'random' else None)
    for full, shape, taps in [(k, s, t) for k in ('conv_grp', 'conv_grp_shared') for s, t in G.GRP_CONV] + \
                             [(k, s, 1) for k in ('dense_grp', 'dense_grp_shared') for s in G.GRP_DENSE]:
        p = Prob.get(full, shape, taps, mode)
        bias = torch.stack([_bias(mode, 80 + g, p.N) for g in range(3)])
        rows = bias.repeat_interleave(p.M, 0)
        x = _arena(p.a[0] if p.shared else p.a)        # the wrappers take contiguous operands
        if 'conv' in full:
            Nb, H, W, Ci, Co = shape
            out = torch.empty((3, Nb, H, W, Co), device=DEV)
            S.conv_fwd_grp(x, _arena(p.b.reshape(3, Co, p.K)), bias=_arena(bias), act=S.ACT_RELU, out=out)
        else:
            out = torch.empty((3, p.M, p.N), device=DEV)
            S.linear_grp(x, _arena(p.b), _arena(bias), act=S.ACT_RELU, out=out)
        r, Ss = _ref(p, bias=rows, act=G.ACT_RELU)
        yard = G.epilogue32(p.yard(), bias=rows, act=G.ACT_RELU) if mode == 'random' else None
        _run_candidates(S, seen, 'conv_fwd_grp' if 'conv' in full else 'linear_grp', out, r, Ss, p.K, mode, yard)
