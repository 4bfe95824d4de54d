"""rk_x6p_gemm (csrc/kernels/x6p.hip): every tile 0-12 with 32- and 64-deep K-tiles (tile + 16), both ring depths,
the warp-specialised variants, grouped, strided, broadcast, row-interleaved, accumulating and split-K launches
against the fp64 references of tests/pt_refs.py (anchored and shown to bite in tests/test_pt_refs.py).  The entry
point is called directly, each launch once.

Judging.  exact, wide_a, wide_b and wide_mm (sgemm_refs' sets: integers whose bf16 pieces reach hi, mid and lo of
either side and the mid * mid term) must come back bit for bit.  RANDOM is held element by element to
n_x6(K) * 2^-23 * S and, per output row and per output column, to sgemm_refs.YARD times the error of the same GEMM
accumulated in plain fp32 on the CPU.  Every split-K slab is judged against its own K range.

Guards.  The operands are bf16 planes 64 elements inside a larger bf16-NaN storage, with NaN in the lda - K padding
columns; bytesA / bytesB end exactly at the last plane.  The output is NaN-prefilled; the guard rows after every
group, the ldc - N padding columns, the columns between row-interleaved groups and the gaps between split-K slabs
must still be NaN.  A NaN in the output is an unwritten element or an over-read operand.

A launcher refusal (a ring that does not fit the LDS: 3 stages of tiles 7 / 8, 64-deep K-tiles of tiles 0, 7, 8, 9
at any depth and of 1, 2, 5, 6, 10, 11 at depth 3; 4 splits over 5 K-tiles) is predicted by pt_refs.expected_status
and asserted, never skipped.  Reached here and nowhere else in the suite: the KT = 64 instantiation of every kernel
(test_tiles_k_loops_and_arguments[*-64]), lda > K, ldb > K, ldc > N, gsA == 0, gsB == 0, K of one K-tile, row-interleaved groups with
guard columns.

The worst error / tolerance and yardstick ratio per tile and K-tile depth are printed at the end (pytest -s).

Measured on an MI355X, worst over the sweep (error / hard tolerance, yardstick ratio against the gate of 4); tiles
of one shape, warp-specialised or not, accumulate in the same order and gave the same figures:
    32-deep K-tiles   128x128 (tiles 0, 9) 0.0092, 1.28    128x64 (1, 5, 10) 0.0066, 1.55    64x128 (2, 6, 11) 0.0073, 1.48
                      64x64 (3, 4, 12) 0.0071, 1.62        256x128 (7) 0.0089, 1.63          128x256 (8) 0.0086, 1.29
    64-deep K-tiles   128x64 (1, 5, 10) 0.0058, 1.66       64x128 (2, 6, 11) 0.0038, 1.80    64x64 (3, 4, 12) 0.0040, 1.64
                      tiles 0, 7, 8, 9 are refused at either ring depth (two stages are 192 KiB and more)
2716 launches checked, 1158 refusals asserted; every exact and exact-wide set came back bit for bit, no guard element
was overwritten.  No kernel bug was found: the KT = 64 instantiations, which nothing had run, are right.
"""
import re

import pytest
import torch

import pt_refs as P
import sgemm_refs as G
import wino_refs as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
NAN = float('nan')
PAD = 64
COUNT = {}
ENTRY = 'rk_x6p_gemm'


@pytest.fixture(scope='module')
def S():
    from rafiki_amd.ops import _lib, f32
    _lib.lib()   # loud failure if the native library is missing
    yield f32
    Prob._cache.clear()
    for tag in sorted(COUNT):
        ran, refused = COUNT[tag]
        print('WORST {:34s} err / hard tol {:.4f}   yardstick ratio {:.3f}   launches {} refusals {}'.format(
            tag, R.WORST.get(tag, 0.0), R.YWORST.get(tag, 0.0), ran, refused))
    print('launches checked {}, refusals asserted {}'.format(sum(v[0] for v in COUNT.values()),
                                                             sum(v[1] for v in COUNT.values())))


@pytest.fixture(autouse=True)
def _stop_after_a_fault():
    """A kernel fault is sticky: end the session at the first one instead of launching on a faulted device."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:
        pytest.exit('GPU fault: {}'.format(exc), returncode=3)


def _count(tag, ran):
    c = COUNT.setdefault(tag, [0, 0])
    c[0 if ran else 1] += 1


def _status(fn):
    from rafiki_amd.ops._lib import KernelError
    try:
        fn()
    except KernelError as e:
        return int(re.search(r'status (-?\d+)', str(e)).group(1))
    return 0


def _arena(t, dtype):
    """Device copy of the flat t as a view PAD elements inside a NaN-filled storage that runs PAD past it."""
    buf = torch.full((2 * PAD + t.numel(),), NAN, dtype=dtype, device=DEV)
    v = buf[PAD:PAD + t.numel()]
    v.copy_(t.to(DEV, dtype))
    return v


class Prob:
    """Operands a [3][M][K], b [3][N][K] of one (mode, M, N, K) on the host; references and device planes per layout."""
    _cache = {}

    @classmethod
    def get(cls, mode, M, N, K):
        key = (mode, M, N, K)
        if key not in cls._cache:
            if len(cls._cache) > 24:
                cls._cache.clear()
            cls._cache[key] = cls(*key)
        return cls._cache[key]

    def __init__(self, mode, M, N, K):
        self.mode, self.M, self.N, self.K = mode, M, N, K
        self.a, self.b = P.gemm_problem(mode, M, N, K)
        if mode != 'random':
            assert P.exact_ok(torch.einsum('gmk,gnk->gmn', self.a.abs(), self.b.abs()))
        self._dev, self._ref, self._yard = {}, {}, {}

    def dev(self, which, groups, ld):
        key = (which, groups, ld)
        if key not in self._dev:
            t = (self.a if which == 'a' else self.b)[:groups]
            h = P.pack_planes(t, ld)
            self._dev[key] = (h, _arena(h, BF16))
        return self._dev[key]

    def yard(self, ga, gb):
        if (ga, gb) not in self._yard:
            self._yard[(ga, gb)] = G.yardstick(self.a[ga], self.b[gb])
        return self._yard[(ga, gb)]


def launch(S, tile, nst, p, L, *, accumulate=False, tag):
    """One launch under layout L; returns (status, the flat output on the host or None, the prior or None)."""
    from rafiki_amd.ops import _lib
    kt = 64 if tile >> 4 else 32
    ga, gb = (1 if L['gsA'] == 0 else L['groups']), (1 if L['gsB'] == 0 else L['groups'])
    (A_h, A_d), (B_h, B_d) = p.dev('a', ga, L['lda']), p.dev('b', gb, L['ldb'])
    assert A_h.numel() == L['sizeA'] and B_h.numel() == L['sizeB']
    buf = torch.full((L['sizeC'] + PAD,), NAN, dtype=F32, device=DEV)
    idx = P.c_index(L)
    prior = None
    if accumulate:
        prior = P.ints(5, idx.shape, -6, 6) if p.mode != 'random' else G.normal_f32(5, idx.shape)
        buf[idx.reshape(-1).to(DEV)] = prior.reshape(-1).to(DEV, F32)
    want = P.expected_status(ENTRY, tile=tile, nst=nst, flags=int(accumulate),
                             **{k: L[k] for k in ('M', 'N', 'K', 'groups', 'splits', 'lda', 'ldb', 'ldc', 'psA', 'psB',
                                                  'gsA', 'gsB', 'gsC', 'slabStride', 'bytesA', 'bytesB')})
    st = _status(lambda: _lib.call(ENTRY, tile, nst, S._p(A_d), S._p(B_d), S._p(buf), L['M'], L['N'], L['K'], L['lda'],
                                   L['ldb'], L['ldc'], L['psA'], L['psB'], L['gsA'], L['gsB'], L['gsC'], L['groups'],
                                   int(accumulate), L['splits'], L['slabStride'], L['bytesA'], L['bytesB'], S._s()))
    what = 'tile {} nst {} {} {}'.format(tile, nst, p.mode, {k: v for k, v in L.items() if not k.startswith('size')})
    assert st == want, '{}: status {} (expected {})'.format(what, st, want)
    if st != 0:
        assert accumulate or bool(torch.isnan(buf).all()), 'a refused launch wrote something'
        _count(tag, False)
        return st, None, None
    torch.cuda.synchronize()
    _count(tag, True)
    host = buf.to('cpu', F64)
    assert P.guards_ok(host, idx), '{}: wrote outside the output (guard rows, padding columns or slab gaps)'.format(what)
    acc, Sg = P.gemm_planes(A_h, B_h, L, kt)
    got = host[idx]
    rng = P.slab_ranges(L['K'], kt, L['splits'])
    for s, (k0, k1) in enumerate(rng):
        for g in range(L['groups']):
            ref, Ssg, n = acc[s, g], Sg[s, g], P.n_x6(k1 - k0)
            yard = None
            if p.mode == 'random':
                ia, ib = (0 if L['gsA'] == 0 else g), (0 if L['gsB'] == 0 else g)
                yard = p.yard(ia, ib) if L['splits'] == 1 else G.yardstick(p.a[ia][:, k0:k1], p.b[ib][:, k0:k1])
            if prior is not None:
                ref, Ssg, n = ref + prior[s, g], Ssg + prior[s, g].abs(), n + 1
                yard = None if yard is None else G.f32r(yard + prior[s, g])
            P.judge_mat(tag, got[s, g], ref, P.tol_of(n, Ssg), p.mode, yard, '{} slab {} group {}'.format(what, s, g))
    return 0, host, prior


@pytest.mark.parametrize('kt', (32, 64))
@pytest.mark.parametrize('tile', range(13))
def test_tiles_k_loops_and_arguments(S, tile, kt):
    """One tile at one K-tile depth: (1, 8), (BM - 1, BN + 1) and more than one block each way, K of 1, 2, 3 and 5
    K-tiles (fewer than the ring prologue, equal to it, one wrap, a wrap for both depths), ring depths 2 and 3, all
    five input sets; then, on (BM - 1, BN + 1) over 5 K-tiles: 3 groups, lda = K + 8 with ldc = N + 4, broadcast B,
    broadcast A, row-interleaved groups, accumulate, split-K 2 and 3 (the last split gets one K-tile) and the
    refused 4 splits."""
    t = tile + (16 if kt == 64 else 0)
    tag = '{} tile {:2d} kt {}'.format(ENTRY, tile, kt)
    shapes = P.gemm_shapes(tile)
    for si, (M, N) in enumerate(shapes):
        for nk in P.K_TILES:
            for mode in G.MODES:
                p = Prob.get(mode, M, N, nk * kt)
                for nst in (2, 3):
                    launch(S, t, nst, p, P.gemm_layout(M, N, nk * kt, 1), tag=tag)
    M, N = shapes[1]
    K = 5 * kt
    for mode in ('exact', 'random'):
        p = Prob.get(mode, M, N, K)
        for kw in (dict(), dict(lda=K + 8, ldc=N + 4), dict(bcast_b=True), dict(bcast_a=True), dict(interleave=True),
                   dict(interleave=True, bcast_b=True, ldc=3 * (N + 4) + 5)):
            launch(S, t, 2, p, P.gemm_layout(M, N, K, 3, **kw), tag=tag)
        launch(S, t, 3, p, P.gemm_layout(M, N, K, 3, lda=K + 8, ldb=K + 16), tag=tag)
        launch(S, t, 2, p, P.gemm_layout(M, N, K, 1), accumulate=True, tag=tag)
        launch(S, t, 2, p, P.gemm_layout(M, N, K, 3, ldc=N + 4), accumulate=True, tag=tag)
        for splits, kw in ((2, dict()), (3, dict()), (3, dict(interleave=True)), (2, dict(ldc=N + 4, bcast_b=True)),
                           (4, dict())):
            L = P.gemm_layout(M, N, K, 3, splits=splits, **kw)
            st, _, _ = launch(S, t, 2, p, L, tag=tag)
            if splits == 4:
                assert st == -1


def test_launcher_refusals(S):
    """Every argument check of rk_x6p_gemm once on valid small tensors, with the status expected_status predicts."""
    p = Prob.get('exact', 63, 65, 64)
    base = P.gemm_layout(63, 65, 64, 2)
    seen = set()
    for tile, nst, change in (
            (0, 4, {}), (13, 2, {}), (29, 2, {}), (32, 2, {}), (-1, 2, {}), (0, 2, dict(M=0)), (0, 2, dict(groups=0)),
            (0, 2, dict(splits=0)), (0, 2, dict(splits=2, slabStride=base['gsC'])),
            (0, 2, dict(K=48)), (19, 2, dict(K=32)), (0, 2, dict(lda=68)), (0, 2, dict(ldb=60)), (0, 2, dict(lda=56)),
            (0, 2, dict(psA=63 * 64 - 1)), (0, 2, dict(bytesB=0)), (0, 2, dict(ldc=64)),
            (0, 2, dict(gsA=3 * 63 * 64 - 8)), (0, 2, dict(gsC=60, ldc=128)), (0, 2, dict(gsC=66, ldc=130)),
            (0, 2, dict(bytesA=base['bytesA'] - 2)), (0, 2, dict(bytesB=base['bytesB'] - 2)),
            (7, 3, {}), (16, 2, {}), (17, 3, {}), (25, 2, {})):
        L = dict(base, **change)
        want = P.expected_status(ENTRY, tile=tile, nst=nst, **{k: v for k, v in L.items() if not k.startswith('size')})
        assert want != 0, (tile, nst, change)
        from rafiki_amd.ops import _lib
        (_, A_d), (_, B_d) = p.dev('a', 2, 64), p.dev('b', 2, 64)
        buf = torch.full((base['sizeC'] + PAD,), NAN, dtype=F32, device=DEV)
        st = _status(lambda: _lib.call(ENTRY, tile, nst, S._p(A_d), S._p(B_d), S._p(buf), L['M'], L['N'], L['K'],
                                       L['lda'], L['ldb'], L['ldc'], L['psA'], L['psB'], L['gsA'], L['gsB'], L['gsC'],
                                       L['groups'], 0, L['splits'], L['slabStride'], L['bytesA'], L['bytesB'], S._s()))
        assert st == want, (tile, nst, change, st, want)
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf).all()), 'a refused launch wrote something'
        _count(ENTRY + ' refusals', False)
        seen.add(want)
    assert seen == {-1, -2}
