"""The references of tests/pt_refs.py are anchored (composed, they are the convolution and its weight gradient), their
absolute-value companions bound them, the exact and wide sets are exact and reach every bf16 piece, and the judges of
tests/test_x6p_gemm_gpu.py / tests/test_wino_pt_gpu.py bite: wrong kernels written as mutants of the references are
rejected at the sweep shapes under the judge and tolerance used there.  A mutant is asserted on every sweep shape it
changes anything on (tiles in (n, tx, ty) order is the identity where a map is one tile high or wide: it is caught
on (2, 8, 16), and asserted to be the identity elsewhere).  expected_status is held to a hand-worked table with a
case for every return line of every launcher.  CPU only."""
import pytest
import torch
import torch.nn.functional as TF

import pt_refs as P
import sgemm_refs as G
import wino_refs as R

F64, F32 = torch.float64, torch.float32
IDS = lambda v: '-'.join(map(str, v)) if isinstance(v, tuple) else str(v)   # noqa: E731
CASES = [s + (c,) for s in P.SPATIAL for c in P.CHANNELS]


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _rand(seed, shape, scale=1.0):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed), dtype=F64) * scale


def _rejected(fn, *a, **kw):
    try:
        fn('mutant', *a, **kw)
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------- anchors
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_stages_compose_to_the_convolution(case):
    """v_of -> 36 GEMMs -> conv_out (position- and tile-major, one and three slabs) against wino_refs.fused_conv and
    conv2d; m_of / v_of -> sum over tiles -> wgrad_out against wino_refs.fused_wgrad and autograd."""
    Nb, H, W, C = case
    N, T = C + 4, P.tiles(Nb, H, W)
    x, w, dy = _rand(1, (Nb, H, W, C)), _rand(2, (N, 9, C), (9 * C) ** -0.5), _rand(3, (Nb, H, W, N))
    xd = _nchw(x).clone().requires_grad_(True)
    wd = w.reshape(N, 3, 3, C).permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = TF.conv2d(xd, wd, padding=1)
    gw = torch.autograd.grad(y, wd, _nchw(dy))[0].permute(0, 2, 3, 1).reshape(N, 9, C)
    y = y.detach().permute(0, 2, 3, 1)
    U = R.transform_weights(w, 4)
    V = P.v_of(x)
    assert V.shape == (36, T, C)
    Yp = torch.einsum('qtc,qnc->qtn', V, U)
    for tmajor in (0, 1):
        flat = (Yp.permute(1, 0, 2) if tmajor else Yp).reshape(-1)
        got = P.conv_out(flat, Nb, H, W, N, tmajor=tmajor)['out']
        assert (got - y).abs().max() < 1e-12 and (got - R.fused_conv(x, U, 4)).abs().max() < 1e-12
        slab = 36 * T * N + 20
        buf = torch.full((2 * slab + 36 * T * N,), float('nan'), dtype=F64)
        parts = [_rand(4, flat.shape), _rand(5, flat.shape)]
        for k, p in enumerate(parts + [flat - parts[0] - parts[1]]):
            buf[k * slab:k * slab + flat.numel()] = p
        got = P.conv_out(buf, Nb, H, W, N, nslab=3, slab=slab, tmajor=tmajor)['out']
        assert (got - y).abs().max() < 1e-12
    M = P.m_of(dy)
    assert M.shape == (36, T, N)
    dU = torch.einsum('qtk,qtc->qkc', M, V)
    got = P.wgrad_out(dU.reshape(-1), N, C)
    ref, _ = R.fused_wgrad(dy, x, 4)
    assert (got - gw).abs().max() < 1e-12 * Nb * H * W and (got - ref[0]).abs().max() < 1e-12 * Nb * H * W
    prior = _rand(6, (N, 9, C))
    got = P.wgrad_out(dU.reshape(-1), N, C, accumulate=True, prior=prior)
    assert (got - gw - prior).abs().max() < 1e-12 * Nb * H * W


def test_normalise_on_load_anchor():
    Nb, H, W, C = 3, 4, 12, 8
    x, pro = _rand(7, (Nb, H, W, C)), R.draw_pro('random', 8, C)
    xn = (x * pro[0] + pro[1]).clamp_min(0)
    assert (P.v_of(x, pro) - P.v_of(xn)).abs().max() < 1e-12
    assert (P.v_of(x, pro) - P.v_of(x, pro, mutant='pad_relu_shift')).abs().max() > 1e-3


def test_planes_sum_back_and_split_once():
    for mode in ('exact', 'wide', 'random'):
        t = P.draw_mat(mode, 3, (5, 7, 9))
        p = P.planes(t)
        assert p.shape == (5, 3, 7, 9) and torch.equal(P.unplanes(p), t)
        for k in range(3):   # a piece is a bf16 value: splitting it again gives (piece, 0, 0)
            q = P.planes(p[:, k])
            assert torch.equal(q[:, 0], p[:, k]) and not bool(q[:, 1:].any())
        assert torch.equal(P.planes_t(t)[:, 1], p[:, 1].transpose(-1, -2))
    assert P.pieces_used(P.draw_mat('wide', 3, (40, 40)))[1] > 0.3


@pytest.mark.parametrize('kt', (32, 64))
def test_gemm_planes_is_the_product_and_its_slabs_sum(kt):
    M, N, K = 37, 21, 5 * kt
    a, b = P.gemm_problem('random', M, N, K)
    for kw in (dict(), dict(lda=K + 8, ldc=N + 4), dict(bcast_b=True), dict(interleave=True)):
        L = P.gemm_layout(M, N, K, 3, **kw)
        A = P.pack_planes(a, L['lda'])
        B = P.pack_planes(b[:1] if kw.get('bcast_b') else b, L['ldb'])
        assert A.numel() == L['sizeA'] and B.numel() == L['sizeB']
        acc, S = P.gemm_planes(A, B, L, kt)
        for g in range(3):
            bb = b[0 if kw.get('bcast_b') else g]
            assert bool(((acc[0, g] - a[g] @ bb.t()).abs() <= 2.0 ** -25 * S[0, g]).all())
            assert torch.equal(acc[0, g], G.x6_gemm(a[g], bb))
            assert bool((S[0, g] >= (a[g].abs() @ bb.abs().t()) * (1 - 1e-12)).all())
        for splits in (2, 3):
            Ls = P.gemm_layout(M, N, K, 3, splits=splits, **kw)
            accs, Ss = P.gemm_planes(A, B, Ls, kt)
            assert accs.shape[0] == splits and (accs.sum(0) - acc[0]).abs().max() < 1e-12
            assert (Ss.sum(0) - S[0]).abs().max() < 1e-9
            idx = P.c_index(Ls).reshape(-1)
            assert idx.unique().numel() == idx.numel() and int(idx.max()) < Ls['sizeC']
        assert P.slab_ranges(K, kt, 4) is None and P.slab_ranges(K, kt, 3)[-1] == (4 * kt, 5 * kt)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_absolute_companions_bound_and_tolerances_dominate_fp32(case):
    """|stage| <= S, and the same stage in plain fp32 is within n 2^-23 S of the fp64 one."""
    Nb, H, W, C = case
    T = P.tiles(Nb, H, W)
    x, dy, pro = P.draw_x('random', 1, case), P.draw_dy('random', 2, case), R.draw_pro('random', 3, max(C, 8))
    pro = (pro[0][:C], pro[1][:C])
    for ref, S, n, y32 in (
            (P.v_of(x), P.v_of(x, absval=True), P.N_BT6, P.v_of(x.to(F32))),
            (P.v_of(x, pro), P.v_of(x, pro, absval=True), P.N_BT6 + P.N_PRO,
             P.v_of((x.to(F32) * pro[0].to(F32) + pro[1].to(F32)).clamp_min(0))),
            (P.m_of(dy), P.m_of(dy, absval=True), P.N_A6, P.m_of(dy.to(F32)))):
        assert bool((ref.abs() <= S * (1 + 1e-12)).all())
        assert bool(((y32.to(F64) - ref).abs() <= P.tol_of(n, S)).all())
    yt = P.draw_yt('random', 4, 36 * T * C)
    r = P.conv_out(yt, Nb, H, W, C)
    assert bool((r['acc'].abs() <= r['S'] * (1 + 1e-12)).all())
    AT = R.mats(4, dtype=F32)[1]
    y32 = torch.einsum('pi,ijnyxk,qj->nypxqk', AT, yt.to(F32).reshape(6, 6, Nb, H // 4, W // 4, C), AT)
    assert bool(((y32.reshape(Nb, H, W, C).to(F64) - r['out']).abs() <= r['tol']).all())
    du = P.draw_yt('random', 5, 36 * C * C)
    ref, S = P.wgrad_out(du, C, C), P.wgrad_out(du, C, C, absval=True)
    Gm = R.mats(4, dtype=F32)[2]
    w32 = torch.einsum('iy,ijkc,jx->kyxc', Gm, du.to(F32).reshape(6, 6, C, C), Gm).reshape(C, 9, C)
    assert bool((ref.abs() <= S * (1 + 1e-12)).all())
    assert bool(((w32.to(F64) - ref).abs() <= P.tol_of(P.n_wgrad_out(), S)).all())


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_exact_and_wide_sets_are_exact_and_reach_every_piece(case):
    Nb, H, W, C = case
    pro = R.draw_pro('exact', 3, max(C, 8))
    pro = (pro[0][:C], pro[1][:C])
    for mode in ('exact', 'wide'):
        x, dy = P.draw_x(mode, 1, case), P.draw_dy(mode, 2, case)
        for v, S in ((P.v_of(x), P.v_of(x, absval=True)), (P.v_of(x, pro), P.v_of(x, pro, absval=True)),
                     (P.m_of(dy), P.m_of(dy, absval=True))):
            assert P.exact_ok(S) and torch.equal(v, v.round()) and torch.equal(P.f32r(v), v)
            if mode == 'wide':
                mid, lo = P.pieces_used(v)
                assert mid > 0.3 and lo > 0.05, (mid, lo)
    yt = P.draw_yt('exact', 4, 36 * P.tiles(Nb, H, W) * C)
    r = P.conv_out(yt, Nb, H, W, C)
    assert P.exact_ok(3 * r['S'] + 3.0)


def test_wide_gemm_sets_reach_the_pieces():
    """Every (shape, K, set) of the GEMM sweep keeps S below 2^24; the wide sets reach the pieces they are for."""
    shapes = sorted({s for tile in range(13) for s in P.gemm_shapes(tile)})
    for M, N in shapes:
        for K in sorted({nk * kt for nk in P.K_TILES for kt in (32, 64)}):
            for mode in G.EXACT_MODES:
                a, b = P.gemm_problem(mode, M, N, K)
                assert P.exact_ok(torch.einsum('gmk,gnk->gmn', a.abs(), b.abs())), (mode, M, N, K)
                if M * K < 2000:
                    continue
                ua, ub = P.pieces_used(a), P.pieces_used(b)
                if mode == 'wide_a':
                    assert ua[1] > 0.3
                if mode == 'wide_b':
                    assert ub[1] > 0.3
                if mode == 'wide_mm':
                    assert ua[0] > 0.3 and ub[0] > 0.3


# ------------------------------------------------------------------------------------------ mutants
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_transform_mutants_are_rejected(case):
    """q = b * 6 + a, tiles in (n, tx, ty) order, H and W swapped in the decode, the padding normalised: on the
    exact set (bit for bit) and on RANDOM under the stage's hard tolerance."""
    Nb, H, W, C = case
    square_free = H // 4 > 1 and W // 4 > 1
    pro = R.draw_pro('exact', 3, max(C, 8))
    pro = (pro[0][:C], pro[1][:C])
    for mode in ('exact', 'wide', 'random'):
        x, dy = P.draw_x(mode, 1, case), P.draw_dy(mode, 2, case)
        for fn, t, n in ((P.v_of, x, P.N_BT6), (P.m_of, dy, P.N_A6)):
            ref, tol = fn(t), P.tol_of(n, fn(t, absval=True))
            P.judge('ok', ref, ref, tol, mode)
            for mu in ('q_swap', 'hw_swap', 'tile_order'):
                bad = fn(t, mutant=mu)
                if mu == 'tile_order' and not square_free:
                    assert torch.equal(bad, ref)
                    continue
                assert _rejected(P.judge, bad, ref, tol, mode), (mu, mode)
                assert _rejected(P.judge_planes, P.planes(bad), ref, tol, mode), (mu, mode)
            if mode != 'exact':      # the exact set's values are one bf16 piece: the wide set is what tells the planes apart
                assert _rejected(P.judge_planes, P.planes(ref, mutant='plane_order'), ref, tol, mode)
        p = pro if mode != 'random' else tuple(v[:C] for v in R.draw_pro('random', 3, max(C, 8)))
        ref, tol = P.v_of(x, p), P.tol_of(P.N_BT6 + P.N_PRO, P.v_of(x, p, absval=True))
        assert _rejected(P.judge, P.v_of(x, p, mutant='pad_relu_shift'), ref, tol, mode)


def _conv_out_inputs(mode, Nb, H, W, N, nslab, slab):
    T = P.tiles(Nb, H, W)
    yt = P.with_slabs(P.draw_yt(mode, 1, 36 * T * N), nslab, slab, 2, mode)
    bias = R.draw_bias(mode, 3, N)
    scale, shift = G.draw_scale_shift(4, N)
    return yt, bias, (scale, shift), G.draw_decision(5, (Nb * H * W, N)), G.draw_pool_y(6, Nb, H, W, N, scale)


@pytest.mark.parametrize('N', (5, 6, 67, 70))
@pytest.mark.parametrize('sp', P.SPATIAL, ids=IDS)
def test_output_transform_mutants_are_rejected(sp, N):
    Nb, H, W = sp
    T = P.tiles(Nb, H, W)
    slab = 36 * T * N + 64
    for mode in ('exact', 'random'):
        yt, bias, ss, y, y2 = _conv_out_inputs(mode, Nb, H, W, N, 3, slab)
        kw = dict(nslab=3, slab=slab, exact=mode != 'random')
        for tmajor in (0, 1):
            ref = P.conv_out(yt, Nb, H, W, N, tmajor=tmajor, **kw)
            mus = ['q_swap', 'tmajor', 'last_slab_dropped', 'slab_stride'] + (['tile_order'] if H > 4 and W > 4 else [])
            for mu in mus:
                bad = P.conv_out(yt, Nb, H, W, N, tmajor=tmajor, mutant=mu, **kw)['out']
                assert _rejected(P.judge, bad, ref['out'], ref['tol'], mode), (mu, mode, tmajor)
        for flags in (R.STATS | R.RELU, R.BIAS | R.RELU | R.STATS):
            ref = P.conv_out(yt, Nb, H, W, N, flags, bias=bias, **kw)
            bad = P.conv_out(yt, Nb, H, W, N, flags, bias=bias, mutant='stats_after_act', **kw)
            v = ref['acc'].reshape(-1, N) + (bias if flags & R.BIAS else 0.0)
            P.judge_sums('ok', ref['sums'], ref['sums'], ref['sums_tol'], mode, v)
            assert _rejected(P.judge_sums, bad['sums'], ref['sums'], ref['sums_tol'], mode, v), (mode, flags)
        ref = P.conv_out(yt, Nb, H, W, N, R.BNP, bias=ss, gate=y2, **kw)
        bad = P.conv_out(yt, Nb, H, W, N, R.BNP, bias=ss, gate=y2, mutant='bnp_last_max', **kw)
        pos, yb = G.bnp_route(y2, ss[0], ss[1], Nb, H, W)
        v = ref['out'].reshape(-1, N) * pos.to(F64)
        # the last maximum instead of the first cannot be seen here: the kernel forms only (sum dz, sum dz * y_best), and
        # tied maxima of relu(y * scale + shift) share their y or are zero (tests/test_sgemm_refs.py says the same of
        # the fp32 engine); routing on y instead of relu(z) is the BNP mutant that shows, and it is rejected
        assert torch.equal(bad['sums'], ref['sums'])
        bad = P.conv_out(yt, Nb, H, W, N, R.BNP, bias=ss, gate=y2, mutant='bnp_route_on_y', **kw)
        assert _rejected(P.judge_sums, bad['sums'], ref['sums'], ref['sums_tol'], mode, v, '', yb, 1.0 / 64)
        # a statistic that counts an element twice, against the output of the same launch
        ref = P.conv_out(yt, Nb, H, W, N, R.STATS, **kw)
        own = P.own_sums(ref['out'])
        twice = ref['sums'] + torch.stack([ref['out'][0, 0, 0], ref['out'][0, 0, 0] ** 2])
        P.judge_sums('ok', ref['sums'], own[0], own[1], mode, ref['out'].reshape(-1, N))
        assert _rejected(P.judge_sums, twice, own[0], own[1], mode, ref['out'].reshape(-1, N))


@pytest.mark.parametrize('Co,Ci', [(4, 8), (12, 4), (40, 12), (8, 40)])
def test_weight_gradient_output_mutants_are_rejected(Co, Ci):
    slab = 36 * Co * Ci + 64
    prior = G.normal_f32(9, (Co, 9, Ci))
    for kind in ('random', 'onehot'):
        if kind == 'random':
            du = P.with_slabs(P.draw_yt('random', 1, 36 * Co * Ci), 3, slab, 2, 'random')
        else:
            du = P.with_slabs(torch.zeros(36 * Co * Ci, dtype=F64), 3, slab, 2, 'exact')
            du[(7 * Co + Co - 1) * Ci + 1] = 1.0
        kw = dict(nslab=3, slab=slab, accumulate=True, prior=prior)
        ref = P.wgrad_out(du, Co, Ci, **kw)
        tol = P.tol_of(P.n_wgrad_out(3, True), P.wgrad_out(du, Co, Ci, absval=True, **kw))
        P.judge('ok', ref, ref, tol, 'random')
        for mu in ('q_swap', 'last_slab_dropped', 'slab_stride', 'no_accumulate'):
            bad = P.wgrad_out(du, Co, Ci, mutant=mu, **kw)
            assert _rejected(P.judge, bad, ref, tol, 'random', None, '', 'wgrad'), (mu, kind)


@pytest.mark.parametrize('tile', range(13))
def test_gemm_mutants_are_rejected(tile):
    """One X6 term dropped (each of the six: by the exact-wide set that reaches it bit for bit, and on RANDOM by the
    hard tolerance or the yardstick), a K-tile read from the previous ring stage, row M of a group written into the
    next group, accumulate ignored."""
    reach = dict(hh='exact', hm='wide_b', mh='wide_a', hl='wide_b', lh='wide_a', mm='wide_mm')
    for kt in (32, 64):
        M, N = P.gemm_shapes(tile)[2]
        K = 5 * kt
        L = P.gemm_layout(M, N, K, 1)
        for mode in G.MODES:
            a, b = P.gemm_problem(mode, M, N, K, groups=1)
            A, B = P.pack_planes(a, K), P.pack_planes(b, K)
            ref, S = P.gemm_planes(A, B, L, kt)
            tol = P.tol_of(P.n_x6(K), S)
            yard = G.yardstick(a[0], b[0]) if mode == 'random' else None
            P.judge_mat('ok', ref[0, 0], ref[0, 0], tol[0, 0], mode, yard)
            for t in P.X6_TERMS:
                if mode in (reach[t], 'random'):
                    bad, _ = P.gemm_planes(A, B, L, kt, drop=t)
                    assert _rejected(P.judge_mat, bad[0, 0], ref[0, 0], tol[0, 0], mode, yard), (t, mode, kt)
            if mode in ('exact', 'random'):
                bad, _ = P.gemm_planes(A, B, L, kt, mutant='stale_stage')
                assert _rejected(P.judge_mat, bad[0, 0], ref[0, 0], tol[0, 0], mode, yard), (mode, kt)
    M, N = P.gemm_shapes(tile)[1]
    for kw in (dict(), dict(ldc=N + 4), dict(interleave=True)):
        L = P.gemm_layout(M, N, 32, 3, **kw)
        vals = _rand(1, (1, 3, M, N))
        idx = P.c_index(L)
        assert P.guards_ok(P.place_c(vals, L), idx)
        if not kw.get('interleave'):
            assert not P.guards_ok(P.place_c(vals, L, mutant='row_spill'), idx)
    L = P.gemm_layout(M, N, 32, 3)
    prior = _rand(2, (1, 3, M, N))
    good, bad = P.place_c(vals, L, prior), P.place_c(vals, L, prior, mutant='no_accumulate')
    idx = P.c_index(L)
    assert _rejected(P.judge_mat, bad[idx][0, 1], good[idx][0, 1], 1e-6 * torch.ones(M, N, dtype=F64), 'random')


# --------------------------------------------------------------------------------- expected statuses
def test_expected_status_table():
    """Hand-worked: one case and more for every return line of every launcher."""
    E = P.expected_status
    g = dict(M=64, N=64, K=64)
    table = [
        ('rk_x6p_gemm', dict(tile=0, **g), 0),
        ('rk_x6p_gemm', dict(tile=0, M=0, N=64, K=64), -1), ('rk_x6p_gemm', dict(tile=0, nst=4, **g), -1),
        ('rk_x6p_gemm', dict(tile=13, **g), -1), ('rk_x6p_gemm', dict(tile=29, **g), -1),
        ('rk_x6p_gemm', dict(tile=32, **g), -1), ('rk_x6p_gemm', dict(tile=-1, **g), -1),
        ('rk_x6p_gemm', dict(tile=0, splits=0, **g), -1), ('rk_x6p_gemm', dict(tile=0, groups=0, **g), -1),
        ('rk_x6p_gemm', dict(tile=0, splits=2, flags=1, slabStride=4096, **g), -1),     # split-K cannot accumulate
        ('rk_x6p_gemm', dict(tile=0, splits=2, slabStride=4095, **g), -1),              # slabs overlap
        ('rk_x6p_gemm', dict(tile=0, splits=2, slabStride=4096, **g), 0),
        ('rk_x6p_gemm', dict(tile=0, M=64, N=64, K=48), -2),                            # K % 32
        ('rk_x6p_gemm', dict(tile=19, M=64, N=64, K=96), -2),                           # K % 64 with tile + 16
        ('rk_x6p_gemm', dict(tile=0, lda=68, **g), -2), ('rk_x6p_gemm', dict(tile=0, ldb=56, **g), -2),
        ('rk_x6p_gemm', dict(tile=0, lda=72, **g), 0),
        ('rk_x6p_gemm', dict(tile=0, psA=4095, **g), -1), ('rk_x6p_gemm', dict(tile=0, bytesB=0, **g), -1),
        ('rk_x6p_gemm', dict(tile=0, ldc=63, **g), -2),
        ('rk_x6p_gemm', dict(tile=0, M=1 << 20, N=512, K=32), -2),                      # C of 2 GiB
        ('rk_x6p_gemm', dict(tile=0, M=1 << 19, N=8, K=1024), -2),                      # three A planes of 2 GiB
        ('rk_x6p_gemm', dict(tile=0, groups=2, gsA=4096, **g), -1),                     # groups overlap in A
        ('rk_x6p_gemm', dict(tile=0, groups=2, gsB=0, **g), 0),                         # broadcast B
        ('rk_x6p_gemm', dict(tile=0, groups=2, gsC=64, ldc=64, **g), -1),               # interleaved, ldc too small
        ('rk_x6p_gemm', dict(tile=0, groups=2, gsC=64, ldc=128, **g), 0),
        ('rk_x6p_gemm', dict(tile=0, groups=2, gsC=32, ldc=128, **g), -1),
        ('rk_x6p_gemm', dict(tile=0, bytesA=2 * 3 * 4096 - 2, **g), -1),                # the last plane is cut short
        ('rk_x6p_gemm', dict(tile=0, bytesA=2 * 3 * 4096, **g), 0),
        ('rk_x6p_gemm', dict(tile=0, M=64, N=64, K=160, splits=4, slabStride=4096), -1),  # 5 K-tiles: 2 + 2 + 1
        ('rk_x6p_gemm', dict(tile=0, M=64, N=64, K=160, splits=3, slabStride=4096), 0),
        ('rk_x6p_gemm', dict(tile=0, nst=3, **g), 0),        # 3 x 48 KiB
        ('rk_x6p_gemm', dict(tile=7, nst=3, **g), -2),       # 3 x 72 KiB
        ('rk_x6p_gemm', dict(tile=7, nst=2, **g), 0),
        ('rk_x6p_gemm', dict(tile=16, **g), -2),             # 64-deep 128 x 128: 2 x 96 KiB
        ('rk_x6p_gemm', dict(tile=17, **g), 0), ('rk_x6p_gemm', dict(tile=17, nst=3, **g), -2),
        ('rk_x6p_gemm', dict(tile=19, nst=3, **g), 0), ('rk_x6p_gemm', dict(tile=28, nst=3, **g), 0),
        ('rk_x6p_gemm', dict(tile=23, **g), -2), ('rk_x6p_gemm', dict(tile=25, **g), -2),
        ('rk_x6p_split', dict(rows=3, cols=5), 0), ('rk_x6p_split', dict(rows=3, cols=5, ldd=8), 0),
        ('rk_x6p_split', dict(rows=0, cols=5), -1), ('rk_x6p_split', dict(rows=3, cols=5, lds=4), -1),
        ('rk_x6p_split', dict(rows=3, cols=5, ldd=4), -1), ('rk_x6p_split', dict(rows=3, cols=5, ldd=8, ps=23), -1),
        ('rk_x6p_split_t', dict(rows=37, cols=5, ldd=64), 0), ('rk_x6p_split_t', dict(rows=37, cols=5, ldd=40), 0),
        ('rk_x6p_split_t', dict(rows=37, cols=5, ldd=36), -1), ('rk_x6p_split_t', dict(rows=37, cols=5, ldd=38), -1),
        ('rk_x6p_split_t', dict(rows=37, cols=0, ldd=64), -1), ('rk_x6p_split_t', dict(rows=37, cols=5, lds=4, ldd=64), -1),
        ('rk_x6p_split_t', dict(rows=37, cols=5, ldd=40, ps=199), -1),
        ('rk_x6p_split_t', dict(rows=37, cols=5, ldd=40, ps=202), -1),                  # 8-byte stores: ps % 4
        ('rk_x6p_split_t', dict(rows=37, cols=5, ldd=40, ps=204), 0),
        ('rk_x6p_w4_weights', dict(Co=40, Ci=12), 0), ('rk_x6p_w4_weights', dict(Co=0, Ci=12), -1),
        ('rk_x6p_w4_weights', dict(Co=40, Ci=12, u=False, ut=False), -1),
        ('rk_x6p_w4_weights', dict(Co=40, Ci=12, u=False), 0),
        ('rk_x6p_w4_weights', dict(Co=1 << 12, Ci=1 << 13), -2),
        ('rk_wino4_pt_output', dict(Co=8, Ci=4), 0), ('rk_wino4_pt_output', dict(Co=8, Ci=0), -1),
        ('rk_wino4_pt_output', dict(Co=8, Ci=4, nslab=0), -1),
        ('rk_wino4_pt_output', dict(Co=8, Ci=4, nslab=2, slab=1151), -1),
        ('rk_wino4_pt_output', dict(Co=8, Ci=4, nslab=2, slab=1152), 0),
        ('rk_wino4_pt_output', dict(Co=8, Ci=6), -2), ('rk_wino4_pt_output', dict(Co=1 << 13, Ci=1 << 13), -2),
    ]
    sp = dict(Nb=2, H=8, W=4)
    for entry, big in (('rk_wino4_pt_input', 1 << 20), ('rk_x6p_w4_input', 1 << 19)):
        table += [(entry, dict(C=8, **sp), 0), (entry, dict(Nb=0, H=8, W=4, C=8), -1), (entry, dict(Nb=2, H=6, W=4, C=8), -1),
                  (entry, dict(Nb=2, H=8, W=2, C=8), -1), (entry, dict(C=0, **sp), -1), (entry, dict(C=6, **sp), -2),
                  (entry, dict(Nb=big, H=4, W=4, C=64), -2)]
    table.append(('rk_wino4_pt_input', dict(Nb=1 << 19, H=4, W=4, C=64), 0))
    for entry, big in (('rk_wino4_pt_transform', 1 << 20), ('rk_x6p_w4_wgrad_transform', 1 << 19)):
        table += [(entry, dict(Co=8, Ci=4, **sp), 0), (entry, dict(Nb=2, H=8, W=5, Co=8, Ci=4), -1),
                  (entry, dict(Co=0, Ci=4, **sp), -1), (entry, dict(Co=8, Ci=-4, **sp), -1),
                  (entry, dict(Co=6, Ci=4, **sp), -2), (entry, dict(Co=8, Ci=2, **sp), -2),
                  (entry, dict(Nb=big, H=4, W=4, Co=64, Ci=4), -2), (entry, dict(Nb=big, H=4, W=4, Co=4, Ci=64), -2)]
    # 108 T C below 2^31 but the NHWC tensor itself at 2^31 elements: the 32-bit pixel index
    table.append(('rk_x6p_w4_wgrad_transform', dict(Nb=1 << 18, H=4, W=4, Co=512, Ci=4), -2))
    table.append(('rk_x6p_w4_input', dict(Nb=1 << 18, H=4, W=4, C=512), -2))
    co = dict(N=6, **sp)
    table += [('rk_wino4_pt_conv_out', dict(**co), 0), ('rk_wino4_pt_conv_out', dict(Nb=2, H=8, W=6, N=6), -1),
              ('rk_wino4_pt_conv_out', dict(Nb=2, H=8, W=4, N=0), -1), ('rk_wino4_pt_conv_out', dict(nslab=0, **co), -1),
              ('rk_wino4_pt_conv_out', dict(flags=R.LRELU | R.RELU, **co), -1),
              ('rk_wino4_pt_conv_out', dict(flags=R.LRELU | R.STATS, stats=True, **co), -1),
              ('rk_wino4_pt_conv_out', dict(flags=R.LRELU | R.BIAS, bias=True, **co), 0),
              ('rk_wino4_pt_conv_out', dict(flags=R.STATS, **co), -1),
              ('rk_wino4_pt_conv_out', dict(flags=R.STATS, stats=True, **co), 0),
              ('rk_wino4_pt_conv_out', dict(flags=R.BNB, stats=True, bias=True, **co), -1),
              ('rk_wino4_pt_conv_out', dict(flags=R.BNP, stats=True, gate=True, **co), -1),
              ('rk_wino4_pt_conv_out', dict(flags=R.BNP, stats=True, gate=True, bias=True, **co), 0),
              ('rk_wino4_pt_conv_out', dict(flags=R.BIAS, **co), -1),
              ('rk_wino4_pt_conv_out', dict(Nb=1 << 15, H=16, W=16, N=4096), -2),
              ('rk_wino4_pt_conv_out', dict(nslab=2, slab=36 * 4 * 6 - 1, **co), -1),
              ('rk_wino4_pt_conv_out', dict(nslab=2, slab=36 * 4 * 6, **co), 0),
              ('rk_wino4_pt_conv_out', dict(flags=R.POOLED, bias=True, **co), 0)]   # no pooling here: the bit is ignored
    for entry, args, want in table:
        assert E(entry, **args) == want, (entry, args, E(entry, **args), want)
    seen = {(e, w) for e, _, w in table}
    for e in {e for e, _, _ in table}:
        assert (e, 0) in seen and (e, -1) in seen, e
    assert P.wgrad_form(16, 4, 8, 8, 40) == 'staged' and P.wgrad_form(2, 8, 16, 8, 8) == 'fallback'
    assert P.wgrad_form(16, 4, 8, 12, 8) == 'fallback'
    assert [P.conv_out_form(n) for n in (5, 6, 67, 70)] == ['scalar', 'vector2', 'scalar', 'vector2']
    assert [P.conv_out_form(n, 4) for n in (6, 68, 70)] == ['scalar', 'vector4', 'scalar']


def test_gemm_sweep_shapes():
    for tile, (BM, BN, _) in enumerate(P.TILES):
        s = P.gemm_shapes(tile)
        assert s[0] == (1, 8) and s[1] == (BM - 1, BN + 1)
        assert s[2][0] > BM and s[2][1] > BN and max(s[2]) <= 300
    assert P.gemm_shapes(7)[2] == (257, 130) and P.gemm_shapes(8)[2] == (130, 257)
    assert P.gemm_shapes(0)[2] == (161, 249)
