"""tests/sgemm_refs.py itself (CPU only): every reference anchored to plain loops and to torch fp64
(conv2d, conv_transpose2d, autograd) at 1e-12, the EXACT / EXACT-WIDE preconditions of every shape of the sweep,
and a list of wrong formulas that must each differ on an exact set AND leave the RANDOM gate.

Margins of the mutants on RANDOM as printed by ``pytest -s``: worst row / column rms ratio against the fp32
yardstick divided by the gate 4 (for the statistics mutants: worst |error| / tolerance, gate 1):
    wrap_lr 2.0e6   bottom_next 2.0e6   noflip 3.5e6   swap_khkw 1.9e6   parity_pixel 5.6e6   tap_table 3.9e6
    drop_last_k 2.3e5   drop_last_chunk 5.6e5   drop_last_ktile 5.6e5   ktile_twice 2.2e6   ktile_split_drop 2.0e6
    X6 term dropped: hh 1.7e6   hm 3.8e3   mh 3.6e3   hl 4.9   lh 5.1   mm 5.2
    gate_ge0 inf (the yardstick is exact where the gate closes)   grp_bias0 2.7e6
    stats_after_act 1.3e4   bnb_unmasked 1.6e4   bnp_route_on_y 9.8e3
"""
import pytest
import torch
import torch.nn.functional as TF

import sgemm_refs as G

F64 = torch.float64


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _assemble(name, a, b, taps=9, mutant=None, gemm_mutant=None):
    """Output [rows][N] of a one-slab problem (parity groups scattered to their pixels, groups stacked)."""
    vs = G.view(name.replace('_shared', ''), a, b, taps, mutant=mutant)
    outs = [G.gemm(A, B, mutant=gemm_mutant)[0][0] for A, B in vs]
    if name == 's2t':
        Nb, h, w, _ = a.shape
        full = torch.zeros(4 * Nb * h * w, outs[0].shape[1], dtype=F64)
        for g in range(4):
            full[G.s2t_rows(Nb, h, w, g, mutant)] = outs[g]
        return full
    return torch.cat(outs)


# ------------------------------------------------------------------------------------------ anchors
def test_gemm_is_the_plain_triple_loop():
    a, b = G.problem('dense', (5, 3, 70), 1, 'random')
    (A, B), = G.view('dense', a, b)
    for splits in (1, 2, 3, 5):
        slabs, S = G.gemm(A, B, splits)
        rng = G.split_ranges(70, splits)
        assert len(rng) == splits and rng[0][0] == 0 and max(h for _, h in rng) == 70
        for s, (lo, hi) in enumerate(rng):
            assert (lo % 32 == 0 or lo == 70) and (hi % 32 == 0 or hi == 70)
            for m in range(5):
                for n in range(3):
                    acc = sum(float(A[m, k]) * float(B[n, k]) for k in range(lo, hi))
                    ab = sum(abs(float(A[m, k]) * float(B[n, k])) for k in range(lo, hi))
                    assert abs(float(slabs[s, m, n]) - acc) < 1e-12 and abs(float(S[s, m, n]) - ab) < 1e-12
    assert G.split_ranges(70, 5)[3:] == [(70, 70), (70, 70)]        # ktPer = 1: two empty slabs
    _close(G.gemm(A, B, 5)[0].sum(0), A @ B.t())


@pytest.mark.parametrize('shape,taps', [((2, 5, 6, 8, 12), 9), ((2, 4, 4, 8, 12), 1)])
def test_conv_kinds_against_torch(shape, taps):
    Nb, H, W, Ci, Co = shape
    k, pad = (3, 1) if taps == 9 else (1, 0)
    x, w = G.problem('conv', shape, taps, 'random')
    w4 = w.reshape(Co, k, k, Ci).permute(0, 3, 1, 2)
    xt = _nchw(x).clone().requires_grad_(True)
    wt = w4.clone().requires_grad_(True)
    y = TF.conv2d(xt, wt, padding=pad)
    _close(_assemble('conv', x, w, taps), y.detach().permute(0, 2, 3, 1).reshape(-1, Co))
    dy = G.normal_f32(3, (Nb, H, W, Co))
    gx, gw = torch.autograd.grad(y, (xt, wt), _nchw(dy))
    _close(_assemble('dgrad', dy, w, taps), gx.permute(0, 2, 3, 1).reshape(-1, Ci))
    if taps == 9:   # the engine's form: a forward conv of dy with the flipped, transposed weights
        _close(_assemble('conv', dy, G.flip_transpose(w), taps), gx.permute(0, 2, 3, 1).reshape(-1, Ci))
    _close(_assemble('wgrad', dy, x, taps), gw.permute(0, 2, 3, 1).reshape(Co, -1))


def test_dense_kinds_against_torch():
    for name, ref in (('dense', lambda a, b: a @ b.t()), ('dx', lambda a, b: a @ b), ('dw', lambda a, b: a.t() @ b)):
        a, b = G.problem(name, (7, 5, 36), 1, 'random')
        _close(_assemble(name, a, b), ref(a, b))


def test_resampling_kinds_against_torch():
    Nb, H, W, Ci, Co = 2, 6, 8, 4, 8
    x, Wt = G.problem('s2', (Nb, H, W, Ci, Co), 16, 'random')
    w4 = Wt.reshape(Co, 4, 4, Ci).permute(0, 3, 1, 2)
    xt = _nchw(x).clone().requires_grad_(True)
    wt = w4.clone().requires_grad_(True)
    y = TF.conv2d(xt, wt, stride=2, padding=1)
    _close(_assemble('s2', x, Wt, 16), y.detach().permute(0, 2, 3, 1).reshape(-1, Co))
    g = G.normal_f32(5, (Nb, H // 2, W // 2, Co))
    gx, gw = torch.autograd.grad(y, (xt, wt), _nchw(g))
    _close(_assemble('s2t', g, Wt, 16), gx.permute(0, 2, 3, 1).reshape(-1, Ci))
    _close(_assemble('s2t', g, Wt, 16),
           TF.conv_transpose2d(_nchw(g), w4, stride=2, padding=1).permute(0, 2, 3, 1).reshape(-1, Ci))
    _close(_assemble('s2w', g, x, 16), gw.permute(0, 2, 3, 1).reshape(Co, -1))
    # the gather itself against plain loops
    A = G.gcols(x, H // 2, W // 2, 2, G.S2_TAPS)
    for row in (0, 5, Nb * (H // 2) * (W // 2) - 1):
        n, i, j = row // ((H // 2) * (W // 2)), (row // (W // 2)) % (H // 2), row % (W // 2)
        for t, (dy, dx) in enumerate(G.S2_TAPS):
            hi, wi = 2 * i + dy, 2 * j + dx
            want = x[n, hi, wi] if 0 <= hi < H and 0 <= wi < W else torch.zeros(Ci, dtype=F64)
            assert bool((A[row, t * Ci:(t + 1) * Ci] == want).all())


def test_grouped_views():
    for name in ('conv_grp', 'conv_grp_shared', 'dense_grp', 'dense_grp_shared'):
        shape, taps = ((2, 4, 4, 8, 12), 9) if 'conv' in name else ((6, 5, 36), 1)
        a, b = G.problem(name, shape, taps, 'random')
        assert a.shape[0] == (1 if 'shared' in name else 3) and b.shape[0] == 3
        vs = G.view(name.replace('_shared', ''), a, b, taps)
        for g in range(3):
            ag = a[0 if 'shared' in name else g]
            want = G.view('conv' if 'conv' in name else 'dense', ag, b[g], taps)[0]
            assert bool((vs[g][0] == want[0]).all()) and bool((vs[g][1] == want[1]).all())


def test_split3_and_the_six_terms():
    x = G.normal_f32(1, (64, 48)) * torch.exp2(G.ints(2, (64, 48), -20, 20))
    hi, mid, lo = G.split3(x)
    assert bool((hi + mid + lo == x).all())
    assert bool((mid.abs() <= 2.0 ** -8 * hi.abs()).all()) and bool((lo.abs() <= 2.0 ** -16 * hi.abs()).all())
    y = G.normal_f32(3, (40, 48))
    yh, ym, yl = G.split3(y)
    dropped = mid @ yl.t() + lo @ ym.t() + lo @ yl.t()
    _close(G.x6_gemm(x, y) + dropped, x @ y.t(), 1e-13)
    S = x.abs() @ y.abs().t()
    assert bool(((G.x6_gemm(x, y) - x @ y.t()).abs() <= 2.0 ** -25 * S).all())


def test_yardstick_is_an_fp32_accumulation():
    a, b = G.problem('dense', (40, 24, 132), 1, 'random')
    (A, B), = G.view('dense', a, b)
    slabs, S = G.gemm(A, B)
    y = G.yardstick(A, B)
    assert bool((y == G.f32r(y)).all()) and bool(((y - slabs[0]).abs() <= 132 * 2.0 ** -24 * S[0]).all())
    assert float((y - slabs[0]).abs().max()) > 0
    assert G.rms_ratio(y, slabs[0], y) == 1.0 and G.rms_ratio(slabs[0], slabs[0], y) == 0.0


def test_epilogue_order_against_plain_code():
    acc, S = G.ints(1, (6, 4), -9, 9), G.ints(2, (6, 4), 10, 20)
    bias, gate, prior = G.draw_bias('exact', 3, 4), G.draw_decision(4, (6, 4)), G.ints(5, (6, 4), -3, 3)
    r = G.epilogue(acc, S, 36, alpha=0.5, bias=bias, stats=True, act=G.ACT_LRELU, slope=0.25, gate=gate, prior=prior)
    for m in range(6):
        for n in range(4):
            v = float(acc[m, n]) * 0.5 + float(bias[n])
            v = v if v > 0 else v * 0.25
            v = v if float(gate[m, n]) > 0 else 0.0
            assert float(r['out'][m, n]) == v + float(prior[m, n])
    pre = acc * 0.5 + bias
    assert bool((r['sums'][0] == pre.sum(0)).all()) and bool((r['sums'][1] == (pre * pre).sum(0)).all())
    # BNB: masked value, sums of the masked value; BNP: the value unchanged, sums routed by the first maximum
    y = G.draw_decision(6, (6, 4))
    scale, shift = G.draw_scale_shift(7, 4)
    r = G.epilogue(acc, S, 36, bnb=(y, scale, shift))
    mask = (y * scale + shift > 0).to(F64)
    assert bool((r['out'] == acc * mask).all()) and bool((r['sums'][0] == (acc * mask).sum(0)).all())
    assert bool((r['sums'][1] == (acc * mask * y).sum(0)).all())
    y2 = G.draw_pool_y(8, 1, 2, 2, 4, scale)
    acc4 = acc[:4]
    r = G.epilogue(acc4, S[:4], 36, bnp=(y2, scale, shift, 1, 2, 2))
    assert bool((r['out'] == acc4).all())
    pooled = TF.max_pool2d(_nchw((y2 * scale + shift).clamp_min(0)), 2, return_indices=True)[1]
    yb = _nchw(y2).reshape(1, 4, -1).gather(2, pooled.reshape(1, 4, -1)).permute(0, 2, 1).reshape(4, 4)
    dz = acc4 * ((yb * scale + shift) > 0).to(F64)
    assert bool((r['sums'][0] == dz.sum(0)).all()) and bool((r['sums'][1] == (dz * yb).sum(0)).all())


def test_yardstick_epilogue_is_the_epilogue_in_fp32():
    acc, S = G.normal_f32(1, (9, 8)), G.normal_f32(2, (9, 8)).abs() + 1
    bias, gate, prior = G.draw_bias('random', 3, 8), G.draw_gate(4, (9, 8)), G.normal_f32(5, (9, 8))
    for kw in (dict(alpha=0.5, bias=bias, act=G.ACT_RELU), dict(bias=bias, act=G.ACT_LRELU, slope=0.2),
               dict(gate=gate), dict(prior=prior), {}):
        r, y = G.epilogue(acc, S, 1, **kw), G.epilogue32(acc, **kw)
        assert bool((y == G.f32r(y)).all()) and bool(((y - r['out']).abs() <= r['tol']).all())
    ia, ib = G.ints(6, (9, 8), -9, 9), G.draw_bias('exact', 7, 8)
    kw = dict(alpha=0.5, bias=ib, act=G.ACT_LRELU, slope=0.2, gate=gate)
    assert bool((G.epilogue32(ia, **kw) == G.epilogue(ia, S, 1, exact=True, **kw)['out']).all())


# ------------------------------------------------------------------------------------ preconditions
@pytest.mark.parametrize('name,shape,taps', G.SWEEP + [(k, s, 1) for k, s in G.BIG_LAYER.items()],
                         ids=lambda v: '-'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_exact_preconditions(name, shape, taps):
    for mode in G.EXACT_MODES:
        a, b = G.problem(name, shape, taps, mode)
        for A, B in G.view(name.replace('_shared', ''), a, b, taps):
            S = A.abs() @ B.abs().t()
            assert G.exact_ok(S), (mode, float(S.max()))
            assert float(S.max()) > 0
            if mode != 'exact':   # the three dropped terms are exactly zero: the six-term product is the product
                assert bool((G.x6_gemm(A, B) == A @ B.t()).all())


def test_the_threshold_layer_is_one_layer():
    """(batch, in, out) = (256, 2048, 512): dy [256][512], w [512][2048], x [256][2048] in all three GEMMs."""
    x, w = G.problem('dense', G.BIG_LAYER['dense'], 1, 'exact')
    dy, w2 = G.problem('dx', G.BIG_LAYER['dx'], 1, 'exact')
    dy2, x2 = G.problem('dw', G.BIG_LAYER['dw'], 1, 'exact')
    assert x.shape == x2.shape == (256, 2048) and w.shape == w2.shape == (512, 2048)
    assert dy.shape == dy2.shape == (256, 512)
    for name, a, b, mnk in (('dense', x, w, (256, 512, 2048)), ('dx', dy, w2, (256, 2048, 512)),
                            ('dw', dy2, x2, (512, 2048, 256))):
        (A, B), = G.view(name, a, b)
        assert (A.shape[0], B.shape[0], A.shape[1]) == mnk


def test_rms_ratio_reports_what_it_pooled():
    ref = G.normal_f32(1, (40, 8))
    yard, got, info = ref + 1e-7 * G.normal_f32(2, (40, 8)), ref + 1e-7 * G.normal_f32(3, (40, 8)), {}
    assert 0.3 < G.rms_ratio(got, ref, yard, info) < 3.0
    assert info == dict(rows=0, rows_pooled=40, cols=8, cols_pooled=0)     # 8-wide rows are judged together
    got2 = got.clone()
    got2[7, 3] += 1e-5                 # one bad element still shows, in its column and in the pooled rows
    assert G.rms_ratio(got2, ref, yard) > G.YARD


def test_wide_sets_use_the_pieces_they_are_for():
    a, b = G.problem('dense', (264, 132, 132), 1, 'wide_a')
    assert G.pieces_used(a)[1] > 0.2 and G.pieces_used(b) == (0.0, 0.0)
    a, b = G.problem('dense', (264, 132, 132), 1, 'wide_b')
    assert G.pieces_used(b)[1] > 0.2 and G.pieces_used(a) == (0.0, 0.0)
    a, b = G.problem('dense', (264, 132, 132), 1, 'wide_mm')
    for t in (a, b):
        mid, lo = G.pieces_used(t)
        assert mid > 0.6 and lo == 0.0    # 256 s + t with 8 significant bits (255, 510 ...) sits in hi alone
    # 17 significant bits never reach lo: the signed residual of hi fits the 8 bits of mid
    x17 = (2 * torch.arange(2 ** 15, 2 ** 16) + 1).to(F64)
    assert G.pieces_used(x17)[1] == 0.0


# ------------------------------------------------------------------------------------------ mutants
MARGINS = {}
CONV, CONVT, S2, DENSE = (3, 6, 6, 12, 40), 9, (1, 12, 12, 24, 40), (37, 20, 132)
VIEW_MUTANTS = [('wrap_lr', 'conv', CONV, 9), ('bottom_next', 'conv', CONV, 9), ('noflip', 'dgrad', CONV, 9),
                ('swap_khkw', 's2', S2, 16), ('parity_pixel', 's2t', S2, 16), ('tap_table', 's2t', S2, 16)]
GEMM_MUTANTS = ['drop_last_k', 'drop_last_chunk', 'drop_last_ktile']


def _gate(name, got, ref, yard, exact_pairs):
    assert any(bool((g != r).any()) for g, r in exact_pairs), '{}: invisible on the exact sets'.format(name)
    ratio = G.rms_ratio(got, ref, yard)
    MARGINS[name] = ratio
    print('mutant {:18s} leaves the yardstick gate {} by a factor {:.3g}'.format(name, G.YARD, ratio / G.YARD))
    assert ratio > G.YARD, (name, ratio)


def _yard(name, a, b, taps):
    vs = G.view(name, a, b, taps)
    outs = [G.yardstick(A, B) for A, B in vs]
    if name == 's2t':
        Nb, h, w, _ = a.shape
        full = torch.zeros(4 * Nb * h * w, outs[0].shape[1], dtype=F64)
        for g in range(4):
            full[G.s2t_rows(Nb, h, w, g)] = outs[g]
        return full
    return torch.cat(outs)


@pytest.mark.parametrize('mutant,name,shape,taps', VIEW_MUTANTS)
def test_gather_mutants_are_rejected(mutant, name, shape, taps):
    pairs = []
    for mode in ('exact', 'wide_a', 'random'):
        a, b = G.problem(name, shape, taps, mode)
        pairs.append((_assemble(name, a, b, taps, mutant=mutant), _assemble(name, a, b, taps)))
    _gate(mutant, pairs[2][0], pairs[2][1], _yard(name, a, b, taps), pairs[:2])


@pytest.mark.parametrize('mutant', GEMM_MUTANTS)
def test_k_tail_mutants_are_rejected(mutant):
    pairs = []
    for mode in ('exact', 'wide_mm', 'random'):
        a, b = G.problem('dense', DENSE, 1, mode)
        pairs.append((_assemble('dense', a, b, gemm_mutant=mutant), _assemble('dense', a, b)))
    _gate(mutant, pairs[2][0], pairs[2][1], _yard('dense', a, b, 1), pairs[:2])


@pytest.mark.parametrize('mutant,slab', [('ktile_twice', 0), ('ktile_split_drop', 1)])
def test_split_boundary_mutants_are_rejected(mutant, slab):
    pairs = []
    for mode in ('exact', 'wide_a', 'random'):
        a, b = G.problem('dense', DENSE, 1, mode)
        (A, B), = G.view('dense', a, b)
        pairs.append((G.gemm(A, B, 3, mutant=mutant)[0][slab], G.gemm(A, B, 3)[0][slab]))
    lo, hi = G.split_ranges(DENSE[2], 3)[slab]
    _gate(mutant, pairs[2][0], pairs[2][1], G.yardstick(A[:, lo:hi], B[:, lo:hi]), pairs[:2])


@pytest.mark.parametrize('term', G.X6_TERMS)
def test_each_dropped_x6_term_is_rejected(term):
    pairs = []
    for mode in ('wide_a', 'wide_b', 'wide_mm', 'random'):
        a, b = G.problem('dense', DENSE, 1, mode)
        (A, B), = G.view('dense', a, b)
        pairs.append((G.x6_gemm(A, B, drop=term), A @ B.t()))
    _gate('x6_' + term, pairs[3][0], pairs[3][1], G.yardstick(A, B), pairs[:3])
    # and the hard bound alone would not have noticed the small terms: that is what the yardstick is for
    S = A.abs() @ B.abs().t()
    if term in ('hl', 'lh', 'mm'):
        assert bool(((pairs[3][0] - pairs[3][1]).abs() <= G.n_x6(DENSE[2]) * G.U32 * S).all())


def test_gate_and_group_bias_mutants_are_rejected():
    pairs = []
    for mode in ('exact', 'random'):
        a, b = G.problem('dx', DENSE, 1, mode)
        (A, B), = G.view('dx', a, b)
        slabs, S = G.gemm(A, B)
        gate = G.draw_gate(9, slabs[0].shape)
        assert int((gate == 0).sum()) > 0 and int((gate > 0).sum()) > 0
        ref = G.epilogue(slabs[0], S[0], DENSE[2], gate=gate)['out']
        pairs.append((G.epilogue(slabs[0], S[0], DENSE[2], gate=gate, mutant='gate_ge0')['out'], ref))
    _gate('gate_ge0', pairs[1][0], pairs[1][1], G.yardstick(A, B) * (gate > 0), pairs[:1])
    pairs = []
    for mode in ('exact', 'random'):
        a, b = G.problem('dense_grp', DENSE, 1, mode)
        vs = G.view('dense_grp', a, b)
        bias = torch.stack([G.draw_bias(mode, 20 + g, DENSE[1]) for g in range(3)])
        outs = [[G.epilogue(*[t[0] for t in G.gemm(A, B)], DENSE[2], bias=bias[g if ok else 0])['out']
                 for g, (A, B) in enumerate(vs)] for ok in (False, True)]
        pairs.append((torch.cat(outs[0]), torch.cat(outs[1])))
    yard = torch.cat([G.yardstick(A, B) + bias[g] for g, (A, B) in enumerate(vs)])
    _gate('grp_bias0', pairs[1][0], pairs[1][1], yard, pairs[:1])


def test_statistics_mutants_are_rejected():
    """Statistics are judged channel by channel against their own tolerance: the mutant's sums must differ on
    EXACT and miss the RANDOM tolerance."""
    shape = (2, 4, 4, 8, 12)
    Nb, H, W, Ci, Co = shape
    for mutant in ('stats_after_act', 'bnb_unmasked', 'bnp_route_on_y'):
        seen = {}
        for mode in ('exact', 'random'):
            a, b = G.problem('conv', shape, 9, mode)
            (A, B), = G.view('conv', a, b)
            slabs, S = G.gemm(A, B)
            scale, shift = G.draw_scale_shift(11, Co)
            kw = {'stats_after_act': dict(stats=True, act=G.ACT_RELU),
                  'bnb_unmasked': dict(bnb=(G.draw_decision(12, (Nb * H * W, Co)), scale, shift)),
                  'bnp_route_on_y': dict(bnp=(G.draw_pool_y(13, Nb, H, W, Co, scale), scale, shift, Nb, H, W))}[mutant]
            ref = G.epilogue(slabs[0], S[0], 9 * Ci, **kw)
            mut = G.epilogue(slabs[0], S[0], 9 * Ci, mutant=mutant, **kw)
            seen[mode] = (mut['sums'], ref['sums'], ref['sums_tol'])
        assert bool((seen['exact'][0] != seen['exact'][1]).any()), mutant
        m, r, t = seen['random']
        ratio = float(((m - r).abs() / t).max())
        MARGINS[mutant] = ratio
        print('mutant {:18s} misses the statistics tolerance by a factor {:.3g}'.format(mutant, ratio))
        assert ratio > 1.0, (mutant, ratio)
    y = G.draw_pool_y(13, Nb, H, W, Co, scale)
    assert G.decisions_inexact(y, scale, shift) == 0


def test_bnp_on_the_last_maximum_cannot_be_seen_in_this_family():
    """FLAG_BNP of the fp32 engine leaves the pooled gradient as it is and only forms (sum dz, sum dz * y_best).
    Tied maxima of relu(y * scale + shift) either share their y (the map is injective for scale != 0) or are all
    zero (dz = 0), so routing to the LAST maximum gives the same sums: this mutant of igemm_refs is equivalent
    here, on inputs full of ties.  The routing is pinned by 'bnp_route_on_y' above instead."""
    Nb, H, W, Co = 2, 4, 4, 12
    scale, shift = G.draw_scale_shift(11, Co)
    y2 = G.draw_pool_y(13, Nb, H, W, Co, scale)
    win = y2.reshape(Nb, H, 2, W, 2, Co).permute(0, 1, 3, 2, 4, 5).reshape(-1, 4, Co)
    assert int((win[:, 0] == win[:, 3]).sum()) > Nb * H * W    # ties are there
    acc, S = G.ints(1, (Nb * H * W, Co), -9, 9), G.ints(2, (Nb * H * W, Co), 10, 20)
    kw = dict(bnp=(y2, scale, shift, Nb, H, W))
    assert bool((G.epilogue(acc, S, 8, mutant='bnp_last_max', **kw)['sums'] == G.epilogue(acc, S, 8, **kw)['sums']).all())
