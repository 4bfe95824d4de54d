"""The pre-transformed F(4x4) path stage by stage (csrc/kernels/winograd4.hip: rk_wino4_pt_input,
rk_wino4_pt_transform, rk_wino4_pt_output, rk_wino4_pt_conv_out, rk_x6p_w4_input, rk_x6p_w4_wgrad_transform,
rk_x6p_w4_weights; csrc/kernels/x6p.hip: rk_x6p_split, rk_x6p_split_t) and end to end, against the fp64 references of
tests/pt_refs.py (anchored and shown to bite in tests/test_pt_refs.py).  The entry points are called directly, each
launch once; every stage is fed synthetic input and judged alone.

Judging.  The exact and wide sets (integers; the wide ones carry 18 significant bits, so the mid and lo planes of
the producers are live) must come back bit for bit, planes as split3 of the reference.  RANDOM is held element by
element to n * 2^-23 * S with the stage's own count; planes must also be the canonical split of their own sum.
G^T dU G has 1/6 and 1/24 in it: no exact set, one-hot dU instead.  Statistics are judged twice, against the fp64
sums and against the output the same launch wrote (pt_refs.own_sums), with slot masks 0 and 3.  The end-to-end paths
(f32.wino4_conv_pt, f32.wino4_wgrad_pt on planes and on fp32 operands, once per config the tuner may pick) are held
to the composed tolerance and to sgemm_refs.YARD times the same algorithm in plain fp32.

Guards.  Every operand is a view 64 elements inside a larger NaN-filled storage (bf16 NaN for planes), every output
NaN-prefilled with NaN guard elements behind it, between split-K slabs and in padding columns; the rows of the
statistics past the slot mask stay NaN.  A launcher refusal is predicted by pt_refs.expected_status and asserted.

Which test reaches the kernels nothing else in the suite runs:
  w4pt_conv_out_kernel (scalar: odd N)               test_conv_out[*-5], [*-67]
  w4pt_conv_outv_kernel<4> (RAFIKI_PT_OUT_VW=4)      test_process_wide_switches -> test_conv_out[*-68] in the child
                                                     (and its scalar fallback there: N = 6, 70)
  w4pt_x_kernel<true, 2> (RAFIKI_PT_X_VW=2)          test_process_wide_switches -> test_x6p_w4_input in the child
  w4pt_dyT_kernel / w4pt_xT_kernel (fallback form)   test_x6p_w4_wgrad_transform on every shape but (16, 4, 8) x C % 8
  slab strides above 36 T N / 36 Co Ci, tmajor = 0 with slabs   test_conv_out, test_pt_output

Measured on an MI355X, worst error / hard tolerance over the sweep (the end-to-end paths also worst yardstick
ratio against the gate of 4):
    rk_wino4_pt_input 0.23, with pro 0.12       rk_wino4_pt_transform 0.26 (with xpro the same)      rk_wino4_pt_output 0.10
    rk_x6p_w4_input (4 and 2 channels per thread alike) 0.23, with pro 0.12          rk_x6p_w4_weights 0.18
    rk_x6p_w4_wgrad_transform staged 0.24, fallback 0.29          rk_x6p_split, rk_x6p_split_t: equal to split3 throughout
    rk_wino4_pt_conv_out, statistics included: 8-byte kernel 0.27, scalar 0.23, 16-byte (child process) 0.27
    wino4_conv_pt planes 0.0004, 0.92    fp32 operands 0.0033, 1.16    wino4_wgrad_pt planes 0.0002, 1.01    fp32 0.0008, 1.38
2835 launches checked and 78 refusals asserted in the parent, 2196 launches in the child; every exact and wide set came
back bit for bit and no guard element was overwritten.  No arithmetic bug was found.  One launcher was tightened:
rk_x6p_split_t now refuses a plane stride that is no multiple of 4 (its 8-byte stores to the mid and lo planes would
be misaligned; the launcher checked only ldd), and test_x6p_split_and_split_t asserts the refusal.
"""
import os
import re
import subprocess
import sys

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
IDS = lambda v: '-'.join(map(str, v)) if isinstance(v, tuple) else str(v)   # noqa: E731
CHILD = 'RAFIKI_PT_TEST_CHILD'
OUT_VW = 4 if os.environ.get('RAFIKI_PT_OUT_VW') == '4' else 2
X_VW = 2 if os.environ.get('RAFIKI_PT_X_VW') == '2' else 4
CASES = [s + (c,) for s in P.SPATIAL for c in P.CHANNELS]
MODES = ('exact', 'wide', 'random')
LRELU_SETS = [R.LRELU, R.BIAS | R.LRELU]
SLOPE = 0.2


@pytest.fixture(scope='module')
def S():
    from rafiki_amd.ops import _lib, f32
    _lib.lib()   # loud failure if the native library is missing
    yield f32
    _CO.clear()
    for tag in sorted(COUNT):
        ran, refused = COUNT[tag]
        print('WORST {:44s} err / hard tol {:.4f}   yardstick ratio {:.3f}   launches {} refusals {}'.format(
            tag, max(R.WORST.get(tag, 0.0), R.WORST.get(tag + ' sums', 0.0)), R.YWORST.get(tag, 0.0), ran, refused))
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


# ------------------------------------------------------------------------------------------ helpers
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


def _arena(t, dtype=F32):
    """Device copy of t as a contiguous view PAD elements inside a NaN-filled storage that runs PAD past it."""
    buf = torch.full((2 * PAD + t.numel(),), NAN, dtype=dtype, device=DEV)
    v = buf[PAD:PAD + t.numel()].view(t.shape)
    v.copy_(t.to(DEV, dtype))
    return v


def _out(n, dtype=F32, extra=PAD):
    return torch.full((n + extra,), NAN, dtype=dtype, device=DEV)


def _run(S, tag, entry, want, bufs, *args):
    """One launch: the status is what expected_status said; a refused launch wrote nothing.  True if it ran."""
    from rafiki_amd.ops import _lib
    st = _status(lambda: _lib.call(entry, *args, S._s()))
    assert st == want, '{} {}: status {} (expected {})'.format(tag, args, st, want)
    torch.cuda.synchronize()
    _count(tag, st == 0)
    if st != 0:
        for b in bufs:
            assert bool(torch.isnan(b).all()), '{}: a refused launch wrote something'.format(tag)
    return st == 0


def _host(buf, n, tag):
    h = buf.to('cpu', F64)
    assert bool(torch.isnan(h[n:]).all()), '{}: wrote past the output'.format(tag)
    return h[:n]


def _pro(mode, C):
    return R.draw_pro('random' if mode == 'random' else 'exact', 3 + C, C)


# ------------------------------------------------------------------- fp32 transforms: B^T d B, A dY A^T
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_fp32_transforms(S, case):
    """rk_wino4_pt_input with and without pro, rk_wino4_pt_transform (both halves, Co != Ci) with and without xpro."""
    Nb, H, W, C = case
    Co = P.CHANNELS[(P.CHANNELS.index(C) + 1) % 4]
    T = P.tiles(Nb, H, W)
    for mode in MODES:
        x, dy = P.draw_x(mode, 1 + sum(case), case), P.draw_dy(mode, 2 + sum(case), (Nb, H, W, Co))
        x_d, dy_d = _arena(x), _arena(dy)
        mref, mtol = P.m_of(dy), P.tol_of(P.N_A6, P.m_of(dy, absval=True))
        for pro in (None, _pro(mode, C)):
            pro_d = None if pro is None else _arena(torch.cat(pro))
            vref = P.v_of(x, pro)
            Sv = P.v_of(x, pro, absval=True)
            assert mode == 'random' or P.exact_ok(Sv)
            vtol = P.tol_of(P.N_BT6 + (P.N_PRO if pro else 0), Sv)
            what = '{} {}{}'.format(case, mode, ' pro' if pro else '')
            v = _out(36 * T * C)
            tag = 'rk_wino4_pt_input' + (' pro' if pro else '')
            assert _run(S, tag, 'rk_wino4_pt_input', P.expected_status('rk_wino4_pt_input', Nb=Nb, H=H, W=W, C=C), [v],
                        S._p(x_d), S._p(v), Nb, H, W, C, S._p(pro_d))
            P.judge(tag, _host(v, 36 * T * C, tag).view(36, T, C), vref, vtol, mode, None, what)
            m, v = _out(36 * T * Co), _out(36 * T * C)
            tag = 'rk_wino4_pt_transform' + (' xpro' if pro else '')
            assert _run(S, tag, 'rk_wino4_pt_transform',
                        P.expected_status('rk_wino4_pt_transform', Nb=Nb, H=H, W=W, Co=Co, Ci=C), [m, v],
                        S._p(dy_d), S._p(x_d), S._p(m), S._p(v), Nb, H, W, Co, C, S._p(pro_d))
            P.judge(tag, _host(v, 36 * T * C, tag).view(36, T, C), vref, vtol, mode, None, what + ' v')
            P.judge(tag, _host(m, 36 * T * Co, tag).view(36, T, Co), mref, mtol, mode, None, what + ' m')


# ----------------------------------------------------------------------------------- plane producers
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_x6p_w4_input(S, case):
    """V planes [36][3][T][C], with and without pro (RAFIKI_PT_X_VW picks 4 or 2 channels per thread)."""
    Nb, H, W, C = case
    T = P.tiles(Nb, H, W)
    for mode in MODES:
        x = P.draw_x(mode, 1 + sum(case), case)
        x_d = _arena(x)
        for pro in (None, _pro(mode, C)):
            pro_d = None if pro is None else _arena(torch.cat(pro))
            ref, Sv = P.v_of(x, pro), P.v_of(x, pro, absval=True)
            assert mode == 'random' or P.exact_ok(Sv)
            if mode == 'wide':
                assert min(P.pieces_used(ref)) > 0
            tag = 'rk_x6p_w4_input vw{}{}'.format(X_VW, ' pro' if pro else '')
            v = _out(108 * T * C, BF16)
            assert _run(S, tag, 'rk_x6p_w4_input', P.expected_status('rk_x6p_w4_input', Nb=Nb, H=H, W=W, C=C), [v],
                        S._p(x_d), S._p(v), Nb, H, W, C, S._p(pro_d))
            P.judge_planes(tag, _host(v, 108 * T * C, tag).view(36, 3, T, C), ref,
                           P.tol_of(P.N_BT6 + (P.N_PRO if pro else 0), Sv), mode, '{} {}'.format(case, mode))


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_x6p_w4_wgrad_transform(S, case):
    """M^T [36][3][Co][T] and V^T [36][3][Ci][T]: the LDS-staged form (T % 32 == 0, Co % 8 == 0, Ci % 8 == 0) and the
    fallback pair everywhere else."""
    Nb, H, W, Ci = case
    T = P.tiles(Nb, H, W)
    for Co in sorted({Ci, P.CHANNELS[(P.CHANNELS.index(Ci) + 1) % 4]}):
        tag = 'rk_x6p_w4_wgrad_transform ' + P.wgrad_form(Nb, H, W, Co, Ci)
        for mode in MODES:
            x, dy = P.draw_x(mode, 1 + sum(case), case), P.draw_dy(mode, 2 + sum(case), (Nb, H, W, Co))
            x_d, dy_d = _arena(x), _arena(dy)
            mt, vt = _out(108 * T * Co, BF16), _out(108 * T * Ci, BF16)
            assert _run(S, tag, 'rk_x6p_w4_wgrad_transform',
                        P.expected_status('rk_x6p_w4_wgrad_transform', Nb=Nb, H=H, W=W, Co=Co, Ci=Ci), [mt, vt],
                        S._p(dy_d), S._p(x_d), S._p(mt), S._p(vt), Nb, H, W, Co, Ci)
            what = '{} Co {} {}'.format(case, Co, mode)
            for buf, C, ref, Sa, n in ((mt, Co, P.m_of(dy), P.m_of(dy, absval=True), P.N_A6),
                                       (vt, Ci, P.v_of(x), P.v_of(x, absval=True), P.N_BT6)):
                assert mode == 'random' or P.exact_ok(Sa)
                P.judge_planes(tag, _host(buf, 108 * T * C, tag).view(36, 3, C, T), ref.transpose(1, 2),
                               P.tol_of(n, Sa.transpose(1, 2)), mode, what)


@pytest.mark.parametrize('Co,Ci', [(40, 12), (12, 40), (33, 7), (64, 32)])
def test_x6p_w4_weights(S, Co, Ci):
    """u only, ut only and both; G has 1/6 and 1/24: RANDOM only, the planes the canonical split of their sum."""
    tag = 'rk_x6p_w4_weights'
    w = R.draw_w('random', 3 + Co + Ci, Co, Ci)
    w_d = _arena(w)
    n = 108 * Co * Ci
    for which in ('both', 'u', 'ut'):
        bufs = {k: _out(n, BF16) for k in ('u', 'ut') if which in ('both', k)}
        assert _run(S, tag, tag, P.expected_status(tag, Co=Co, Ci=Ci, u='u' in bufs, ut='ut' in bufs), list(bufs.values()),
                    S._p(w_d), S._p(bufs.get('u')), S._p(bufs.get('ut')), Co, Ci)
        for k, buf in bufs.items():
            ref = R.transform_weights(w, 4, k == 'ut')
            tol = P.tol_of(P.N_G6, R.transform_weights(w, 4, k == 'ut', absval=True))
            P.judge_planes(tag, _host(buf, n, tag).view(36, 3, ref.shape[1], ref.shape[2]), ref, tol, 'random',
                           '{} ({}, {}) {}'.format(k, Co, Ci, which))


@pytest.mark.parametrize('rows,cols', [(37, 5), (130, 70), (64, 64), (3, 129)])
def test_x6p_split_and_split_t(S, rows, cols):
    """rk_x6p_split with lds > cols and ldd > cols (the padding columns stay NaN); rk_x6p_split_t with rows no
    multiple of 64 or of 4, ldd the next multiple of 4 and of 32, a plane stride above cols * ldd: the K padding is
    exact zeros.  A plane stride that would misalign its 8-byte stores is refused."""
    for mode in MODES:
        src = P.draw_mat(mode, rows + cols, (rows, cols))
        lds = cols + 3
        padded = torch.full((rows, lds), NAN, dtype=F64)
        padded[:, :cols] = src
        src_d = _arena(padded)
        want = P.planes(src)
        for ldd, ps in ((cols, rows * cols), (cols + 5, rows * (cols + 5) + 7)):
            tag = 'rk_x6p_split'
            dst = _out(3 * ps, BF16)
            assert _run(S, tag, tag, P.expected_status(tag, rows=rows, cols=cols, lds=lds, ldd=ldd, ps=ps), [dst],
                        S._p(src_d), S._p(dst), rows, cols, lds, ldd, ps)
            h = _host(dst, 3 * ps, tag)
            view = torch.as_strided(h, (3, rows, ldd), (ps, ldd, 1))
            assert torch.equal(view[:, :, :cols], want), '{} {} {}: planes are not split3 of the source'.format(tag, mode, ldd)
            keep = torch.ones(3 * ps, dtype=torch.bool)
            keep[(torch.arange(3)[:, None, None] * ps + torch.arange(rows)[None, :, None] * ldd
                  + torch.arange(cols)[None, None, :]).reshape(-1)] = False
            assert bool(torch.isnan(h[keep]).all()), '{}: wrote into the padding'.format(tag)
        tag = 'rk_x6p_split_t'
        for ldd in sorted({P.cdiv(rows, 4) * 4, P.cdiv(rows, 32) * 32}):
            for ps in (cols * ldd, cols * ldd + 8, cols * ldd + 6):
                dst = _out(3 * ps, BF16)
                ok = _run(S, tag, tag, P.expected_status(tag, rows=rows, cols=cols, lds=lds, ldd=ldd, ps=ps), [dst],
                          S._p(src_d), S._p(dst), rows, cols, lds, ldd, ps)
                assert ok == (ps % 4 == 0)
                if not ok:
                    continue
                h = _host(dst, 3 * ps, tag)
                view = torch.as_strided(h, (3, cols, ldd), (ps, ldd, 1))
                assert torch.equal(view[:, :, :rows], want.transpose(1, 2)), '{} {} ldd {}'.format(tag, mode, ldd)
                assert bool((view[:, :, rows:] == 0).all()), '{}: the K padding is not zero'.format(tag)
                if ps > cols * ldd:
                    assert bool(torch.isnan(torch.as_strided(h, (2, ps - cols * ldd), (ps, 1), cols * ldd)).all())


# -------------------------------------------------------------------------------- G^T dU G
@pytest.mark.parametrize('Co,Ci', [(4, 8), (12, 4), (40, 12), (8, 40)])
def test_pt_output(S, Co, Ci):
    """nslab 1 and 3, the slab stride equal to and above 36 Co Ci, accumulation onto a prior; random dU and one-hot
    dU (a wrong (q, co, ci) decode lands the 3x3 pattern G[a] G[b]^T in the wrong place)."""
    tag, dense = 'rk_wino4_pt_output', 36 * Co * Ci
    n = Co * 9 * Ci
    for kind in ('random', 'onehot0', 'onehot1'):
        for nslab, slab in ((1, 0), (1, dense), (3, dense), (3, dense + 64)):
            if kind == 'random':
                du = P.with_slabs(P.draw_yt('random', Co + Ci, dense), nslab, max(slab, dense), 9, 'random')
            else:
                du = P.with_slabs(torch.zeros(dense, dtype=F64), nslab, max(slab, dense), 9, 'zero')
                q, co, ci = (7, Co - 1, 1) if kind == 'onehot0' else (32, 0, Ci - 1)
                du[(nslab - 1) * max(slab, dense) + (q * Co + co) * Ci + ci] = 1.0
            du_d = _arena(du)
            for accumulate in (False, True):
                prior = G.normal_f32(5, (Co, 9, Ci)) if accumulate else None
                out = _out(n)
                if accumulate:
                    out[:n] = prior.reshape(-1).to(DEV, F32)
                want = P.expected_status(tag, Co=Co, Ci=Ci, nslab=nslab, slab=slab)
                assert _run(S, tag, tag, want, [], S._p(du_d), S._p(out), Co, Ci, int(accumulate), nslab, slab)
                kw = dict(nslab=nslab, slab=slab, accumulate=accumulate, prior=prior)
                ref = P.wgrad_out(du, Co, Ci, **kw)
                tol = P.tol_of(P.n_wgrad_out(nslab, accumulate), P.wgrad_out(du, Co, Ci, absval=True, **kw))
                P.judge(tag, _host(out, n, tag).view(Co, 9, Ci), ref, tol, 'random', None,
                        '({}, {}) {} nslab {} slab {} acc {}'.format(Co, Ci, kind, nslab, slab, accumulate), 'wgrad')


# -------------------------------------------------------------------------------- A^T Y' A + epilogues
_CO = {}


def _co_problem(mode, sp, N, nslab, slab):
    key = (mode, sp, N, nslab, slab)
    if key not in _CO:
        Nb, H, W = sp
        T = P.tiles(Nb, H, W)
        seed = 17 * sum(sp) + N
        yt = P.with_slabs(P.draw_yt(mode, seed, 36 * T * N), nslab, slab, seed + 50, mode)
        bias = R.draw_bias(mode, seed + 1, N)
        scale, shift = G.draw_scale_shift(seed + 2, N)
        y, y2 = G.draw_decision(seed + 3, (Nb * H * W, N)), G.draw_pool_y(seed + 4, Nb, H, W, N, scale)
        assert G.decisions_inexact(y, scale, shift) == 0 and G.decisions_inexact(y2, scale, shift) == 0
        _CO[key] = dict(yt=yt, bias=bias, ss=(scale, shift), y=y, y2=y2, yt_d=_arena(yt), bias_d=_arena(bias),
                        ss_d=_arena(torch.cat([scale, shift])), y_d=_arena(y), y2_d=_arena(y2))
    return _CO[key]


def check_conv_out(S, sp, N, mode, flags, tmajor, nslab, slab, mask):
    Nb, H, W = sp
    T = P.tiles(Nb, H, W)
    p = _co_problem(mode, sp, N, nslab, slab)
    tag = 'rk_wino4_pt_conv_out ' + P.conv_out_form(N, OUT_VW)
    what = '{} N {} {} flags {} tmajor {} nslab {} slab {} mask {}'.format(sp, N, mode, flags, tmajor, nslab, slab, mask)
    bn = flags & (R.BNB | R.BNP)
    stats = bool(flags & (R.STATS | R.BNB | R.BNP))
    bias_d = p['ss_d'] if bn else p['bias_d'] if flags & R.BIAS else None
    gate_d = p['y_d'] if flags & R.BNB else p['y2_d'] if flags & R.BNP else None
    slope = SLOPE if flags & R.LRELU else 0.0
    n = Nb * H * W * N
    out = _out(n, extra=2 * N + PAD)
    acc = None
    if stats:   # one more row than the slot mask reaches: it must still be NaN afterwards
        acc = torch.zeros((mask + 2, 2, N), dtype=F64, device=DEV)
        acc[mask + 1] = NAN
    want = P.expected_status('rk_wino4_pt_conv_out', Nb=Nb, H=H, W=W, N=N, flags=flags, nslab=nslab, slab=slab,
                             stats=stats, gate=gate_d is not None, bias=bias_d is not None)
    assert want == 0
    assert _run(S, tag, 'rk_wino4_pt_conv_out', want, [out], S._p(p['yt_d']), S._p(out), S._p(bias_d), S._p(acc), mask,
                S._p(gate_d), Nb, H, W, N, flags, nslab, slab, tmajor, slope)
    got = _host(out, n, tag).view(Nb, H, W, N)
    exact = mode != 'random'
    r = P.conv_out(p['yt'], Nb, H, W, N, flags, bias=p['ss'] if bn else p['bias'],
                   gate=p['y'] if flags & R.BNB else p['y2'] if flags & R.BNP else None, nslab=nslab, slab=slab,
                   tmajor=tmajor, slope=slope, exact=exact)
    if exact:
        assert P.exact_ok(r['S'] + 3.0)
    P.judge(tag, got, r['out'], r['tol'], mode, None, what)
    if not stats:
        return
    h = acc.to('cpu')
    assert bool(torch.isnan(h[mask + 1]).all()), '{}: wrote past the statistics slots'.format(tag)
    sums = h[:mask + 1].sum(0)
    o = got.reshape(-1, N)
    if flags & R.STATS:
        v, second, unit = r['acc'].reshape(-1, N) + (p['bias'] if flags & R.BIAS else 0.0), None, 1.0
        own = None if flags & R.RELU else P.own_sums(o)       # behind a ReLU the output no longer holds v
    elif flags & R.BNB:
        v, second, unit = r['out'].reshape(-1, N), p['y'], 1.0 / 64
        own = P.own_sums(o, p['y'])
    else:
        pos, yb = G.bnp_route(p['y2'], p['ss'][0], p['ss'][1], Nb, H, W)
        v, second, unit = r['out'].reshape(-1, N) * pos.to(F64), yb, 1.0 / 64
        own = P.own_sums(o * pos.to(F64), yb)
    P.judge_sums(tag + ' sums', sums, r['sums'], r['sums_tol'], mode, v, what, second, unit)
    if own is not None:
        P.judge_sums(tag + ' sums', sums, own[0], own[1], mode, v, what + ' against its own output', second, unit)


@pytest.mark.parametrize('N', (5, 6, 67, 68, 70))
@pytest.mark.parametrize('sp', P.SPATIAL, ids=IDS)
def test_conv_out(S, sp, N):
    """Synthetic Y' (integer on the exact set: the output is right to the bit) through every flag set of
    wino_refs.FLAG_SETS (the pooling bit has no meaning here and is ignored) and the two leaky-ReLU sets;
    position- and tile-major, 1 and 3 slabs at a stride above 36 T N, slot masks 0 and 3.  N = 6, 70 the 8-byte
    kernel (70: a ragged 64-channel block), 68 the same (the 16-byte kernel under RAFIKI_PT_OUT_VW=4, where 6 and 70
    fall to the scalar one), 5 and 67 the scalar kernel."""
    T = P.tiles(*sp)
    slab = 36 * T * N + 64
    k = 0
    for mode in ('exact', 'random'):
        for flags in R.FLAG_SETS + LRELU_SETS:
            for tmajor, nslab, sl in ((0, 1, 0), (1, 1, 0), (0, 3, slab), (1, 3, slab)):
                check_conv_out(S, sp, N, mode, flags, tmajor, nslab, sl, mask=(0, 3)[k % 2])
                k += 1
            k += 1      # so that every (layout, slabs) meets both slot masks
    check_conv_out(S, sp, N, 'random', R.STATS, 1, 3, 36 * T * N, mask=3)     # the slabs back to back


# ------------------------------------------------------------------------------------- end to end
def _conv_e2e(S, tag, C, call, n, **kw):
    Nb, H, W, N = 16, 4, 8, 40
    x, U, _ = R.conv_problem('random', 4, (Nb, H, W, C, N))
    ref, Sa = R.fused_conv(x, U, 4), R.fused_conv(x, U, 4, absval=True)
    yard = R.fused_conv(x.to(F32), U.to(F32), 4).to(F64)
    got = call(x.to(DEV, F32), U)
    torch.cuda.synchronize()
    _count(tag, True)
    R.judge(tag, got, ref, P.tol_of(n, Sa), 'random', yard, 'C {} {}'.format(C, kw), MO=4)


def test_end_to_end_conv(S):
    """f32.wino4_conv_pt once per WINO4_PTX_CFGS entry (planes; C = 32 per requested split, so the split count is
    real) and once per _pt_cfgs tile (fp32 operands), T = 32 tiles, against wino_refs.fused_conv."""
    assert len(S.WINO4_PTX_CFGS) > 0
    for _, code, splits in S.WINO4_PTX_CFGS:
        tile, nst = S.x6p_unpack(code)
        C = 32 * splits
        eff = S.x6p_splits(C, splits)
        _conv_e2e(S, 'wino4_conv_pt planes', C,
                  lambda x, U: S.wino4_conv_pt(x, P.planes(U).to(DEV, BF16).contiguous(), tile=tile, nst=nst, splits=splits),
                  P.n_conv_e2e(C, slabs=eff), tile=tile, nst=nst, splits=splits)
    for _, tile, nst in S._pt_cfgs(0):
        _conv_e2e(S, 'wino4_conv_pt fp32', 32,
                  lambda x, U: S.wino4_conv_pt(x, U.to(DEV, F32).contiguous(), tile=tile, nst=nst),
                  P.n_conv_e2e(32, planes_=False, x6=bool(tile & S.X6)), tile=tile, nst=nst)


def _wgrad_e2e(S, tag, T, call, n, **kw):
    Nb, H, W, Ci, Co = T // 2, 4, 8, 32, 40
    dy, x = R.wgrad_problem('random', 4, (Nb, H, W, Ci, Co))
    ref, Sa = R.fused_wgrad(dy, x, 4)[0][0], R.fused_wgrad(dy, x, 4, absval=True)[0][0]
    yard = R.fused_wgrad(dy.to(F32), x.to(F32), 4)[0][0].to(F64)
    for accumulate in (False, True):
        prior = G.normal_f32(5, (Co, 9, Ci))
        out = prior.to(DEV, F32).contiguous() if accumulate else torch.full((Co, 9, Ci), NAN, dtype=F32, device=DEV)
        call(dy.to(DEV, F32), x.to(DEV, F32), out, accumulate)
        torch.cuda.synchronize()
        _count(tag, True)
        R.judge(tag, out, ref + prior if accumulate else ref,
                P.tol_of(n + int(accumulate), Sa + (prior.abs() if accumulate else 0.0)), 'random',
                G.f32r(yard + prior) if accumulate else yard, 'T {} acc {} {}'.format(T, accumulate, kw), layout='wgrad')


def test_end_to_end_wgrad(S):
    """f32.wino4_wgrad_pt once per _wino4_ptx_wgrad_cands entry (planes; T = 32 tiles per requested split) and once
    per _pt_cfgs tile (fp32 operands), plain and accumulating, against wino_refs.fused_wgrad."""
    cands = S._wino4_ptx_wgrad_cands(64, 4, 8, 64, 32)     # T = 128: the split counts 1, 2 and 4 are all real
    assert len(cands) > 0
    for _, code, splits in cands:
        tile, nst = S.x6p_unpack(code)
        T = 32 * splits
        _wgrad_e2e(S, 'wino4_wgrad_pt planes', T,
                   lambda dy, x, out, acc: S.wino4_wgrad_pt(dy, x, out, accumulate=acc, tile=tile, nst=nst, planes=True,
                                                            splits=splits),
                   P.n_wgrad_e2e(T, slabs=splits), tile=tile, nst=nst, splits=splits)
    for _, tile, nst in S._pt_cfgs(0):
        _wgrad_e2e(S, 'wino4_wgrad_pt fp32', 32,
                   lambda dy, x, out, acc: S.wino4_wgrad_pt(dy, x, out, accumulate=acc, tile=tile, nst=nst),
                   P.n_wgrad_e2e(32, planes_=False, x6=bool(tile & S.X6)), tile=tile, nst=nst)


# ---------------------------------------------------------------------------------------- refusals
def test_launcher_refusals(S):
    """Every argument check of the nine launchers once on valid small tensors, with the predicted status."""
    x_d = _arena(R.draw_x('exact', 1, (2, 8, 4, 8)))
    f, b = _out(36 * 4 * 8 * 3), _out(108 * 4 * 8 * 3, BF16)
    seen = set()

    def go(entry, bufs, args, **kw):
        want = P.expected_status(entry, **kw)
        assert want != 0, (entry, kw)
        _run(S, entry + ' refusals', entry, want, bufs, *args)
        seen.add((entry, want))
    sp = dict(Nb=2, H=8, W=4)
    for entry, buf, big in (('rk_wino4_pt_input', f, 1 << 20), ('rk_x6p_w4_input', b, 1 << 19)):
        for kw in (dict(sp, Nb=0, C=8), dict(sp, H=6, C=8), dict(sp, W=2, C=8), dict(sp, C=0), dict(sp, C=6),
                   dict(Nb=big, H=4, W=4, C=64)):
            go(entry, [buf], (S._p(x_d), S._p(buf), kw['Nb'], kw['H'], kw['W'], kw['C'], None), **kw)
    go('rk_x6p_w4_input', [b], (S._p(x_d), S._p(b), 1 << 18, 4, 4, 512, None), Nb=1 << 18, H=4, W=4, C=512)
    for entry, o1, o2, big in (('rk_wino4_pt_transform', f, f, 1 << 20), ('rk_x6p_w4_wgrad_transform', b, b, 1 << 19)):
        for kw in (dict(sp, W=5, Co=8, Ci=4), dict(sp, Co=0, Ci=4), dict(sp, Co=8, Ci=-4), dict(sp, Co=6, Ci=4),
                   dict(sp, Co=8, Ci=2), dict(Nb=big, H=4, W=4, Co=64, Ci=4), dict(Nb=big, H=4, W=4, Co=4, Ci=64)):
            tail = (None,) if entry == 'rk_wino4_pt_transform' else ()
            go(entry, [o1], (S._p(x_d), S._p(x_d), S._p(o1), S._p(o2), kw['Nb'], kw['H'], kw['W'], kw['Co'], kw['Ci']) + tail,
               **kw)
    go('rk_x6p_w4_wgrad_transform', [b], (S._p(x_d), S._p(x_d), S._p(b), S._p(b), 1 << 18, 4, 4, 512, 4),
       Nb=1 << 18, H=4, W=4, Co=512, Ci=4)
    for kw in (dict(Co=0, Ci=12), dict(Co=8, Ci=8, u=False, ut=False), dict(Co=1 << 12, Ci=1 << 13)):
        go('rk_x6p_w4_weights', [b], (S._p(x_d), S._p(b) if kw.get('u', True) else None,
                                      S._p(b) if kw.get('ut', True) else None, kw['Co'], kw['Ci']), **kw)
    for kw in (dict(Co=8, Ci=0), dict(Co=8, Ci=4, nslab=0), dict(Co=8, Ci=4, nslab=2, slab=1151), dict(Co=8, Ci=6),
               dict(Co=1 << 13, Ci=1 << 13)):
        go('rk_wino4_pt_output', [f], (S._p(x_d), S._p(f), kw['Co'], kw['Ci'], 0, kw.get('nslab', 1), kw.get('slab', 0)), **kw)
    for kw in (dict(rows=0, cols=5), dict(rows=3, cols=5, lds=4), dict(rows=3, cols=5, ldd=4), dict(rows=3, cols=5, ldd=8, ps=23)):
        go('rk_x6p_split', [b], (S._p(x_d), S._p(b), kw['rows'], kw['cols'], kw.get('lds', kw['cols']),
                                 kw.get('ldd', kw['cols']), kw.get('ps', kw['rows'] * kw.get('ldd', kw['cols']))), **kw)
    for kw in (dict(rows=37, cols=0, ldd=64), dict(rows=37, cols=5, lds=4, ldd=64), dict(rows=37, cols=5, ldd=36),
               dict(rows=37, cols=5, ldd=38), dict(rows=37, cols=5, ldd=40, ps=196), dict(rows=37, cols=5, ldd=40, ps=202)):
        go('rk_x6p_split_t', [b], (S._p(x_d), S._p(b), kw['rows'], kw['cols'], kw.get('lds', kw['cols']), kw['ldd'],
                                   kw.get('ps', kw['cols'] * kw['ldd'])), **kw)
    co = dict(sp, N=6)
    st = torch.zeros((2, 2, 6), dtype=F64, device=DEV)
    for kw in (dict(co, W=6), dict(co, N=0), dict(co, nslab=0), dict(co, flags=R.LRELU | R.RELU),
               dict(co, flags=R.LRELU | R.STATS, stats=True), dict(co, flags=R.STATS),
               dict(co, flags=R.BNB, stats=True, bias=True), dict(co, flags=R.BNP, stats=True, gate=True),
               dict(co, flags=R.BIAS), dict(Nb=1 << 15, H=16, W=16, N=4096), dict(co, nslab=2, slab=36 * 4 * 6 - 1)):
        go('rk_wino4_pt_conv_out', [f], (S._p(x_d), S._p(f), S._p(x_d) if kw.get('bias') else None,
                                         S._p(st) if kw.get('stats') else None, 0, S._p(x_d) if kw.get('gate') else None,
                                         kw['Nb'], kw['H'], kw['W'], kw['N'], kw.get('flags', 0), kw.get('nslab', 1),
                                         kw.get('slab', 0), 0, 0.0), **kw)
    assert bool((st == 0).all())
    for entry in ('rk_wino4_pt_input', 'rk_x6p_w4_input', 'rk_wino4_pt_transform', 'rk_x6p_w4_wgrad_transform',
                  'rk_wino4_pt_output', 'rk_wino4_pt_conv_out', 'rk_x6p_w4_weights'):
        assert (entry, -1) in seen and (entry, -2) in seen, entry


# ------------------------------------------------------------------------- the process-wide switches
def test_process_wide_switches():
    """RAFIKI_PT_OUT_VW and RAFIKI_PT_X_VW are read once per process: one fresh child runs the conv_out and
    x6p_w4_input tests of this file under RAFIKI_PT_OUT_VW=4 (the 16-byte kernel at N = 68, its scalar fallback at
    N = 6 and 70) and RAFIKI_PT_X_VW=2 (two channels per thread)."""
    if os.environ.get(CHILD):
        pytest.skip('this is the child')
    env = dict(os.environ, RAFIKI_PT_OUT_VW='4', RAFIKI_PT_X_VW='2')
    env[CHILD] = '1'
    try:
        r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-m', 'gpu', '-k',
                            'conv_out or x6p_w4_input', '-q', '-s', '-p', 'no:cacheprovider'], env=env, timeout=900,
                           capture_output=True, text=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    except subprocess.TimeoutExpired:
        pytest.exit('the child of test_process_wide_switches timed out: nothing more is started', returncode=3)
    print(r.stdout[-3000:])
    if r.returncode < 0 or r.returncode == 3:
        pytest.exit('the child of test_process_wide_switches died (status {}): nothing more is started\n{}'.format(
            r.returncode, r.stdout[-2000:] + r.stderr[-2000:]), returncode=3)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert 'rk_wino4_pt_conv_out vector4' in r.stdout and 'rk_x6p_w4_input vw2' in r.stdout, r.stdout[-3000:]
