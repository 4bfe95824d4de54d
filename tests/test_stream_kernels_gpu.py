"""The three streaming kernels of the fp32 step at the shapes where their launch structure can go wrong, against the
fp64 references and with the bounds of the existing tests of the same entry points (tests/test_wino_pt_gpu.py for
rk_wino4_pt_conv_out, tests/test_bn_gpu.py for rk_bnf_bwd_reduce and rk_bnf_fwd; helpers reused by import).

rk_wino4_pt_conv_out: w4pt_conv_outv_kernel is a 256-thread block of 8 tiles x 64 channels per step (8-byte
accesses) that walks the tile groups of a grid capped at PT_OUT_CAP = 512 blocks.  A thread sums the 16 elements of
its tile and a wave its 2 tile lanes in fp32 (32 terms: within pt_refs.sums_exact's 64 and own_sums' 16 + 4
roundings); across the walk and the block the sums are fp64.  So the checks are those of tests/test_wino_pt_gpu.py,
unchanged: outputs element by element (the exact set to the bit), the slot sums against fp64 (the exact set to the
bit wherever sums_exact holds) and against the output the same launch wrote.  In addition the slots are prefilled
with known values: the launch must add onto them.
Cases: T = 3 (a tail group that is partly empty), N = 72 and N = 6 (a ragged 64-channel group), and T past one walk
of the capped grid.  The cap is 512 blocks, so with one channel block (N <= 64) a walk covers 4096 tiles (the 160 of
a smaller cap would not walk): Nb = 2050 (T = 8200) makes every block iterate at least twice and block 0 three
times, at N = 6 with 1 and 3 slabs and at N = 64 (every lane live) with 1 slab; Nb = 1030 (T = 4120, N = 64, 1 and 3
slabs) leaves all but the first three blocks at one step.  Every case: both layouts, slot masks 0 and 7, the four
flag sets, the exact and the random set.

rk_bnf_bwd_reduce (kernel unchanged: a raised grid regroups its fp32 partial sums and moved the training result;
the cases pin any later change of its grid): C = 512 with 5 pixel rows (with 64 blocks most have no row and must
add nothing); C = 4 on an odd pooled 5x5 map; blocks 1 and 64; SL 1 and 8.

rk_bnf_fwd pooled (kernel unchanged: loading the first window before the slot fold measured 1 us slower per step):
one vector in all at C = 4, 2x2 (every other thread is out of range), and a 6x6 map (the division path of idiv).
"""
import pytest
import torch

import bn_refs as B
import pt_refs as P
import sgemm_refs as G
import test_bn_gpu as TB
import test_wino_pt_gpu as WT
import wino_refs as R
from test_bn_gpu import ops  # noqa: F401  (fixture)
from test_wino_pt_gpu import S  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

DEV = 'cuda'
F64, F32 = torch.float64, torch.float32
NAN = float('nan')
FLAG_SETS = {'bias_relu_stats': R.BIAS | R.RELU | R.STATS, 'bnb': R.BNB, 'bnp': R.BNP, 'bias_lrelu': R.BIAS | R.LRELU}
# (Nb, H, W), N, slab counts
CO_CASES = {
    'tail_T3': ((3, 4, 4), 64, (1, 3)),
    'ragged_N72': ((3, 4, 4), 72, (1, 3)),
    'ragged_N6': ((3, 4, 4), 6, (1, 3)),
    'walk_N6': ((2050, 8, 8), 6, (1, 3)),
    'walk_N64': ((2050, 8, 8), 64, (1,)),
    'walk_part_N64': ((1030, 8, 8), 64, (1, 3)),
}
MODES = ('exact', 'random')


@pytest.fixture(autouse=True)
def _stop_after_a_fault():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:
        pytest.exit('GPU fault: {}'.format(exc), returncode=3)


def _prefill(mask, N):
    """A slot table of known non-zero values (exact in fp64 next to integer sums) and a NaN row past the mask."""
    acc = torch.empty((mask + 2, 2, N), dtype=F64)
    for sl in range(mask + 1):
        acc[sl, 0], acc[sl, 1] = 3.5 + sl, -1.25 - sl
    acc[mask + 1] = NAN
    return acc


def check_conv_out(S, sp, N, mode, flags, tmajor, nslab, mask):
    Nb, H, W = sp
    T = P.tiles(Nb, H, W)
    slab = 36 * T * N + 64 if nslab > 1 else 0
    p = WT._co_problem(mode, sp, N, nslab, slab)
    tag = 'rk_wino4_pt_conv_out stream ' + P.conv_out_form(N, WT.OUT_VW)
    what = '{} N {} {} flags {} tmajor {} nslab {} mask {}'.format(sp, N, mode, flags, tmajor, nslab, mask)
    bn = flags & (R.BNB | R.BNP)
    stats = bool(flags & (R.STATS | R.BNB | R.BNP))
    bias_d = p['ss_d'] if bn else p['bias_d'] if flags & R.BIAS else None
    gate_d = p['y_d'] if flags & R.BNB else p['y2_d'] if flags & R.BNP else None
    slope = WT.SLOPE if flags & R.LRELU else 0.0
    n = Nb * H * W * N
    out = WT._out(n, extra=2 * N + WT.PAD)
    pre = _prefill(mask, N) if stats else None
    acc = pre.to(DEV) if stats else None
    assert WT._run(S, tag, 'rk_wino4_pt_conv_out', 0, [out], S._p(p['yt_d']), S._p(out), S._p(bias_d), S._p(acc), mask,
                   S._p(gate_d), Nb, H, W, N, flags, nslab, slab, tmajor, slope)
    got = WT._host(out, n, tag).view(Nb, H, W, N)
    r = P.conv_out(p['yt'], Nb, H, W, N, flags, bias=p['ss'] if bn else p['bias'],
                   gate=p['y'] if flags & R.BNB else p['y2'] if flags & R.BNP else None, nslab=nslab, slab=slab,
                   tmajor=tmajor, slope=slope, exact=mode != 'random')
    if mode != 'random':
        assert P.exact_ok(r['S'] + 3.0)
    P.judge(tag, got, r['out'], r['tol'], mode, None, what)
    if not stats:
        return
    h = acc.to('cpu')
    assert bool(torch.isnan(h[mask + 1]).all()), '{}: wrote past the statistics slots'.format(tag)
    sums = (h[:mask + 1] - pre[:mask + 1]).sum(0)          # what the launch added onto the prefilled slots
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


@pytest.mark.parametrize('fset', sorted(FLAG_SETS))
@pytest.mark.parametrize('case', sorted(CO_CASES))
def test_conv_out_walk(S, case, fset):
    sp, N, slabs = CO_CASES[case]
    for i, mode in enumerate(MODES):
        for tmajor in (0, 1):
            for j, nslab in enumerate(slabs):   # every (layout, slabs) meets both slot masks over the two sets
                check_conv_out(S, sp, N, mode, FLAG_SETS[fset], tmajor, nslab, (0, 7)[(i + tmajor + j) % 2])
    if sp[0] > 64:
        WT._CO.clear()      # the large problems are not kept for the rest of the session


# ------------------------------------------------------------------------------------------- BN backward statistics
BWD_SHAPES = {'C512_5rows': ((5, 1, 1, 512), False), 'C512_5rows_pooled': ((5, 2, 2, 512), True),
              'C4_odd': ((2, 5, 5, 4), False), 'C4_odd_pooled': ((2, 5, 5, 4), True)}
_BWD = {}


def _bwd_case(name):
    """The case and its fp64 / fp32-yardstick sums, computed once."""
    if name not in _BWD:
        shape, pool = BWD_SHAPES[name]
        c = B.Case('f32', shape, decide=[(pool, B.ACT_RELU, B.SLOPE)])
        co, args = c.coeffs, (pool, B.ACT_RELU, B.SLOPE)
        assert B.ambiguous(c.y, co[2], co[3], *args) == 0
        ref = B.bwd_sums(c.dout[pool], c.y, co[2], co[3], *args)
        r32 = [B.bwd_sums(c.dout[pool], c.y, co[2], co[3], *args, dtype=F32, order=k) for k in range(B.ORDERS)]
        dz = B.dz_of(c.dout[pool], c.y, co[2], co[3], *args)
        _BWD[name] = (c, ref, r32, (B.sum_floor(dz), B.sum_floor(dz * c.y.to(F64))))
    return _BWD[name]


@pytest.mark.parametrize('SL', (1, 8))
@pytest.mark.parametrize('blocks', (1, 64))
@pytest.mark.parametrize('name', sorted(BWD_SHAPES))
def test_bnf_bwd_reduce_sums(ops, name, blocks, SL):
    from rafiki_amd.ops import _lib
    _, Sf = ops
    (shape, pool), (c, ref, r32, floor) = BWD_SHAPES[name], _bwd_case(name)
    Nb, H, W, C = shape
    acc = torch.zeros(SL, 2, C, dtype=F64, device=DEV)
    y, dout, co = c.y.to(DEV), c.dout[pool].to(DEV), c.coeffs.to(DEV)
    _lib.call('rk_bnf_bwd_reduce', Sf._p(dout), Sf._p(y), Sf._p(co), Sf._p(acc), SL, blocks, Nb, H, W, C, int(pool),
              B.ACT_RELU, B.SLOPE, Sf._s())
    torch.cuda.synchronize()
    got = acc.cpu().sum(0)
    for i, what in enumerate(('sum dz', 'sum dz*y')):
        TB.check_f32('rk_bnf_bwd_reduce', '{} blocks={} SL={} {}'.format(name, blocks, SL, what), got[i], ref[i],
                     [r[i] for r in r32], floor=floor[i])


# ------------------------------------------------------------------------------------------- BN forward, pooled
@pytest.mark.parametrize('shape', [(1, 2, 2, 4), (2, 6, 6, 64)])
def test_bnf_fwd_pooled_small_maps(ops, shape):
    _, Sf = ops
    c = B.case('f32', shape)
    y, C = c.y.to(DEV), shape[3]
    ref_fin, r32_fin, (g, b, rm, rv, eps, mom, n) = TB._fin_refs(c, c.sums)
    oshape = TB._out_shape(shape, True)
    for act in B.acts_of(shape):
        ref, r32 = TB._fwd_refs(c, c.coeffs, True, act, B.SLOPE)
        for SL in (1, 8):       # train mode: coefficients and running statistics from the slots, then the output
            out, co, drm, drv = TB._nan(oshape), TB._nan((4, C)), TB._d(rm), TB._d(rv)
            Sf.bn_fwd(y, TB._d(B.split_slots(c.sums, SL, SL)), n, TB._d(g), TB._d(b), eps, drm, drv, mom, pool=True,
                      act=act, slope=B.SLOPE, coeffs=co, out=out)
            tag = '{} pooled act={} SL={}'.format(shape, act, SL)
            TB._check_fin('rk_bnf_fwd', tag, (co[0], co[1], co[2], co[3], drm, drv), ref_fin, r32_fin)
            TB.check_f32('rk_bnf_fwd', tag + ' out', out, ref, r32)
        eco = TB._eval_co(c)    # eval mode: scale / shift given
        eref, er32 = TB._fwd_refs(c, eco, True, act, B.SLOPE)
        out = TB._nan(oshape)
        Sf.bn_eval(y, TB._d(eco[2]), TB._d(eco[3]), pool=True, act=act, slope=B.SLOPE, out=out)
        TB.check_f32('rk_bnf_fwd', '{} pooled eval act={}'.format(shape, act), out, eref, er32)
