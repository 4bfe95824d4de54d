"""The BatchNorm kernels of csrc/kernels/bn.hip (bf16: F = rafiki_amd.ops.functional) and csrc/kernels/bnf.hip
(fp32: S = rafiki_amd.ops.f32) against the fp64 formulas of tests/bn_refs.py, stage by stage and channel by
channel.  tests/test_bn_refs.py anchors those formulas to torch autograd and shows that the tolerances used
here reject the plausible wrong formulas.

Every stage is fed from the reference, not from the kernel before it: coefficients are the fp32 roundings of
bn_refs.finalize in fp64, slot tables come from split_slots, partial-row tables from split_rows.  Every output
buffer is prefilled with NaN.  Tolerances are those of bn_refs (4 x the fp32 yardstick per channel; one bf16
rounding plus the yardstick for bf16 tensors; Frobenius 1e-5 over the well-conditioned channels for fp32
outputs).  No input leaves a sign or argmax decision inside the guard band (asserted), so nothing is masked.
Every figure is printed before it is asserted (pytest -s); the worst per entry point is printed at the end.
"""
import math

import pytest
import torch

import bn_refs as B

pytestmark = pytest.mark.gpu

DEV = 'cuda'
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
NAN = float('nan')
WORST = {}
SMALL = 100000          # elements: above it a shape runs one slot count, not all
POW2_SL = (1, 2, 4, 8)
ANY_SL = (1, 2, 3, 4, 5, 8)


@pytest.fixture(scope='module')
def ops():
    from rafiki_amd.ops import _lib, f32, functional
    _lib.lib()  # loud failure if the native library is missing
    yield functional, f32
    for entry in sorted(WORST):
        w = WORST[entry]
        print('WORST {:32s} rel err {:.3e}  e_ref {:.3e}  err / tol {:.3f}'.format(entry, w[0], w[1], w[2]))


@pytest.fixture(autouse=True)
def _stop_after_a_fault():
    """A kernel fault is sticky: end the session at the first one instead of launching on a faulted device."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:
        pytest.exit('GPU fault: {}'.format(exc), returncode=3)


def _note(entry, rel, e, ratio):
    w = WORST.get(entry, (0.0, 0.0, 0.0))
    WORST[entry] = (max(w[0], rel), e if ratio >= w[2] else w[1], max(w[2], ratio))


def _d(t, dtype=None):
    return None if t is None else t.to(DEV, dtype) if dtype else t.to(DEV)


def _nan(shape, dtype=F32):
    return torch.full(tuple(shape), NAN, dtype=dtype, device=DEV)


def _ratio(err, tol):
    assert bool((err[tol == 0] == 0).all()), 'an output that must be exact is not'
    live = tol > 0
    return float((err[live] / tol[live]).max()) if bool(live.any()) else 0.0


def check_f32(entry, tag, got, ref, ref32, noise=None, floor=None):
    """An fp32 output, per channel: err_c <= 4 * max(e_ref * max|ref_c|, a_c) (+ what the reference itself is
    uncertain by, where bn_refs names that), and Frobenius <= 1e-5."""
    got = got.detach().to(ref.device, F64)
    assert not bool(got.isnan().any()), (tag, 'unwritten elements')
    tol, e = B.tol_f32(ref32, ref, noise, floor)
    errc, mag = B.chan_err(got, ref), B.chan_mag(ref)
    rel = float((errc / mag.clamp_min(1e-300))[mag > 0].max()) if bool((mag > 0).any()) else 0.0
    fro = B.frob(got, ref)
    print('{} {}: rel err {:.3e}  e_ref {:.3e}  frobenius {:.3e}'.format(entry, tag, rel, e, fro), end='')
    ratio = _ratio(errc, tol)
    print('  err / tol {:.3f}'.format(ratio))
    _note(entry, rel, e, ratio)
    assert ratio <= 1.0, (entry, tag, ratio, int((errc / tol.clamp_min(1e-300)).argmax()))
    assert fro <= B.FROB, (entry, tag, fro)


def check_bf16(entry, tag, got, ref, ref32, noise=None):
    """A bf16 tensor, elementwise: |got - ref| <= 2^-8 |ref| + 4 a_c."""
    assert got.dtype == BF16
    got = got.detach().to(ref.device, F64)
    assert not bool(got.isnan().any()), (tag, 'unwritten elements')
    tol = B.tol_bf16(ref32, ref, noise)
    err = (got - ref).abs()
    _, e = B.yardstick(ref32, ref)
    ratio = _ratio(err, tol)
    rel = float(err.max() / ref.abs().max().clamp_min(1e-300))
    print('{} {}: max err / max|ref| {:.3e}  e_ref {:.3e}  err / tol {:.3f}'.format(entry, tag, rel, e, ratio))
    _note(entry, rel, e, ratio)
    assert ratio <= 1.0, (entry, tag, ratio)


def _settled(c, pool, act, slope=B.SLOPE, co=None):
    co = c.coeffs if co is None else co
    assert B.ambiguous(c.y, co[2], co[3], pool, act, slope) == 0


def _combos(shape, neg=False):
    out = [(p, a, B.SLOPE) for p in B.pools_of(shape) for a in B.acts_of(shape)]
    if neg and tuple(shape) == B.NEG_SLOPE_SHAPE:
        out.append((True, B.ACT_LRELU, B.NEG_SLOPE))
    return out


def _slot_counts(shape, counts=POW2_SL):
    return counts if math.prod(shape) <= SMALL else (2,)


def _ydev(c):
    return _d(c.y, BF16 if c.kind == 'bf16' else None)


def _fin_refs(c, sums, count=None, gamma=True, beta=True, running=True, hyper=None, dsums=None, ill_only=False):
    eps, mom = (c.eps, c.momentum) if hyper is None else B.HYPER[hyper]
    g, b = (c.gamma if gamma else None), (c.beta if beta else None)
    rm, rv = (c.rm, c.rv) if running else (None, None)
    n = c.count if count is None else count
    ref, r32, noise = B.finalize_refs(sums, n, g, b, eps, rm, rv, mom, dsums, ill_only)
    return (ref, noise) if noise is not None else ref, r32, (g, b, rm, rv, eps, mom, n)


def _check_fin(entry, tag, got, ref, r32):
    ref, noise = ref if len(ref) == 2 else (ref, (None,) * 6)
    for name, a, r, y, nz in zip(('mean', 'rstd', 'scale', 'shift', 'rm', 'rv'), got, ref, r32, noise):
        if r is not None:
            check_f32(entry, '{} {}'.format(tag, name), a, r, y, nz)


# ------------------------------------------------------------------------------------------- statistics
@pytest.mark.parametrize('shape', B.BF16_SHAPES + tuple(B.ROW_SHAPE + (C,) for C in B.ROW_CHANNELS))
def test_channel_stats(ops, shape):
    F, _ = ops
    c = B.case('bf16', shape)
    part = F.channel_stats(_ydev(c).view(-1, shape[3]))
    assert part.shape[0] == F.bn_partial_rows(c.count, shape[3])
    got = part.double().sum(0)
    for i, (r, y, fl) in enumerate(zip(*B.stats_refs(c.y))):
        check_f32('F.channel_stats', '{} {}'.format(shape, ('sum', 'sumsq')[i]), got[i], r, y, floor=fl)


@pytest.mark.parametrize('shape', B.F32_SHAPES)
def test_col_stats(ops, shape):
    """(sum a, sum a^2), (sum a, sum a*b), and both onto a table whose every slot is non-zero: only slot 0 may
    change, and by exactly the sums."""
    _, S = ops
    c = B.case('f32', shape)
    C = shape[3]
    a, b = c.y.reshape(-1, C), c.dout[False].reshape(-1, C)
    for two in (False, True):
        other = b if two else a
        ref = torch.stack([B.colsum(a.double()), B.colsum(a.double() * other.double())])
        r32 = [[B.colsum(a, k) for k in range(B.ORDERS)],
               [B.colsum(B._prod(a, other, F32, k), k) for k in range(B.ORDERS)]]
        floor = B.sum_floor(a), B.sum_floor(a.double() * other.double())
        for SL in POW2_SL:
            for onto in (False, True):
                base = B.split_slots(c.sums * 0.5, SL, 7 + SL) if onto else torch.zeros(SL, 2, C, dtype=F64)
                acc = _d(base.clone())
                S.col_stats(_d(a), acc, _d(b) if two else None)
                assert torch.equal(acc[1:].cpu(), base[1:])
                got = acc[0].cpu() - base[0]
                for i in range(2):
                    check_f32('S.col_stats', '{} b={} SL={} onto={} row {}'.format(shape, two, SL, onto, i), got[i],
                              ref[i], r32[i], floor=floor[i])


# ------------------------------------------------------------------------------------------- finalize
def _finalize_fwd(F, c, table, refs, tag):
    ref, r32, (g, b, rm, rv, eps, mom, n) = refs
    C = c.shape[3]
    outs, drm, drv = _nan((4, C)), _d(rm), _d(rv)
    F.bn_finalize_fwd(_d(table), n, _d(g), _d(b), eps, drm, drv, mom, outs=outs)
    _check_fin('F.bn_finalize_fwd', tag, (outs[0], outs[1], outs[2], outs[3], drm, drv), ref, r32)


@pytest.mark.parametrize('R', B.ROW_COUNTS)
@pytest.mark.parametrize('C', B.ROW_CHANNELS)
def test_bn_finalize_fwd_rows(ops, C, R):
    """Every row count around the 8-rows-at-a-time loop of rows_sum2 (R >= 113), the 16 row lanes and the 512-row
    cut of _shrink_rows, at C = 8 (half a block idle), 24 (C % 16 != 0) and 520 (33 blocks).

    R = 513 and 2000 first pass through an fp32 fold, and E[x^2] - mean^2 amplifies its roundings in the two
    ill-conditioned channels.  Measured on an MI355X against the 4 x yardstick margin: rstd of the constant
    channel 3.1e-4 relative (651 x the margin at C = 8, R = 513; the yardstick happens to get var = 0 exactly
    there) and 1.5e-4 (1.1 x, R = 2000); of the mean = 8 std channel 8.7e-7 (1.8 x, C = 24, R = 513).  Those two
    channels, at R > 512 only, are therefore granted the fold's worst case on top (bn_refs.ROWS_NOISE: the sums
    within 10 * 2^-24 of sum |row|, pushed through the formula; 2.5e-2 relative for that rstd); every other
    channel and every R <= 512 keep the 4 x margin."""
    F, _ = ops
    c = B.row_case(C)
    table, sums = B.split_rows(c.sums, R, R)
    refs = _fin_refs(c, sums, dsums=B.rows_noise(table), ill_only=R > 512)
    _finalize_fwd(F, c, table, refs, 'C={} R={}'.format(C, R))


@pytest.mark.parametrize('variant', ['hyper0', 'hyper1', 'no_gamma', 'no_beta', 'count_1', 'no_running'])
@pytest.mark.parametrize('shape', [(3, 5, 3, 24), (4, 8, 8, 64), (2, 2, 2, 2056)])
def test_bn_finalize_fwd_variants(ops, shape, variant):
    """Both (eps, momentum) pairs, gamma / beta absent, no running statistics, and count == 1 (one pixel: the
    variance is 0 up to the rounding of the table, which can put it below 0, and the running variance keeps the
    biased value)."""
    F, _ = ops
    c = B.case('bf16', shape)
    sums, count = c.sums, None
    if variant == 'count_1':
        sums, count = torch.stack(B.stats(c.y[:1, :1, :1])), 1
    table, sums = B.split_rows(sums, 5, 11)
    refs = _fin_refs(c, sums, count, gamma=variant != 'no_gamma', beta=variant != 'no_beta',
                     running=variant != 'no_running', hyper={'hyper0': 0, 'hyper1': 1}.get(variant))
    _finalize_fwd(F, c, table, refs, '{} {}'.format(shape, variant))


@pytest.mark.parametrize('shape', B.BF16_SHAPES)
def test_bn_eval_coeffs(ops, shape):
    F, _ = ops
    c = B.case('bf16', shape)
    C = shape[3]
    for g, b in ((c.gamma, c.beta), (None, c.beta), (c.gamma, None)):
        ref, r32 = B.eval_coeffs(g, b, c.rm, c.rv, c.eps, F64), B.eval_coeffs(g, b, c.rm, c.rv, c.eps, F32)
        outs = _nan((4, C))
        F.bn_eval_coeffs(_d(g), _d(b), _d(c.rm), _d(c.rv), c.eps, outs=outs)
        for i, name in enumerate(('scale', 'shift')):
            check_f32('F.bn_eval_coeffs', '{} gamma={} beta={} {}'.format(shape, g is not None, b is not None, name),
                      outs[2 + i], ref[i], r32[i])


@pytest.mark.parametrize('shape', B.F32_SHAPES)
def test_f32_bn_finalize(ops, shape):
    _, S = ops
    c = B.case('f32', shape)
    for hyper in (0, 1):
        ref, r32, (g, b, rm, rv, eps, mom, n) = _fin_refs(c, c.sums, hyper=hyper)
        for SL in POW2_SL:
            co, drm, drv = _nan((4, shape[3])), _d(rm), _d(rv)
            S.bn_finalize(_d(c.y), _d(B.split_slots(c.sums, SL, SL)), n, _d(g), _d(b), eps, drm, drv, mom, coeffs=co)
            _check_fin('S.bn_finalize', '{} hyper={} SL={}'.format(shape, hyper, SL),
                       (co[0], co[1], co[2], co[3], drm, drv), ref, r32)


# ------------------------------------------------------------------------------------------- forward
def _out_shape(shape, pool):
    N, H, W, C = shape
    return (N, H // 2, W // 2, C) if pool else shape


def _fwd_refs(c, co, pool, act, slope):
    return B.fwd(c.y, co[2], co[3], pool, act, slope, F64), B.fwd(c.y, co[2], co[3], pool, act, slope, F32)


def _edge_moved(y):
    """y with the rows / columns that no floor-mode window covers replaced: a pooled output must not notice."""
    N, H, W, C = y.shape
    y2 = y.clone()
    y2[:, 2 * (H // 2):] = 3.0
    y2[:, :, 2 * (W // 2):] = -3.0
    return y2


@pytest.mark.parametrize('shape', B.BF16_SHAPES)
def test_bn_act_fwd(ops, shape):
    F, _ = ops
    c = B.case('bf16', shape)
    y, co = _ydev(c), _d(c.coeffs)
    for pool, act, slope in _combos(shape, neg=True):
        ref, r32 = _fwd_refs(c, c.coeffs, pool, act, slope)
        out = _nan(_out_shape(shape, pool), BF16)
        F.bn_act_fwd(y, co[2], co[3], pool=pool, act=act, slope=slope, out=out)
        check_bf16('F.bn_act_fwd', '{} pool={} act={} slope={}'.format(shape, pool, act, slope), out, ref, r32)
        if pool and (shape[1] % 2 or shape[2] % 2):
            out2 = F.bn_act_fwd(_edge_moved(y), co[2], co[3], pool=pool, act=act, slope=slope)
            assert torch.equal(out, out2)


def _acc_counts(shape):
    return ANY_SL if math.prod(shape) <= SMALL else (2,)


@pytest.mark.parametrize('shape', B.BF16_SHAPES)
def test_bn_act_fwd_acc(ops, shape):
    """The fused finalize + apply: coefficients, running statistics and the output from a slot table, with every
    slot count 1..8 its launcher takes (acc_sums predicates s < SL).  C > 1024 is refused by design."""
    F, _ = ops
    from rafiki_amd.ops._lib import KernelError
    c = B.case('bf16', shape)
    y, C = _ydev(c), shape[3]
    ref_fin, r32_fin, (g, b, rm, rv, eps, mom, n) = _fin_refs(c, c.sums)
    if C > 1024:
        out, co, drm = _nan(shape, BF16), _nan((4, C)), _d(rm)
        with pytest.raises(KernelError):
            F.bn_act_fwd_acc(y, _d(B.split_slots(c.sums, 1, 1)), n, _d(g), _d(b), eps, drm, _d(rv), mom, coeffs=co,
                             out=out)
        torch.cuda.synchronize()
        assert bool(out.isnan().all()) and bool(co.isnan().all()) and torch.equal(drm.cpu(), rm)
        return
    for pool, act, slope in _combos(shape):
        ref, r32 = _fwd_refs(c, c.coeffs, pool, act, slope)
        for SL in _acc_counts(shape):
            out, co, drm, drv = _nan(_out_shape(shape, pool), BF16), _nan((4, C)), _d(rm), _d(rv)
            F.bn_act_fwd_acc(y, _d(B.split_slots(c.sums, SL, SL)), n, _d(g), _d(b), eps, drm, drv, mom, coeffs=co,
                             pool=pool, act=act, slope=slope, out=out)
            tag = '{} pool={} act={} SL={}'.format(shape, pool, act, SL)
            _check_fin('F.bn_act_fwd_acc', tag, (co[0], co[1], co[2], co[3], drm, drv), ref_fin, r32_fin)
            check_bf16('F.bn_act_fwd_acc', tag + ' out', out, ref, r32)


@pytest.mark.parametrize('shape', B.F32_SHAPES)
def test_f32_bn_fwd(ops, shape):
    _, S = ops
    c = B.case('f32', shape)
    y, C = _d(c.y), shape[3]
    ref_fin, r32_fin, (g, b, rm, rv, eps, mom, n) = _fin_refs(c, c.sums)
    for pool, act, slope in _combos(shape, neg=True):
        ref, r32 = _fwd_refs(c, c.coeffs, pool, act, slope)
        for SL in _slot_counts(shape):
            out, co, drm, drv = _nan(_out_shape(shape, pool)), _nan((4, C)), _d(rm), _d(rv)
            S.bn_fwd(y, _d(B.split_slots(c.sums, SL, SL)), n, _d(g), _d(b), eps, drm, drv, mom, pool=pool, act=act,
                     slope=slope, coeffs=co, out=out)
            tag = '{} pool={} act={} slope={} SL={}'.format(shape, pool, act, slope, SL)
            _check_fin('S.bn_fwd', tag, (co[0], co[1], co[2], co[3], drm, drv), ref_fin, r32_fin)
            check_f32('S.bn_fwd', tag + ' out', out, ref, r32)


def _eval_co(c):
    sc, sh = B.eval_coeffs(c.gamma, c.beta, c.rm, c.rv, c.eps, F64)
    return torch.stack([sc, sh, sc, sh]).to(F32)       # rows 2, 3 as in a coefficient table


@pytest.mark.parametrize('shape', B.F32_SHAPES)
def test_f32_bn_eval(ops, shape):
    _, S = ops
    c = B.case('f32', shape)
    co = _eval_co(c)
    y, dco = _d(c.y), _d(co)
    for pool, act, slope in _combos(shape):
        ref, r32 = _fwd_refs(c, co, pool, act, slope)
        out = _nan(_out_shape(shape, pool))
        S.bn_eval(y, dco[2], dco[3], pool=pool, act=act, slope=slope, out=out)
        check_f32('S.bn_eval', '{} pool={} act={}'.format(shape, pool, act), out, ref, r32)
        if pool and (shape[1] % 2 or shape[2] % 2):
            assert torch.equal(out, S.bn_eval(_edge_moved(y), dco[2], dco[3], pool=pool, act=act, slope=slope))


@pytest.mark.parametrize('shape', [s for s in B.F32_SHAPES if math.prod(s) <= SMALL])
def test_f32_bn_eval_grp(ops, shape):
    """Three stacked batches, each with coefficients of its own, each against fp64 (not against S.bn_eval)."""
    _, S = ops
    c = B.case('f32', shape)
    co = _eval_co(c)
    ys = torch.stack([c.y, c.y.flip(0) * 0.5 + 0.25, -c.y.roll(1, 1)])
    ys[..., B.CONST] = B.CONST_Y
    scale = torch.stack([co[2], co[2] * 1.5, -co[2]])
    shift = torch.stack([co[3], co[3] - 0.25, co[3] + 0.5])
    for pool, act, slope in _combos(shape):
        out = _nan((3,) + tuple(_out_shape(shape, pool)))
        S.bn_eval_grp(_d(ys), _d(scale), _d(shift), pool=pool, act=act, slope=slope, out=out)
        for g in range(3):
            ref = B.fwd(ys[g], scale[g], shift[g], pool, act, slope, F64)
            r32 = B.fwd(ys[g], scale[g], shift[g], pool, act, slope, F32)
            check_f32('S.bn_eval_grp', '{} pool={} act={} group {}'.format(shape, pool, act, g), out[g], ref, r32)


# ------------------------------------------------------------------------------------------- backward
def _bwd_refs(c, pool, act, slope, sums=None, co=None, gamma=True, count=None, dsums=None, ill_only=False):
    """sums given (a table): known to 1e-15 of themselves unless dsums says otherwise."""
    if sums is not None and dsums is None:
        dsums = B.SLOT_NOISE * sums.abs()
    return B.bwd_refs(c.dout[pool], c.y, c.coeffs if co is None else co, c.gamma if gamma is True else gamma,
                      c.count if count is None else count, pool, act, slope, sums, dsums, ill_only)


def _check_bwd(entry, tag, c, dy, dg, db, refs, base=None):
    ref, r32, noise, floor = refs
    noise, floor = noise or (None,) * 3, floor or (None,) * 3
    (check_bf16 if c.kind == 'bf16' else check_f32)(entry, tag + ' dy', dy, ref[0], r32[0], noise[0])
    for name, got, r, ys, nz, fl, b0 in zip(('dgamma', 'dbeta'), (dg, db), ref[1:], r32[1:], noise[1:], floor[1:],
                                            base or (None, None)):
        if got is not None:
            if b0 is not None:          # accumulate=True: what was added onto the buffer, up to its fp32 rounding
                r, ys = r + b0.double(), [(y + b0).double() for y in ys]
            check_f32(entry, '{} {}'.format(tag, name), got, r, ys, nz, fl)


MODES = ('write', 'accumulate', 'none')


def _grad_bufs(c, mode):
    if mode == 'none':
        return None, None, None
    if mode == 'accumulate':
        return _d(c.dgamma0), _d(c.dbeta0), (c.dgamma0, c.dbeta0)
    C = c.shape[3]
    return _nan((C,)), _nan((C,)), None


def _modes(shape):
    return MODES if tuple(shape) in ((3, 5, 3, 24), (4, 8, 8, 64), (2, 7, 6, 32), (3, 5, 3, 12)) else MODES[:1]


@pytest.mark.parametrize('shape', B.BF16_SHAPES)
def test_bn_bwd(ops, shape):
    """reduce -> finalize -> apply (+ the odd-map edge kernel) over fp32 partial rows: no atomics, so a second run
    gives the same bits."""
    F, _ = ops
    c = B.case('bf16', shape)
    y, co, g = _ydev(c), _d(c.coeffs), _d(c.gamma)
    for pool, act, slope in _combos(shape, neg=True):
        _settled(c, pool, act, slope)
        dout, refs = _d(c.dout[pool], BF16), _bwd_refs(c, pool, act, slope)
        for mode in _modes(shape):
            dg, db, base = _grad_bufs(c, mode)
            dy = _nan(shape, BF16)
            F.bn_bwd(dout, y, co, g, pool=pool, act=act, slope=slope, dgamma=dg, dbeta=db, dy=dy,
                     accumulate=mode == 'accumulate')
            _check_bwd('F.bn_bwd', '{} pool={} act={} slope={} {}'.format(shape, pool, act, slope, mode), c, dy, dg, db,
                       refs, base)
            if mode == 'write':
                dg2, db2, dy2 = _nan(dg.shape), _nan(db.shape), _nan(shape, BF16)
                F.bn_bwd(dout, y, co, g, pool=pool, act=act, slope=slope, dgamma=dg2, dbeta=db2, dy=dy2)
                assert torch.equal(dy, dy2) and torch.equal(dg, dg2) and torch.equal(db, db2)
    if shape == (4, 8, 8, 64):      # gamma absent: k1 = rstd
        refs = _bwd_refs(c, True, B.ACT_RELU, B.SLOPE, gamma=None)
        dg, db, dy = _nan((64,)), _nan((64,)), _nan(shape, BF16)
        F.bn_bwd(_d(c.dout[True], BF16), y, co, None, pool=True, act=B.ACT_RELU, dgamma=dg, dbeta=db, dy=dy)
        _check_bwd('F.bn_bwd', '{} gamma=None'.format(shape), c, dy, dg, db, refs)


@pytest.mark.parametrize('R', B.ROW_COUNTS)
@pytest.mark.parametrize('C', B.ROW_CHANNELS)
def test_bn_bwd_part_rows(ops, C, R):
    """part=: the sums come from a given partial-row table (rows_sum2 and _shrink_rows on the backward side).

    As in test_bn_finalize_fwd_rows, the fp32 fold of R > 512 rows shows in the constant channel, whose
    sum dz*xhat = rstd * (sum dz*y - mean * sum dz) cancels completely: measured dgamma there 23 x the 4 x
    yardstick margin (C = 520, R = 513), 16 x (C = 8), 2.9 x and 1.2 x (C = 24, R = 513 and 2000).  The two
    ill-conditioned channels at R > 512 are granted the fold's worst case on top (bn_refs.ROWS_NOISE)."""
    F, _ = ops
    c = B.row_case(C)
    pool, act = R % 2 == 1, B.ACTS[R % 3]
    _settled(c, pool, act)
    table, sums = B.split_rows(B.bwd_sums(c.dout[pool], c.y, c.coeffs[2], c.coeffs[3], pool, act), R, R + 1)
    mode = MODES[(R // 2) % 3]
    (dg, db, base), dy = _grad_bufs(c, mode), _nan(c.shape, BF16)
    F.bn_bwd(_d(c.dout[pool], BF16), _ydev(c), _d(c.coeffs), _d(c.gamma), pool=pool, act=act, slope=B.SLOPE, dgamma=dg,
             dbeta=db, dy=dy, part=_d(table), accumulate=mode == 'accumulate')
    _check_bwd('F.bn_bwd(part=)', 'C={} R={} pool={} act={} {}'.format(C, R, pool, act, mode), c, dy, dg, db,
               _bwd_refs(c, pool, act, B.SLOPE, sums=sums, dsums=B.rows_noise(table), ill_only=R > 512), base)


@pytest.mark.parametrize('reduced', [False, True])
@pytest.mark.parametrize('shape', B.BF16_SHAPES)
def test_bn_bwd_acc(ops, shape, reduced):
    """The atomic reduce into a zeroed slot table + the fused finalize / apply; reduced=True: the apply half alone
    on a given table, with every slot count 1..8.  C = 96 runs with the table bn_acc_buffer sizes (a slot count of
    5 was refused by the reduce).  C > 1024 is refused by design."""
    F, _ = ops
    from rafiki_amd.ops._lib import KernelError
    c = B.case('bf16', shape)
    y, co, g, C = _ydev(c), _d(c.coeffs), _d(c.gamma), shape[3]
    if C > 1024:
        dy, dg = _nan(shape, BF16), _nan((C,))
        with pytest.raises(KernelError):
            F.bn_bwd_acc(_d(c.dout[False], BF16), y, co, g, torch.zeros(1, 2, C, dtype=F64, device=DEV), dgamma=dg,
                         dy=dy, reduced=reduced)
        torch.cuda.synchronize()
        assert bool(dy.isnan().all()) and bool(dg.isnan().all())
        return
    for pool, act, slope in _combos(shape):
        _settled(c, pool, act, slope)
        dout = _d(c.dout[pool], BF16)
        sums64 = B.bwd_sums(c.dout[pool], c.y, c.coeffs[2], c.coeffs[3], pool, act, slope)
        counts = (_acc_counts(shape) if reduced else POW2_SL) + (() if reduced else (F.bn_slots(C),))
        for SL in sorted(set(counts)):
            if reduced:
                table = B.split_slots(sums64, SL, SL + 2)
                acc, refs = _d(table), _bwd_refs(c, pool, act, slope, sums=table.sum(0))
            else:
                acc = F.bn_acc_buffer(C, DEV) if SL == F.bn_slots(C) else torch.zeros(SL, 2, C, dtype=F64, device=DEV)
                assert acc.shape[0] == SL
                refs = _bwd_refs(c, pool, act, slope)
            for mode in _modes(shape) if SL == 2 else MODES[:1]:
                dg, db, base = _grad_bufs(c, mode)
                dy = _nan(shape, BF16)
                acc_in = acc.clone()
                F.bn_bwd_acc(dout, y, co, g, acc_in, pool=pool, act=act, slope=slope, dgamma=dg, dbeta=db, dy=dy,
                             accumulate=mode == 'accumulate', reduced=reduced)
                _check_bwd('F.bn_bwd_acc(reduced={})'.format(reduced),
                           '{} pool={} act={} SL={} {}'.format(shape, pool, act, SL, mode), c, dy, dg, db, refs, base)
                if reduced:
                    assert torch.equal(acc_in, acc)


@pytest.mark.parametrize('reduced', [False, True])
@pytest.mark.parametrize('shape', B.F32_SHAPES)
def test_f32_bn_bwd(ops, shape, reduced):
    """bnf_bwd_reduce (power-of-two C <= 1024) or the col_stats route (no pool, no activation), then the apply.
    A channel count that is no power of two takes neither with pooling or an activation: ValueError."""
    _, S = ops
    c = B.case('f32', shape)
    y, co, g, C = _d(c.y), _d(c.coeffs), _d(c.gamma), shape[3]
    pow2 = C <= 1024 and not C & (C - 1)
    for pool, act, slope in _combos(shape, neg=True):
        dout = _d(c.dout[pool])
        if not pow2 and not reduced and (pool or act != B.ACT_NONE):
            dy = _nan(shape)
            with pytest.raises(ValueError):
                S.bn_bwd(dout, y, co, g, torch.zeros(1, 2, C, dtype=F64, device=DEV), pool=pool, act=act, dy=dy)
            assert bool(dy.isnan().all())
            continue
        _settled(c, pool, act, slope)
        sums64 = B.bwd_sums(c.dout[pool], c.y, c.coeffs[2], c.coeffs[3], pool, act, slope)
        for SL in _slot_counts(shape):
            if reduced:
                table = B.split_slots(sums64, SL, SL + 3)
                acc, refs = _d(table), _bwd_refs(c, pool, act, slope, sums=table.sum(0))
            else:
                acc, refs = torch.zeros(SL, 2, C, dtype=F64, device=DEV), _bwd_refs(c, pool, act, slope)
            for mode in _modes(shape) if SL == 2 else MODES[:1]:
                dg, db, base = _grad_bufs(c, mode)
                dy = _nan(shape)
                S.bn_bwd(dout, y, co, g, acc.clone(), pool=pool, act=act, slope=slope, dgamma=dg, dbeta=db, dy=dy,
                         accumulate=mode == 'accumulate', reduced=reduced)
                _check_bwd('S.bn_bwd(reduced={})'.format(reduced),
                           '{} pool={} act={} slope={} SL={} {}'.format(shape, pool, act, slope, SL, mode), c, dy, dg,
                           db, refs, base)


@pytest.mark.parametrize('shape', [(2, 4, 4, 4), (2, 7, 6, 32), (4, 8, 8, 64), (37, 1, 1, 784)])
def test_f32_bn_bwd_count_inf(ops, shape):
    """count = inf with unit coefficients (mean 0, rstd 1, scale 1, shift 0, gamma 1): dy is the activation mask /
    pool routing of dout, dbeta = sum dz; the uncovered edge of an odd map is exactly 0."""
    _, S = ops
    c = B.case('f32', shape)
    C = shape[3]
    co = torch.stack([torch.zeros(C), torch.ones(C), torch.ones(C), torch.zeros(C)])
    ones = torch.ones(C)
    for pool, act, slope in _combos(shape):
        _settled(c, pool, act, slope, co)
        refs = _bwd_refs(c, pool, act, slope, co=co, gamma=ones, count=math.inf)
        dg, db, dy = _nan((C,)), _nan((C,)), _nan(shape)
        S.bn_bwd(_d(c.dout[pool]), _d(c.y), _d(co), _d(ones), torch.zeros(2, 2, C, dtype=F64, device=DEV), pool=pool,
                 act=act, slope=slope, dgamma=dg, dbeta=db, dy=dy, count=math.inf)
        _check_bwd('S.bn_bwd(count=inf)', '{} pool={} act={}'.format(shape, pool, act), c, dy, dg, db, refs)
        if pool:
            N, H, W, _ = shape
            assert torch.count_nonzero(dy[:, 2 * (H // 2):]) == 0 and torch.count_nonzero(dy[:, :, 2 * (W // 2):]) == 0


# ------------------------------------------------------------------------------------------- large
@pytest.mark.parametrize('i', range(len(B.LARGE)))
def test_fused_entries_large(ops, i):
    """F.bn_act_fwd_acc and F.bn_bwd_acc (1024-block grids) at the sizes where bn_act_fwd_body /
    bn_bwd_apply_body enter their U-way unrolled, coefficient-hoisted sweep and hand over to the tail loop:
    1,114,112 vectors > 4 x 262,144 without pooling (U = 4), 540,672 > 2 x 262,144 with (U = 2).  ReLU; the
    fp64 reference is computed on the device."""
    F, _ = ops
    (shape, pool), c = B.LARGE[i], B.large_case(i)
    act, C = B.ACT_RELU, shape[3]
    N, H, W, _ = shape
    vectors = N * (H // 2 if pool else H) * (W // 2 if pool else W) * C // 8
    assert vectors > (2 if pool else 4) * 1024 * 256 and vectors % ((2 if pool else 4) * 1024 * 256) != 0
    yd, dd, cod = _d(c.y), _d(c.dout[pool]), _d(c.coeffs)
    assert B.ambiguous(yd, cod[2], cod[3], pool, act) == 0
    y, dout, g = yd.bfloat16(), dd.bfloat16(), _d(c.gamma)
    ref_fin, r32_fin, (_, b, rm, rv, eps, mom, n) = _fin_refs(c, c.sums)
    out, co, drm, drv = _nan(_out_shape(shape, pool), BF16), _nan((4, C)), _d(rm), _d(rv)
    F.bn_act_fwd_acc(y, _d(B.split_slots(c.sums, 2, 2)), n, g, _d(b), eps, drm, drv, mom, coeffs=co, pool=pool, act=act,
                     out=out)
    tag = '{} pool={}'.format(shape, pool)
    _check_fin('F.bn_act_fwd_acc', tag, (co[0], co[1], co[2], co[3], drm, drv), ref_fin, r32_fin)
    check_bf16('F.bn_act_fwd_acc', tag + ' out', out, B.fwd(yd, cod[2], cod[3], pool, act, dtype=F64),
               B.fwd(yd, cod[2], cod[3], pool, act, dtype=F32))
    ref, r32, _, floor = B.bwd_refs(dd, yd, cod, g, c.count, pool, act)
    dg, db, dy = _nan((C,)), _nan((C,)), _nan(shape, BF16)
    F.bn_bwd_acc(dout, y, cod, g, torch.zeros(2, 2, C, dtype=F64, device=DEV), pool=pool, act=act, dgamma=dg, dbeta=db,
                 dy=dy)
    check_bf16('F.bn_bwd_acc(reduced=False)', tag + ' dy', dy, ref[0], r32[0])
    check_f32('F.bn_bwd_acc(reduced=False)', tag + ' dgamma', dg, ref[1], r32[1], floor=floor[1])
    check_f32('F.bn_bwd_acc(reduced=False)', tag + ' dbeta', db, ref[2], r32[2], floor=floor[2])
