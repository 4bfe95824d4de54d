"""Every fused Winograd conv, weight-gradient and weight-transform variant (csrc/kernels/winograd.hip,
winograd4.hip, wino_wt.h) against the fp64 references of tests/wino_refs.py (anchored and shown to bite in
tests/test_wino_refs.py).  The entry points are called directly, each launch once.

Judging.  The exact sets (integer x, an integer-valued U handed to the kernel as is, blocked variants through
w4b_index; ``exact_w`` for the F(2x2) weight transform) must come back bit for bit.  RANDOM is held element by
element to the hard tolerance n * 2^-23 * S and, per output channel and per in-tile position (weight gradient: per
output channel and per tap), to sgemm_refs.YARD times the error of the same algorithm in plain fp32 on the CPU.
Statistics are judged twice: against the fp64 reference's sums, and against the sums of the output the same launch
wrote (wino_refs.own_sums), which notices an element counted twice or a masked one counted.

Guards.  Every output is NaN-prefilled and followed by NaN guard rows (between the groups of a grouped launch too)
that must still be NaN; every operand (x, u, bias, gate, pro, dy) is a view 64 floats inside a larger NaN-filled
storage.  A NaN in the output is an unwritten element or an over-read.  The kernels bound their x / u / y (dy) accesses
by buffer descriptors, which return zero and drop stores out of range: for those three the arena proves less than
for the plainly addressed bias, gate, pro, statistics and weight-gradient output.

A launcher refusal is predicted by wino_refs.expected_status and asserted, never skipped.  The worst error /
tolerance and yardstick ratio per entry point and variant are printed at the end (pytest -s) with the launches
checked and refusals asserted.

Measured on an MI355X, worst over the sweep (error / hard tolerance, yardstick ratio against the gate of 4); the
variants of one entry point run the same arithmetic in the same order and gave the same figures:
    rk_wino_conv_grp v0-1, rk_wino2s_conv_grp v0-3   0.024, 1.44   grouped 0.027, 1.71   statistics 0.071
    rk_wino4_conv_grp v0-5                           0.0085, 2.68  grouped 0.0096, 2.35  statistics 0.045
    rk_wino4_conv_grp v3-5, normalise-on-load        0.0039, 2.02                        statistics 0.033
    rk_wino_wgrad                                    0.054, 1.50
    rk_wino4_wgrad v0-2                              0.0071, 2.17  with xpro (v0, v1) 0.0036, 2.22
    rk_wino_weights 0.26   rk_wino4_weights 0.21   rk_wino4b_weights 0.21   (no yardstick: element bound only)
1893 launches checked, 386 refusals asserted; every exact set came back bit for bit.
"""
import re

import pytest
import torch

import sgemm_refs as G
import wino_refs as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
F64, F32 = torch.float64, torch.float32
NAN = float('nan')
PAD = 64
COUNT = {}
IDS = lambda v: '-'.join(map(str, v)) if isinstance(v, tuple) else str(v)   # noqa: E731
W2, W2S, W4 = 'rk_wino_conv_grp', 'rk_wino2s_conv_grp', 'rk_wino4_conv_grp'
WEIGHTS = {'rk_wino_weights': 2, 'rk_wino4_weights': 4, 'rk_wino4b_weights': 4}
WGRADS = [('rk_wino_wgrad', 0, False), ('rk_wino4_wgrad', 0, False), ('rk_wino4_wgrad', 1, False),
          ('rk_wino4_wgrad', 2, False), ('rk_wino4_wgrad', 0, True), ('rk_wino4_wgrad', 1, True)]


@pytest.fixture(scope='module')
def S():
    from rafiki_amd.ops import _lib, f32
    _lib.lib()   # loud failure if the native library is missing
    yield f32
    Prob._cache.clear()
    for tag in sorted(set(R.WORST) | set(COUNT)):
        ran, refused = COUNT.get(tag, COUNT.get(tag.replace(' sums', ''), (0, 0)))
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


# ------------------------------------------------------------------------------------------ helpers
def _tag(entry, variant, pro=False):
    return '{} v{}{}'.format(entry, variant, ' pro' if pro else '')


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


def _nan_free_guards(host, spans, what):
    """host: the whole flat buffer; spans [(lo, hi)] the written ranges: everything else must still be NaN."""
    keep = torch.ones(host.numel(), dtype=torch.bool)
    for lo, hi in spans:
        keep[lo:hi] = False
    assert bool(torch.isnan(host[keep]).all()), '{}: wrote outside the output'.format(what)


class Prob:
    """One conv problem on the host and the device: operands in NaN arenas, the fp64 accumulator, S, the yardstick."""
    _cache = {}

    @classmethod
    def get(cls, mode, MO, shape, pro=False, salt=0):
        key = (mode, MO, tuple(shape), pro, salt)
        if key not in cls._cache:
            cls._cache[key] = cls(*key)
        return cls._cache[key]

    def __init__(self, mode, MO, shape, pro, salt):
        self.mode, self.MO, self.shape = mode, MO, shape
        Nb, H, W, C, N = shape
        self.x, self.U, self.pro = R.conv_problem(mode, MO, shape, pro, salt)
        self.acc = R.fused_conv(self.x, self.U, MO, pro=self.pro)
        self.S = R.fused_conv(self.x, self.U, MO, pro=self.pro, absval=True)
        if mode != 'random':
            assert R.exact_ok(self.S + 3.0), 'exact-set precondition: S >= 2^24'
        self.yard = R.fused_conv(self.x.to(F32), self.U.to(F32), MO, pro=self.pro).to(F64) if mode == 'random' else None
        self.n = R.n_fwd(MO, C, pro=pro)
        self.x_d = _arena(self.x)
        self.pro_d = _arena(torch.cat(self.pro)) if pro else None
        self._u = {}
        seed = 13 * sum(shape) + MO
        self.bias = R.draw_bias(mode, seed, N)
        self.scale, self.shift = G.draw_scale_shift(seed + 1, N)
        self.y = G.draw_decision(seed + 2, (Nb * H * W, N))
        self.y2 = G.draw_pool_y(seed + 3, Nb, H, W, N, self.scale)
        assert G.decisions_inexact(self.y, self.scale, self.shift) == 0
        assert G.decisions_inexact(self.y2, self.scale, self.shift) == 0
        self._dev = {}

    def u_d(self, blocked):
        if blocked not in self._u:
            self._u[blocked] = _arena(R.to_blocked(self.U) if blocked else self.U)
        return self._u[blocked]

    def dev(self, name):
        if name not in self._dev:
            t = {'bias': self.bias, 'ss': torch.cat([self.scale, self.shift]), 'y': self.y, 'y2': self.y2}[name]
            self._dev[name] = _arena(t)
        return self._dev[name]


def fwd_launch(S, entry, variant, shape, x_d, u_d, flags, *, bias=None, stats=False, gate=None, pro=None, groups=1,
               gx=0, gu=0, gbias=0, tag=None, alloc=None):
    """One launch into a NaN-prefilled buffer whose groups are 2 N guard floats apart.  Returns (status, the groups'
    outputs [groups][Nb][Ho][Wo][N] fp64 on the host or None, the statistics [2][N] summed over the slots or None).
    alloc: the floats to allocate for a launch that must be refused (its claimed shape may be far larger)."""
    from rafiki_amd.ops import _lib
    Nb, H, W, C, N = shape
    Ho, Wo = (H // 2, W // 2) if flags & R.POOL else (H, W)
    ysize = max(Nb * Ho * Wo * N, 1)
    gy = ysize + 2 * N
    buf = torch.full((alloc or groups * gy + PAD,), NAN, dtype=F32, device=DEV)
    slots = S.bn_slots(N) if 0 < N <= 4096 else 1
    acc = None
    if stats:   # one more row than the slot mask reaches: it must still be NaN afterwards
        acc = torch.zeros((slots + 1, 2, min(N, 4096)), dtype=F64, device=DEV)
        acc[slots] = NAN
    args = [S._p(x_d), S._p(u_d), S._p(buf), S._p(bias), S._p(acc), slots - 1 if stats else 0, S._p(gate), Nb, H, W, C, N,
            flags, variant, groups, gx, gu, gy, gbias]
    if entry == W4:
        args.append(S._p(pro))
    st = _status(lambda: _lib.call(entry, *args, S._s()))
    tag = tag or _tag(entry, variant, pro is not None)
    if st != 0:
        assert bool(torch.isnan(buf).all()), 'a refused launch wrote something'
        _count(tag, False)
        return st, None, None
    torch.cuda.synchronize()
    _count(tag, True)
    host = buf.to('cpu', F64)
    _nan_free_guards(host, [(g * gy, g * gy + ysize) for g in range(groups)], tag)
    out = torch.stack([host[g * gy:g * gy + ysize].view(Nb, Ho, Wo, N) for g in range(groups)])
    sums = None
    if stats:
        h = acc.to('cpu')
        assert bool(torch.isnan(h[slots]).all()), '{}: wrote past the statistics slots'.format(tag)
        sums = h[:slots].sum(0)
    return 0, out, sums


def check_epilogue(S, entry, variant, p, flags, pro=False):
    """One launch of one flag combination on problem p, judged against the fp64 epilogue reference."""
    MO, blocked = R.FWD[(entry, variant)][0], R.FWD[(entry, variant)][3]
    Nb, H, W, C, N = p.shape
    mode, tag = p.mode, _tag(entry, variant, pro)
    what = '{} {} flags {}'.format(p.shape, mode, flags)
    bn = flags & (R.BNB | R.BNP)
    bias_d = p.dev('ss') if bn else p.dev('bias') if flags & R.BIAS else None
    gate_d = p.dev('y') if flags & R.BNB else p.dev('y2') if flags & R.BNP else None
    stats = bool(flags & (R.STATS | R.BNB | R.BNP))
    want = R.expected_status(entry, variant, p.shape, flags=flags, bias=bias_d is not None, stats=stats,
                             gate=gate_d is not None, pro=pro)
    st, out, sums = fwd_launch(S, entry, variant, p.shape, p.x_d, p.u_d(blocked), flags, bias=bias_d, stats=stats,
                               gate=gate_d, pro=p.pro_d)
    assert st == want, '{} {}: status {} (expected {})'.format(tag, what, st, want)
    if st != 0:
        return
    exact = mode != 'random'
    if flags & R.POOL:
        ref, tol = R.pooled(p.acc, p.S, p.n, p.bias)
        yard = R.pool2(G.f32r(p.yard + p.bias).clamp_min(0)) if not exact else None
        R.judge(tag, out[0], ref, tol, mode, yard, what, MO=MO // 2)
        return
    kw = {}
    if flags & R.BIAS:
        kw['bias'] = p.bias
    if flags & R.RELU:
        kw['act'] = G.ACT_RELU
    ykw = dict(kw)
    if flags & R.STATS:
        kw['stats'] = True
    if flags & R.BNB:
        kw['bnb'] = (p.y, p.scale, p.shift)
    if flags & R.BNP:
        kw['bnp'] = (p.y2, p.scale, p.shift, Nb, H, W)
    r = G.epilogue(p.acc.reshape(-1, N), p.S.reshape(-1, N), p.n, exact=exact, **kw)
    yard = None
    if not exact:
        yard = G.epilogue32(p.yard.reshape(-1, N), **ykw)
        if flags & R.BNB:
            yard = yard * G.bnb_mask(p.y, p.scale, p.shift).to(F64)
        yard = yard.reshape(Nb, H, W, N)
    R.judge(tag, out[0], r['out'].reshape(Nb, H, W, N), r['tol'].reshape(Nb, H, W, N), mode, yard, what, MO=MO)
    if not stats:
        return
    # the terms the epilogue summed, from the reference (for the exactness rule) and from the output it wrote
    o = out[0].reshape(-1, N)
    if flags & R.STATS:
        v, second, unit = p.acc.reshape(-1, N) + (p.bias if flags & R.BIAS else 0.0), None, 1.0
        own = None if flags & R.RELU else R.own_sums(o, MO)     # behind a ReLU the output no longer holds v
    elif flags & R.BNB:
        v, second, unit = r['out'], p.y, 1.0 / 64
        own = R.own_sums(o, MO, second=p.y)
    else:
        pos, yb = G.bnp_route(p.y2, p.scale, p.shift, Nb, H, W)
        v, second, unit = r['out'] * pos.to(F64), yb, 1.0 / 64
        own = R.own_sums(o * pos.to(F64), MO, second=yb)
    R.judge_sums(tag + ' sums', sums, r['sums'], r['sums_tol'], mode, v, MO, what, second, unit)
    if own is not None:
        R.judge_sums(tag + ' sums', sums, own[0], own[1], mode, v, MO, what + ' against its own output', second, unit)


# ------------------------------------------------------- 1. every forward variant x shape x epilogue
@pytest.mark.parametrize('si', range(len(R.SHAPES4)))
@pytest.mark.parametrize('entry,variant', sorted(R.FWD), ids=IDS)
def test_forward_variants_and_epilogues(S, entry, variant, si):
    """Every flag combination with a compile-time instantiation (none, STATS, BIAS | RELU, BNB, BNP, POOLED) and
    what falls to the run-time flags (bias alone, ReLU alone, bias + STATS, ReLU + STATS, bias + ReLU + STATS) on
    the exact set and on RANDOM.  rk_wino_conv_grp refuses POOLED; that is asserted."""
    MO = R.FWD[(entry, variant)][0]
    shape = R.shapes(MO)[si]
    for mode in ('exact', 'random'):
        p = Prob.get(mode, MO, shape)
        for flags in R.FLAG_SETS:
            check_epilogue(S, entry, variant, p, flags)


@pytest.mark.parametrize('si', range(len(R.SHAPES4)))
@pytest.mark.parametrize('variant', R.PRO_VARIANTS)
def test_normalise_on_load_rows(S, variant, si):
    """The three PRO rows of W4_ROWS against fp64 conv(relu(x * scale + shift)), scale and shift of both signs, plain
    and with statistics; (2, 4, 4, 512, 32) is W4_PRO_MAXC channels.  Everything else the PRO rows refuse."""
    shape = R.shapes(4)[si]
    for mode in ('exact', 'random'):
        p = Prob.get(mode, 4, shape, pro=True)
        for flags in (0, R.STATS, R.BIAS | R.RELU, R.POOLED, R.BNB):
            check_epilogue(S, W4, variant, p, flags, pro=True)


# --------------------------------------------------------------------------------- grouped launches
@pytest.mark.parametrize('shared', (True, False), ids=('shared-x', 'x-per-group'))
@pytest.mark.parametrize('entry,variant', sorted(R.FWD), ids=IDS)
def test_grouped_launches(S, entry, variant, shared):
    """G = 3 convs in one grid, plain, bias + ReLU, bias alone and pooled, each group against its own reference;
    statistics in a grouped launch are refused."""
    MO, blocked = R.FWD[(entry, variant)][0], R.FWD[(entry, variant)][3]
    tag = _tag(entry, variant) + ' grp'
    for shape in (R.shapes(MO)[0], R.shapes(MO)[2]):
        Nb, H, W, C, N = shape
        for mode in ('exact', 'random'):
            ps = [Prob.get(mode, MO, shape, salt=g) for g in range(3)]
            xs = [ps[0].x] * 3 if shared else [q.x for q in ps]
            x_d = _arena(xs[0] if shared else torch.stack(xs))
            us = [R.to_blocked(q.U) if blocked else q.U for q in ps]
            u_d = _arena(torch.stack(us))
            bias = torch.stack([q.bias for q in ps])
            bias_d = _arena(bias)
            accs = [(R.fused_conv(xs[g], ps[g].U, MO), R.fused_conv(xs[g], ps[g].U, MO, absval=True),
                     None if mode != 'random' else R.fused_conv(xs[g].to(F32), ps[g].U.to(F32), MO).to(F64))
                    for g in range(3)]
            assert mode == 'random' or all(R.exact_ok(a[1] + 3.0) for a in accs)
            for flags in (0, R.BIAS | R.RELU, R.BIAS, R.POOLED, R.STATS):
                want = R.expected_status(entry, variant, shape, flags=flags, groups=3, bias=bool(flags & R.BIAS),
                                         stats=bool(flags & R.STATS))
                st, out, _ = fwd_launch(S, entry, variant, shape, x_d, u_d, flags, groups=3,
                                        bias=bias_d if flags & R.BIAS else None, stats=bool(flags & R.STATS),
                                        gx=0 if shared else xs[0].numel(), gu=us[0].numel(), gbias=N, tag=tag)
                assert st == want, (tag, shape, flags, st, want)
                if st != 0:
                    continue
                for g, (acc, Sg, yd) in enumerate(accs):
                    what = '{} {} flags {} group {}'.format(shape, mode, flags, g)
                    if flags & R.POOL:
                        ref, tol = R.pooled(acc, Sg, ps[g].n, bias[g])
                        yard = None if yd is None else R.pool2(G.f32r(yd + bias[g]).clamp_min(0))
                        R.judge(tag, out[g], ref, tol, mode, yard, what, MO=MO // 2)
                        continue
                    kw = dict(bias=bias[g]) if flags & R.BIAS else {}
                    if flags & R.RELU:
                        kw['act'] = G.ACT_RELU
                    r = G.epilogue(acc.reshape(-1, N), Sg.reshape(-1, N), ps[g].n, exact=mode != 'random', **kw)
                    yard = None if yd is None else G.epilogue32(yd.reshape(-1, N), **kw).reshape(acc.shape)
                    R.judge(tag, out[g], r['out'].reshape(acc.shape), r['tol'].reshape(acc.shape), mode, yard, what, MO=MO)


# --------------------------------------------------------------------------------- weight gradients
def wgrad_launch(S, entry, variant, shape, dy_d, x_d, splits, *, accumulate=False, prior=None, xpro=None, tag=None):
    from rafiki_amd.ops import _lib
    Nb, H, W, Ci, Co = shape
    slab = Co * 9 * Ci
    buf = torch.full((splits * slab + PAD,), NAN, dtype=F32, device=DEV)
    if prior is not None:
        buf[:slab] = prior.to(DEV, F32).reshape(-1)
    args = [S._p(dy_d), S._p(x_d), S._p(buf), Nb, H, W, Co, Ci, splits, int(accumulate)]
    if entry == 'rk_wino4_wgrad':
        args += [variant, S._p(xpro)]
    st = _status(lambda: _lib.call(entry, *args, S._s()))
    if st != 0:
        assert prior is not None or bool(torch.isnan(buf).all()), 'a refused launch wrote something'
        _count(tag, False)
        return st, None
    torch.cuda.synchronize()
    _count(tag, True)
    host = buf.to('cpu', F64)
    _nan_free_guards(host, [(0, splits * slab)], tag)
    return 0, host[:splits * slab].view(splits, Co, 9, Ci)


@pytest.mark.parametrize('si', range(len(R.SHAPES4)))
@pytest.mark.parametrize('entry,variant,xpro', WGRADS, ids=IDS)
def test_weight_gradient_variants_and_splits(S, entry, variant, xpro, si):
    """1, 2 and 4 splits (the last split short wherever the tile count is no multiple of the split size; a split
    count that leaves a split empty is refused), every slab against its own tiles, and accumulation onto a prior.
    F(2x2) also on the exact set (G^T only halves: the result is right to the bit)."""
    MO = 2 if entry == 'rk_wino_wgrad' else 4
    shape = R.shapes(MO)[si]
    Nb, H, W, Ci, Co = shape
    T = Nb * (H // MO) * (W // MO)
    tag = _tag(entry, variant, xpro)
    for mode in (('exact', 'random') if MO == 2 else ('random',)):
        dy, x = R.wgrad_problem(mode, MO, shape)
        pro = R.draw_pro(mode, 5 + sum(shape), Ci) if xpro else None
        dy_d, x_d = _arena(dy), _arena(x)
        pro_d = _arena(torch.cat(pro)) if xpro else None
        for splits in (1, 2, 4):
            want = R.expected_status(entry, variant, shape, splits=splits, pro=xpro)
            st, got = wgrad_launch(S, entry, variant, shape, dy_d, x_d, splits, xpro=pro_d, tag=tag)
            assert st == want, (tag, shape, splits, st, want)
            if st != 0:
                continue
            ref, tiles = R.fused_wgrad(dy, x, MO, splits, pro=pro)
            Sg, _ = R.fused_wgrad(dy, x, MO, splits, pro=pro, absval=True)
            if mode != 'random':
                assert R.exact_ok(Sg.sum(0) + 6.0, 0.25)
            yard = R.fused_wgrad(dy.to(F32), x.to(F32), MO, splits, pro=pro)[0].to(F64) if mode == 'random' else None
            assert sum(tiles) == T
            for s, t in enumerate(tiles):
                R.judge(tag, got[s], ref[s], R.n_wgrad(MO, t, pro=xpro) * R.U32 * Sg[s], mode,
                        None if yard is None else yard[s], '{} {} splits {} slab {}'.format(shape, mode, splits, s),
                        layout='wgrad')
            if splits == 1:
                prior = R.ints(7, (Co, 9, Ci), -6, 6) if mode != 'random' else G.normal_f32(7, (Co, 9, Ci))
                st, got = wgrad_launch(S, entry, variant, shape, dy_d, x_d, 1, accumulate=True, prior=prior,
                                       xpro=pro_d, tag=tag)
                assert st == 0
                tol = R.n_wgrad(MO, T, pro=xpro, prior=True) * R.U32 * (Sg[0] + prior.abs())
                R.judge(tag, got[0], ref[0] + prior, tol, mode, None if yard is None else G.f32r(yard[0] + prior),
                        '{} {} accumulate'.format(shape, mode), layout='wgrad')


# -------------------------------------------------------------------------------- weight transforms
@pytest.mark.parametrize('si', range(len(R.SHAPES4)))
@pytest.mark.parametrize('entry', sorted(WEIGHTS))
def test_weight_transforms_against_g_g_gt(S, entry, si):
    """u and ut element by element against fp64 G g G^T / G flip(g) G^T under N_WEIGHTS * 2^-23 * S; ``exact_w``
    must match to the bit for F(2x2); the rows of a blocked set padded up to 32 stay zero and nothing is written
    past either set."""
    from rafiki_amd.ops import _lib
    MO = WEIGHTS[entry]
    Ci, Co = R.SHAPES4[si][3], R.SHAPES4[si][4]
    blocked = entry == 'rk_wino4b_weights'
    for mode in (('exact_w', 'random') if MO == 2 else ('random',)):
        w = R.draw_w(mode, 3 + Co + Ci, Co, Ci)
        w_d = _arena(w)
        P = (MO + 2) ** 2
        nu, nut = (R.blocked_numel(Co, Ci), R.blocked_numel(Ci, Co)) if blocked else (P * Co * Ci, P * Co * Ci)
        for which in ('both', 'u', 'ut'):
            bufs = {k: torch.full((n + PAD,), NAN, dtype=F32, device=DEV) for k, n in (('u', nu), ('ut', nut))
                    if which in ('both', k)}
            for k, n in (('u', nu), ('ut', nut)):
                if blocked and k in bufs:
                    bufs[k][:n] = 0.0          # the producer zero-fills; the kernel leaves the padded rows alone
            _lib.call(entry, S._p(w_d), S._p(bufs.get('u')), S._p(bufs.get('ut')), Co, Ci, S._s())
            torch.cuda.synchronize()
            _count(entry, True)
            for k, buf in bufs.items():
                dgrad = k == 'ut'
                n = nut if dgrad else nu
                host = buf.to('cpu', F64)
                assert bool(torch.isnan(host[n:]).all()), '{} {}: wrote past the set'.format(entry, k)
                ref = R.transform_weights(w, MO, dgrad)
                tol = R.N_WEIGHTS[MO] * R.U32 * R.transform_weights(w, MO, dgrad, absval=True)
                got = host[:n]
                if blocked:
                    idx = R.blocked_index(*ref.shape[1:]).reshape(-1)
                    rest = torch.ones(n, dtype=torch.bool)
                    rest[idx] = False
                    assert int(rest.sum()) == 36 * (-ref.shape[1] % 32) * ref.shape[2]
                    assert bool((got[rest] == 0).all()), '{} {}: a padded row is not zero'.format(entry, k)
                    got = got[idx]
                R.judge(entry, got.view(ref.shape), ref, tol, 'exact' if mode == 'exact_w' else 'random', None,
                        '{} ({}, {}) {}'.format(k, Co, Ci, mode))


# ---------------------------------------------------------------------------------------- refusals
def test_launcher_refusals(S):
    """Every argument check of rk_wino_conv_grp, gfwd_dispatch + launch_gfwd, rk_wino_wgrad, rk_wino4_wgrad and the
    weight transforms once, on valid small tensors, with the status wino_refs.expected_status predicts."""
    from rafiki_amd.ops import _lib
    p4, p2 = Prob.get('exact', 4, (1, 12, 20, 8, 8)), Prob.get('exact', 2, (1, 6, 10, 8, 8))
    pp = Prob.get('exact', 4, (1, 12, 20, 8, 8), pro=True)
    seen = set()

    def fwd(entry, variant, *, shape=None, flags=0, bias=False, stats=False, gate=False, pro=False, groups=1):
        p = p2 if entry in (W2, W2S) else pp if pro else p4
        shape = shape or p.shape
        want = R.expected_status(entry, variant, shape, flags=flags, bias=bias, stats=stats, gate=gate, pro=pro,
                                 groups=groups)
        assert want != 0, (entry, variant, shape, flags)
        blocked = R.FWD.get((entry, variant), (0, 0, 0, False))[3]
        st, _, _ = fwd_launch(S, entry, variant, shape, p.x_d, p.u_d(blocked), flags, bias=p.dev('ss') if bias else None,
                              stats=stats, gate=p.dev('y2') if gate else None, pro=pp.pro_d if pro else None,
                              groups=groups, tag=entry + ' refusals', alloc=4096)
        assert st == want, (entry, variant, shape, flags, st, want)
        seen.add(want)
    for entry in (W2, W2S, W4):
        MO = 2 if entry != W4 else 4
        top = {W2: 2, W2S: 4, W4: 6}[entry]
        fwd(entry, top), fwd(entry, -1)
        fwd(entry, 0, shape=(0, MO, MO, 8, 8)), fwd(entry, 0, shape=(1, MO + 1, MO, 8, 8)), fwd(entry, 0, shape=(1, MO, MO - 1, 8, 8))
        fwd(entry, 0, shape=(1, MO, MO, 12, 8)), fwd(entry, 0, shape=(1, MO, MO, 0, 8)), fwd(entry, 0, shape=(1, MO, MO, 8, 0))
        fwd(entry, 0, groups=0)
        fwd(entry, 0, flags=R.STATS), fwd(entry, 0, flags=R.BNB, stats=True), fwd(entry, 0, flags=R.BNP, stats=True, gate=True)
        fwd(entry, 0, flags=R.BNB, stats=True, bias=True), fwd(entry, 0, flags=R.BIAS), fwd(entry, 0, flags=R.BIAS | R.RELU)
        for fl in (R.STATS, R.BNB, R.BNP):
            fwd(entry, 0, flags=fl, stats=True, bias=True, gate=True, groups=2)
        fwd(entry, 0, flags=R.POOL), fwd(entry, 0, flags=R.POOL | R.BIAS, bias=True)
        fwd(entry, 0, shape=(1 << 14, 1 << 10, 1 << 10, 8, 8))         # 2^30 tiles and more
        fwd(entry, 0, shape=(1 << 9, 1 << 8, 1 << 8, 16, 8))           # x of 2 GiB
        fwd(entry, 0, shape=(1 << 9, 1 << 8, 1 << 8, 8, 16))           # y of 2 GiB
        fwd(entry, 0, shape=(1 << 7, 1 << 8, 1 << 8, 8, 16), flags=R.BNP, stats=True, bias=True, gate=True)   # its gate
        fwd(entry, 0, shape=(1, MO, MO, 1 << 13, 1 << 13))             # u of 2 GiB
    fwd(W4, 0, pro=True), fwd(W4, 2, pro=True), fwd(W4, 7, pro=True)
    for v in R.PRO_VARIANTS:
        fwd(W4, v, pro=True, groups=2), fwd(W4, v, pro=True, flags=R.BIAS | R.RELU, bias=True)
        fwd(W4, v, pro=True, flags=R.POOLED, bias=True), fwd(W4, v, pro=True, shape=(1, 4, 4, 520, 8))
        fwd(W4, v, pro=True, flags=R.BNB, stats=True, bias=True, gate=True)
    assert seen == {-1, -2}

    dy_d, x_d = _arena(R.draw_x('exact', 1, (2, 4, 4, 16))), _arena(R.draw_x('exact', 2, (2, 4, 4, 16)))

    def wg(entry, variant=0, shape=(2, 4, 4, 16, 16), **kw):
        want = R.expected_status(entry, variant, shape, **kw)
        assert want != 0, (entry, variant, shape, kw)
        st, _ = wgrad_launch(S, entry, variant, shape, dy_d, x_d, kw.get('splits', 1), accumulate=kw.get('accumulate', False),
                             xpro=pp.pro_d if kw.get('pro') else None, tag=entry + ' refusals')
        assert st == want, (entry, variant, shape, kw, st, want)
    for entry in ('rk_wino_wgrad', 'rk_wino4_wgrad'):
        MO = 2 if entry == 'rk_wino_wgrad' else 4
        wg(entry, shape=(0, 4, 4, 16, 16)), wg(entry, shape=(2, MO + 1, 4, 16, 16)), wg(entry, shape=(2, 4, MO + 1, 16, 16))
        wg(entry, shape=(2, 4, 4, 0, 16)), wg(entry, shape=(2, 4, 4, 16, 0)), wg(entry, splits=0)
        wg(entry, splits=2, accumulate=True)
        wg(entry, shape=(1, 4, 4, 16, 16), splits=2)                   # the second split would be empty
        wg(entry, shape=(1 << 12, 1 << 7, 1 << 7, 8, 8))               # 2^22 tiles and more: the fp32 tile decode
        wg(entry, shape=(1 << 8, 1 << 7, 1 << 7, 128, 8)), wg(entry, shape=(1 << 8, 1 << 7, 1 << 7, 8, 128))
    wg('rk_wino4_wgrad', 3), wg('rk_wino4_wgrad', -1), wg('rk_wino4_wgrad', 2, pro=True)

    w_d = _arena(R.draw_w('random', 1, 8, 8))
    buf = torch.full((36 * 32 * 12 + PAD,), NAN, device=DEV)
    for entry in sorted(WEIGHTS):
        bad = [(0, 8, True, True), (8, 0, True, True), (8, 8, False, False)]
        if entry == 'rk_wino4b_weights':
            bad += [(8, 12, True, False), (12, 8, False, True)]
        for Co, Ci, u, ut in bad:
            st = _status(lambda: _lib.call(entry, S._p(w_d), S._p(buf) if u else None, S._p(buf) if ut else None, Co, Ci, S._s()))
            assert st == -1, (entry, Co, Ci, u, ut, st)
            _count(entry + ' refusals', False)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all()), 'a refused launch wrote something'
