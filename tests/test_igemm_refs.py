"""tests/igemm_refs.py anchored and shown to bite (CPU only).

Anchors: every reference against a plain Python loop over pixels and taps and against fp64 torch conv2d,
conv_transpose2d and autograd at tiny shapes (<= 1e-12).

Gates: each plausible wrong formula ("mutant") is applied to the reference at every shape tests/test_igemm_gpu.py
runs, and the comparison that file makes must reject it: on EXACT the stored result differs in at least one
element, on RANDOM some element is off by at least 10 x its tolerance.  The margins are printed (pytest -s).
Four entries of that list cannot be met as stated, for arithmetic reasons, and are held to what can be:
  * a bf16 accumulator is judged on the fp32 epilogue, which every kind but the fused upscale also runs with
    (behind a single K-tile it is the bf16 output's own rounding, and at nine K-tiles it reaches 9 x, not 10 x,
    of a bf16 element's tolerance);
  * truncation is off by at most one bf16 ulp, the tolerance is half an ulp plus the fp32 term, so the ratio
    stays below 2: RANDOM must still reject it (a tenth of the elements or more over tolerance), EXACT does wherever
    the +-300 bias channels are present;
  * routing the pooled gradient to the LAST maximal act(z) of a window changes nothing: two elements of a channel
    tie at a positive value only if their y are equal, and at zero both route nothing (identity asserted).  The
    routing mistake that can exist, the maximum of y instead of act(y*scale + shift), is rejected.
"""
import pytest
import torch
import torch.nn.functional as TF

import igemm_refs as R

F64 = torch.float64
MODES = ('exact', 'random')
_IDS = lambda v: '-'.join(map(str, v)) if isinstance(v, tuple) else str(v)   # noqa: E731


# ------------------------------------------------------------------------------------------- anchors
def _loop_conv(x, w, taps, sign=1, up=False):
    """y[n,h,w,co] = sum_t sum_ci x[...] * w[co,t,ci], the plainest possible way."""
    N, H, W, C = x.shape
    Ho, Wo = (2 * H, 2 * W) if up else (H, W)
    Co = w.shape[0]
    y = torch.zeros(N, Ho, Wo, Co, dtype=F64)
    for n in range(N):
        for h in range(Ho):
            for ww in range(Wo):
                for t in range(taps):
                    dy, dx = (t // 3 - 1, t % 3 - 1) if taps == 9 else (0, 0)
                    hh, wx = h + sign * dy, ww + sign * dx
                    if not (0 <= hh < Ho and 0 <= wx < Wo):
                        continue
                    px = x[n, hh >> 1, wx >> 1] if up else x[n, hh, wx]
                    y[n, h, ww] += w[:, t, :] @ px
    return y


@pytest.mark.parametrize('taps', [9, 1])
@pytest.mark.parametrize('N,H,W,Ci,Co', [(2, 3, 4, 3, 5), (1, 1, 1, 2, 2), (2, 2, 5, 4, 3)])
def test_anchor_conv_forward_dgrad_wgrad(N, H, W, Ci, Co, taps):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, H, W, Ci, generator=g, dtype=F64)
    w = torch.randn(Co, taps, Ci, generator=g, dtype=F64)
    dy = torch.randn(N, H, W, Co, generator=g, dtype=F64)
    k = 3 if taps == 9 else 1
    # forward
    A, B = R.operands(0, x, w, taps)
    y = (A @ B.t()).reshape(N, H, W, Co)
    assert (y - _loop_conv(x, w, taps)).abs().max() <= 1e-12
    xt = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    wt = w.reshape(Co, k, k, Ci).permute(0, 3, 1, 2).clone().requires_grad_(True)
    yt = TF.conv2d(xt, wt, padding=k // 2)
    assert (y - yt.detach().permute(0, 2, 3, 1)).abs().max() <= 1e-12
    yt.backward(dy.permute(0, 3, 1, 2))
    # data gradient: autograd, conv_transpose2d, the plain loop with flipped taps on transposed weights
    A, B = R.operands(1, dy, w, taps)
    dx = (A @ B.t()).reshape(N, H, W, Ci)
    assert (dx - xt.grad.permute(0, 2, 3, 1)).abs().max() <= 1e-12
    ct = TF.conv_transpose2d(dy.permute(0, 3, 1, 2), wt.detach(), padding=k // 2)
    assert (dx - ct.permute(0, 2, 3, 1)).abs().max() <= 1e-12
    assert (dx - _loop_conv(dy, w.permute(2, 1, 0), taps, sign=-1)).abs().max() <= 1e-12
    # weight gradient
    A, B = R.operands(2, dy, x, taps)
    dw = (A @ B.t()).reshape(Co, taps, Ci)
    assert (dw - wt.grad.permute(0, 2, 3, 1).reshape(Co, taps, Ci)).abs().max() <= 1e-12
    if taps == 9:   # ConvWT: the data gradient is the forward conv of dy on the flipped transpose
        A, B = R.operands(0, dy, R.flip_transpose(w))
        assert ((A @ B.t()).reshape(N, H, W, Ci) - dx).abs().max() <= 1e-12
        wf = R.flip_transpose(w)
        for ci in range(Ci):
            for t in range(9):
                for co in range(Co):
                    assert wf[ci, 8 - t, co] == w[co, t, ci]


@pytest.mark.parametrize('N,H,W,Ci,Co', [(2, 2, 3, 3, 4), (1, 1, 1, 2, 3)])
def test_anchor_upscale_conv(N, H, W, Ci, Co):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(N, H, W, Ci, generator=g, dtype=F64)
    w = torch.randn(Co, 9, Ci, generator=g, dtype=F64)
    A, B = R.operands(6, x, w)
    y = (A @ B.t()).reshape(N, 2 * H, 2 * W, Co)
    assert (y - _loop_conv(x, w, 9, up=True)).abs().max() <= 1e-12
    xu = TF.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode='nearest')
    yt = TF.conv2d(xu, w.reshape(Co, 3, 3, Ci).permute(0, 3, 1, 2), padding=1)
    assert (y - yt.permute(0, 2, 3, 1)).abs().max() <= 1e-12


def test_anchor_dense_and_slabs():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(7, 200, generator=g, dtype=F64)
    w = torch.randn(5, 200, generator=g, dtype=F64)
    dy = torch.randn(7, 5, generator=g, dtype=F64)
    for kind, a, b, ref in ((3, x, w, x @ w.t()), (4, dy, w, dy @ w), (5, dy, x, dy.t() @ x)):
        A, B = R.operands(kind, a, b)
        assert ((A @ B.t()) - ref).abs().max() <= 1e-12
    A, B = R.operands(3, x, w)
    for splits in (1, 2, 3, 4):
        slabs, S = R.gemm(A, B, splits)
        rng = R.split_ranges(200, splits)
        assert slabs.shape[0] == len(rng) == R.effective_splits(200, splits)
        assert all(lo % 64 == 0 for lo, _ in rng) and rng[-1][1] == 200
        assert (slabs.sum(0) - x @ w.t()).abs().max() <= 1e-12
        assert (S.sum(0) - x.abs() @ w.abs().t()).abs().max() <= 1e-12
    assert [hi - lo for lo, hi in R.split_ranges(200, 3)] == [128, 72]      # 4 K-tiles over 3 splits: 2 + 2
    assert [hi - lo for lo, hi in R.split_ranges(512, 3)] == [192, 192, 128]


def test_anchor_bnp_route_is_torch_max_pool():
    """First maximal act(z) of each 2x2 window = torch max_pool2d's index on relu(z), wherever that is decided."""
    N, H, W, C = 2, 2, 4, 6
    scale, shift = R.draw_scale_shift(5, C)
    y2 = R.draw_pool_y(6, N, H, W, C, scale)
    assert R.decisions_inexact(y2, scale, shift) == 0
    pos, yb = R.bnp_route(y2, scale, shift, N, H, W)
    z = (y2 * scale + shift).permute(0, 3, 1, 2)
    _, idx = TF.max_pool2d(z.clamp_min(0), 2, return_indices=True)
    ysel = y2.permute(0, 3, 1, 2).reshape(N, C, -1).gather(2, idx.reshape(N, C, -1)).reshape(N, C, H, W)
    zsel = z.reshape(N, C, -1).gather(2, idx.reshape(N, C, -1)).reshape(N, C, H, W)
    pos_t = (zsel > 0).permute(0, 2, 3, 1).reshape(-1, C)
    assert torch.equal(pos, pos_t)
    assert torch.equal(yb[pos], ysel.permute(0, 2, 3, 1).reshape(-1, C)[pos])
    # the draw has what it promises: negative-scale channels, tied windows, all-nonpositive windows
    win = y2.reshape(N, H, 2, W, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, 4, C)
    zw = win * scale + shift
    assert bool((scale < 0).any()) and bool((zw.max(1).values <= 0).all(1).any())
    assert bool((win[:, 0] == win[:, 3]).all(1).any())


def test_rounding_helpers():
    t = torch.tensor([256.0, 257.0, 258.0, 259.0, 301.0, 303.0, -300.25, 1.00390625], dtype=F64)
    assert R.bf16r(t).tolist() == [256.0, 256.0, 258.0, 260.0, 300.0, 304.0, -300.0, 1.0]      # ties to even
    assert R.bf16_trunc(t).tolist() == [256.0, 256.0, 258.0, 258.0, 300.0, 302.0, -300.0, 1.0]
    b = R.draw_bias('exact', 1, 72, big=True)
    assert bool((b * 4 == (b * 4).round()).all()) and bool((b.abs() > 256).any())
    y = R.draw_decision(2, (50, 8))
    assert torch.equal(R.bf16r(y), y) and float(y.abs().max()) <= 255 / 64


# ---------------------------------------------------------------------------------------------- gates
def _judge(mut, ref, E, out_bf16, mode):
    """The comparison of test_igemm_gpu._check on a simulated kernel output.  EXACT: number of stored elements
    that differ.  RANDOM: the largest error / tolerance."""
    if mode == 'exact':
        return int(((R.bf16r(mut) if out_bf16 else mut) != (R.bf16r(ref) if out_bf16 else ref)).sum())
    got = R.bf16r(mut) if out_bf16 else R.f32r(mut)
    tol = R.tol_bf16(ref, E) if out_bf16 else E
    err = (got - ref).abs()
    return float(torch.where(tol > 0, err / tol.clamp_min(1e-300), (err > 0).to(F64) * 1e30).max())


def _bites(name, margin, mode, case):
    print('MARGIN {:16s} {:7s} {:28s} {}'.format(name, mode, str(case), margin if mode == 'exact' else round(margin, 1)))
    assert margin >= (1 if mode == 'exact' else 10.0), (name, mode, case, margin)


_PROBLEMS = {}


def _problem(kind, shape, taps, mode):
    key = (kind, shape, taps, mode)
    if key not in _PROBLEMS:
        a, b = R.problem(kind, shape, taps, mode)
        A, B = R.operands(kind, a, b, taps)
        _PROBLEMS[key] = (a, b, A, B)
    return _PROBLEMS[key]


def _valid(kind, shape, taps):
    """Launches the GPU file expects to be refused have no gate to show."""
    if kind == 1 and shape[4] & (shape[4] - 1):
        return False
    if kind == 4 and shape[2] % 8:
        return False
    return True


GATED = [c for c in R.SWEEP if _valid(*c)]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('kind,shape,taps', GATED, ids=_IDS)
def test_gemm_mutants_are_rejected(kind, shape, taps, mode):
    """Last product dropped, last 8-channel chunk dropped, a K-tile counted twice across a split boundary, the
    last split's last K-tile dropped, the accumulator rounded to bf16 between K-tiles (RANDOM only)."""
    a, b, A, B = _problem(kind, shape, taps, mode)
    K = A.shape[1]
    bf = kind not in (2, 5)
    slabs, S = R.gemm(A, B)
    if mode == 'exact':
        assert R.exact_ok(S[0])
    ref, E = R.fp32_out(slabs[0], S[0], K)
    for name in ('drop_last_k', 'drop_last_chunk'):
        mut = R.gemm(A, B, mutant=name)[0][0]
        _bites(name, _judge(mut, ref, E, bf, mode), mode, (kind, shape, taps))
    kt = R.cdiv(K, R.BK)
    if kt >= 2:   # the split-K mutants, on the fp32 slabs of two splits
        s2, S2 = R.gemm(A, B, 2)
        rng = R.split_ranges(K, 2)
        for name in ('ktile_twice', 'drop_last_ktile'):
            m2 = R.gemm(A, B, 2, mutant=name)[0]
            worst = max(_judge(m2[s], s2[s], R.fp32_out(s2[s], S2[s], rng[s][1] - rng[s][0])[1], False, mode)
                        for s in range(len(rng)))
            _bites(name, worst, mode, (kind, shape, taps))
    if mode == 'random':
        # every kind but the fused upscale also runs with the fp32 epilogue, the sharper gate for this one (behind
        # a single K-tile the rounded accumulator IS the bf16 output; the upscale shapes have two K-tiles or more)
        mut = R.gemm(A, B, mutant='acc_bf16')[0][0]
        assert kind != 6 or kt >= 2
        _bites('acc_bf16', _judge(mut, ref, E, kind == 6, mode), mode, (kind, shape, taps))


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('kind,shape,taps', [c for c in GATED if c[0] in (0, 1, 2, 6) and c[2] == 9], ids=_IDS)
def test_gather_mutants_are_rejected(kind, shape, taps, mode):
    """Left/right padding that wraps into the neighbouring row, bottom padding that reads the next image, kh and
    kw swapped, taps not flipped (data gradient), (h>>1)+dy in place of (h+dy)>>1 (fused upscale)."""
    a, b, A, B = _problem(kind, shape, taps, mode)
    K = A.shape[1]
    bf = kind != 2
    slabs, S = R.gemm(A, B)
    ref, E = R.fp32_out(slabs[0], S[0], K)
    names = {0: ('wrap_lr', 'bottom_next', 'swap_khkw'), 1: ('wrap_lr', 'bottom_next', 'swap_khkw', 'noflip'),
             2: ('wrap_lr', 'bottom_next', 'swap_khkw'), 6: ('up_gather', 'swap_khkw')}[kind]
    for name in names:
        Am, Bm = R.operands(kind, a, b, taps, mutant=name)
        mut = R.gemm(Am, Bm)[0][0]
        _bites(name, _judge(mut, ref, E, bf, mode), mode, (kind, shape))


def _epilogue_problem(shape, mode):
    a, b, A, B = _problem(0, shape, 9, mode)
    slabs, S = R.gemm(A, B)
    return slabs[0], S[0], A.shape[1], A.shape[0], B.shape[0]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', R.EPI_SHAPES + R.CONV_SHAPES[1:2], ids=_IDS)
def test_epilogue_mutants_are_rejected(shape, mode):
    """Output truncated instead of rounded; statistics taken after the activation; BNB sums over the unrounded
    value (RANDOM only, at the epilogue shapes, whose few rows keep the summation tolerance below the rounding
    noise); BNP routed on y instead of act(z); BNP routed to the last maximum (no observable change)."""
    acc, S, K, M, N = _epilogue_problem(shape, mode)
    Nb, H, W = shape[:3]
    # truncation, at BIAS with alpha = 0.5 and the +-300 channels
    bias = R.draw_bias(mode, 11, N, big=True)
    v, E = R.fp32_out(acc, S, K, alpha=0.5, bias=bias)
    if mode == 'exact':
        bad = int((R.bf16_trunc(v) != R.bf16r(v)).sum())
        _bites('trunc_out', bad, mode, shape)
    else:
        over = ((R.bf16_trunc(v) - v).abs() > R.tol_bf16(v, E)).to(F64).mean().item()
        ratio = ((R.bf16_trunc(v) - v).abs() / R.tol_bf16(v, E)).max().item()
        print('MARGIN trunc_out        random  {:28s} {:.2f} x tol at worst, {:.0%} of the elements over'.format(
            str(shape), ratio, over))
        assert over >= 0.1 and ratio < 2.0
    # statistics after the activation (BIAS|RELU|STATS)
    sb = R.ints(12, (N,), -3, 3) if mode == 'exact' else R.draw_bias(mode, 12, N)
    v, E = R.fp32_out(acc, S, K, bias=sb)
    if mode == 'exact':
        assert R.exact_ok(S, v)
    ref, tol = R.stats_ref(v, E)
    mut = R.stats_ref(v.clamp_min(0), E)[0]
    _bites('stats_after_act', int((mut != ref).sum()) if mode == 'exact' else float(((mut - ref).abs() / tol).max()),
           mode, shape)
    # BNB: sums over the unrounded value, judged as the GPU file does: against the stored values
    scale, shift = R.draw_scale_shift(21, N)
    y = R.draw_decision(22, (M, N))
    assert R.decisions_inexact(y, scale, shift) == 0
    v, E = R.fp32_out(acc, S, K)
    m = R.bnb_mask(y, scale, shift).to(F64)
    assert 0.2 < m.mean().item() < 0.8
    stored = R.bf16r(v) * m
    ref, tol = R.bn_sums(stored, y)
    mut = R.bn_sums(v * m, y)[0]
    if mode == 'random' and shape in R.EPI_SHAPES:
        _bites('bnb_unrounded', float(((mut - ref).abs() / tol).max()), mode, shape)
    # BNP routing
    if not (H & (H - 1)) and not (W & (W - 1)):
        y2 = R.draw_pool_y(23, Nb, H, W, N, scale)
        assert R.decisions_inexact(y2, scale, shift) == 0
        pos, yb = R.bnp_route(y2, scale, shift, Nb, H, W)
        ref, tol = R.bn_sums(R.bf16r(v) * pos.to(F64), yb)
        pos_l, yb_l = R.bnp_route(y2, scale, shift, Nb, H, W, mutant='last_max')
        assert torch.equal(R.bn_sums(R.bf16r(v) * pos_l.to(F64), yb_l)[0], ref)     # unobservable: see the docstring
        pos_y, yb_y = R.bnp_route(y2, scale, shift, Nb, H, W, mutant='route_on_y')
        mut = R.bn_sums(R.bf16r(v) * pos_y.to(F64), yb_y)[0]
        _bites('bnp_route_on_y', int((mut != ref).sum()) if mode == 'exact'
               else float(((mut - ref).abs() / tol.clamp_min(1e-300)).max()), mode, shape)


@pytest.mark.parametrize('kind,shape,taps', GATED, ids=_IDS)
def test_exact_preconditions(kind, shape, taps):
    """EXACT: integer operands, S below 2^24; the references of an EXACT problem are integers (exact in fp32)."""
    a, b, A, B = _problem(kind, shape, taps, 'exact')
    slabs, S = R.gemm(A, B)
    assert R.exact_ok(S[0]) and torch.equal(slabs, slabs.round()) and torch.equal(R.f32r(slabs), slabs)
    assert float(a.abs().max()) <= 2 and float(b.abs().max()) <= 2
    ar, br = R.problem(kind, shape, taps, 'random')[:2]
    assert torch.equal(R.bf16r(ar), ar) and torch.equal(R.bf16r(br), br)      # the kernel's operands exactly
