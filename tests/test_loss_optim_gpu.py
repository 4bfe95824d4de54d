"""The kernels of csrc/kernels/loss_optim.hip (softmax cross-entropy, SGD, Adam, lerp, zeroing, finite
check, ensemble mean, casts, the gather prologue) and the Philox stream against fp64 references that go
through no other kernel of this project (tests/loss_optim_refs.py; tests/test_flat_optim.py anchors those to
torch.optim and shows that each tolerance used here rejects the plausible wrong formulas).

Tolerance of an fp32 output: 4 x e_ref, e_ref the error of the project's fp32 CPU path (or of plain fp32
PyTorch / NumPy) against the same fp64 reference on the same inputs, in the max norm relative to max |ref|.
Outputs the kernel computes with __expf / __logf or stores as bf16 keep the fixed bounds of
tests/test_kernels_gpu.py::test_softmax_xent.  Every figure is printed before it is asserted (pytest -s).
"""
import functools

import numpy as np
import pytest
import torch

import loss_optim_refs as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'


@pytest.fixture(scope='module')
def fn():
    from rafiki_amd.ops import _lib, functional
    _lib.lib()  # loud failure if the native library is missing
    return functional


def _within(what, got, ref, tol):
    e = R.err(got, ref)
    print('{}: kernel err {:.3e}  tolerance 4 x e_ref {:.3e}'.format(what, e, tol))
    assert e <= tol, (what, e, tol)


def _i32(v=0):
    return torch.full((1,), v, dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------- SGD
@pytest.mark.parametrize('mode', list(R.SGD_MODES))
@pytest.mark.parametrize('n', R.SGD_SIZES)
def test_flat_sgd_matches_fp64(fn, n, mode):
    """FlatSGD.step on the GPU (rk_sgd_step with lr_tensor, bump and decay_end as every training step passes
    them): 5 steps of fresh gradients with the device LR multiplier 1, 0.25, 0, 1, 0.25, for every decay_end,
    with and without the bf16 copy.  The largest n walks the grid-stride loop; there decay_end is n / 2 and n
    (decay off and on in the second pass), the same two the sensitivity test covers."""
    w0, grads = R.sgd_inputs(n)
    ends = R.sgd_decay_ends(n) if n < 1 << 20 else [n // 2 // 4 * 4, n]
    dgrads = [g.to(DEV) for g in grads]
    for k, de in enumerate(ends):
        ref = R.run_sgd_ref(w0, grads, mode=mode, decay_end=de)
        fc, oc = R.run_flat_sgd('cpu', w0, grads, mode=mode, decay_end=de)
        tols = R.tolerances((fc.master, oc.mom), ref)
        for with_bf16 in ((True, False) if n < 1 << 20 else (k % 2 == 0,)):
            bump = _i32(0)

            def on_step(i, s, before, f, opt):
                assert int(bump.item()) == i + 1        # exactly one per launch
                if s == 0.0:
                    assert torch.equal(before, f.master)
            f, opt = R.run_flat_sgd(DEV, w0, dgrads, mode=mode, decay_end=de, with_bf16=with_bf16, bump=bump,
                                    on_step=on_step)
            torch.cuda.synchronize()
            tag = 'sgd n={} {} decay_end={} bf16={}'.format(n, mode, de, with_bf16)
            _within(tag + ' w', f.master, ref[0], tols[0])
            if ref[1] is not None:
                _within(tag + ' mom', opt.mom, ref[1], tols[1])
            if with_bf16:
                assert torch.equal(f.bf16, f.master.bfloat16())


@pytest.mark.parametrize('mode', list(R.SGD_MODES))
def test_sgd_step_grad_scale(fn, mode):
    """sgd_step called directly with grad_scale != 1, no lr_tensor, no bump, the default decay_end (all)."""
    n, gs = 4104, R.SGD_GRAD_SCALE
    w0, grads = R.sgd_inputs(n)
    hp = R.SGD_MODES[mode]
    ref = R.run_sgd_ref(w0, grads, mode=mode, decay_end=n, grad_scale=gs, scales=(1.0,) * len(grads))
    fc, oc = R.run_flat_sgd('cpu', w0, [g * gs for g in grads], mode=mode, decay_end=n, scales=(1.0,) * len(grads))
    tols = R.tolerances((fc.master, oc.mom), ref)
    w = w0.to(DEV)
    mom = torch.zeros_like(w) if hp['momentum'] > 0 else None
    for g in grads:
        fn.sgd_step(w, g.to(DEV), mom, lr=R.SGD_HP['lr'], momentum=hp['momentum'], weight_decay=R.SGD_HP['wd'],
                    nesterov=hp['nesterov'], grad_scale=gs)
    _within('sgd_step grad_scale {} w'.format(mode), w, ref[0], tols[0])
    if mom is not None:
        _within('sgd_step grad_scale {} mom'.format(mode), mom, ref[1], tols[1])


@pytest.mark.parametrize('n,decay_end', [(6, 4), (1027, 0), (8, 6), (4104, 4102)])
def test_sgd_step_refuses_unaligned_sizes(fn, n, decay_end):
    from rafiki_amd.ops._lib import KernelError
    gen = torch.Generator().manual_seed(5)
    bufs = [torch.randn(n, generator=gen).to(DEV) for _ in range(3)]
    wb, bump, lr = bufs[0].bfloat16(), _i32(3), torch.ones(1, device=DEV)
    keep = [b.clone() for b in bufs + [wb, bump]]
    with pytest.raises(KernelError):
        fn.sgd_step(bufs[0], bufs[1], bufs[2], wb=wb, lr=0.1, momentum=0.9, weight_decay=1e-2, nesterov=True,
                    lr_tensor=lr, decay_end=decay_end, bump=bump)
    torch.cuda.synchronize()
    for a, b in zip(bufs + [wb, bump], keep):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------- Adam
@functools.lru_cache(maxsize=None)
def _adam_case(b1, b2, decay, gs):
    """Gradients, fp64 reference (w, m, v) and tolerances of one Adam configuration over the live ranges,
    computed once for every kernel form that is checked against it."""
    wd, decoupled = R.ADAM_DECAY[decay]
    f0, fc = R.adam_arena('cpu'), R.adam_arena('cpu')
    live = f0.ranges_of(R.ADAM_LIVE)
    grads = R.fresh_grads(f0.total, R.ADAM_STEPS, 21)
    kw = dict(b1=b1, b2=b2, wd=wd, decoupled=decoupled, live=live)
    ref = R.run_adam_ref(f0, grads, grad_scale=gs, **kw)
    oc = R.run_flat_adam(fc, [g * gs for g in grads], **kw)
    return grads, ref, R.tolerances((fc.master, oc.m, oc.v), ref), kw


def _outside(f, live):
    mask = torch.ones(f.total, dtype=torch.bool, device=f.device)
    for a, b in live:
        mask[a:b] = False
    assert bool(mask.any())
    return mask


def _check_adam(tag, f, m, v, ref, tols, live, f0):
    torch.cuda.synchronize()
    for name, got, r, tol in zip('wmv', (f.master, m, v), ref, tols):
        _within('{} {}'.format(tag, name), got, r, tol)
    assert torch.equal(f.bf16, f.master.bfloat16())
    out = _outside(f, live)
    assert torch.equal(f.master[out], f0.master.to(DEV)[out]) and torch.equal(f.bf16[out], f0.bf16.to(DEV)[out])
    assert torch.count_nonzero(m[out]) == 0 and torch.count_nonzero(v[out]) == 0


@pytest.mark.parametrize('decay', list(R.ADAM_DECAY))
@pytest.mark.parametrize('b1,b2', R.ADAM_BETAS)
@pytest.mark.parametrize('path', ['multi', 'per_segment'])
def test_flat_adam_matches_fp64(fn, monkeypatch, path, b1, b2, decay):
    """FlatAdam.step(live=...) on the GPU through rk_adam_multi (one launch) and through rk_adam_step (one
    launch per segment), each against fp64: per-segment lr * mult, eps * mult and decay, the device step
    counter, a clear skip flag, the bf16 copy; ranges outside the live set bit-identical."""
    grads, ref, tols, kw = _adam_case(b1, b2, decay, 1.0)
    if path == 'per_segment':
        monkeypatch.setattr(fn, 'seg_table_ok', lambda segs: False)
    f, f0 = R.adam_arena(DEV), R.adam_arena('cpu')
    opt = R.run_flat_adam(f, [g.to(DEV) for g in grads], skip_flag=_i32(0), **kw)
    assert bool(opt.__dict__.get('_seg_tables')) == (path == 'multi')
    assert int(opt.t.item()) == R.ADAM_STEPS
    _check_adam('FlatAdam {} b=({}, {}) {}'.format(path, b1, b2, decay), f, opt.m, opt.v, ref, tols, kw['live'], f0)


def _direct_adam(fn, form, f, grads, *, b1, b2, wd, decoupled, live, gs, skip=None, bump=None):
    """The kernels called directly over the live segments with grad_scale: form 'host' (adam_step, host step
    count), 'device' (adam_step, step_tensor already incremented, values 1..5), 'multi' (adam_multi)."""
    m, v, t = torch.zeros_like(f.master), torch.zeros_like(f.master), _i32(0)
    segs = R.live_segments(f, wd, live)
    lr, eps = R.ADAM_HP['lr'], R.ADAM_HP['eps']
    tab = fn.SegTable(f.device, [(a, b) for a, b, _, _ in segs],
                      [(lr * mult, eps * mult, swd, 0.0) for _, _, swd, mult in segs]) if form == 'multi' else None
    for step, g in enumerate(grads, 1):
        f.grad.copy_(g)
        t.fill_(step)
        if form == 'multi':
            fn.adam_multi(f.master, f.grad, m, v, tab, wb=f.bf16, beta1=b1, beta2=b2, decoupled=decoupled,
                          grad_scale=gs, skip_flag=skip, step_tensor=t, bump=bump)
            continue
        for a, b, swd, mult in segs:
            fn.adam_step(f.master[a:b], f.grad[a:b], m[a:b], v[a:b], wb=f.bf16[a:b], lr=lr * mult, beta1=b1,
                         beta2=b2, eps=eps * mult, weight_decay=swd, decoupled=decoupled, grad_scale=gs,
                         skip_flag=skip, **(dict(step=step) if form == 'host' else dict(step_tensor=t)))
    return m, v


@pytest.mark.parametrize('decay', list(R.ADAM_DECAY))
@pytest.mark.parametrize('b1,b2', R.ADAM_BETAS)
def test_adam_kernels_grad_scale_and_step_forms(fn, b1, b2, decay):
    """adam_step with a host step and with a device step_tensor, and adam_multi, with grad_scale != 1: each
    against fp64, and the host and device step forms against each other (both inside the tolerance of the same
    reference, so at most two tolerances apart)."""
    gs = R.ADAM_GRAD_SCALE
    grads, ref, tols, kw = _adam_case(b1, b2, decay, gs)
    dg = [g.to(DEV) for g in grads]
    f0, got = R.adam_arena('cpu'), {}
    for form in ('host', 'device', 'multi'):
        f = R.adam_arena(DEV)
        m, v = _direct_adam(fn, form, f, dg, gs=gs, **kw)
        _check_adam('adam {} b=({}, {}) {}'.format(form, b1, b2, decay), f, m, v, ref, tols, kw['live'], f0)
        got[form] = (f.master, m, v)
    for a, b, r, tol in zip(got['host'], got['device'], ref, tols):
        assert R.err(a.double().cpu() - b.double().cpu() + r, r) <= 2 * tol


@pytest.mark.parametrize('form', ['host', 'device', 'multi'])
def test_adam_skip_flag_changes_nothing(fn, form):
    """skip_flag = 1: w, m, v and the bf16 copy keep every bit; adam_multi's bump still advances."""
    grads, _, _, kw = _adam_case(0.9, 0.999, 'decoupled', R.ADAM_GRAD_SCALE)
    f, f0 = R.adam_arena(DEV), R.adam_arena('cpu')
    bump = _i32(7) if form == 'multi' else None
    m, v = _direct_adam(fn, form, f, [g.to(DEV) for g in grads[:2]], gs=R.ADAM_GRAD_SCALE, skip=_i32(1), bump=bump,
                        **kw)
    torch.cuda.synchronize()
    assert torch.equal(f.master.cpu(), f0.master) and torch.equal(f.bf16.cpu(), f0.bf16)
    assert torch.count_nonzero(m) == 0 and torch.count_nonzero(v) == 0
    if bump is not None:
        assert int(bump.item()) == 9


# ------------------------------------------------------------------------------------------- lerp
@pytest.mark.parametrize('t', R.LERP_T)
def test_lerp_matches_fp64(fn, t):
    """lerp_ (n not a multiple of 4) and lerp_multi (chunk-table ranges, everything outside untouched), fp32
    result and bf16 copy."""
    gen = torch.Generator().manual_seed(31)
    n = 1027
    dst, src = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    ref = R.lerp_ref(dst.double(), src.double(), t)
    tol = R.TOL_FACTOR * R.err(R.lerp_ref(dst, src, t), ref)
    d, db = dst.to(DEV), torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    fn.lerp_(d, src.to(DEV), t, dst_bf16=db)
    _within('lerp_ t={}'.format(t), d, ref, tol)
    assert torch.equal(db, d.bfloat16())

    f = R.adam_arena(DEV)
    live = f.ranges_of(R.ADAM_LIVE)
    dst, src = torch.randn(f.total, generator=gen), f.master.cpu()
    ref = R.lerp_ref(dst.double(), src.double(), t)
    e_ref = R.err(R.lerp_ref(dst, src, t), ref)
    d, db = dst.to(DEV), torch.full((f.total,), 7.0, dtype=torch.bfloat16, device=DEV)
    fn.lerp_multi(d, f.master, t, fn.SegTable(f.device, live), dst_bf16=db)
    out = _outside(f, live)
    assert torch.equal(d[out], dst.to(DEV)[out]) and bool((db[out] == 7.0).all())
    ref[out.cpu()] = dst.double()[out.cpu()]
    _within('lerp_multi t={}'.format(t), d, ref, R.TOL_FACTOR * e_ref)
    assert torch.equal(db[~out], d.bfloat16()[~out])


# ------------------------------------------------------------------------------------------- streaming
@pytest.mark.parametrize('dtype', [torch.float32, torch.int32])
@pytest.mark.parametrize('n', [1, 3, 4, 1027])
def test_zero_inside_a_larger_buffer(fn, n, dtype):
    buf = torch.full((n + 24,), 77, dtype=dtype, device=DEV)
    view = buf[8:8 + n]
    assert view.data_ptr() % 16 == 0     # the native kernel's path, not the torch fill
    fn.zero_(view)
    assert torch.count_nonzero(view) == 0
    assert bool((buf[:8] == 77).all()) and bool((buf[8 + n:] == 77).all())


@pytest.mark.parametrize('n', [1024, 1027])
def test_nonfinite_flag_positions_and_stickiness(fn, n):
    gen = torch.Generator().manual_seed(9)
    clean = torch.randn(n, generator=gen).to(DEV)
    clean[1] = 3.0e38       # large and finite
    flag = _i32(0)
    fn.nonfinite_flag(clean, flag)
    assert int(flag.item()) == 0
    for bad in (float('nan'), float('inf'), float('-inf')):
        for pos in (0, n - 1):
            x = clean.clone()
            x[pos] = bad
            flag = _i32(0)
            fn.nonfinite_flag(x, flag)
            assert int(flag.item()) == 1, (bad, pos)
            fn.nonfinite_flag(clean, flag)      # sticky: a clean call never clears it
            assert int(flag.item()) == 1


def test_ensemble_mean_matches_fp64(fn):
    gen = torch.Generator().manual_seed(12)
    probs = torch.rand(3, 33, 10, generator=gen)
    for weights in (None, torch.tensor([0.5, 2.0, 0.25])):       # do not sum to 1
        w = torch.ones(3) if weights is None else weights
        ref = (probs.double() * w.double()[:, None, None]).sum(0) / w.double().sum()
        e_ref = R.err((probs * w[:, None, None]).sum(0) / w.sum(), ref)
        got = fn.ensemble_mean(probs.to(DEV), None if weights is None else weights.to(DEV))
        _within('ensemble_mean weights={}'.format(weights is not None), got, ref, R.TOL_FACTOR * e_ref)


@pytest.mark.parametrize('C,cpad', [(3, 8), (8, 8), (1, 4)])
@pytest.mark.parametrize('u8', [False, True])
def test_pack_nhwc_scale_and_shift(fn, C, cpad, u8):
    """out = bf16(in * scale + shift), NCHW -> NHWC, channels C..cpad zero.  Bound: round-to-nearest bf16 of
    the exact value is within half a bf16 ulp, at most 2^-8 of it; the fp32 evaluation before the rounding
    adds a few 2^-24 of |in * scale| + |shift| (the uint8 case cancels to near zero at mid-grey)."""
    gen = torch.Generator().manual_seed(13)
    if u8:
        img = torch.randint(0, 256, (2, C, 5, 7), dtype=torch.uint8, generator=gen)
        scale, shift = 2.0 / 255.0, -1.0
    else:
        img = torch.randn(2, C, 5, 7, generator=gen)
        scale, shift = 0.7, 0.3
    out = fn.pack_nhwc(img.to(DEV), cpad, scale, shift)
    ref = (img.double() * scale + shift).permute(0, 2, 3, 1)
    got = out.double().cpu()
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (2, 5, 7, cpad)
    mag = ((img.double() * scale).abs() + abs(shift)).permute(0, 2, 3, 1)
    assert bool(((got[..., :C] - ref).abs() <= 2.0 ** -8 * ref.abs() + 2.0 ** -22 * mag).all())
    assert torch.count_nonzero(got[..., C:]) == 0


def test_cast_bf16_is_round_to_nearest_even(fn):
    gen = torch.Generator().manual_seed(14)
    x = torch.randn(1027, generator=gen)
    x[:6] = torch.tensor([1.00390625, 1.01171875, -1.00390625, 3.0e38, 1e-30, 0.0])    # ties, a near-overflow
    x[6], x[7] = float('inf'), float('-inf')
    dst = torch.empty(1027, dtype=torch.bfloat16, device=DEV)
    fn.cast_bf16(x.to(DEV), dst)
    assert torch.equal(dst.cpu(), x.bfloat16())


# ------------------------------------------------------------------------------------------- softmax
def _xent_launch(variant, logits, labels, ncls, ldd, *, grad_scale, scale, want):
    """One launch of the variant's entry point as its caller makes it -> dict of outputs (host tensors)."""
    from rafiki_amd.ops import _lib, f32 as S, functional as F
    B = logits.shape[0]
    dl_dtype = torch.bfloat16 if variant == 'bf16' else torch.float32
    dl = torch.full((B, ldd), 9.0, dtype=dl_dtype, device=DEV)
    out = dict(dlogits=dl, loss_sum=torch.zeros(1, device=DEV))
    x, y = logits.to(DEV), None if labels is None else labels.to(DEV)
    if variant == 'f32s':      # the tagger's call (engine/tagger.py _body)
        sc = torch.full((1,), scale, device=DEV)
        _lib.call('rk_softmax_xent_f32s', F._p(x), x.stride(0), F._p(y), B, ncls, R.IGNORE, F._p(sc), F._p(dl), ldd,
                  F._p(out['loss_sum']), F._s())
    else:
        if want:
            out.update(probs=torch.full((B, ncls), 9.0, device=DEV), correct=_i32(0), counted=_i32(0))
        (F if variant == 'bf16' else S).softmax_xent(x, y, ncls, dlogits=dl, probs=out.get('probs'),
                                                     loss_sum=out['loss_sum'], correct=out.get('correct'),
                                                     counted=out.get('counted'), grad_scale=grad_scale)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _xent_check(tag, variant, got, ref, ncls, B, gs_total, loss_tol=R.LOSS_TOL, prob_tol=R.PROB_TOL,
                bf16_rel=R.BF16_REL):
    """The fixed bounds: loss per row, probabilities absolute, d(logits) = (p - onehot) * s so the probability
    bound times |s| for fp32 storage and 1e-2 relative (max norm) for bf16 storage.  Returns the figures."""
    dl = got['dlogits'].double()
    e_loss = abs(got['loss_sum'].item() - ref['loss_sum']) / B
    e_dl = (dl[:, :ncls] - ref['dlogits']).abs().max().item()
    fig = dict(loss=e_loss, dl=e_dl)
    assert e_loss < loss_tol, (tag, fig)
    assert torch.count_nonzero(dl[:, ncls:]) == 0, tag       # padding columns exactly zero
    zero_rows = ref['dlogits'].abs().sum(1) == 0
    assert torch.count_nonzero(dl[zero_rows]) == 0, tag      # ignored rows: an all-zero gradient
    if variant == 'bf16':
        fig['dl_rel'] = R.err(dl[:, :ncls], ref['dlogits']) if ref['dlogits'].abs().max() > 0 else e_dl
        assert fig['dl_rel'] < bf16_rel, (tag, fig)
    else:
        assert e_dl <= prob_tol * abs(gs_total), (tag, fig)
    if 'probs' in got:
        fig['probs'] = (got['probs'].double() - ref['probs']).abs().max().item()
        assert fig['probs'] <= prob_tol, (tag, fig)
        assert int(got['counted'].item()) == ref['counted'], tag
        assert int(got['correct'].item()) == ref['correct'], tag
    return fig


@pytest.mark.parametrize('B', R.XENT_B)
@pytest.mark.parametrize('variant', ['bf16', 'f32', 'f32s'])
def test_softmax_xent_matches_fp64(variant, B):
    """functional.softmax_xent (bf16 d(logits)), f32.softmax_xent and rk_softmax_xent_f32s over every class
    count, with the row stride equal to ncls and padded; the padded rows carry ignore_index, -1 and ncls
    labels.  grad_scale default (1 / B) and explicit; the device scale of f32s multiplies loss and gradient."""
    worst = {}
    for ncls in R.XENT_NCLS:
        for padded in (False, True):
            logits, labels = R.xent_inputs(B, ncls, padded)
            for explicit in (False, True):
                if variant == 'f32s':
                    gs, scale = 1.0, (0.37 if explicit else 1.0 / max(1, B))
                else:
                    gs, scale = (0.125 if explicit else 1.0 / B), 1.0
                ref = R.xent_ref(logits, labels, ncls, grad_scale=gs, scale=scale)
                got = _xent_launch(variant, logits, labels, ncls, logits.shape[1], scale=scale,
                                   grad_scale=gs if explicit else None, want=True)
                tag = '{} B={} ncls={} padded={} explicit={}'.format(variant, B, ncls, padded, explicit)
                fig = _xent_check(tag, variant, got, ref, ncls, B, gs * scale)
                for k, v in fig.items():
                    worst[k] = max(worst.get(k, 0.0), v)
    print('softmax {} B={} worst errors {}'.format(variant, B, worst))


def test_softmax_argmax_ties_take_the_first_index():
    """A tie inside one lane's strided loop (columns 3 and 67 = 3 + 64) and one across lanes (5 and 40); the
    reference is NumPy's argmax on the host."""
    from rafiki_amd.ops import f32 as S, functional as F
    ncls = 130
    gen = torch.Generator().manual_seed(4)
    logits = torch.randn(4, ncls, generator=gen)
    for r, (a, b) in enumerate([(3, 67), (3, 67), (5, 40), (5, 40)]):
        logits[r, a] = logits[r, b] = 9.0
    labels = torch.tensor([3, 67, 5, 40], dtype=torch.int32)
    hits = torch.from_numpy(np.argmax(logits.numpy(), axis=1)) == labels
    assert hits.tolist() == [True, False, True, False]
    for mod in (F, S):
        x, y = logits.to(DEV), labels.to(DEV)
        correct = _i32(0)
        mod.softmax_xent(x, y, ncls, correct=correct)
        assert int(correct.item()) == int(hits.sum())
        for r in range(4):
            correct = _i32(0)
            mod.softmax_xent(x[r:r + 1], y[r:r + 1], ncls, correct=correct)
            assert int(correct.item()) == int(hits[r]), r


# large logits: the kernel's error against fp64, measured once on an MI355X (B = 5 rows spanning +-80, every
# class count, both strides):
#   loss per row  bf16 / f32: 4.82e-6        f32s (loss times the scale 0.37): 1.73e-6
#   probs         3.16e-6
#   d(logits)     fp32 storage, per unit of scale: 3.15e-6     bf16 storage, relative: 2.16e-3
# bounds: 4 x the measurement, never above the fixed bounds (which cap the probabilities and with them the
# fp32 gradient: 4 x 3.16e-6 would be 1.26e-5)
BIG_LOSS_TOL = {'bf16': 4 * 4.82e-6, 'f32': 4 * 4.82e-6, 'f32s': 4 * 1.73e-6}
BIG_PROB_TOL = min(4 * 3.16e-6, R.PROB_TOL)
BIG_BF16_REL = min(4 * 2.16e-3, R.BF16_REL)


@pytest.mark.parametrize('variant', ['bf16', 'f32', 'f32s'])
def test_softmax_xent_large_logits(variant):
    B = 5
    worst = {}
    for ncls in R.XENT_NCLS:
        for padded in (False, True):
            logits, labels = R.xent_inputs(B, ncls, padded, seed=1, big=True)
            gs, scale = (1.0, 0.37) if variant == 'f32s' else (1.0 / B, 1.0)
            ref = R.xent_ref(logits, labels, ncls, grad_scale=gs, scale=scale)
            got = _xent_launch(variant, logits, labels, ncls, logits.shape[1], scale=scale, grad_scale=None,
                               want=True)
            fig = _xent_check('big {} ncls={} padded={}'.format(variant, ncls, padded), variant, got, ref, ncls, B,
                              gs * scale, BIG_LOSS_TOL[variant], BIG_PROB_TOL, BIG_BF16_REL)
            fig['dl_per_scale'] = fig['dl'] / (gs * scale)
            for k, v in fig.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print('softmax large logits {} worst errors {}'.format(variant, worst))


def test_softmax_without_labels_writes_only_probs():
    from rafiki_amd.ops import f32 as S, functional as F
    logits, _ = R.xent_inputs(5, 65, padded=True)
    ref = torch.softmax(logits[:, :65].double(), 1)
    for mod in (F, S):
        probs = torch.full((5, 65), 9.0, device=DEV)
        loss, correct, counted = torch.full((1,), 2.5, device=DEV), _i32(4), _i32(6)
        mod.softmax_xent(logits.to(DEV), None, 65, probs=probs, loss_sum=loss, correct=correct, counted=counted)
        assert (probs.double().cpu() - ref).abs().max().item() <= R.PROB_TOL
        assert loss.item() == 2.5 and int(correct.item()) == 4 and int(counted.item()) == 6


# ------------------------------------------------------------------------------------------- gather
def _middle(t, lead, n):
    """A contiguous view of n rows from row `lead` of t: what lies before and after stays allocated."""
    return t[lead:lead + n]


@pytest.mark.parametrize('fmt,B', [('f32', 5), ('f32', 64), ('f32', 256), ('bf16', 5), ('bf16', 64)])
def test_gather_batch_direct(fn, fmt, B):
    """rk_gather_batch on its own: fp32 rows of 12 floats (3 vectors) and bf16 rows of 8 (1 vector); B = 5 and
    B = 64 run one block, B = 256 with 12-float rows (768 vectors) three.  data, labels, sched and lr_table are
    views into the middle of larger sentinel-filled buffers: a counter that does not wrap or a row index that
    is not clamped reads allocated sentinel memory and fails the comparison."""
    nrows, nsteps, gen = 40, 3, torch.Generator().manual_seed(B)
    if fmt == 'f32':
        big = torch.full((nrows + 8, 12), -5.0)
        big[4:4 + nrows] = torch.randn(nrows, 12, generator=gen)
        out_x = torch.full((B, 12), 9.0, device=DEV)
    else:
        big = torch.full((nrows + 8, 8), -5.0, dtype=torch.bfloat16)
        big[4:4 + nrows] = torch.randn(nrows, 8, generator=gen).bfloat16()
        out_x = torch.full((B, 8), 9.0, dtype=torch.bfloat16, device=DEV)
    big_l = torch.full((nrows + 8,), -777, dtype=torch.int32)
    big_l[4:4 + nrows] = torch.randint(0, 10, (nrows,), generator=gen, dtype=torch.int32)
    big_s = torch.full((2 + nsteps + 6, B), 1, dtype=torch.int64)        # sentinel: a valid row, the wrong one
    big_s[2:2 + nsteps] = torch.randint(2, nrows, (nsteps, B), generator=gen)
    big_s[2:2 + nsteps, 0] = torch.tensor([-1, nrows, -1])               # outside the dataset: read row 0
    big_s[2 + 1, B - 1] = nrows + 3
    big_t = torch.full((2 + nsteps + 6,), 55.0)
    big_t[2:2 + nsteps] = torch.tensor([1.0, 0.25, 0.5])
    dbig, dl, ds, dt = big.to(DEV), big_l.to(DEV), big_s.to(DEV), big_t.to(DEV)
    data, labels, sched, table = (_middle(dbig, 4, nrows), _middle(dl, 4, nrows), _middle(ds, 2, nsteps),
                                  _middle(dt, 2, nsteps))
    h_data, h_labels, h_sched = big[4:4 + nrows], big_l[4:4 + nrows], big_s[2:2 + nsteps]
    out_y = torch.full((B,), -9, dtype=torch.int32, device=DEV)
    big_z = torch.full((37 + 16,), float('nan'), dtype=torch.float64, device=DEV)
    zero = big_z[8:8 + 37]
    lr_out = torch.full((1,), -1.0, device=DEV)
    for ctr in (0, 2, 3, 7):        # 3 and 7 wrap to 0 and 1
        counter = _i32(ctr)
        out_x.fill_(9.0)
        out_y.fill_(-9)
        zero.fill_(float('nan'))
        fn.gather_batch(data, labels, sched, counter, out_x, out_y, zero=zero, lr_table=table, lr_out=lr_out)
        torch.cuda.synchronize()
        rx, ry = R.gather_ref(h_data.float().numpy(), h_labels.numpy(), h_sched.numpy(), ctr, nrows)
        assert np.array_equal(out_x.float().cpu().numpy(), rx), ctr
        assert np.array_equal(out_y.cpu().numpy(), ry), ctr
        assert lr_out.item() == big_t[2 + ctr % nsteps].item(), ctr
        assert int(counter.item()) == ctr          # no `done`: the counter is the caller's to advance
        assert torch.count_nonzero(big_z[8:45]) == 0 and bool(big_z[:8].isnan().all()) and \
            bool(big_z[45:].isnan().all())
    counter, done = _i32(1), _i32(0)
    for k in range(3):
        fn.gather_batch(data, labels, sched, counter, out_x, out_y, done=done)
        torch.cuda.synchronize()
        rx, ry = R.gather_ref(h_data.float().numpy(), h_labels.numpy(), h_sched.numpy(), 1 + k, nrows)
        assert np.array_equal(out_x.float().cpu().numpy(), rx) and np.array_equal(out_y.cpu().numpy(), ry)
        assert int(counter.item()) == 2 + k and int(done.item()) == 0
    assert lr_out.item() == big_t[2 + 7 % nsteps].item()     # no table: lr_out is left alone
    assert torch.equal(dbig.cpu(), big) and torch.equal(ds.cpu(), big_s)


# ------------------------------------------------------------------------------------------- scheduled graph
def _engine(dtype, **kw):
    from rafiki_amd.engine.convnet import ConvNetEngine
    args = dict(num_classes=10, in_channels=3, image_size=16, cfg=(16, 'M', 32, 32, 'M'), fc_dims=(32,),
                device=DEV, seed=3, lr=0.05, dtype=dtype, optimizer='sgd')
    args.update(kw)
    return ConvNetEngine(**args)


@pytest.mark.parametrize('dtype', ['bf16', 'fp32'])
def test_scheduled_graph_follows_the_lr_schedule(dtype):
    """set_schedule(lr_scales=...) -> the prologue's lr_table[counter] -> lr_out -> the SGD kernel's lr_ptr,
    replayed, against an eager loop that sets the same multiplier before each step (the tolerances of
    test_scheduled_graph_matches_eager_and_advances_counter / test_scheduled_graph_fp32; an index one off moves
    the result >= 10x past them, tests/test_flat_optim.py).  On the 0.0 step the weights keep every bit."""
    e1, e2 = _engine(dtype), _engine(dtype)
    steps, B = len(R.LR_SCALES), 32
    gen = torch.Generator().manual_seed(7)
    x = torch.zeros((96,) + tuple(e1.input_shape(1))[1:])
    x[..., :3] = torch.randn(x[..., :3].shape, generator=gen)
    data = x.to(e1.act_dtype).to(DEV)
    labels = torch.randint(0, 10, (96,), generator=gen, dtype=torch.int32).to(DEV)
    idx = torch.randint(0, 96, (steps, B), device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    e2.capture_scheduled(data, labels, steps, B)
    e2.set_schedule(idx, lr_scales=R.LR_SCALES)
    for i, s in enumerate(R.LR_SCALES):
        e1.opt.set_lr_scale(s)
        e1.train_step(data[idx[i]].contiguous(), labels[idx[i]].contiguous())
        before = e2.flat.master.clone()
        e2.replay()
        torch.cuda.synchronize()
        assert torch.equal(before, e2.flat.master) == (s == 0.0), (i, s)
    assert int(e2._ctr.item()) == steps
    assert torch.allclose(e1.flat.master, e2.flat.master, rtol=1e-5, atol=1e-6)
    assert torch.allclose(e1.running, e2.running, rtol=1e-4, atol=1e-6)


# ------------------------------------------------------------------------------------------- Philox
@pytest.mark.parametrize('step', R.PHILOX_STEPS)
def test_philox_stream_matches_the_host_twin(fn, step):
    """Uniform and randint draws are the host twin's, bit for bit, at both sizes.  Normal draws follow the
    e_ref rule at n = 1027, where the fp32 NumPy yardstick's maximum over a thousand draws is an estimate of
    fp32's error; at n = 7 that maximum scatters between 5.9e-8 and 2.8e-7 with the seed while the kernel's
    error is the same 4e-8 .. 4e-7 as at n = 1027 (measured on an MI355X), so the short draw is instead held
    to the stronger claim that it is bit-identical to the head of the long one, whose error is bounded."""
    for seed in R.PHILOX_SEEDS:
        for stream in R.PHILOX_STREAMS:
            st = None if step is None else _i32(step)
            normal = {}
            for n in R.PHILOX_SIZES:
                u = fn.philox_(torch.empty(n, device=DEV), fn.RNG_UNIFORM, seed=seed, stream_id=stream, step=st)
                assert torch.equal(u.cpu(), torch.from_numpy(R.philox_uniform(n, seed, stream, step)))
                for hi in (10, 1000003):
                    r = fn.philox_(torch.empty(n, dtype=torch.int32, device=DEV), fn.RNG_RANDINT, seed=seed,
                                   stream_id=stream, step=st, hi=hi)
                    assert torch.equal(r.cpu(), torch.from_numpy(R.philox_randint(n, hi, seed, stream, step)))
                buf = torch.full((n + 5,), 77.0, device=DEV)     # the tail quad must stop at n
                normal[n] = fn.philox_(buf[:n], fn.RNG_NORMAL, seed=seed, stream_id=stream, step=st).clone()
                assert bool((buf[n:] == 77.0).all())
            short, long = (normal[n] for n in R.PHILOX_SIZES)
            ref = R.philox_normal(long.numel(), seed, stream, step)
            e_ref = R.err(R.philox_normal(long.numel(), seed, stream, step, dtype=np.float32), ref)
            _within('philox normal n={} seed={:#x} stream={:#x} step={}'.format(long.numel(), seed, stream, step),
                    long, ref, R.TOL_FACTOR * e_ref)
            assert torch.equal(short, long[:short.numel()])
