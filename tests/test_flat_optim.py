"""CPU side of the loss / optimizer kernel tests (tests/test_loss_optim_gpu.py holds the GPU side).

 a. The CPU paths of FlatSGD and FlatAdam (the project's own statement of what rk_sgd_step / rk_adam_step /
    rk_adam_multi compute) and the fp64 formulas of tests/loss_optim_refs.py against fp64 torch.optim.
 b. The host twin of the Philox4x32-10 stream against the published Random123 vectors.
 c. Sensitivity: each wrong formula a kernel could plausibly carry moves the fp64 reference, on the GPU
    tests' own inputs, by at least 10x the tolerance the GPU test applies there — so a kernel with that error
    cannot pass.
"""
import numpy as np
import pytest
import torch

import loss_optim_refs as R

# worst-case fp32 rounding budget of the CPU paths against fp64, max norm relative to max |w|: per step one
# rounding of the weight (2^-24) and a handful in the update, which is a fraction of max |w| here
CPU_PATH_TOL = R.ADAM_STEPS * 4 * 2.0 ** -24


def _torch_optim(kind, w0, grads, segs, *, lr, scales=None, **kw):
    """fp64 torch.optim over one parameter per segment (a, b, wd, lr_mult) -> (w, state tensors...)."""
    w0 = w0.double()
    ps = [torch.nn.Parameter(w0[a:b].clone()) for a, b, _, _ in segs]
    if kind == 'sgd':
        opt = torch.optim.SGD([dict(params=[p], weight_decay=wd) for p, (_, _, wd, _) in zip(ps, segs)], lr=lr, **kw)
    else:
        cls = torch.optim.AdamW if kw.pop('decoupled') else torch.optim.Adam
        eps = kw.pop('eps')
        opt = cls([dict(params=[p], weight_decay=wd, lr=lr * mult, eps=eps * mult)
                   for p, (_, _, wd, mult) in zip(ps, segs)], **kw)
    for i, g in enumerate(grads):
        for p, (a, b, _, mult) in zip(ps, segs):
            p.grad = g[a:b].double().clone()
        if scales is not None:
            for grp in opt.param_groups:
                grp['lr'] = lr * scales[i]
        opt.step()
    out = [w0.clone()]
    keys = ('momentum_buffer',) if kind == 'sgd' else ('exp_avg', 'exp_avg_sq')
    for k in keys:
        out.append(torch.zeros_like(w0))
    for p, (a, b, _, _) in zip(ps, segs):
        out[0][a:b] = p.detach()
        for j, k in enumerate(keys, 1):
            if k in opt.state[p] and opt.state[p][k] is not None:
                out[j][a:b] = opt.state[p][k]
    return out


# ------------------------------------------------------------------------------------- a. CPU paths
@pytest.mark.parametrize('mode', list(R.SGD_MODES))
def test_flat_sgd_cpu_path_matches_fp64_torch_optim(mode):
    n, decay_end = 5760, 5120
    w0, grads = R.sgd_inputs(n)
    hp = R.SGD_MODES[mode]
    ref = _torch_optim('sgd', w0, grads, [(0, decay_end, R.SGD_HP['wd'], 1.0), (decay_end, n, 0.0, 1.0)],
                       lr=R.SGD_HP['lr'], scales=R.SGD_SCALES, momentum=hp['momentum'], nesterov=hp['nesterov'])
    w64, mom64 = R.run_sgd_ref(w0, grads, mode=mode, decay_end=decay_end)
    assert R.err(w64, ref[0]) < 1e-13
    f, opt = R.run_flat_sgd('cpu', w0, grads, mode=mode, decay_end=decay_end, with_bf16=True)
    e = R.err(f.master, ref[0])
    print('FlatSGD cpu vs fp64 torch.optim', mode, 'w', e)
    assert e < CPU_PATH_TOL
    if mom64 is not None:
        assert R.err(mom64, ref[1]) < 1e-13
        assert R.err(opt.mom, ref[1]) < CPU_PATH_TOL
    assert torch.equal(f.bf16, f.master.bfloat16())


@pytest.mark.parametrize('decay', list(R.ADAM_DECAY))
@pytest.mark.parametrize('b1,b2', R.ADAM_BETAS)
@pytest.mark.parametrize('live', [False, True])
def test_flat_adam_cpu_path_matches_fp64_torch_optim(b1, b2, decay, live):
    """Adam and AdamW with per-segment equalized-LR multipliers (lr * mult, eps * mult), whole arena and a
    live subset; parameters outside the live set stay bit-identical."""
    wd, decoupled = R.ADAM_DECAY[decay]
    f = R.adam_arena('cpu')
    f0 = R.adam_arena('cpu')
    rng = f.ranges_of(R.ADAM_LIVE) if live else None
    grads = R.fresh_grads(f.total, R.ADAM_STEPS, 21)
    segs = R.live_segments(f0, wd, rng)
    assert len({m for _, _, _, m in segs}) > 2      # several lr_mult != 1 segments
    ref = _torch_optim('adam', f0.master, grads, segs, lr=R.ADAM_HP['lr'], eps=R.ADAM_HP['eps'], betas=(b1, b2),
                       decoupled=decoupled)
    mine = R.run_adam_ref(f0, grads, b1=b1, b2=b2, wd=wd, decoupled=decoupled, live=rng)
    opt = R.run_flat_adam(f, grads, b1=b1, b2=b2, wd=wd, decoupled=decoupled, live=rng)
    assert int(opt.t.item()) == R.ADAM_STEPS
    for name, a64, a32, r in zip('wmv', mine, (f.master, opt.m, opt.v), ref):
        assert R.err(a64, r) < 1e-12, name
        e = R.err(a32, r)
        print('FlatAdam cpu vs fp64 torch.optim', (b1, b2, decay, live), name, e)
        assert e < CPU_PATH_TOL, name
    if live:
        mask = torch.ones(f.total, dtype=torch.bool)
        for a, b in rng:
            mask[a:b] = False
        assert mask.any()
        assert torch.equal(f.master[mask], f0.master[mask])
        assert torch.count_nonzero(opt.m[mask]) == 0 and torch.count_nonzero(opt.v[mask]) == 0
    assert torch.equal(f.bf16, f.master.bfloat16())


def test_flat_adam_cpu_path_skip_flag_changes_nothing():
    f, f0 = R.adam_arena('cpu'), R.adam_arena('cpu')
    grads = R.fresh_grads(f.total, 2, 22)
    opt = R.run_flat_adam(f, grads, b1=0.9, b2=0.999, wd=1e-2, decoupled=True,
                          skip_flag=torch.ones(1, dtype=torch.int32))
    assert int(opt.t.item()) == 0
    assert torch.equal(f.master, f0.master) and torch.equal(f.bf16, f0.bf16)
    assert torch.count_nonzero(opt.m) == 0 and torch.count_nonzero(opt.v) == 0


# ------------------------------------------------------------------------------------- b. Philox
def test_philox_twin_reproduces_the_random123_vectors():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, out in kat:
        assert tuple(int(x) for x in R.philox4x32_10(ctr, key)) == out
    # the three at once: the array form is the scalar form per element
    got = R.philox4x32_10([np.array([k[0][i] for k in kat[:2]], dtype=np.uint64) for i in range(4)], (0, 0))
    assert tuple(int(x) for x in got[0]) == kat[0][2]


def test_philox_twin_stream_mapping():
    """Element 4q + j is word j of counter (q, 0, stream_id, step) under key (seed low, seed high); uniform is
    (x >> 8) * 2^-24 and randint min(int(u * hi), hi - 1)."""
    seed, stream, step, n = R.PHILOX_SEEDS[1], R.PHILOX_STREAMS[1], 5, 1027
    w = R.philox_words(n, seed, stream, step)
    assert w.dtype == np.uint32 and w.shape == (n,)
    for q in (0, 1, 256):
        one = R.philox4x32_10((q, 0, stream, step), (seed & 0xFFFFFFFF, seed >> 32))
        assert np.array_equal(w[4 * q:4 * q + 4], one[:min(4, n - 4 * q)])
    assert np.array_equal(R.philox_words(7, seed, stream, step), w[:7])
    assert np.array_equal(R.philox_words(n, seed, stream, None), R.philox_words(n, seed, stream, 0))
    for other in ((seed ^ (1 << 40), stream, step), (seed, stream + 1, step), (seed, stream, step + 1)):
        assert not np.array_equal(R.philox_words(n, *other)[:4], w[:4])
    u = R.philox_uniform(n, seed, stream, step)
    assert u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 1.0
    assert np.array_equal(u.astype(np.float64) * 2.0 ** 24, (w >> 8).astype(np.float64))
    for hi in (1, 10, 1 << 24, (1 << 31) - 1):
        r = R.philox_randint(n, hi, seed, stream, step)
        assert r.dtype == np.int32 and r.min() >= 0 and r.max() <= hi - 1
    assert np.array_equal(R.philox_randint(n, 1 << 24, seed, stream, step), (w >> 8).astype(np.int32))
    z = R.philox_normal(n, seed, stream, step)
    z32 = R.philox_normal(n, seed, stream, step, dtype=np.float32)
    assert z.dtype == np.float64 and z32.dtype == np.float32 and np.isfinite(z).all()
    assert abs(z.mean()) < 0.15 and abs(z.std() - 1.0) < 0.1 and np.abs(z32 - z).max() < 1e-5


# ------------------------------------------------------------------------------------- c. sensitivity
def _visible(wrong, ref, tols):
    """The wrong formula's outputs differ from the reference's by >= SENSITIVITY x the tolerance in at least
    one output the GPU test checks."""
    return any(R.err(a, r) >= R.SENSITIVITY * t for a, r, t in zip(wrong, ref, tols) if r is not None)


def _sgd_cases():
    for n in R.SGD_SIZES:
        ends = R.sgd_decay_ends(n) if n < 1 << 20 else [n // 2 // 4 * 4, n]
        for mode in R.SGD_MODES:
            for de in ends:
                yield n, mode, de


@pytest.mark.parametrize('n', R.SGD_SIZES)
def test_sgd_tolerance_catches_wrong_formulas(n):
    """decay_end moved by one 4-element vector, Nesterov flipped, the LR multipliers taken one step late."""
    w0, grads = R.sgd_inputs(n)
    for n_, mode, de in _sgd_cases():
        if n_ != n:
            continue
        ref = R.run_sgd_ref(w0, grads, mode=mode, decay_end=de)
        f, opt = R.run_flat_sgd('cpu', w0, grads, mode=mode, decay_end=de)
        tols = R.tolerances((f.master, opt.mom), ref)
        moved = de + 4 if de < n else de - 4
        assert _visible(R.run_sgd_ref(w0, grads, mode=mode, decay_end=moved), ref, tols), (mode, de, 'decay_end')
        if mode != 'plain':     # without a momentum buffer the flag has no meaning
            flipped = R.run_sgd_ref(w0, grads, mode=mode, decay_end=de, nesterov=not R.SGD_MODES[mode]['nesterov'])
            assert _visible(flipped, ref, tols), (mode, de, 'nesterov')
        late = R.run_sgd_ref(w0, grads, mode=mode, decay_end=de, scales=(R.SGD_SCALES[-1],) + R.SGD_SCALES[:-1])
        assert _visible(late, ref, tols), (mode, de, 'lr scale index')


@pytest.mark.parametrize('mode', list(R.SGD_MODES))
def test_sgd_tolerance_catches_ignored_grad_scale(mode):
    n, gs = 4104, R.SGD_GRAD_SCALE
    w0, grads = R.sgd_inputs(n)
    ref = R.run_sgd_ref(w0, grads, mode=mode, decay_end=n, grad_scale=gs)
    f, opt = R.run_flat_sgd('cpu', w0, [g * gs for g in grads], mode=mode, decay_end=n)
    tols = R.tolerances((f.master, opt.mom), ref)
    assert _visible(R.run_sgd_ref(w0, grads, mode=mode, decay_end=n), ref, tols)


@pytest.mark.parametrize('decay', list(R.ADAM_DECAY))
@pytest.mark.parametrize('b1,b2', R.ADAM_BETAS)
@pytest.mark.parametrize('gs', [1.0, R.ADAM_GRAD_SCALE])
def test_adam_tolerance_catches_wrong_formulas(b1, b2, decay, gs):
    """Bias correction c1 dropped, 1 - beta2 formed from the fp32 beta2, coupled and decoupled decay swapped,
    grad_scale ignored — on the arena, gradients and live set of the GPU test.  1 - fp32(0.99) is off by
    9.5e-7 relative, inside fp32 rounding of the second moment itself, so only beta2 = 0.999 (1.3e-5) can
    and must show that one."""
    wd, decoupled = R.ADAM_DECAY[decay]
    f, f0 = R.adam_arena('cpu'), R.adam_arena('cpu')
    rng = f.ranges_of(R.ADAM_LIVE)
    grads = R.fresh_grads(f.total, R.ADAM_STEPS, 21)
    kw = dict(b1=b1, b2=b2, wd=wd, decoupled=decoupled, live=rng)
    ref = R.run_adam_ref(f0, grads, grad_scale=gs, **kw)
    opt = R.run_flat_adam(f, [g * gs for g in grads], **kw)
    tols = R.tolerances((f.master, opt.m, opt.v), ref)
    print('adam tolerances (w, m, v)', (b1, b2, decay, gs), tols)
    if b1 > 0:
        assert _visible(R.run_adam_ref(f0, grads, grad_scale=gs, drop_c1=True, **kw), ref, tols), 'c1'
    if b2 == 0.999:
        omb2 = 1.0 - float(np.float32(b2))
        assert _visible(R.run_adam_ref(f0, grads, grad_scale=gs, omb2=omb2, **kw), ref, tols), 'omb2'
    if wd > 0:
        swapped = dict(kw, decoupled=not decoupled)
        assert _visible(R.run_adam_ref(f0, grads, grad_scale=gs, **swapped), ref, tols), 'decay form'
    if gs != 1.0:
        assert _visible(R.run_adam_ref(f0, grads, grad_scale=1.0, **kw), ref, tols), 'grad_scale'


@pytest.mark.parametrize('t', [x for x in R.LERP_T if x != 0.5])    # at 0.5 the swap is the same formula
def test_lerp_tolerance_catches_swapped_t(t):
    gen = torch.Generator().manual_seed(31)
    dst, src = torch.randn(1027, generator=gen), torch.randn(1027, generator=gen)
    ref = R.lerp_ref(dst.double(), src.double(), t)
    tol = R.TOL_FACTOR * R.err(R.lerp_ref(dst, src, t), ref)
    assert R.err(R.lerp_ref(dst.double(), src.double(), 1.0 - t), ref) >= R.SENSITIVITY * max(tol, 2.0 ** -24)


@pytest.mark.parametrize('B', R.XENT_B)
def test_softmax_bounds_catch_counted_ignored_rows(B):
    for ncls in R.XENT_NCLS:
        logits, labels = R.xent_inputs(B, ncls, padded=True)
        gs = 1.0 / B
        ref = R.xent_ref(logits, labels, ncls, grad_scale=gs)
        bad = R.xent_ref(logits, labels, ncls, grad_scale=gs, count_ignored=True)
        assert ref['counted'] < B and bad['counted'] == B
        if ncls > 1:    # one class: the loss and the gradient are zero whatever the label
            assert abs(bad['loss_sum'] - ref['loss_sum']) / B >= R.SENSITIVITY * R.LOSS_TOL
            assert (bad['dlogits'] - ref['dlogits']).abs().max().item() >= R.SENSITIVITY * R.PROB_TOL * gs
            assert R.err(bad['dlogits'], ref['dlogits']) >= R.SENSITIVITY * R.BF16_REL


def _cpu_engine():
    from rafiki_amd.engine.convnet import ConvNetEngine
    return ConvNetEngine(num_classes=10, in_channels=3, image_size=16, cfg=(16, 'M', 32, 32, 'M'), fc_dims=(32,),
                         device='cpu', seed=3, lr=0.05, dtype='fp32')


def test_scheduled_lr_tolerance_catches_table_index_off_by_one():
    """The scheduled-graph tests compare a replayed graph with an eager loop at allclose(rtol=1e-5,
    atol=1e-6).  The same eager loop (here on the CPU path of the engine) with the LR table read one entry
    late or one early ends >= 10x that bound away."""
    gen = torch.Generator().manual_seed(7)
    steps, B = len(R.LR_SCALES), 32
    e0 = _cpu_engine()
    x = torch.zeros((steps,) + tuple(e0.input_shape(B)))
    x[..., :3] = torch.randn(x[..., :3].shape, generator=gen)
    y = torch.randint(0, 10, (steps, B), generator=gen, dtype=torch.int32)

    def run(scales):
        e = _cpu_engine()
        for i in range(steps):
            e.opt.set_lr_scale(scales[i])
            e.train_step(x[i], y[i])
        return e.flat.master.clone()
    ref = run(R.LR_SCALES)
    for wrong in (R.LR_SCALES[1:] + R.LR_SCALES[:1], R.LR_SCALES[-1:] + R.LR_SCALES[:-1]):
        got = run(wrong)
        excess = ((got - ref).abs() / (1e-6 + 1e-5 * ref.abs())).max().item()
        assert excess >= R.SENSITIVITY, (wrong, excess)
