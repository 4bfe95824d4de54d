"""Global-norm gradient clipping, CPU side (tests/test_grad_clip_gpu.py holds the kernels).

 a. The CPU paths of FlatSGD / FlatAdam with ``clip_norm`` (the project's host statement of rk_grad_sumsq +
    rk_sgd_step_clip / rk_adam_step_clip) against fp64 torch: clip_grad_norm_, then the fp64 formulas of
    tests/loss_optim_refs.py.  Tolerance: TOL_FACTOR * e_ref, e_ref the error of the same formulas evaluated in
    plain fp32 on the same inputs (R.tolerances).
 b. inf measures without changing a bit; a non-finite gradient skips the step.
 c. Argument validation of the engines, the knob plumbing of the models, and the arena norm of a ConvNetEngine
    against the fp64 norm over the real (unpadded) parameters.
"""
import math

import numpy as np
import pytest
import torch

import loss_optim_refs as R

STEPS = 5
GRAD_SCALES = (0.1, 1.0, 0.1, 1.0, 0.1)     # times N(0, 1): norms about 0.09 and 0.9 sqrt(n)


def _cap(n):
    """Between the two norms GRAD_SCALES gives: the steps scaled 1.0 clip, the others do not."""
    return 0.4 * math.sqrt(n)


def _grads(n, seed):
    return [g * s for g, s in zip(R.fresh_grads(n, STEPS, seed), GRAD_SCALES)]


def _clipped64(g, max_norm):
    """(the fp64 gradient after torch's clip_grad_norm_, its fp64 norm before)."""
    p = torch.nn.Parameter(torch.zeros(g.numel(), dtype=torch.float64))
    p.grad = g.double().clone()
    norm = torch.nn.utils.clip_grad_norm_([p], max_norm)
    return p.grad, float(norm)


def _coef(norm, max_norm):
    return min(1.0, max_norm / (norm + 1e-6))


def _cpu_ctx():
    from rafiki_amd.parallel.context import TrialContext, use_context
    return use_context(TrialContext(device=torch.device('cpu')))


# ------------------------------------------------------------------------------------- a. CPU paths
@pytest.mark.parametrize('mode', list(R.SGD_MODES))
def test_flat_sgd_cpu_clip_matches_fp64(mode):
    from rafiki_amd.engine.flat import FlatSGD
    n, decay_end = 5760, 5120
    w0, _ = R.sgd_inputs(n)
    grads, cap, hp = _grads(n, 31), _cap(n), R.SGD_MODES[mode]
    kw = dict(lr=R.SGD_HP['lr'], momentum=hp['momentum'], wd=R.SGD_HP['wd'], nesterov=hp['nesterov'],
              decay_end=decay_end)
    w64, m64 = w0.double(), (torch.zeros(n, dtype=torch.float64) if hp['momentum'] > 0 else None)
    w32, m32 = w0.clone(), (torch.zeros(n) if hp['momentum'] > 0 else None)
    f = R.bare_arena('cpu', w0, decay_end, True)
    opt = FlatSGD(f, R.SGD_HP['lr'], momentum=hp['momentum'], weight_decay=R.SGD_HP['wd'], nesterov=hp['nesterov'],
                  clip_norm=cap)
    norms = []
    for g in grads:
        g64, norm = _clipped64(g, cap)
        norms.append(norm)
        w64, m64 = R.sgd_ref(w64, g64, m64, **kw)
        w32, m32 = R.sgd_ref(w32, g, m32, grad_scale=float(np.float32(_coef(norm, cap))), **kw)   # the fp32 yardstick
        f.grad.copy_(g)
        opt.step()
        assert opt.clip.read()['last_norm'] == pytest.approx(norm, rel=2.0 ** -22)
    tols = R.tolerances((w32, m32), (w64, m64))
    for name, got, ref, tol in zip(('w', 'mom'), (f.master, opt.mom), (w64, m64), tols):
        if ref is not None:
            e = R.err(got, ref)
            print('FlatSGD cpu clip', mode, name, e, 'tol', tol)
            assert e <= tol, name
    st = opt.clip.read()
    clipped = sum(nm > cap for nm in norms)
    assert 0 < clipped < STEPS                       # both kinds of step occurred
    assert (st['clipped'], st['skipped'], st['steps']) == (clipped, 0, STEPS)
    assert st['max_norm'] == pytest.approx(max(norms), rel=1e-6)
    assert st['mean_norm'] == pytest.approx(sum(norms) / STEPS, rel=1e-6)
    assert torch.equal(f.bf16, f.master.bfloat16())


@pytest.mark.parametrize('decay', list(R.ADAM_DECAY))
@pytest.mark.parametrize('b1,b2', [R.ADAM_BETAS[0], R.ADAM_BETAS[-1]])
def test_flat_adam_cpu_clip_matches_fp64(b1, b2, decay):
    from rafiki_amd.engine.flat import FlatAdam
    wd, decoupled = R.ADAM_DECAY[decay]
    f, f0 = R.adam_arena('cpu'), R.adam_arena('cpu')
    n = f.total
    grads, cap = _grads(n, 41), _cap(n)
    segs = R.live_segments(f0, wd, None)
    opt = FlatAdam(f, R.ADAM_HP['lr'], betas=(b1, b2), eps=R.ADAM_HP['eps'], weight_decay=wd, decoupled=decoupled,
                   clip_norm=cap)
    state = {torch.float64: None, torch.float32: None}
    for dt in state:
        w = f0.master.to(dt).clone()
        state[dt] = [w, torch.zeros_like(w), torch.zeros_like(w)]
    norms = []
    for t, g in enumerate(grads, 1):
        g64, norm = _clipped64(g, cap)
        norms.append(norm)
        for dt, (w, m, v) in state.items():
            # fp64: torch's clipped gradient; fp32 (the yardstick): the fp32 gradient times the fp32 coefficient
            gg = g64 if dt == torch.float64 else g * float(np.float32(_coef(norm, cap)))
            for a, b, swd, mult in segs:
                w[a:b], m[a:b], v[a:b] = R.adam_ref(w[a:b], gg[a:b], m[a:b], v[a:b], lr=R.ADAM_HP['lr'] * mult,
                                                    b1=b1, b2=b2, eps=R.ADAM_HP['eps'] * mult, wd=swd,
                                                    decoupled=decoupled, t=t)
        f.grad.copy_(g)
        opt.step()
    tols = R.tolerances(state[torch.float32], state[torch.float64])
    for name, got, ref, tol in zip('wmv', (f.master, opt.m, opt.v), state[torch.float64], tols):
        e = R.err(got, ref)
        print('FlatAdam cpu clip', (b1, b2, decay), name, e, 'tol', tol)
        assert e <= tol, name
    st = opt.clip.read()
    clipped = sum(nm > cap for nm in norms)
    assert 0 < clipped < STEPS
    assert (st['clipped'], st['skipped'], st['steps']) == (clipped, 0, STEPS)
    assert int(opt.t.item()) == STEPS


# ------------------------------------------------------------------------------------- b. inf and non-finite
@pytest.mark.parametrize('kind', ['sgd', 'adam'])
def test_inf_measures_and_changes_no_bit(kind):
    from rafiki_amd.engine.flat import FlatAdam, FlatSGD
    n = 4104 if kind == 'sgd' else R.adam_arena('cpu').total
    w0, _ = R.sgd_inputs(n)
    grads = _grads(n, 51)
    out = []
    for clip_norm in (None, float('inf')):
        # (FlatAdam walks the arena's parameter specs: a bare arena has none)
        f = R.bare_arena('cpu', w0, n // 2 // 4 * 4, True) if kind == 'sgd' else R.adam_arena('cpu')
        opt = FlatSGD(f, 0.1, clip_norm=clip_norm) if kind == 'sgd' else \
            FlatAdam(f, 1e-2, weight_decay=1e-2, clip_norm=clip_norm)
        for g in grads:
            f.grad.copy_(g)
            opt.step()
        out.append((f, opt))
    (f_off, o_off), (f_inf, o_inf) = out
    assert o_off.clip is None
    assert torch.equal(f_off.master, f_inf.master) and torch.equal(f_off.bf16, f_inf.bf16)
    assert not torch.equal(f_off.master, (w0 if kind == 'sgd' else R.adam_arena('cpu').master))
    st = o_inf.clip.read()
    assert (st['clipped'], st['skipped'], st['steps']) == (0, 0, STEPS)
    assert st['last_norm'] == pytest.approx(float(grads[-1].double().norm()), rel=2.0 ** -22)
    assert float(o_inf.clip.stats[1]) == 1.0
    o_inf.clip.reset()
    assert o_inf.clip.read()['steps'] == 0


@pytest.mark.parametrize('kind', ['sgd', 'adam'])
@pytest.mark.parametrize('bad', [float('inf'), float('nan')])
def test_nonfinite_gradient_skips_the_step(kind, bad):
    from rafiki_amd.engine.flat import FlatAdam, FlatSGD
    n = 1028 if kind == 'sgd' else R.adam_arena('cpu').total
    w0, grads = R.sgd_inputs(n)
    f = R.bare_arena('cpu', w0, n, True) if kind == 'sgd' else R.adam_arena('cpu')
    opt = FlatSGD(f, 0.1, clip_norm=1.0) if kind == 'sgd' else FlatAdam(f, 1e-2, clip_norm=1.0)
    f.grad.copy_(grads[0])
    opt.step()
    state = [f.master, f.bf16] + ([opt.mom] if kind == 'sgd' else [opt.m, opt.v])
    before = [t.clone() for t in state]
    f.grad.copy_(grads[1])
    f.grad[517] = bad
    opt.step()
    for t, b in zip(state, before):
        assert torch.equal(t, b)
    st = opt.clip.read()
    assert (st['skipped'], st['steps'], st['clipped']) == (1, 2, 1)
    assert math.isfinite(st['mean_norm']) and math.isfinite(st['max_norm'])
    f.grad.copy_(grads[2])
    opt.step()                                       # and the next finite step runs
    assert not torch.equal(f.master, before[0])
    assert opt.clip.read()['steps'] == 3


def test_flat_adam_live_ranges_refuse_clipping():
    from rafiki_amd.engine.flat import FlatAdam
    f = R.adam_arena('cpu')
    opt = FlatAdam(f, 1e-2, clip_norm=1.0)
    with pytest.raises(NotImplementedError):
        opt.step(live=f.ranges_of(R.ADAM_LIVE))


# ------------------------------------------------------------------------------------- c. engines and models
TINY = dict(num_classes=10, in_channels=3, image_size=8, cfg=(8, 'M', 8, 'M'), fc_dims=(16,), device='cpu', seed=0,
            dtype='fp32')


@pytest.mark.parametrize('bad', [0, 0.0, -1.0, float('nan'), 'big', True])
def test_engines_refuse_a_bad_clip_norm(bad):
    from rafiki_amd.engine.convnet import ConvNetEngine
    from rafiki_amd.engine.flat import check_clip_norm
    with pytest.raises(ValueError):
        ConvNetEngine(clip_norm=bad, **TINY)
    with pytest.raises(ValueError):
        check_clip_norm(bad)         # what TaggerEngine(clip_norm=...) and the optimizers run on their argument


def test_engine_clip_norm_argument():
    import inspect
    from rafiki_amd.engine.convnet import ConvNetEngine
    from rafiki_amd.engine.tagger import TaggerEngine
    assert inspect.signature(TaggerEngine.__init__).parameters['clip_norm'].default is None
    off = ConvNetEngine(**TINY)
    assert off.clip_norm is None and off.opt.clip is None
    with pytest.raises(RuntimeError):
        off.grad_stats()
    for opt in ('sgd', 'adam'):
        for v in (2.5, float('inf'), 3):
            eng = ConvNetEngine(clip_norm=v, optimizer=opt, **TINY)
            assert eng.clip_norm == float(v) and eng.opt.clip.max_norm == float(v)
            assert eng.grad_stats() == {'last_norm': 0.0, 'mean_norm': 0.0, 'max_norm': 0.0, 'clipped': 0,
                                        'skipped': 0, 'steps': 0}


def test_model_knobs():
    from rafiki_amd.model import FloatKnob
    from rafiki_amd.models import ZOO, model_file
    from rafiki_amd.models.pos_tagging import PyBiLstm, PyBiLstmClip
    from rafiki_amd.models.vgg_small import VggSmall, VggSmallClip, VggSmallDrop
    assert ZOO['VggSmallClip'] == ('vgg_small.py', 'IMAGE_CLASSIFICATION')
    assert ZOO['PyBiLstmClip'] == ('pos_tagging.py', 'POS_TAGGING')
    assert model_file('VggSmallClip').endswith('vgg_small.py') and model_file('PyBiLstmClip').endswith('pos_tagging.py')
    for cls, base, lo, hi in ((VggSmallClip, VggSmallDrop, 0.5, 10.0), (PyBiLstmClip, PyBiLstm, 0.25, 8.0)):
        k = cls.get_knob_config()
        assert set(k) == set(base.get_knob_config()) | {'clip_norm'}
        assert 'clip_norm' not in base.get_knob_config()
        assert isinstance(k['clip_norm'], FloatKnob) and k['clip_norm'].is_exp
        assert (k['clip_norm'].value_min, k['clip_norm'].value_max) == (lo, hi)
    with _cpu_ctx():
        assert VggSmall()._regularisers() == {}
        assert VggSmall(clip_norm=0, track_grad_norm=False)._regularisers() == {}
        assert VggSmall(clip_norm=2.0)._regularisers() == {'clip_norm': 2.0}
        assert VggSmall(clip_norm=2.0, track_grad_norm=True)._regularisers() == {'clip_norm': 2.0}
        assert VggSmall(track_grad_norm=True)._regularisers() == {'clip_norm': float('inf')}
        for bad in (-1.0, float('inf'), float('nan')):
            with pytest.raises(ValueError):
                VggSmall(clip_norm=bad)._regularisers()
            with pytest.raises(ValueError):
                PyBiLstm(clip_norm=bad)._clip_norm()
        assert PyBiLstm()._clip_norm() is None and PyBiLstm(clip_norm=0.0)._clip_norm() is None
        assert PyBiLstm(clip_norm=1.5)._clip_norm() == 1.5


def _logged(monkeypatch):
    """Every logger.log(**metrics) of a trial, as a list of dicts."""
    from rafiki_amd.model import logger
    rows, log = [], logger.log

    def rec(*a, **kw):
        if kw:
            rows.append(dict(kw))
        return log(*a, **kw)
    monkeypatch.setattr(logger, 'log', rec)
    return rows


def _norm_rows(rows, epochs):
    rows = [r for r in rows if 'grad_norm' in r]
    assert [r['epoch'] for r in rows] == list(range(epochs))
    for r in rows:
        assert set(r) == {'grad_norm', 'grad_norm_max', 'clipped_share', 'epoch'}
        assert 0.0 < r['grad_norm'] <= r['grad_norm_max'] < float('inf') and 0.0 <= r['clipped_share'] <= 1.0
    return rows


def test_vgg_small_clip_trial(monkeypatch):
    """A VggSmallClip trial end to end on the CPU path: the knob reaches the engine, the three series are logged
    once per epoch, and a model rebuilt from the dumped parameters (no training) clips nothing."""
    from rafiki_amd.models.vgg_small import VggSmall, VggSmallClip
    rows = _logged(monkeypatch)
    train = 'synthetic://image?n=128&size=16&channels=3&classes=10&seed=0'
    knobs = dict(epochs=2, learning_rate=0.05, momentum=0.9, weight_decay=5e-4, batch_size=32, width_mult=0.5,
                 image_size=16, augment='none', mix='none', label_smoothing=0.0, dropout=0.0, feature_dropout=0.0,
                 seed=3)
    with _cpu_ctx():
        m = VggSmallClip(clip_norm=0.5, **knobs)
        m.train(train)
        assert m._engine.clip_norm == 0.5
        got = _norm_rows(rows, 2)
        assert any(r['clipped_share'] > 0.0 for r in got)        # a fresh VGG's gradient norm is far above 0.5
        assert 0.0 <= m.evaluate(train) <= 1.0
        m2 = VggSmallClip(clip_norm=0.5, **knobs)
        m2.load_parameters(m.dump_parameters())
        assert m2._engine.clip_norm is None
        del rows[:]
        t = VggSmall(track_grad_norm=True, **knobs)
        t.train(train)
        assert t._engine.clip_norm == float('inf')
        assert all(r['clipped_share'] == 0.0 for r in _norm_rows(rows, 2))
        del rows[:]
        off = VggSmall(clip_norm=0, **knobs)
        off.train(train)
        assert off._engine.clip_norm is None and not [r for r in rows if 'grad_norm' in r]


def test_pybilstm_clip_trial(monkeypatch):
    """A PyBiLstmClip trial on the CPU (torch modules + clip_grad_norm_): the same three series."""
    from rafiki_amd.models.pos_tagging import PyBiLstm, PyBiLstmClip
    rows = _logged(monkeypatch)
    knobs = dict(epochs=2, word_embed_dims=16, word_rnn_hidden_size=16, word_dropout=0.01, learning_rate=0.05,
                 batch_size=32)
    with _cpu_ctx():
        m = PyBiLstmClip(clip_norm=0.05, **knobs)    # a fresh tagger's gradient norm is about 0.1
        m.train('synthetic://corpus?n=96&seed=0')
        got = _norm_rows(rows, 2)
        assert any(r['clipped_share'] > 0.0 for r in got)
        assert 0.0 <= m.evaluate('synthetic://corpus?n=32&seed=1') <= 1.0
        del rows[:]
        PyBiLstm(**knobs).train('synthetic://corpus?n=96&seed=0')
        assert not [r for r in rows if 'grad_norm' in r]


@pytest.mark.parametrize('optimizer', ['sgd', 'adam'])
def test_engine_norm_is_the_norm_of_the_real_parameters(optimizer):
    """grad_stats()['last_norm'] of a CPU engine step against the fp64 norm of the gradients of reference_loss over
    the real parameters (the stem's padding channels and the padded classes left out): the arena's padding holds
    no gradient.  Bound 1e-5: what the project's fp32 gradients are held to against fp64 (tests/test_tagger_gpu.py),
    the norm being no worse than its worst element."""
    from rafiki_amd.engine.convnet import ConvNetEngine
    eng = ConvNetEngine(clip_norm=float('inf'), optimizer=optimizer, **TINY)
    gen = torch.Generator().manual_seed(5)
    x = torch.zeros(eng.input_shape(8))
    x[..., :3] = torch.randn((8, 8, 8, 3), generator=gen)
    y = torch.randint(0, 10, (8,), generator=gen, dtype=torch.int32)
    fl = eng.flat
    real = {n: fl.w(n).detach().double().clone().requires_grad_(True) for n in fl.names()}
    loss, _ = eng.reference_loss(x.double(), y, real, training=True)
    grads = dict(zip(fl.names(), torch.autograd.grad(loss, [real[n] for n in fl.names()])))
    grads['conv0.w'] = grads['conv0.w'][..., :3]
    grads['out.w'], grads['out.b'] = grads['out.w'][:10], grads['out.b'][:10]
    want = math.sqrt(sum(float(g.pow(2).sum()) for g in grads.values()))
    eng.train_step(x, y)
    st = eng.grad_stats()
    assert st['steps'] == 1 and st['last_norm'] == pytest.approx(want, rel=1e-5)
    # and the whole arena, padding included, carries exactly the gradients of its specs
    assert float(fl.grad.double().pow(2).sum()) == pytest.approx(
        sum(float(fl.g(n).double().pow(2).sum()) for n in fl.names()), rel=1e-12)
    eng.reset_metrics()
    assert eng.grad_stats()['steps'] == 0
