"""Global-norm gradient clipping on the GPU: rk_grad_sumsq, rk_sgd_step_clip / rk_adam_step_clip, and the engines
that run them inside their captured steps (tests/test_grad_clip.py holds the CPU side).

 1. The reduce kernel against the fp64 norm: |norm - ref| <= 2^-22 ref — the fp64 accumulation error (n 2^-53) is
    negligible, the square root and the rounding to fp32 contribute at most 2^-24 each — and bit-equal partials
    from two launches.
 2. The coefficient path: a clipped step is the bits of the unclipped entry point called with grad_scale = coef.
 3. ConvNetEngine (tiny net, fp32 / bf16, SGD / Adam): the norm it reports, zero padding, inf = off bit for bit in
    eager steps, capture and capture_scheduled, a binding cap, and no trace of the warm-up steps.
 4. TaggerEngine against the fp64 module with clip_grad_norm_ + torch.optim.Adam, and replay = eager.
Every figure is printed before it is asserted (pytest -s).
"""
import math

import numpy as np
import pytest
import torch

import loss_optim_refs as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NORM_TOL = 2.0 ** -22
STATS = ('last_norm', 'last_coef', 'norm_sum', 'norm_max', 'clipped', 'skipped', 'steps')


@pytest.fixture(scope='module')
def fn():
    from rafiki_amd.ops import _lib, functional
    _lib.lib()  # loud failure if the native library is missing
    return functional


def _i32(v=0):
    return torch.full((1,), v, dtype=torch.int32, device=DEV)


def _partials(fn, g):
    part = torch.full((fn.sumsq_parts(g.numel()),), -1.0, dtype=torch.float64, device=DEV)
    return fn.grad_sumsq(g, part)


def _norm32(part):
    """The optimizer kernels' norm of the partials: the fp32 rounding of the square root of their fp64 sum."""
    return float(np.float32(math.sqrt(float(part.cpu().sum()))))


def _coef32(norm, max_norm):
    """min(1, max_norm / (norm + 1e-6)) in fp32 operations, as the kernels and clip_grad_norm_ form it."""
    return float(min(np.float32(1.0), np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))))


# ------------------------------------------------------------------------------------------- 1. the reduce
def _sumsq_input(kind, n):
    gen = torch.Generator().manual_seed(n % 1000 + len(kind))
    if kind == 'normal':
        return torch.randn(n, generator=gen)
    if kind == 'wide':      # magnitudes from 1e-20 to 1e+10, both signs
        mag = torch.pow(10.0, torch.rand(n, generator=gen, dtype=torch.float64) * 30.0 - 20.0)
        return (mag * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1)).float()
    return torch.full((n,), 1e20)      # every square overflows fp32


@pytest.mark.parametrize('kind', ['normal', 'wide', 'huge'])
@pytest.mark.parametrize('n', R.SGD_SIZES)
def test_grad_sumsq_matches_fp64(fn, n, kind):
    g = _sumsq_input(kind, n)
    ref = float(g.double().pow(2).sum().sqrt())
    gd = g.to(DEV)
    a, b = _partials(fn, gd), _partials(fn, gd)
    torch.cuda.synchronize()
    assert a.numel() == {4: 1, 1028: 2, 4104: 5}.get(n, 256)      # a function of n alone
    assert torch.equal(a, b)
    assert bool(torch.isfinite(a).all()) and bool((a >= 0).all())
    norm = _norm32(a)
    print('grad_sumsq n={} {}: norm {:.9e} ref {:.9e} rel {:.3e} bound {:.3e}'.format(
        n, kind, norm, ref, abs(norm - ref) / ref, NORM_TOL))
    assert math.isfinite(norm) and abs(norm - ref) <= NORM_TOL * ref
    assert torch.equal(gd.cpu(), g)                                 # the gradients are only read


def test_grad_sumsq_refuses_bad_arguments(fn):
    from rafiki_amd.ops._lib import KernelError
    g = torch.ones(4104, device=DEV)
    with pytest.raises(ValueError):
        fn.grad_sumsq(g, torch.zeros(4, dtype=torch.float64, device=DEV))       # 5 partials, not 4
    with pytest.raises(ValueError):
        fn.grad_sumsq(g, torch.zeros(5, dtype=torch.float32, device=DEV))
    with pytest.raises(KernelError):
        fn.grad_sumsq(torch.ones(6, device=DEV), torch.zeros(1, dtype=torch.float64, device=DEV))   # n % 4


# ------------------------------------------------------------------------------------------- 2. the coefficient
def _sgd_bufs(n, with_wb, seed=0):
    gen = torch.Generator().manual_seed(100 + n + seed)
    w, g, mom = (torch.randn(n, generator=gen).to(DEV) for _ in range(3))
    return dict(w=w, g=g, mom=mom, wb=w.bfloat16() if with_wb else None)


def _run_sgd(fn, b, mode, **kw):
    """One sgd_step on copies of the buffers b -> (w, mom, wb, bump)."""
    hp = R.SGD_MODES[mode]
    w, mom = b['w'].clone(), (b['mom'].clone() if hp['momentum'] > 0 else None)
    wb = None if b['wb'] is None else b['wb'].clone()
    bump, lr = _i32(5), torch.full((1,), 0.5, device=DEV)
    n = w.numel()
    fn.sgd_step(w, b['g'], mom, wb=wb, lr=R.SGD_HP['lr'], momentum=hp['momentum'], weight_decay=R.SGD_HP['wd'],
                nesterov=hp['nesterov'], lr_tensor=lr, decay_end=n // 2 // 4 * 4, bump=bump, **kw)
    torch.cuda.synchronize()
    return w, mom, wb, bump


def _same(xs, ys):
    for x, y in zip(xs, ys):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.dtype == y.dtype and torch.equal(x, y)


@pytest.mark.parametrize('with_wb', [True, False])
@pytest.mark.parametrize('n', [4, 4104])
@pytest.mark.parametrize('mode', list(R.SGD_MODES))
def test_sgd_clip_is_grad_scale_coef(fn, mode, n, with_wb):
    b = _sgd_bufs(n, with_wb)
    part = _partials(fn, b['g'])
    ref = float(b['g'].double().norm())
    cap = 0.5 * ref
    stats = torch.zeros(fn.CLIP_STATS, device=DEV)
    got = _run_sgd(fn, b, mode, clip=(part, cap, stats))
    st = dict(zip(STATS, stats.tolist()))
    print('sgd clip', mode, n, with_wb, st)
    assert abs(st['last_norm'] - ref) <= NORM_TOL * ref
    assert st['last_coef'] == _coef32(st['last_norm'], cap) and 0.49 < st['last_coef'] < 0.51
    assert (st['norm_sum'], st['norm_max']) == (st['last_norm'], st['last_norm'])
    assert (st['clipped'], st['skipped'], st['steps']) == (1.0, 0.0, 1.0)
    want = _run_sgd(fn, b, mode, grad_scale=st['last_coef'])
    _same(got, want)
    assert int(got[3]) == 6 and not torch.equal(got[0], b['w'])
    # a second clipped step accumulates; a cap above the norm leaves coef = 1, and inf is grad_scale = 1
    _run_sgd(fn, b, mode, clip=(part, 4.0 * ref, stats))
    st = dict(zip(STATS, stats.tolist()))
    assert (st['last_coef'], st['clipped'], st['steps']) == (1.0, 1.0, 2.0)
    assert st['norm_sum'] == float(np.float32(st['last_norm']) + np.float32(st['last_norm']))
    _same(_run_sgd(fn, b, mode, clip=(part, float('inf'), None)), _run_sgd(fn, b, mode))


@pytest.mark.parametrize('bad', [float('inf'), float('nan')])
@pytest.mark.parametrize('mode', list(R.SGD_MODES))
def test_sgd_clip_skips_a_nonfinite_norm(fn, mode, bad):
    n = 4104
    b = _sgd_bufs(n, True, seed=1)
    b['g'][n - 3] = bad
    stats = torch.zeros(fn.CLIP_STATS, device=DEV)
    w, mom, wb, bump = _run_sgd(fn, b, mode, clip=(_partials(fn, b['g']), 1.0, stats))
    _same((w, wb), (b['w'], b['wb']))
    if mom is not None:
        assert torch.equal(mom, b['mom'])
    assert int(bump) == 6                            # the step counter still advances
    st = dict(zip(STATS, stats.tolist()))
    assert not math.isfinite(st['last_norm']) and st['last_coef'] == 0.0
    assert (st['norm_sum'], st['norm_max'], st['clipped'], st['skipped'], st['steps']) == (0.0, 0.0, 0.0, 1.0, 1.0)


def _adam_bufs(n, with_wb):
    gen = torch.Generator().manual_seed(200 + n)
    w, g, m = (torch.randn(n, generator=gen).to(DEV) for _ in range(3))
    v = torch.rand(n, generator=gen).to(DEV)
    return dict(w=w, g=g, m=m, v=v, wb=w.bfloat16() if with_wb else None)


def _run_adam(fn, b, betas, decoupled, **kw):
    w, m, v = b['w'].clone(), b['m'].clone(), b['v'].clone()
    wb = None if b['wb'] is None else b['wb'].clone()
    fn.adam_step(w, b['g'], m, v, wb=wb, lr=R.ADAM_HP['lr'], beta1=betas[0], beta2=betas[1], eps=R.ADAM_HP['eps'],
                 weight_decay=R.ADAM_HP['wd'], decoupled=decoupled, step_tensor=_i32(3), **kw)
    torch.cuda.synchronize()
    return w, m, v, wb


@pytest.mark.parametrize('with_wb', [True, False])
@pytest.mark.parametrize('n', [4, 4104])
@pytest.mark.parametrize('betas', [R.ADAM_BETAS[0], R.ADAM_BETAS[-1]])
def test_adam_clip_is_grad_scale_coef(fn, betas, n, with_wb):
    b = _adam_bufs(n, with_wb)
    part = _partials(fn, b['g'])
    ref = float(b['g'].double().norm())
    cap = 0.5 * ref
    for decoupled in (False, True):
        stats = torch.zeros(fn.CLIP_STATS, device=DEV)
        got = _run_adam(fn, b, betas, decoupled, clip=(part, cap, stats))
        st = dict(zip(STATS, stats.tolist()))
        print('adam clip', betas, n, with_wb, decoupled, st)
        assert abs(st['last_norm'] - ref) <= NORM_TOL * ref
        assert st['last_coef'] == _coef32(st['last_norm'], cap) and 0.49 < st['last_coef'] < 0.51
        assert (st['clipped'], st['skipped'], st['steps']) == (1.0, 0.0, 1.0)
        _same(got, _run_adam(fn, b, betas, decoupled, grad_scale=st['last_coef']))
        assert not torch.equal(got[0], b['w'])
        # without a stats block (the later launches of a step that spans several arena segments)
        _same(got, _run_adam(fn, b, betas, decoupled, clip=(part, cap, None)))
        _same(_run_adam(fn, b, betas, decoupled, clip=(part, float('inf'), None)), _run_adam(fn, b, betas, decoupled))


@pytest.mark.parametrize('bad', [float('inf'), float('nan')])
def test_adam_clip_skips_a_nonfinite_norm(fn, bad):
    b = _adam_bufs(4104, True)
    b['g'][7] = bad
    stats = torch.zeros(fn.CLIP_STATS, device=DEV)
    got = _run_adam(fn, b, R.ADAM_BETAS[-1], True, clip=(_partials(fn, b['g']), 1.0, stats))
    _same(got, (b['w'], b['m'], b['v'], b['wb']))
    st = dict(zip(STATS, stats.tolist()))
    assert (st['last_coef'], st['clipped'], st['skipped'], st['steps']) == (0.0, 0.0, 1.0, 1.0)


def test_flat_adam_clips_every_segment_by_the_arena_norm(fn):
    """FlatAdam.step on the GPU over an arena of several segments (decay / no decay, LR multipliers): one reduce,
    every segment's launch scaled by the same coefficient, the stats counted once — against the same optimizer
    stepping pre-scaled gradients."""
    from rafiki_amd.engine.flat import FlatAdam
    fa, fb = R.adam_arena(DEV), R.adam_arena(DEV)
    grads = [g.to(DEV) for g in R.fresh_grads(fa.total, 3, 61)]
    cap = 0.5 * min(float(g.double().norm()) for g in grads)
    oa = FlatAdam(fa, 1e-2, weight_decay=1e-2, clip_norm=cap)
    ob = FlatAdam(fb, 1e-2, weight_decay=1e-2)
    assert len(fa.segments(1e-2)) > 2
    for g in grads:
        fa.grad.copy_(g)
        oa.step()
        coef = float(oa.clip.stats[1])
        for a, b, wd, mult in fb.segments(1e-2):     # the unclipped entry point, grad_scale = coef
            if a == 0:
                fn.add_int_(ob.t, 1)
            fn.adam_step(fb.master[a:b], g[a:b], ob.m[a:b], ob.v[a:b], wb=fb.bf16[a:b], lr=1e-2 * mult,
                         eps=1e-8 * mult, weight_decay=wd, step_tensor=ob.t, grad_scale=coef)
    torch.cuda.synchronize()
    _same((fa.master, oa.m, oa.v, fa.bf16, oa.t), (fb.master, ob.m, ob.v, fb.bf16, ob.t))
    st = oa.clip.read()
    assert (st['clipped'], st['skipped'], st['steps']) == (3, 0, 3)


# ------------------------------------------------------------------------------------------- 3. ConvNetEngine
NB, NSTEPS = 8, 3


def _engine(dtype, optimizer, clip_norm):
    from rafiki_amd.engine.convnet import ConvNetEngine
    return ConvNetEngine(num_classes=10, in_channels=3, image_size=8, cfg=(8, 'M', 8, 'M'), fc_dims=(16,), device=DEV,
                         seed=3, lr=1e-2 if optimizer == 'sgd' else 1e-3, optimizer=optimizer, dtype=dtype,
                         clip_norm=clip_norm)


def _dataset(eng, n):
    g = torch.Generator().manual_seed(1)
    x = torch.zeros(eng.input_shape(n))
    x[..., :3] = torch.randn(n, 8, 8, 3, generator=g)
    y = torch.randint(0, eng.num_classes, (n,), generator=g, dtype=torch.int32)
    return x.to(eng.act_dtype).to(DEV), y.to(DEV)


def _train(eng, how, data, labels):
    """NSTEPS steps over the batches data[k * NB:(k + 1) * NB] -> the master weights."""
    if how == 'capture':
        eng.capture(NB)
        assert eng.clip_norm is None or eng.grad_stats()['steps'] == 0       # the warm-up steps left nothing
    elif how == 'scheduled':
        eng.capture_scheduled(data, labels, NSTEPS, NB)
        assert eng.clip_norm is None or eng.grad_stats()['steps'] == 0
        eng.set_schedule(torch.arange(NSTEPS * NB, device=DEV).view(NSTEPS, NB), epoch=0)
    for k in range(NSTEPS):
        x, y = data[k * NB:(k + 1) * NB], labels[k * NB:(k + 1) * NB]
        if how == 'eager':
            eng.train_step(x, y)
        elif how == 'capture':
            eng.step_graph(x, y)
        else:
            eng.replay()
    torch.cuda.synchronize()
    return eng.flat.master.clone()


@pytest.mark.parametrize('optimizer', ['sgd', 'adam'])
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_convnet_engine_clips_inside_the_step(dtype, optimizer):
    warm = _engine(dtype, optimizer, None)
    data, labels = _dataset(warm, NSTEPS * NB)
    for how in ('eager', 'capture', 'scheduled'):        # the autotuner's sweeps happen here, once per shape
        _train(_engine(dtype, optimizer, None), how, data, labels)
    # the norm the optimizer launch reports is the norm of the arena, and the arena's padding holds nothing
    eng = _engine(dtype, optimizer, float('inf'))
    fl = eng.flat
    eng.forward_backward(data[:NB], labels[:NB])
    eng.opt.step()
    torch.cuda.synchronize()
    st = eng.grad_stats()
    ref = float(fl.grad.double().cpu().norm())
    print('engine', dtype, optimizer, 'last_norm', st['last_norm'], 'arena fp64', ref)
    assert st['steps'] == 1 and ref > 0 and abs(st['last_norm'] - ref) <= NORM_TOL * ref
    real = sum(float(fl.g(n).double().pow(2).sum()) for n in fl.names())
    assert float(fl.grad.double().pow(2).sum()) == pytest.approx(real, rel=1e-12)
    assert int(fl.grad.count_nonzero()) == sum(int(fl.g(n).count_nonzero()) for n in fl.names())
    first_norm = st['last_norm']
    # measuring changes no bit, in any of the three ways to step
    plain = {}
    for how in ('eager', 'capture', 'scheduled'):
        plain[how] = _train(_engine(dtype, optimizer, None), how, data, labels)
        e = _engine(dtype, optimizer, float('inf'))
        assert torch.equal(_train(e, how, data, labels), plain[how]), how
        st = e.grad_stats()
        assert (st['clipped'], st['skipped'], st['steps']) == (0, 0, NSTEPS), how
        assert 0.0 < st['mean_norm'] <= st['max_norm'] < float('inf')
    # a cap at half the first step's norm binds at every step, reproducibly, and changes the weights
    runs = []
    for _ in range(2):
        e = _engine(dtype, optimizer, 0.5 * first_norm)
        runs.append(_train(e, 'scheduled', data, labels))
        st = e.grad_stats()
        print('engine', dtype, optimizer, 'clipped run', st)
        assert st['clipped'] == st['steps'] == NSTEPS and st['skipped'] == 0
    assert torch.equal(runs[0], runs[1])
    assert not torch.equal(runs[0], plain['scheduled'])
    e.reset_metrics()
    assert e.grad_stats()['steps'] == 0


# ------------------------------------------------------------------------------------------- 4. TaggerEngine
class Net(torch.nn.Module):
    def __init__(self, V, E, H, NT):
        super().__init__()
        self.emb = torch.nn.Embedding(V, E, padding_idx=0)
        self.drop = torch.nn.Dropout(0.0)
        self.lstm = torch.nn.LSTM(E, H, batch_first=True, bidirectional=True)
        self.out = torch.nn.Linear(2 * H, NT)

    def loss(self, x, y):
        logits = self.out(self.lstm(self.emb(torch.from_numpy(x)))[0])
        return torch.nn.functional.cross_entropy(logits.reshape(-1, logits.shape[-1]), torch.from_numpy(y).reshape(-1),
                                                 ignore_index=-100)


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def test_tagger_engine_clips_like_clip_grad_norm():
    """Three clipped Adam steps of the native tagger against the fp64 module stepped by clip_grad_norm_ +
    torch.optim.Adam, with the bounds of tests/test_tagger_gpu.py::test_tagger_adam_update_matches_fp64 (moments
    1e-6 relative, weights 1e-6 absolute); and the replayed graph against eager steps, bit for bit."""
    from rafiki_amd.engine.tagger import TaggerEngine
    torch.manual_seed(5)
    V, E, H, NT, B, L = 11, 5, 3, 4, 2, 3
    lr, betas, eps = 0.02, (0.9, 0.999), 1e-8
    net = Net(V, E, H, NT).to(DEV)
    ref = Net(V, E, H, NT).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in net.state_dict().items()})
    rng = np.random.default_rng(6)
    batches = []
    for _ in range(3):
        x = rng.integers(1, V, (B, L))
        y = rng.integers(0, NT, (B, L))
        x[1, L - 1], y[1, L - 1] = 0, -100             # one padding token
        batches.append((x.astype(np.int64), y.astype(np.int64)))
    ref.loss(*batches[0]).backward()
    first = math.sqrt(sum(float(p.grad.pow(2).sum()) for p in ref.parameters()))
    ref.zero_grad()
    cap = 0.5 * first
    eager = TaggerEngine(net, lr=lr, dropout=0.0, betas=betas, eps=eps, clip_norm=cap)
    graph = TaggerEngine(net, lr=lr, dropout=0.0, betas=betas, eps=eps, clip_norm=cap)
    opt = torch.optim.Adam(ref.parameters(), lr=lr, betas=betas, eps=eps)
    for t, (x, y) in enumerate(batches, 1):
        opt.zero_grad()
        ref.loss(x, y).backward()
        norm = float(torch.nn.utils.clip_grad_norm_(ref.parameters(), cap))
        opt.step()
        eager.step(x, y, graph=False)
        graph.step(x, y, graph=True)
        torch.cuda.synchronize()
        st = eager.grad_stats()
        arena = float(eager.g.double().cpu().norm())
        print('tagger step', t, 'norm', st['last_norm'], 'arena fp64', arena, 'module fp64', norm)
        assert abs(st['last_norm'] - arena) <= NORM_TOL * arena
        assert st['last_norm'] == pytest.approx(norm, rel=1e-5)       # the padded rows hold no gradient
        assert int(eager.g.count_nonzero()) == sum(int(v.count_nonzero()) for v in eager.grads().values())
        assert (st['clipped'], st['skipped'], st['steps']) == (t, 0, t)
        w, m, v = eager._unpad(eager.w), eager._unpad(eager.m), eager._unpad(eager.v)
        for k, p in ref.named_parameters():
            ew = float((w[k].double().cpu() - p.detach()).abs().max())
            em, ev = _rel(m[k].cpu(), opt.state[p]['exp_avg']), _rel(v[k].cpu(), opt.state[p]['exp_avg_sq'])
            print('  {:28s} w abs {:.3e}  m rel {:.3e}  v rel {:.3e}'.format(k, ew, em, ev))
            assert ew < 1e-6 and em < 1e-6 and ev < 1e-6, (t, k, ew, em, ev)
    assert len(graph._graphs) == 1
    assert torch.equal(eager.w, graph.w) and torch.equal(eager.m, graph.m) and torch.equal(eager.v, graph.v)
    assert torch.equal(eager.clip.stats, graph.clip.stats)
    eager.take_loss()
    assert eager.grad_stats()['steps'] == 0
    graph.close()
