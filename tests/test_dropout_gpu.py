"""Dropout on the GPU: the kernel rk_dropout against the oracles of tests/dropout_refs.py (bit-exact), its replay
inside a captured graph, the fp32 and bf16 engines' dropped steps against autograd through the reference loss with
the oracle's multipliers, the scheduled graph's step identity, and the model loops."""
import functools

import numpy as np
import pytest
import torch

import dropout_refs as DR

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SITE = DR.DROP_STREAM
SIZES = (4, 8, 1032, 4 * 1024 + 8, 256 * 2048)     # one vector, two, a ragged block, blocks + a tail, the features
RATES = (0.1, 0.5, 0.9)
STEP, EPOCH = 5, 3


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@functools.lru_cache(maxsize=None)
def _input(n, bf16):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g)
    return x.bfloat16() if bf16 else x


def _word(v):
    return torch.tensor([v], dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize('pointers', [False, True], ids=['null', 'words'])
@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
def test_kernel_matches_the_oracle(bf16, pointers):
    from rafiki_amd.ops import f32 as S
    from rafiki_amd.ops import functional as F
    assert S.dropout_ is F.dropout_
    step, epoch = (_word(STEP), _word(EPOCH)) if pointers else (None, None)
    for n in SIZES:
        if bf16 and n == 4:
            continue                # half a bf16 vector: refused (test_refusals)
        for p in RATES:
            x = _input(n, bf16)
            got = F.dropout_(x.to(DEV), p, seed=DR.SEED, site=SITE, step=step, epoch=epoch)
            want = DR.dropped(x, DR.SEED, SITE, EPOCH if pointers else 0, STEP if pointers else 0, p)
            assert torch.equal(_bits(got), _bits(want)), (n, p)
    # the site and the seed's high word reach the counter and the key
    x = _input(1032, bf16)
    for seed, site in ((DR.SEED, SITE + 1), (DR.SEED + (1 << 32), SITE), (DR.SEED + 1, SITE)):
        got = F.dropout_(x.to(DEV), 0.5, seed=seed, site=site, step=step, epoch=epoch)
        want = DR.dropped(x, seed, site, EPOCH if pointers else 0, STEP if pointers else 0, 0.5)
        assert torch.equal(_bits(got), _bits(want)), (seed, site)
        assert not torch.equal(_bits(got), _bits(DR.dropped(x, DR.SEED, SITE, EPOCH if pointers else 0,
                                                            STEP if pointers else 0, 0.5)))


@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
def test_dropped_nonfinite_values_become_zero(bf16):
    from rafiki_amd.ops import functional as F
    n = 1032
    keep = DR.keep(DR.SEED, SITE, 0, 0, n, 0.5)
    x = _input(n, bf16).clone()
    vals = [float('inf'), float('nan'), float('-inf')]
    for i in range(n):
        x[i] = vals[i % 3] if i % 2 else x[i]      # every odd element, kept or dropped
    got = F.dropout_(x.to(DEV), 0.5, seed=DR.SEED, site=SITE).cpu()
    k = torch.from_numpy(keep)
    odd = torch.arange(n) % 2 == 1
    assert int((~k & odd).sum()) > 100 and int((k & odd).sum()) > 100
    assert torch.equal(_bits(got[~k]), _bits(torch.zeros(int((~k).sum()), dtype=x.dtype)))
    kept = got[k & odd].float()
    src = x[k & odd].float()
    assert torch.equal(torch.isnan(kept), torch.isnan(src)) and torch.equal(torch.isinf(kept), torch.isinf(src))
    assert torch.equal(torch.nan_to_num(kept, 0.0), torch.nan_to_num(src, 0.0))     # inf * 2 keeps its sign


@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
def test_a_middle_slice_leaves_its_neighbours_alone(bf16):
    from rafiki_amd.ops import functional as F
    x = _input(4 * 1024 + 8, bf16)
    buf = x.to(DEV)
    lo, n = 1024, 1032
    F.dropout_(buf[lo:lo + n], 0.5, seed=DR.SEED, site=SITE, step=_word(STEP), epoch=_word(EPOCH))
    got = buf.cpu()
    assert torch.equal(_bits(got[:lo]), _bits(x[:lo])) and torch.equal(_bits(got[lo + n:]), _bits(x[lo + n:]))
    assert torch.equal(_bits(got[lo:lo + n]), _bits(DR.dropped(x[lo:lo + n], DR.SEED, SITE, EPOCH, STEP, 0.5)))


def test_refusals_leave_the_buffer_untouched():
    from rafiki_amd.ops import _lib
    from rafiki_amd.ops import functional as F
    for bf16 in (False, True):
        x = _input(1032, bf16)
        buf = x.to(DEV)
        for p in (1.0, -0.1, 1.5, float('nan'), float('inf'), float('-inf')):
            with pytest.raises(_lib.KernelError):
                F.dropout_(buf, p, seed=DR.SEED, site=SITE)
        with pytest.raises(_lib.KernelError):         # not a whole number of 16-byte vectors
            F.dropout_(buf[:1032 - (4 if bf16 else 2)], 0.5, seed=DR.SEED, site=SITE)
        with pytest.raises(_lib.KernelError):         # a whole number of vectors, but not 16-byte aligned
            F.dropout_(buf[2:2 + 1024], 0.5, seed=DR.SEED, site=SITE)
        with pytest.raises(ValueError):
            F.dropout_(buf.view(-1, 2)[:, 0], 0.5, seed=DR.SEED, site=SITE)
        with pytest.raises(ValueError):
            F.dropout_(buf, 0.5, seed=DR.SEED, site=SITE, step=torch.zeros(1, dtype=torch.int64, device=DEV))
        with pytest.raises(ValueError):
            F.dropout_(buf, 0.5, seed=DR.SEED, site=SITE, epoch=torch.zeros(1, dtype=torch.int32))
        # n / 4 >= 2^32: the quad index would not fit its counter word.  The launcher refuses before any launch
        stream = torch.cuda.current_stream().cuda_stream
        assert _lib.lib().rk_dropout(buf.data_ptr(), 1 << 34, int(bf16), 0.5, DR.SEED, SITE, None, None, stream) == -1
        assert _lib.lib().rk_dropout(buf.data_ptr(), -8, int(bf16), 0.5, DR.SEED, SITE, None, None, stream) == -1
        assert _lib.lib().rk_dropout(None, 0, int(bf16), 0.5, DR.SEED, SITE, None, None, stream) == 0
        F.dropout_(buf[:0], 0.5, seed=DR.SEED, site=SITE)
        torch.cuda.synchronize()
        assert torch.equal(_bits(buf), _bits(x))
    with pytest.raises(ValueError):
        F.dropout_(torch.zeros(8, dtype=torch.float16, device=DEV), 0.5, seed=1, site=SITE)
    with pytest.raises(ValueError):
        F.dropout_(torch.zeros(8), 0.5, seed=1, site=SITE)


def test_a_replayed_graph_draws_for_the_words_at_replay_time():
    from rafiki_amd.ops import functional as F
    from rafiki_amd.ops.graphs import capture
    n = 1032
    x = _input(n, False)
    src, buf, step, epoch = x.to(DEV), torch.zeros(n, device=DEV), _word(0), _word(EPOCH)

    # the graph holds the one launch and nothing else (no copy node): the buffer is refilled before each replay,
    # on the stream the replay follows
    def launch():
        F.dropout_(buf, 0.5, seed=DR.SEED, site=SITE, step=step, epoch=epoch)
    launch()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with capture(g):
        launch()
    torch.cuda.synchronize()
    outs = []
    for st in (0, 1, 0):
        step.fill_(st)
        buf.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        outs.append(buf.cpu())
        assert torch.equal(_bits(outs[-1]), _bits(DR.dropped(x, DR.SEED, SITE, EPOCH, st, 0.5))), st
    assert torch.equal(_bits(outs[0]), _bits(outs[2])) and not torch.equal(_bits(outs[0]), _bits(outs[1]))
    epoch.fill_(EPOCH + 1)
    buf.copy_(src)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf.cpu()), _bits(DR.dropped(x, DR.SEED, SITE, EPOCH + 1, 0, 0.5)))


# ------------------------------------------------------------------------------------------- the engines
B, P, FP = 64, 0.5, 0.25


def _engine(**kw):
    from rafiki_amd.engine.convnet import ConvNetEngine
    args = dict(num_classes=10, in_channels=3, image_size=16, cfg=(16, 'M', 32, 32, 'M'), fc_dims=(32,),
                device=DEV, seed=3, lr=0.05, dtype='fp32')
    keep = kw.pop('keep_dropped', False)
    args.update(kw)
    eng = ConvNetEngine(**args)
    eng.keep_dropped = keep       # the debug hook: the forward keeps the tensors it dropped in eng._dropped
    return eng


def _batch(eng, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(eng.input_shape(n))
    x[..., :3] = torch.randn(n, 16, 16, 3, generator=g)
    y = torch.randint(0, eng.num_classes, (n,), generator=g, dtype=torch.int32)
    return x.to(eng.act_dtype).to(DEV), y.to(DEV)


def _mults(eng, epoch, step, n=B, dtype=torch.float64):
    return DR.engine_multipliers(3, epoch, step, n, eng.feat_dim, [f[2] for f in eng.fcs], eng.dropout,
                                 eng.feature_dropout, dtype)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _check_grads(eng, grads, loss, tag):
    """The bound of tests/test_engine_gpu.py::test_grads_match_reference."""
    n = int(eng.seen.item())
    print(tag, 'loss', eng.loss_sum.item() / n, loss.item())
    assert abs(eng.loss_sum.item() / n - loss.item()) < 1e-2 * max(1.0, loss.item())
    for name, g in zip(eng.flat.names(), grads):
        got = eng.flat.g(name).double().cpu()
        g = g.double().cpu()
        fro = ((got - g).norm() / g.norm().clamp_min(1e-12)).item()
        cos = torch.nn.functional.cosine_similarity(got.flatten(), g.flatten(), 0).item()
        print(tag, name, round(fro, 6), round(cos, 6))
        assert fro < 0.12 and cos > 0.99, (name, fro, cos)


def _ref64(eng, x, y, drop):
    fl = eng.flat
    params = {n: fl.w(n).detach().double().cpu().clone().requires_grad_(True) for n in fl.names()}
    loss, _ = eng.reference_loss(x.double().cpu(), y.cpu(), params, training=True, drop=drop)
    return loss, torch.autograd.grad(loss, [params[n] for n in fl.names()])


@pytest.mark.parametrize('classes', [10, 40], ids=['fused-head', 'unfused-head'])
def test_fp32_engine_grads_match_fp64_autograd(classes):
    from rafiki_amd.ops import f32 as S
    eng = _engine(num_classes=classes, dropout=P, feature_dropout=FP, keep_dropped=True)
    assert (eng.fused_head and S.head_ok(eng.ncls_p, eng.d_last)) == (classes == 10)
    x, _ = _batch(eng, B)
    # Inputs chosen so that every parameter's gradient depends on the masks.  With random labels at initialisation
    # the output bias gradient, mean_b(softmax_b - onehot_b), is dominated by the label histogram, which no mask
    # touches (on the CPU it moved by only 0.16 - 0.34 under another step's masks).  So the output weights are four
    # times their initial scale (the predictions then depend on which units survive) and the labels are what the
    # fp64 oracle predicts under the right masks: the right gradient is the small residual of a net that fits its
    # labels, and any other masks change the predictions themselves (on the CPU: >= 1.7 for every parameter)
    eng.flat.w('out.w').mul_(4.0)
    params = {n: eng.flat.w(n).detach().double().cpu() for n in eng.flat.names()}
    _, logits = eng.reference_loss(x.double().cpu(), None, params, training=True, drop=_mults(eng, 2, 5))
    y = logits.argmax(1).to(torch.int32).to(DEV)
    eng.set_step(2, 5)
    eng.forward_backward(x, y)
    torch.cuda.synchronize()
    loss, grads = _ref64(eng, x, y, _mults(eng, 2, 5))
    _check_grads(eng, grads, loss, 'f32-drop-{}'.format(classes))
    # the check is not vacuous: the gradient without dropout, and the one of another step's multipliers, each lie
    # three bounds away from the right one, for every parameter
    for tag, drop in (('none', None), ('other-step', _mults(eng, 2, 6)), ('other-epoch', _mults(eng, 3, 5))):
        _, wrong = _ref64(eng, x, y, drop)
        for name, g, w in zip(eng.flat.names(), grads, wrong):
            d = _rel(w, g)
            print('sensitivity', tag, name, round(d, 4))
            assert d >= 0.36, (tag, name, d)
    # the forward left the oracle's zero pattern in the dropped tensors
    for site, t in eng._dropped.items():
        keep = torch.from_numpy(DR.keep(3, site, 2, 5, t.numel(), P if site > SITE else FP)).reshape(t.shape)
        assert (t.cpu()[~keep] == 0).all() and (t.cpu()[keep] != 0).float().mean() > 0.2, site
    assert set(eng._dropped) == {SITE, SITE + 1}


@pytest.mark.parametrize('classes', [10, 40], ids=['fused-head', 'unfused-head'])
def test_fp32_engine_without_a_hidden_layer(classes):
    """No FC layer: feature dropout acts on the output layer's input, and the gradient that arrives at it is the
    head's ungated dz (fused head) or the output layer's linear_dx."""
    eng = _engine(num_classes=classes, fc_dims=(), dropout=P, feature_dropout=FP)
    x, y = _batch(eng, B)
    eng.set_step(1, 2)
    eng.forward_backward(x, y)
    torch.cuda.synchronize()
    drop = _mults(eng, 1, 2)
    assert set(drop) == {SITE}
    loss, grads = _ref64(eng, x, y, drop)
    _check_grads(eng, grads, loss, 'f32-drop-nofc-{}'.format(classes))


def test_bf16_engine_grads_match_the_emulating_oracle():
    eng = _engine(dtype='bf16', dropout=P, feature_dropout=FP, keep_dropped=True)
    x, y = _batch(eng, B)
    eng.set_step(2, 5)
    eng.forward_backward(x, y)
    torch.cuda.synchronize()
    fl = eng.flat
    params = {n: fl.w(n).detach().clone().requires_grad_(True) for n in fl.names()}
    loss, _ = eng.reference_loss(x, y, params, training=True, emulate_bf16=True,
                                 drop=_mults(eng, 2, 5, dtype=torch.float32))
    grads = torch.autograd.grad(loss, [params[n] for n in fl.names()])
    _check_grads(eng, grads, loss, 'bf16-drop')
    for site, t in eng._dropped.items():
        keep = torch.from_numpy(DR.keep(3, site, 2, 5, t.numel(), P if site > SITE else FP)).reshape(t.shape)
        assert (t.cpu()[~keep] == 0).all() and (t.cpu()[keep] != 0).float().mean() > 0.2, site


def _dataset(eng, n, seed=1):
    return _batch(eng, n, seed=seed)


def _follows(t, keep):
    """The dropped tensor ``t`` is zero wherever ``keep`` is false."""
    return bool((t.cpu().reshape(-1)[~torch.from_numpy(keep)] == 0).all())


def test_scheduled_graph_draws_per_epoch_and_step():
    eng = _engine(dropout=P, feature_dropout=FP, lr=1e-3, keep_dropped=True)      # a small step: the ReLU layers stay about half on
    n, steps = 32, 3
    data, labels = _dataset(eng, 96)
    eng.capture_scheduled(data, labels, steps, n)
    g = torch.Generator(device=DEV).manual_seed(4)
    masks = {}
    for epoch in (0, 1):
        eng.set_schedule(torch.randperm(96, device=DEV, generator=g).view(steps, n), epoch=epoch)
        for s in range(steps):
            eng.replay()
            torch.cuda.synchronize()
            assert int(eng._ctr.item()) == s + 1
            for site, rate in ((SITE, FP), (SITE + 1, P)):
                t = eng._dropped[site]
                keep = masks[(site, epoch, s)] = DR.keep(3, site, epoch, s, t.numel(), rate)
                assert _follows(t, keep), (site, epoch, s)
                kept = t.cpu().reshape(-1)[torch.from_numpy(keep)]
                # not vacuous: survivors are there, enough of them for the cross-check below to bite (a ReLU
                # layer leaves about half; 1 in 20 of >= 1024 elements is already dozens per foreign mask)
                assert (kept != 0).float().mean() > 0.05, (site, epoch, s)
    assert int(eng._ctr.item()) == 3
    assert torch.isfinite(eng.flat.master).all()
    # the last replay (epoch 1, step 2) follows no other (epoch, step)'s mask, the one of epoch 0 included
    for (site, epoch, s), keep in masks.items():
        if (epoch, s) != (1, 2):
            assert not _follows(eng._dropped[site], keep), (site, epoch, s)
    for site in (SITE, SITE + 1):
        assert not np.array_equal(masks[(site, 0, 0)], masks[(site, 1, 0)])


def test_scheduled_graph_needs_the_sgd_counter():
    eng = _engine(dropout=P, optimizer='adam', lr=1e-3)
    data, labels = _dataset(eng, 64)
    with pytest.raises(NotImplementedError):
        eng.capture_scheduled(data, labels, 2, 32)


def test_zero_rates_are_todays_step(monkeypatch):
    """Rates of 0: the same launches as an engine built without the arguments, and after three replays the same
    master weights, bit for bit.  Non-zero rates add four dropout launches (two forward, two backward)."""
    from rafiki_amd.ops import _lib
    calls, call = [], _lib.call

    def counting(name, *args):
        calls.append(name)
        return call(name, *args)
    monkeypatch.setattr(_lib, 'call', counting)
    n, steps = 32, 3
    warm = _engine()
    data, labels = _dataset(warm, 96)
    warm.capture_scheduled(data, labels, steps, n)         # the autotuner's sweeps happen here, once per shape
    warm.set_schedule(torch.arange(96, device=DEV).view(steps, n))
    warm.replay()
    torch.cuda.synchronize()
    del warm
    masters, launches = [], []
    for kw in ({}, dict(dropout=0.0, feature_dropout=0.0), dict(dropout=P, feature_dropout=FP)):
        eng = _engine(**kw)
        del calls[:]
        eng.capture_scheduled(data, labels, steps, n)      # two warm-up steps and the captured one
        launches.append(list(calls))
        eng.set_schedule(torch.arange(96, device=DEV).view(steps, n), epoch=0)
        for _ in range(steps):
            eng.replay()
        torch.cuda.synchronize()
        masters.append(eng.flat.master.clone())
        assert (eng._drop_step is None) == (not kw.get('dropout'))     # a rate of 0 adds no buffer
        assert not eng._dropped                                        # and the hook is off unless asked for
    assert 'rk_dropout' not in launches[0] and launches[0] == launches[1]
    assert [c for c in launches[2] if c != 'rk_dropout'] == launches[0]
    assert launches[2].count('rk_dropout') == 3 * 4
    assert torch.equal(masters[0], masters[1])
    assert not torch.equal(masters[0], masters[2])


# ------------------------------------------------------------------------------------------- the models
@pytest.mark.parametrize('optimizer', ['sgd', 'adam'])
def test_model_loops_drop_per_epoch_and_step(optimizer, monkeypatch):
    """NativeImageClassifier.train on the GPU, two epochs: the scheduled graph (SGD, its own counter and
    set_schedule's epoch) and the captured step fed by set_step (Adam) both drop with the multipliers of each
    (epoch, step); evaluate takes no training step and launches no dropout."""
    from rafiki_amd.engine.convnet import ConvNetEngine
    from rafiki_amd.models.image_classifier import NativeImageClassifier
    from rafiki_amd.ops import _lib
    from rafiki_amd.ops.graphs import device_sync
    from rafiki_amd.parallel.context import TrialContext, use_context

    class Tiny(NativeImageClassifier):
        DEFAULT_IMAGE_SIZE = 16

        def _engine_kwargs(self, num_classes, channels, image_size):
            return dict(cfg=(16, 'M', 32, 32, 'M'), fc_dims=(32,), optimizer=optimizer, lr=1e-3, weight_decay=0.0)

    seen, set_steps, calls = [], [], []
    replay, step_graph, set_step, call = ConvNetEngine.replay, ConvNetEngine.step_graph, ConvNetEngine.set_step, _lib.call

    def snapshot(self):
        device_sync(self.device)
        seen.append({site: t.clone() for site, t in self._dropped.items()})

    def rec_replay(self):
        replay(self)
        snapshot(self)

    def rec_step_graph(self, x, labels):
        step_graph(self, x, labels)
        snapshot(self)

    def rec_set_step(self, epoch, step):
        set_steps.append((epoch, step))
        return set_step(self, epoch, step)

    def counting(name, *args):
        calls.append(name)
        return call(name, *args)
    monkeypatch.setattr(ConvNetEngine, 'replay', rec_replay)
    monkeypatch.setattr(ConvNetEngine, 'step_graph', rec_step_graph)
    monkeypatch.setattr(ConvNetEngine, 'set_step', rec_set_step)
    monkeypatch.setattr(ConvNetEngine, 'keep_dropped', True)      # the debug hook, for the engine train() builds
    uri = 'synthetic://image?n=128&size=16&channels=3&classes=10&seed=0'
    with use_context(TrialContext(device=torch.device(DEV))):
        m = Tiny(epochs=2, batch_size=32, image_size=16, dropout=P, feature_dropout=FP, seed=9)
        m.train(uri)
        eng = m._engine
        assert (eng._sched_graph if optimizer == 'sgd' else eng._graph) is not None
        assert eng.dropout == P and eng.feature_dropout == FP
        assert len(seen) == 8
        order = [(e, b) for e in (0, 1) for b in range(4)]
        assert set_steps == ([] if optimizer == 'sgd' else order)
        for i, (epoch, b) in enumerate(order):
            assert set(seen[i]) == {SITE, SITE + 1}
            for site, rate in ((SITE, FP), (SITE + 1, P)):
                t = seen[i][site]
                assert _follows(t, DR.keep(9, site, epoch, b, t.numel(), rate)), (site, epoch, b)
                for (e2, b2) in order:
                    if (e2, b2) != (epoch, b):
                        assert not _follows(t, DR.keep(9, site, e2, b2, t.numel(), rate)), (site, epoch, b, e2, b2)
        monkeypatch.setattr(_lib, 'call', counting)
        assert isinstance(m.evaluate(uri), float)
        assert len(seen) == 8 and calls and 'rk_dropout' not in calls
        monkeypatch.setattr(_lib, 'call', call)
        m.destroy()
