"""Dropout on the CPU: the host twin (rafiki_amd/ops/dropout.py) against the oracles of tests/dropout_refs.py, the
CPU engine's dropped step against autograd through its reference loss, the argument and knob checks, and a
VggSmallDrop trial with a crash and a resume."""
import math
import pickle

import numpy as np
import pytest
import torch

import dropout_refs as DR

from rafiki_amd.ops import dropout as D

SEEDS = (DR.SEED, (7 << 32) + 3)
SITES = (DR.DROP_STREAM, DR.DROP_STREAM + 1)


# ------------------------------------------------------------------------------------------- the twin
def test_constants():
    assert D.DROP_STREAM == DR.DROP_STREAM == 0x6472
    for p in (0.1, 0.25, 0.5, 0.9):
        assert D.inv_keep(p) == DR.inv_keep(p)


@pytest.mark.parametrize('n', [4, 8, 1028])
@pytest.mark.parametrize('seed', SEEDS)
def test_keep_matches_the_oracle(seed, n):
    for site in SITES:
        for step in (0, 5):
            for epoch in (0, 5):
                got = D.keep(seed, site, epoch, step, n, 0.5)
                assert got.dtype == np.bool_ and got.shape == (n,)
                assert np.array_equal(got, DR.keep(seed, site, epoch, step, n, 0.5)), (site, step, epoch)


def test_site_step_epoch_and_seed_each_change_the_mask():
    base = D.keep(DR.SEED, DR.DROP_STREAM, 3, 7, 1028, 0.5)
    assert np.array_equal(base, D.keep(DR.SEED, DR.DROP_STREAM, 3, 7, 1028, 0.5))
    others = [D.keep(DR.SEED, DR.DROP_STREAM + 1, 3, 7, 1028, 0.5), D.keep(DR.SEED, DR.DROP_STREAM, 4, 7, 1028, 0.5),
              D.keep(DR.SEED, DR.DROP_STREAM, 3, 8, 1028, 0.5), D.keep(DR.SEED + 1, DR.DROP_STREAM, 3, 7, 1028, 0.5),
              D.keep(DR.SEED + (1 << 32), DR.DROP_STREAM, 3, 7, 1028, 0.5),
              D.keep(DR.SEED, DR.DROP_STREAM, 7, 3, 1028, 0.5)]       # (epoch, step) swapped
    for o in others:
        # two independent fair masks of 1028 elements agree on about half: 514 +- 16; far from all
        assert 400 < int((o == base).sum()) < 628
    # a shorter tensor is a prefix of a longer one (the draw of element i does not depend on n)
    assert np.array_equal(D.keep(DR.SEED, DR.DROP_STREAM, 3, 7, 10, 0.5), base[:10])


@pytest.mark.parametrize('p', [0.1, 0.5, 0.9])
def test_keep_rate(p):
    n = 65536
    k = D.keep(DR.SEED, 0x6472, 3, 7, n, p)
    dev = abs(int(k.sum()) / n - (1.0 - p))
    print('keep-rate deviation', p, round(dev, 5), 'bound', round(4 * math.sqrt(p * (1 - p) / n), 5))
    assert dev <= 4.0 * math.sqrt(p * (1.0 - p) / n)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float64])
def test_apply_selects_and_scales(dtype):
    g = torch.Generator().manual_seed(1)
    t = torch.randn(6, 36, generator=g).to(dtype)
    t[0, 0], t[0, 1], t[0, 2], t[0, 3] = float('inf'), float('nan'), float('-inf'), float('nan')
    keep = DR.keep(DR.SEED, DR.DROP_STREAM, 2, 9, t.numel(), 0.5).reshape(6, 36)
    assert not keep[0, :4].all()       # at least one of the non-finite values is dropped: it must come out as 0
    before = t.clone()
    out = D.apply(t, DR.SEED, DR.DROP_STREAM, 2, 9, 0.5)
    assert torch.equal(torch.nan_to_num(t, 1.0, 2.0, 3.0), torch.nan_to_num(before, 1.0, 2.0, 3.0))   # not in place
    assert out.dtype == dtype and out.shape == t.shape
    kt = torch.from_numpy(keep)
    assert (out[~kt] == 0).all()                                    # a dropped inf / NaN is a zero
    if dtype == torch.float64:
        want = t * DR.inv_keep(0.5)
    else:
        want = DR.dropped(t, DR.SEED, DR.DROP_STREAM, 2, 9, 0.5)
    assert torch.equal(torch.nan_to_num(out[kt], 1.0, 2.0, 3.0), torch.nan_to_num(want[kt], 1.0, 2.0, 3.0))
    m = D.multipliers(DR.SEED, DR.DROP_STREAM, 2, 9, (6, 36), 0.5)
    assert torch.equal(m, DR.multipliers(DR.SEED, DR.DROP_STREAM, 2, 9, (6, 36), 0.5, torch.float32))


# ------------------------------------------------------------------------------------------- the CPU engine
def _engine(**kw):
    from rafiki_amd.engine.convnet import ConvNetEngine
    args = dict(num_classes=10, in_channels=3, image_size=16, cfg=(16, 'M', 32, 32, 'M'), fc_dims=(32,),
                device='cpu', seed=3, lr=0.05, dtype='fp32')
    args.update(kw)
    return ConvNetEngine(**args)


def _batch(eng, B, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(eng.input_shape(B))
    x[..., :3] = torch.randn(B, 16, 16, 3, generator=g)
    return x, torch.randint(0, 10, (B,), generator=g, dtype=torch.int32)


def _flat_grads(eng):
    return torch.cat([eng.flat.g(n).flatten() for n in eng.flat.names()]).clone()


def _autograd(eng, x, y, drop):
    fl = eng.flat
    params = {n: fl.w(n).detach().clone().requires_grad_(True) for n in fl.names()}
    loss, _ = eng.reference_loss(x, y, params, training=True, drop=drop)
    return torch.cat([g.flatten() for g in torch.autograd.grad(loss, [params[n] for n in fl.names()])])


def test_zero_rates_are_the_plain_engine():
    plain, zero = _engine(), _engine(dropout=0.0, feature_dropout=0.0)
    x, y = _batch(plain, 16)
    zero.set_step(2, 5)
    plain.forward_backward(x, y)
    zero.forward_backward(x, y)
    assert torch.equal(_flat_grads(plain), _flat_grads(zero))
    assert torch.equal(plain.loss_sum, zero.loss_sum)
    # reference_loss without the argument, with None and with an empty table: one result
    a = plain.reference_loss(x, y)[0]
    assert torch.equal(a, plain.reference_loss(x, y, drop=None)[0]) and torch.equal(a, plain.reference_loss(x, y, drop={})[0])


def test_cpu_engine_drops_with_the_step_multipliers():
    B = 16
    eng = _engine(dropout=0.5, feature_dropout=0.25)
    assert eng.feat_dim == 512 and [f[2] for f in eng.fcs] == [32]
    x, y = _batch(eng, B)
    grads = {}
    for at in ((0, 0), (0, 1), (1, 0)):
        eng.set_step(*at)
        eng.forward_backward(x, y)
        grads[at] = _flat_grads(eng)
        drop = DR.engine_multipliers(3, at[0], at[1], B, 512, [32], 0.5, 0.25, torch.float32)
        assert set(drop) == {DR.DROP_STREAM, DR.DROP_STREAM + 1}
        want = _autograd(eng, x, y, drop)
        assert torch.allclose(grads[at], want, rtol=1e-5, atol=1e-8), at
    rel = lambda a, b: ((a - b).norm() / b.norm()).item()
    assert rel(grads[(0, 1)], grads[(0, 0)]) > 0.3 and rel(grads[(1, 0)], grads[(0, 0)]) > 0.3
    assert rel(grads[(1, 0)], grads[(0, 1)]) > 0.3
    assert rel(_autograd(eng, x, y, None), grads[(0, 0)]) > 0.3      # and none of them is the undropped gradient
    # only the dropout rate of a kind that is on contributes its sites
    half = _engine(dropout=0.5)
    half.set_step(0, 1)
    half.forward_backward(x, y)
    want = _autograd(half, x, y, DR.engine_multipliers(3, 0, 1, B, 512, [32], 0.5, 0.0, torch.float32))
    assert torch.allclose(_flat_grads(half), want, rtol=1e-5, atol=1e-8)
    # evaluation never drops: the same weights in an engine without dropout give the same probabilities
    plain = _engine()
    plain.load_state_dict(eng.state_dict())
    assert torch.equal(eng.forward_eval(x), plain.forward_eval(x))
    assert set(eng.state_dict()) == set(plain.state_dict())


def test_no_fc_layer_drops_the_features_only():
    eng = _engine(fc_dims=(), dropout=0.5, feature_dropout=0.25)     # dropout has no hidden layer to act on
    x, y = _batch(eng, 8)
    eng.set_step(4, 2)
    eng.forward_backward(x, y)
    drop = DR.engine_multipliers(3, 4, 2, 8, 512, [], 0.5, 0.25, torch.float32)
    assert set(drop) == {DR.DROP_STREAM}
    assert torch.allclose(_flat_grads(eng), _autograd(eng, x, y, drop), rtol=1e-5, atol=1e-8)


def test_argument_checks():
    for bad in (1.0, -0.1, 1.5, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            _engine(dropout=bad)
        with pytest.raises(ValueError):
            _engine(feature_dropout=bad)
    with pytest.raises(ValueError):      # a flat-input net's features are the caller's input buffer
        _engine(cfg=(), image_size=8, in_channels=1, feature_dropout=0.2)
    flat = _engine(cfg=(), image_size=8, in_channels=1, dropout=0.2)
    assert flat.dropout == 0.2 and flat.feature_dropout == 0.0


# ------------------------------------------------------------------------------------------- the models
TRAIN = 'synthetic://image?n=128&size=16&channels=3&classes=10&seed=0'


def _cpu(**kw):
    from rafiki_amd.parallel.context import TrialContext, use_context
    return use_context(TrialContext(device=torch.device('cpu'), **kw))


def test_knobs():
    from rafiki_amd.model import FloatKnob
    from rafiki_amd.models import ZOO
    from rafiki_amd.models.feed_forward import FeedForward
    from rafiki_amd.models.vgg16 import Vgg16
    from rafiki_amd.models.vgg_small import (VggSmall, VggSmallAug, VggSmallDrop, VggSmallProbe, VggSmallReg,
                                             VggSmallTrial)
    assert ZOO['VggSmallDrop'] == ('vgg_small.py', 'IMAGE_CLASSIFICATION')
    k = VggSmallDrop.get_knob_config()
    assert set(k) == set(VggSmallReg.get_knob_config()) | {'dropout', 'feature_dropout'}
    assert isinstance(k['dropout'], FloatKnob) and isinstance(k['feature_dropout'], FloatKnob)
    assert (k['dropout'].value_min, k['dropout'].value_max) == (0.0, 0.5)
    assert (k['feature_dropout'].value_min, k['feature_dropout'].value_max) == (0.0, 0.3)
    for cls in (VggSmall, VggSmallAug, VggSmallReg, VggSmallTrial, VggSmallProbe, Vgg16, FeedForward):
        assert not {'dropout', 'feature_dropout'} & set(cls.get_knob_config()), cls
    with _cpu():
        assert VggSmall()._regularisers() == {}
        assert VggSmall(dropout=0.0, feature_dropout=0.0)._regularisers() == {}
        assert VggSmall(dropout=0.3)._regularisers() == {'dropout': 0.3}
        assert VggSmallDrop(dropout=0.3, feature_dropout=0.1, label_smoothing=0.1)._regularisers() == {
            'dropout': 0.3, 'feature_dropout': 0.1, 'label_smoothing': 0.1}
        for name in ('dropout', 'feature_dropout'):
            for bad in (1.0, -0.5):
                with pytest.raises(ValueError):
                    VggSmall(**{name: bad})._regularisers()
        small = 'synthetic://image?n=64&size=8&channels=1&classes=4&seed=0'
        ff = dict(epochs=1, hidden_layer_count=2, hidden_layer_units=8, learning_rate=0.01, batch_size=16, image_size=8)
        with pytest.raises(ValueError):
            FeedForward(feature_dropout=0.2, **ff).train(small)
        m = FeedForward(dropout=0.25, **ff)
        m.train(small)
        assert m._engine.dropout == 0.25 and len(m._engine.fcs) == 2
        assert 0.0 <= m.evaluate(small) <= 1.0


def test_vgg_small_drop_round_trip(monkeypatch):
    from rafiki_amd.engine.convnet import ConvNetEngine
    from rafiki_amd.models.vgg_small import VggSmallDrop
    steps, set_step, fwd = [], ConvNetEngine.set_step, ConvNetEngine._fwd_bwd_cpu

    def rec_set_step(self, epoch, step):
        steps.append(('set', epoch, step))
        return set_step(self, epoch, step)

    def rec_fwd(self, x, labels):
        steps.append(('step',) + tuple(self._drop_at))
        return fwd(self, x, labels)
    monkeypatch.setattr(ConvNetEngine, 'set_step', rec_set_step)
    monkeypatch.setattr(ConvNetEngine, '_fwd_bwd_cpu', rec_fwd)
    knobs = dict(epochs=2, learning_rate=0.05, momentum=0.9, weight_decay=5e-4, batch_size=32, width_mult=0.5,
                 image_size=16, augment='flip', mix='none', label_smoothing=0.1, dropout=0.5, feature_dropout=0.25,
                 seed=3)
    with _cpu():
        m = VggSmallDrop(**knobs)
        m.train(TRAIN)
        eng = m._engine
        assert eng.dropout == 0.5 and eng.feature_dropout == 0.25 and eng.label_smoothing == 0.1
        # every training step was announced, and ran, under its (epoch, step within the epoch)
        want = [(kind, e, b) for e in (0, 1) for b in range(4) for kind in ('set', 'step')]
        assert steps == want
        assert torch.isfinite(eng.flat.master).all()
        score = m.evaluate(TRAIN)
        assert isinstance(score, float) and 0.0 <= score <= 1.0
        params = pickle.loads(pickle.dumps(m.dump_parameters()))
        m2 = VggSmallDrop(**knobs)
        m2.load_parameters(params)
        e2 = m2._engine
        assert e2.dropout == 0.0 and e2.feature_dropout == 0.0 and e2.label_smoothing == 0.0
        images, _, _ = m._load(TRAIN)
        queries = images[:5].tolist()
        p1, p2 = m.predict(queries), m2.predict(queries)
        assert np.asarray(p2).shape == (5, 10) and np.allclose(p1, p2, atol=1e-6)
        assert steps == want                       # evaluate / predict took no training step


def test_resume_redraws_the_same_multipliers(tmp_path, monkeypatch):
    """A run checkpointed after epoch 0, crashed and resumed ends at the master weights of an uninterrupted run:
    the multipliers of epoch 1 depend on (seed, epoch, step) alone."""
    from rafiki_amd.models.image_classifier import NativeImageClassifier
    from rafiki_amd.utils import faults
    from rafiki_amd.utils.checkpoint import TrialCheckpoint

    class Tiny(NativeImageClassifier):
        DEFAULT_IMAGE_SIZE = 16

        def _engine_kwargs(self, num_classes, channels, image_size):
            return dict(cfg=(16, 'M', 32, 32, 'M'), fc_dims=(32,), optimizer='sgd', lr=0.05, weight_decay=0.0)

    knobs = dict(epochs=2, batch_size=32, image_size=16, dropout=0.5, feature_dropout=0.25, seed=5)
    with _cpu():
        a = Tiny(**knobs)
        a.train(TRAIN)
        plain = Tiny(**dict(knobs, dropout=0.0, feature_dropout=0.0))
        plain.train(TRAIN)
    ck = TrialCheckpoint(str(tmp_path), 'drop1')
    monkeypatch.setenv('RAFIKI_FAULT_INJECT', 'crash:epoch=0')
    faults.reset()
    with _cpu(checkpoint=ck):
        with pytest.raises(faults.WorkerCrash):
            Tiny(**knobs).train(TRAIN)
        assert ck.exists()
        monkeypatch.setenv('RAFIKI_FAULT_INJECT', '')
        faults.reset()
        b = Tiny(**knobs)
        b.train(TRAIN)
    assert ck.resumed_from == 0
    assert torch.equal(a._engine.flat.master, b._engine.flat.master)
    assert not torch.equal(a._engine.flat.master, plain._engine.flat.master)     # and dropout did act
