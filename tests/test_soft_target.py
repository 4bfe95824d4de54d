"""Soft targets on the CPU: the per-epoch mixup / CutMix plan and the host twin of the mixing prologue
(rafiki_amd/ops/mix.py) against the oracles of tests/soft_target_refs.py, the engine's argument checks and soft
reference loss, and a VggSmallReg trial on the CPU engine."""
import pickle

import numpy as np
import pytest
import torch

import augment_refs as AR
import soft_target_refs as SR

from rafiki_amd.ops import augment as A
from rafiki_amd.ops import mix as M


# ------------------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize('kind', M.KINDS)
def test_plan_properties(kind):
    H, W, steps = 6, 10, 200
    lam, box = M.plan(7, 3, steps, kind, 1.0, 1.0, H, W)
    assert lam.dtype == np.float32 and lam.shape == (steps,) and box.dtype == np.int32 and box.shape == (steps, 4)
    assert (lam >= 0).all() and (lam <= 1).all()
    y0, y1, x0, x1 = box.T
    assert (0 <= y0).all() and (y0 <= y1).all() and (y1 <= H).all()
    assert (0 <= x0).all() and (x0 <= x1).all() and (x1 <= W).all()
    if kind == 'mixup':
        assert (lam >= 0.5).all() and (lam < 1).any() and not box.any()
    else:
        area = ((y1 - y0) * (x1 - x0)).astype(np.float32)
        assert np.array_equal(lam, np.float32(1.0) - area / np.float32(H * W))
        assert (area > 0).any() and len(set(area.tolist())) > 3
    # equal for equal (seed, epoch), different across epochs and seeds; a longer plan extends a shorter one
    again = M.plan(7, 3, steps, kind, 1.0, 1.0, H, W)
    assert np.array_equal(lam, again[0]) and np.array_equal(box, again[1])
    for other in (M.plan(7, 4, steps, kind, 1.0, 1.0, H, W), M.plan(8, 3, steps, kind, 1.0, 1.0, H, W)):
        assert not np.array_equal(lam, other[0])
    short = M.plan(7, 3, 17, kind, 1.0, 1.0, H, W)
    assert np.array_equal(short[0], lam[:17]) and np.array_equal(short[1], box[:17])
    # prob = 0: no step is mixed; prob = 0.5: some are, and those keep the values of the always-mixed plan
    off = M.plan(7, 3, steps, kind, 1.0, 0.0, H, W)
    assert (off[0] == 1.0).all() and not off[1].any()
    half = M.plan(7, 3, steps, kind, 1.0, 0.5, H, W)
    mixed = half[0] != 1.0
    assert 40 < int(mixed.sum()) < 160
    assert np.array_equal(half[0][mixed], lam[mixed]) and np.array_equal(half[1][mixed], box[mixed])
    with pytest.raises(ValueError):
        M.plan(7, 3, steps, 'cutout', 1.0, 1.0, H, W)


# ------------------------------------------------------------------------------------------- the twin
@pytest.mark.parametrize('fmt', list(AR.FORMATS))
@pytest.mark.parametrize('augment', [None, {'pad': 2, 'flip': 0.5}])
def test_apply_matches_the_oracle(fmt, augment):
    dtype, C = AR.FORMATS[fmt]
    gen = torch.Generator().manual_seed(C)
    data = torch.randn(AR.NROWS, AR.H, AR.W, C, generator=gen).to(getattr(torch, dtype))
    rows = np.concatenate([np.arange(AR.NROWS)[::3], [3, 3, 0, AR.NROWS - 1]])
    host = data.float().numpy()

    def images(r):
        if augment is None:
            return host[r]
        return AR.crop(host, r, *AR.draws(AR.SEED, r, 5, augment['pad'], augment['flip'], AR.STREAM))
    a, p = images(rows), images(SR.partner(rows))
    kw = dict(augment=augment, seed=AR.SEED, epoch=5, stream_id=AR.STREAM)
    for name, box in SR.BOXES.items():
        got = M.apply(data, rows, 'cutmix', 0.25, np.asarray(box), **kw)
        assert got.dtype == data.dtype
        ref = SR.box_mix(a, p, box)
        assert np.array_equal(got.float().numpy(), ref), name
        assert np.array_equal(ref, SR.box_mix(a, p, SR.clamp_box(box, AR.H, AR.W))), name
    assert np.array_equal(SR.box_mix(a, p, SR.BOXES['empty']), a)
    assert np.array_equal(SR.box_mix(a, p, SR.BOXES['whole']), p)
    assert M.clamp_box(SR.BOXES['past'], AR.H, AR.W) == SR.clamp_box(SR.BOXES['past'], AR.H, AR.W) == (0, 4, 6, 10)
    for lam in SR.BLEND_LAMS:
        got = M.apply(data, rows, 'mixup', lam, **kw).float().numpy()
        if lam == 1.0:
            assert np.array_equal(got, a)
        elif lam == 0.0:
            assert np.array_equal(got, p)
        else:
            ref = SR.blend_mix(a, p, lam)
            assert (np.abs(got - ref) <= SR.blend_bound(a, p, ref, dtype == 'bfloat16')).all(), lam
            assert not np.array_equal(got, a) and not np.array_equal(got, p)


# ------------------------------------------------------------------------------------------- the engine
def _engine(**kw):
    from rafiki_amd.engine.convnet import ConvNetEngine
    args = dict(num_classes=10, in_channels=3, image_size=8, cfg=(8, 'M'), fc_dims=(16,), device='cpu', seed=5)
    args.update(kw)
    return ConvNetEngine(**args)


def test_engine_validation():
    ok = {'kind': 'mixup', 'alpha': 1.0, 'prob': 1.0}
    for bad in (dict(ok, kind='cutout'), dict(ok, alpha=0.0), dict(ok, alpha=-1.0), dict(ok, alpha=float('nan')),
                dict(ok, prob=1.5), dict(ok, prob=-0.1), dict(ok, beta=1.0), {'alpha': 1.0}):
        with pytest.raises(ValueError):
            _engine(mix=bad)
    for bad in (-0.1, 1.0, 1.5, float('nan')):
        with pytest.raises(ValueError):
            _engine(label_smoothing=bad)
    with pytest.raises(ValueError):     # an MLP has no image to mix
        _engine(cfg=(), optimizer='adam', input_bn=True, mix=ok)
    eng = _engine()
    assert eng.mix is None and eng.label_smoothing == 0.0 and not eng.soft
    with pytest.raises(RuntimeError):
        eng.mix_batch(torch.zeros(4, 8, 8, eng.cin_p), torch.zeros(4, dtype=torch.int32), torch.arange(2), 0, 0,
                      torch.zeros(2, 8, 8, eng.cin_p), torch.zeros(2, dtype=torch.int32))
    eng = _engine(mix={'kind': 'cutmix'})
    assert eng.mix == {'kind': 'cutmix', 'alpha': 1.0, 'prob': 1.0} and eng.soft
    with pytest.raises(RuntimeError):   # a mixing engine's step needs a mixed batch first
        eng.train_step(torch.zeros(2, 8, 8, eng.cin_p), torch.zeros(2, dtype=torch.int32))


def test_reference_loss_soft_target():
    """The defaults give today's loss; the soft loss is the fp64 oracle's."""
    eng = _engine()
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(12, 8, 8, eng.cin_p, generator=gen)
    y = torch.randint(0, 10, (12,), generator=gen, dtype=torch.int32)
    y2 = SR.second_labels(y, 10, 1)
    hard, logits = eng.reference_loss(x, y, training=True)
    assert torch.equal(hard, torch.nn.functional.cross_entropy(logits, y.long()))
    for lam, eps in SR.LAM_EPS:
        for l2 in (None, y2):
            loss, lg = eng.reference_loss(x.double(), y, {n: eng.flat.w(n).double() for n in eng.flat.names()},
                                          training=True, labels2=l2, lam=lam, smoothing=eps)
            ref = SR.soft_xent_ref(lg.detach(), y, 10, labels2=l2, lam=lam, eps=eps, grad_scale=1.0)
            # eps and lam reach the oracle rounded to fp32, the reference loss as given: 1e-7 covers that
            assert abs(loss.item() - ref['loss_sum'] / 12) < 1e-7 * max(1.0, abs(loss.item())), (lam, eps)
    same, _ = eng.reference_loss(x, y, training=True, labels2=y2, lam=1.0, smoothing=0.0)
    assert abs(same.item() - hard.item()) < 1e-6


@pytest.mark.parametrize('kind', M.KINDS)
def test_cpu_mix_batch_is_the_twin_and_fills_the_loss_buffers(kind):
    eng = _engine(mix={'kind': kind, 'alpha': 1.0, 'prob': 1.0}, augment={'pad': 2, 'flip': 0.5},
                  label_smoothing=0.1)
    gen = torch.Generator().manual_seed(0)
    data = torch.randn(20, 8, 8, eng.cin_p, generator=gen)
    labels = torch.randint(0, 10, (20,), generator=gen, dtype=torch.int32)
    idx = torch.tensor([3, -1, 20, 19, 3, 7])
    rows = AR.clamp_rows(idx.numpy(), 20)
    lam, box = M.plan(5, 2, 4, kind, 1.0, 1.0, 8, 8)
    out_x, out_y = torch.full((6, 8, 8, eng.cin_p), 9.0), torch.full((6,), -9, dtype=torch.int32)
    eng.mix_batch(data, labels, idx, 2, 3, out_x, out_y)
    host = data.numpy()
    a = AR.crop(host, rows, *AR.draws(5, rows, 2, 2, 0.5, A.AUG_STREAM))
    pr = SR.partner(rows)
    p = AR.crop(host, pr, *AR.draws(5, pr, 2, 2, 0.5, A.AUG_STREAM))
    if kind == 'cutmix':
        assert np.array_equal(out_x.numpy(), SR.box_mix(a, p, box[3]))
    else:
        ref = SR.blend_mix(a, p, lam[3])
        assert (np.abs(out_x.numpy() - ref) <= SR.blend_bound(a, p, ref, False)).all()
    assert np.array_equal(out_y.numpy(), labels.numpy()[rows])
    assert np.array_equal(eng._static_y2.numpy(), labels.numpy()[pr])
    assert eng._lam.item() == lam[3] and 0.0 < lam[3] < 1.0
    # the step takes them: its loss is the oracle's for (labels, partner labels, lam, 0.1)
    eng.reset_metrics()
    eng.forward_backward(out_x, out_y)
    _, logits = eng.reference_loss(out_x, None, training=True)
    ref = SR.soft_xent_ref(logits.detach(), out_y, 10, labels2=eng._static_y2, lam=lam[3], eps=0.1, grad_scale=1.0)
    assert abs(eng.loss_sum.item() - ref['loss_sum']) < 1e-4 * ref['loss_sum']
    assert int(eng.correct.item()) == ref['correct'] and int(eng.seen.item()) == 6
    assert bool(eng.flat.grad.isfinite().all()) and float(eng.flat.grad.abs().max()) > 0


def test_flat_input_net_trains_with_label_smoothing():
    eng = _engine(cfg=(), optimizer='adam', input_bn=True, label_smoothing=0.1, lr=1e-2, weight_decay=0.0)
    gen = torch.Generator().manual_seed(0)
    x = torch.zeros(32, eng.feat_dim)
    x[:, :eng.in_dim] = torch.randn(32, eng.in_dim, generator=gen)
    y = torch.randint(0, 10, (32,), generator=gen, dtype=torch.int32)
    losses = []
    for _ in range(30):
        eng.reset_metrics()
        eng.train_step(x, y)
        losses.append(eng.loss_sum.item() / 32)
    assert losses[-1] < 0.7 * losses[0], losses
    _, logits = eng.reference_loss(x, None, training=True)
    ref = SR.soft_xent_ref(logits.detach(), y, 10, eps=0.1, grad_scale=1.0)
    assert ref['loss_sum'] / 32 > 0.1 * np.log(10) * 0.5     # a smoothed loss cannot reach zero


# ------------------------------------------------------------------------------------------- the models
# 16 x 16: the smallest image VggSmall's four pooling stages leave a pixel of (8 x 8 pools away to nothing)
TRAIN = 'synthetic://image?n=128&size=16&channels=3&classes=10&seed=0'


def _cpu():
    from rafiki_amd.parallel.context import TrialContext, use_context
    return use_context(TrialContext(device=torch.device('cpu')))


def test_vgg_small_reg_round_trip(monkeypatch):
    from rafiki_amd.engine.convnet import ConvNetEngine
    from rafiki_amd.models import ZOO
    from rafiki_amd.models.vgg_small import VggSmallReg
    assert ZOO['VggSmallReg'] == ('vgg_small.py', 'IMAGE_CLASSIFICATION')
    seen = []
    step = ConvNetEngine.train_step

    def recording(self, x, labels):
        seen.append((x.clone(), labels.clone(), self._static_y2.clone(), self._lam.item()))
        return step(self, x, labels)
    monkeypatch.setattr(ConvNetEngine, 'train_step', recording)
    knobs = dict(epochs=2, learning_rate=0.05, momentum=0.9, weight_decay=5e-4, batch_size=32, width_mult=0.5,
                 image_size=16, augment='flip', mix='cutmix', mix_prob=1.0, label_smoothing=0.1, seed=3)
    with _cpu():
        m = VggSmallReg(**knobs)
        m.train(TRAIN)
        eng = m._engine
        assert eng.mix == {'kind': 'cutmix', 'alpha': 1.0, 'prob': 1.0} and eng.label_smoothing == 0.1
        assert eng.augment == {'pad': 0, 'flip': 0.5}
        assert len(seen) == 8
        images, labels, _ = m._load(TRAIN)
        x_all, y_all = eng.prepare_inputs(images), torch.from_numpy(np.asarray(labels, dtype=np.int32))
        gen = torch.Generator().manual_seed(3)
        plans = []
        for epoch in (0, 1):
            perm = torch.randperm(128, generator=gen)
            lam, box = M.plan(3, epoch, 4, 'cutmix', 1.0, 1.0, 16, 16)
            plans.append(lam)
            for b in range(4):
                idx = perm[b * 32:(b + 1) * 32].numpy()
                x, y, y2, got_lam = seen[4 * epoch + b]
                host = x_all.numpy()
                a = AR.crop(host, idx, *AR.draws(3, idx, epoch, 0, 0.5, A.AUG_STREAM))
                pr = SR.partner(idx)
                p = AR.crop(host, pr, *AR.draws(3, pr, epoch, 0, 0.5, A.AUG_STREAM))
                assert np.array_equal(x.numpy(), SR.box_mix(a, p, box[b])), (epoch, b)
                assert np.array_equal(y.numpy(), y_all.numpy()[idx]) and np.array_equal(y2.numpy(), y_all.numpy()[pr])
                assert got_lam == lam[b]
        assert not np.array_equal(plans[0], plans[1])
        score = m.evaluate(TRAIN)
        assert isinstance(score, float) and 0.0 <= score <= 1.0
        params = pickle.loads(pickle.dumps(m.dump_parameters()))
        m2 = VggSmallReg(**knobs)
        m2.load_parameters(params)
        e2 = m2._engine
        assert e2.mix is None and e2.label_smoothing == 0.0 and not e2.soft and e2.augment is None
        queries = images[:5].tolist()
        p1, p2 = m.predict(queries), m2.predict(queries)
        assert np.asarray(p2).shape == (5, 10) and np.allclose(p1, p2, atol=1e-6)
        assert len(seen) == 8                    # evaluate / predict took no training step


def test_knob_configs():
    from rafiki_amd.model import CategoricalKnob, FixedKnob, FloatKnob
    from rafiki_amd.models.feed_forward import FeedForward
    from rafiki_amd.models.vgg16 import Vgg16
    from rafiki_amd.models.vgg_small import VggSmall, VggSmallAug, VggSmallProbe, VggSmallReg, VggSmallTrial
    k = VggSmallReg.get_knob_config()
    assert isinstance(k['mix'], CategoricalKnob) and k['mix'].values == ['none', 'mixup', 'cutmix']
    assert isinstance(k['label_smoothing'], FloatKnob)
    assert (k['label_smoothing'].value_min, k['label_smoothing'].value_max) == (0.0, 0.2)
    assert set(k) == set(VggSmallAug.get_knob_config()) | {'mix', 'label_smoothing'}
    assert k['augment'].values == ['none', 'flip', 'crop_flip']
    # the existing configs carry none of the new knobs
    for cls in (VggSmall, VggSmallAug, VggSmallTrial, VggSmallProbe, Vgg16, FeedForward):
        assert not {'mix', 'mix_alpha', 'mix_prob', 'label_smoothing'} & set(cls.get_knob_config()), cls
    assert set(VggSmall.get_knob_config()) == {'epochs', 'learning_rate', 'momentum', 'weight_decay', 'batch_size',
                                               'width_mult', 'image_size', 'augment'}
    assert isinstance(VggSmall.get_knob_config()['augment'], FixedKnob)
    assert set(VggSmallTrial.get_knob_config()) == set(VggSmallProbe.get_knob_config()) == {
        'epochs', 'learning_rate', 'momentum', 'weight_decay', 'batch_size', 'width_mult', 'image_size'}
    with _cpu():
        assert VggSmall()._regularisers() == {}
        assert VggSmall(mix='mixup')._regularisers() == {'mix': {'kind': 'mixup', 'alpha': 1.0, 'prob': 1.0}}
        assert VggSmall(mix='cutmix', mix_alpha=0.4)._regularisers() == {
            'mix': {'kind': 'cutmix', 'alpha': 0.4, 'prob': 0.5}}
        assert VggSmall(label_smoothing=0.1)._regularisers() == {'label_smoothing': 0.1}
        with pytest.raises(ValueError):
            VggSmall(mix='cutout')._regularisers()
        with pytest.raises(ValueError):     # mixup is a `mix`, not an `augment`
            VggSmall(epochs=1, batch_size=16, image_size=16, augment='mixup').train(TRAIN)
        with pytest.raises(ValueError):
            FeedForward(epochs=1, hidden_layer_count=1, hidden_layer_units=8, learning_rate=0.01, batch_size=16,
                        image_size=8, mix='mixup').train('synthetic://image?n=64&size=8&channels=1&classes=4&seed=0')
