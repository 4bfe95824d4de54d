"""The host twin of the crop-and-mirror augmentation (rafiki_amd/ops/augment.py) against the oracles of
tests/augment_refs.py, the inputs of the kernel test, and an augmenting VggSmall trial on the CPU engine."""
import pickle

import numpy as np
import pytest
import torch

import augment_refs as AR
import loss_optim_refs as R

from rafiki_amd.ops import augment as A


@pytest.mark.parametrize('seed', [12345, (1 << 32) + 12345, 0xDEADBEEF12345678])
def test_draws_match_the_philox_oracle(seed):
    rows = np.array([0, 1, 2, 39, 40, 49999, (1 << 32) - 1, 1 << 32, (1 << 32) + 7, (5 << 32) + 3], dtype=np.int64)
    for stream in R.PHILOX_STREAMS:
        for epoch in (0, 5):
            for pad, flip_p in ((0, 0.0), (0, 1.0), (2, 0.5), (4, 0.5), (31, 0.25)):
                dy, dx, flip = A.draws(seed, rows, epoch, pad, flip_p, stream_id=stream)
                ry, rx, rf = AR.draws(seed, rows, epoch, pad, flip_p, stream)
                assert np.array_equal(dy, ry) and np.array_equal(dx, rx) and np.array_equal(flip, rf)
                assert dy.min() >= -pad and dy.max() <= pad and dx.min() >= -pad and dx.max() <= pad
                assert flip.all() if flip_p == 1.0 else not flip.any() if flip_p == 0.0 else True
    # the default stream is the module's constant, and a tensor of rows is taken like an array
    got = A.draws(seed, torch.from_numpy(rows), 5, 2, 0.5)
    ref = AR.draws(seed, rows, 5, 2, 0.5, A.AUG_STREAM)
    assert all(np.array_equal(g, r) for g, r in zip(got, ref))
    # the draw belongs to the row: the same row elsewhere in a batch draws the same
    again = A.draws(seed, rows[::-1].copy(), 5, 2, 0.5)
    assert all(np.array_equal(g[::-1], r) for g, r in zip(again, got))


@pytest.mark.parametrize('fmt', list(AR.FORMATS))
def test_apply_matches_the_pixel_loop(fmt):
    """6 x 10 images (H != W: swapped axes show) with 1, 2 and 3 16-byte vectors per pixel."""
    dtype, C = AR.FORMATS[fmt]
    gen = torch.Generator().manual_seed(C)
    data = torch.randn(AR.NROWS, AR.H, AR.W, C, generator=gen).to(getattr(torch, dtype))
    rows = np.concatenate([np.arange(AR.NROWS), [3, 3, 0, AR.NROWS - 1]])
    for pad, flip_p in AR.PAD_FLIP:
        dy, dx, flip = AR.draws(AR.SEED, rows, 1, pad, flip_p, AR.STREAM)
        got = A.apply(data, torch.from_numpy(rows), dy, dx, flip)
        assert got.dtype == data.dtype and tuple(got.shape) == (len(rows), AR.H, AR.W, C)
        ref = AR.crop(data.float().numpy(), rows, dy, dx, flip)
        assert np.array_equal(got.float().numpy(), ref), (pad, flip_p)
        if (pad, flip_p) == (0, 0.0):
            assert torch.equal(got, data[torch.from_numpy(rows)])
        if (pad, flip_p) == (0, 1.0):
            assert torch.equal(got, data[torch.from_numpy(rows)].flip(2))


def test_the_kernel_test_inputs_reach_every_case():
    """Over the 40 rows of the GPU test at pad 2, flip 0.5: every shift -2..2 in both axes, both mirror states,
    and a zero border on each of the four sides (a condition on the oracle alone)."""
    for epoch in AR.EPOCHS:
        dy, dx, flip = AR.all_rows_draws(2, 0.5, epoch)
        assert set(dy.tolist()) == set(dx.tolist()) == {-2, -1, 0, 1, 2}, epoch
        assert flip.any() and not flip.all()
        # dy < 0: rows above the image (top border); dy > 0: bottom; likewise left and right for dx
        assert (dy < 0).any() and (dy > 0).any() and (dx < 0).any() and (dx > 0).any()
        # and mirrored samples with a border on either side
        assert (flip & (dx < 0)).any() and (flip & (dx > 0)).any()
    d0, d5 = AR.all_rows_draws(2, 0.5, 0), AR.all_rows_draws(2, 0.5, 5)
    assert not all(np.array_equal(a, b) for a, b in zip(d0, d5))
    assert all(np.array_equal(a, b) for a, b in zip(d0, AR.all_rows_draws(2, 0.5, None)))


TRAIN = 'synthetic://image?n=256&size=32&channels=3&classes=10&seed=0'
TEST = 'synthetic://image?n=64&size=32&channels=3&classes=10&seed=1'


def _cpu():
    from rafiki_amd.parallel.context import TrialContext, use_context
    return use_context(TrialContext(device=torch.device('cpu')))


def test_vgg_small_cpu_trial_trains_on_the_twins_batches(monkeypatch):
    from rafiki_amd.engine.convnet import ConvNetEngine
    from rafiki_amd.models.vgg_small import VggSmall
    seen = []
    step = ConvNetEngine.train_step

    def recording(self, x, labels):
        seen.append((x.clone(), labels.clone()))
        return step(self, x, labels)
    monkeypatch.setattr(ConvNetEngine, 'train_step', recording)
    knobs = dict(epochs=1, learning_rate=0.05, momentum=0.9, weight_decay=5e-4, batch_size=64, width_mult=0.5,
                 image_size=32, augment='crop_flip', seed=3)
    with _cpu():
        m = VggSmall(**knobs)
        m.train(TRAIN)
        eng = m._engine
        assert eng.augment == {'pad': 4, 'flip': 0.5}
        assert len(seen) == 4
        images, labels, _ = m._load(TRAIN)
        x_all, y_all = eng.prepare_inputs(images), torch.from_numpy(np.asarray(labels, dtype=np.int32))
        perm = torch.randperm(256, generator=torch.Generator().manual_seed(3))
        changed = 0
        for b, (x, y) in enumerate(seen):
            idx = perm[b * 64:(b + 1) * 64]
            dy, dx, flip = A.draws(3, idx, 0, 4, 0.5)
            assert torch.equal(x, A.apply(x_all, idx, dy, dx, flip)), b
            assert torch.equal(y, y_all[idx]), b
            changed += int((x != x_all[idx]).flatten(1).any(1).sum())
        assert changed > 200         # nearly every image is shifted or mirrored
        # the first batch against the oracle as well (Philox reference + pixel loop)
        idx = perm[:64].numpy()
        ref = AR.crop(x_all.numpy(), idx, *AR.draws(3, idx, 0, 4, 0.5, A.AUG_STREAM))
        assert np.array_equal(seen[0][0].numpy(), ref)
        score = m.evaluate(TEST)
        assert isinstance(score, float) and 0.0 <= score <= 1.0
        params = pickle.loads(pickle.dumps(m.dump_parameters()))
        m2 = VggSmall(**knobs)
        m2.load_parameters(params)
        assert m2._engine.augment is None        # serving never augments
        queries = images[:5].tolist()
        p1, p2 = m.predict(queries), m2.predict(queries)
        assert np.asarray(p2).shape == (5, 10) and np.allclose(p1, p2, atol=1e-6)
        assert len(seen) == 4                    # evaluate / predict took no training step


def test_knob_configs():
    from rafiki_amd.model import CategoricalKnob, FixedKnob
    from rafiki_amd.models.vgg16 import Vgg16
    from rafiki_amd.models.vgg_small import VggSmall, VggSmallAug, VggSmallProbe, VggSmallTrial
    for cls in (VggSmall, Vgg16):
        k = cls.get_knob_config()['augment']
        assert isinstance(k, FixedKnob) and k.value == 'none'
    k = VggSmallAug.get_knob_config()
    assert isinstance(k['augment'], CategoricalKnob) and k['augment'].values == ['none', 'flip', 'crop_flip']
    assert set(k) == set(VggSmall.get_knob_config())
    for cls in (VggSmallTrial, VggSmallProbe):
        assert 'augment' not in cls.get_knob_config()
    with _cpu():
        assert VggSmall()._augment() is None
        assert VggSmall(augment='flip')._augment() == {'pad': 0, 'flip': 0.5}
        assert VggSmall(augment='crop')._augment() == {'pad': 4, 'flip': 0.0}
        assert VggSmall(augment='crop_flip', augment_pad=2)._augment() == {'pad': 2, 'flip': 0.5}
        assert VggSmall(augment='crop', augment_pad=99)._augment() == {'pad': 31, 'flip': 0.0}


def test_validation():
    from rafiki_amd.engine.convnet import ConvNetEngine
    from rafiki_amd.models.feed_forward import FeedForward
    from rafiki_amd.models.vgg_small import VggSmall
    with pytest.raises(ValueError):     # an MLP has no image to crop
        ConvNetEngine(num_classes=10, in_channels=1, image_size=8, cfg=(), fc_dims=(16,), device='cpu',
                      optimizer='adam', input_bn=True, augment={'pad': 1, 'flip': 0.5})
    for bad in ({'pad': 8, 'flip': 0.0}, {'pad': -1, 'flip': 0.0}, {'pad': 1, 'flip': 1.5}, {'pad': 1, 'mirror': 1}):
        with pytest.raises(ValueError):
            ConvNetEngine(num_classes=10, in_channels=3, image_size=8, cfg=(8, 'M'), fc_dims=(16,), device='cpu',
                          augment=bad)
    eng = ConvNetEngine(num_classes=10, in_channels=3, image_size=8, cfg=(8, 'M'), fc_dims=(16,), device='cpu')
    with pytest.raises(RuntimeError):
        eng.augment_batch(torch.zeros(4, 8, 8, eng.cin_p), torch.arange(2), 0, torch.zeros(2, 8, 8, eng.cin_p))
    small = 'synthetic://image?n=64&size=8&channels=1&classes=4&seed=0'
    with _cpu():
        with pytest.raises(ValueError):
            FeedForward(epochs=1, hidden_layer_count=1, hidden_layer_units=8, learning_rate=0.01, batch_size=16,
                        image_size=8, augment='flip').train(small)
        with pytest.raises(ValueError):
            VggSmall(epochs=1, batch_size=16, image_size=8, augment='mixup').train(small)


def test_cpu_augment_batch_clamps_rows_like_the_prologue():
    from rafiki_amd.engine.convnet import ConvNetEngine
    eng = ConvNetEngine(num_classes=10, in_channels=3, image_size=8, cfg=(8, 'M'), fc_dims=(16,), device='cpu',
                        seed=5, augment={'pad': 2, 'flip': 0.5})
    data = torch.randn(20, 8, 8, eng.cin_p, generator=torch.Generator().manual_seed(0))
    idx = torch.tensor([3, -1, 20, 19, 3])
    out = torch.full((5, 8, 8, eng.cin_p), 9.0)
    eng.augment_batch(data, idx, 2, out)
    rows = AR.clamp_rows(idx.numpy(), 20)
    assert rows.tolist() == [3, 0, 0, 19, 3]
    ref = AR.crop(data.numpy(), rows, *AR.draws(5, rows, 2, 2, 0.5, A.AUG_STREAM))
    assert np.array_equal(out.numpy(), ref)
    assert np.array_equal(out[0].numpy(), out[4].numpy())
