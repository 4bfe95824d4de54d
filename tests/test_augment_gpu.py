"""The augmenting step prologue (rk_gather_batch_aug, csrc/kernels/loss_optim.hip) and the engine paths built on
it, against the oracles of tests/augment_refs.py (Philox reference + a pixel loop; nothing of rafiki_amd).  The
kernel copies and never computes, so every image comparison is bit-exact."""
import functools

import numpy as np
import pytest
import torch

import augment_refs as AR
import loss_optim_refs as R
from test_loss_optim_gpu import _engine, _i32, _middle

pytestmark = pytest.mark.gpu

DEV = 'cuda'


@pytest.fixture(scope='module')
def fn():
    from rafiki_amd.ops import _lib, functional
    _lib.lib()  # loud failure if the native library is missing
    return functional


@functools.lru_cache(maxsize=None)
def _dataset(fmt):
    """Host buffers of one format: images [40 + 8, 6, 10, C] and labels, the 40 real rows in the middle of a
    sentinel fill (-5 / -777)."""
    dtype, C = AR.FORMATS[fmt]
    gen = torch.Generator().manual_seed(C)
    big = torch.full((AR.NROWS + 8, AR.H, AR.W, C), -5.0, dtype=getattr(torch, dtype))
    big[4:4 + AR.NROWS] = torch.randn(AR.NROWS, AR.H, AR.W, C, generator=gen).to(big.dtype)
    big_l = torch.full((AR.NROWS + 8,), -777, dtype=torch.int32)
    big_l[4:4 + AR.NROWS] = torch.randint(0, 10, (AR.NROWS,), generator=gen, dtype=torch.int32)
    return big, big_l


@functools.lru_cache(maxsize=None)
def _augmented_rows(fmt, pad, flip_p, epoch):
    """All 40 rows augmented by the oracle (the draw belongs to the row, so a batch is a selection of these)."""
    big, _ = _dataset(fmt)
    dy, dx, flip = AR.all_rows_draws(pad, flip_p, epoch)
    return AR.crop(big[4:4 + AR.NROWS].float().numpy(), np.arange(AR.NROWS), dy, dx, flip)


def _expect(fmt, sched, ctr, pad, flip_p, epoch):
    _, big_l = _dataset(fmt)
    idx = AR.clamp_rows(sched[ctr % AR.NSTEPS], AR.NROWS)
    return _augmented_rows(fmt, pad, flip_p, epoch)[idx], big_l[4:4 + AR.NROWS].numpy()[idx]


@pytest.mark.parametrize('B', [5, 64, 256])
@pytest.mark.parametrize('fmt', list(AR.FORMATS))
def test_gather_batch_aug_direct(fn, fmt, B):
    """rk_gather_batch_aug on its own, laid out as test_gather_batch_direct: data, labels, sched and lr_table are
    views into the middle of sentinel-filled buffers, so a wrong row, a shift past the image or an unwrapped
    counter reads a sentinel (or another image) and fails the comparison instead of faulting.  6 x 10 images of
    1, 2 and 3 vectors per pixel: B = 5 leaves most of one block idle, B = 64 spans several samples per block
    (60-vector rows) and B = 256 with 180-vector rows takes the grid's full stride."""
    big, big_l = _dataset(fmt)
    C = big.shape[-1]
    gen = torch.Generator().manual_seed(B)
    big_s = torch.full((2 + AR.NSTEPS + 6, B), 1, dtype=torch.int64)      # sentinel: a valid row, the wrong one
    big_s[2:2 + AR.NSTEPS] = torch.randint(2, AR.NROWS, (AR.NSTEPS, B), generator=gen)
    big_s[2:2 + AR.NSTEPS, 0] = torch.tensor([-1, AR.NROWS, -1])         # outside the dataset: read row 0
    big_s[2 + 1, B - 1] = AR.NROWS + 3
    big_t = torch.full((2 + AR.NSTEPS + 6,), 55.0)
    big_t[2:2 + AR.NSTEPS] = torch.tensor([1.0, 0.25, 0.5])
    dbig, dl, ds, dt = big.to(DEV), big_l.to(DEV), big_s.to(DEV), big_t.to(DEV)
    data, labels, sched, table = (_middle(dbig, 4, AR.NROWS), _middle(dl, 4, AR.NROWS), _middle(ds, 2, AR.NSTEPS),
                                  _middle(dt, 2, AR.NSTEPS))
    h_sched = big_s[2:2 + AR.NSTEPS].numpy()
    out_x = torch.full((B, AR.H, AR.W, C), 9.0, dtype=big.dtype, device=DEV)
    out_y = torch.full((B,), -9, dtype=torch.int32, device=DEV)
    big_z = torch.full((37 + 16,), float('nan'), dtype=torch.float64, device=DEV)
    zero = big_z[8:8 + 37]
    lr_out = torch.full((1,), -1.0, device=DEV)
    plain = torch.empty_like(out_x)
    for pad, flip_p in AR.PAD_FLIP:
        for epoch in AR.EPOCHS:
            ep = None if epoch is None else _i32(epoch)
            kw = dict(pad=pad, flip_p=flip_p, seed=AR.SEED, stream_id=AR.STREAM, epoch=ep)
            for ctr in (0, 2, 3, 7):        # 3 and 7 wrap to 0 and 1
                counter = _i32(ctr)
                out_x.fill_(9.0)
                out_y.fill_(-9)
                zero.fill_(float('nan'))
                lr_out.fill_(-1.0)
                fn.gather_batch_aug(data, labels, sched, counter, out_x, out_y, zero=zero, lr_table=table,
                                    lr_out=lr_out, **kw)
                torch.cuda.synchronize()
                rx, ry = _expect(fmt, h_sched, ctr, pad, flip_p, epoch)
                what = (pad, flip_p, epoch, ctr)
                assert np.array_equal(out_x.float().cpu().numpy(), rx), what
                assert np.array_equal(out_y.cpu().numpy(), ry), what
                assert lr_out.item() == big_t[2 + ctr % AR.NSTEPS].item(), what
                assert int(counter.item()) == ctr      # no `done`: the counter is the caller's to advance
                assert torch.count_nonzero(big_z[8:45]) == 0 and bool(big_z[:8].isnan().all()) and \
                    bool(big_z[45:].isnan().all())
                if pad == 0 and flip_p in (0.0, 1.0):  # no augmentation / a pure mirror of the plain prologue
                    fn.gather_batch(data, labels, sched, counter, plain, out_y)
                    assert torch.equal(out_x, plain if flip_p == 0.0 else plain.flip(2)), what
            if ep is not None:
                assert int(ep.item()) == epoch
    # with `done` the last block advances the counter: three launches walk steps 1, 2, 0
    kw = dict(pad=2, flip_p=0.5, seed=AR.SEED, stream_id=AR.STREAM, epoch=_i32(5))
    counter, done = _i32(1), _i32(0)
    lr_out.fill_(-1.0)
    for k in range(3):
        fn.gather_batch_aug(data, labels, sched, counter, out_x, out_y, done=done, **kw)
        torch.cuda.synchronize()
        rx, ry = _expect(fmt, h_sched, 1 + k, 2, 0.5, 5)
        assert np.array_equal(out_x.float().cpu().numpy(), rx) and np.array_equal(out_y.cpu().numpy(), ry)
        assert int(counter.item()) == 2 + k and int(done.item()) == 0
    assert lr_out.item() == -1.0                                  # no table: lr_out is left alone
    assert torch.equal(dbig.cpu(), big) and torch.equal(ds.cpu(), big_s)
    assert torch.equal(dl.cpu(), big_l) and torch.equal(dt.cpu(), big_t)


def test_gather_batch_aug_refusals(fn):
    """An unsupported geometry or probability is a KernelError and launches nothing (the outputs keep their fill)."""
    from rafiki_amd.ops._lib import KernelError
    B = 4
    data = torch.randn(8, AR.H, AR.W, 8, device=DEV)
    labels = torch.zeros(8, dtype=torch.int32, device=DEV)
    sched = torch.zeros((1, B), dtype=torch.int64, device=DEV)
    out_x = torch.full((B, AR.H, AR.W, 8), 9.0, device=DEV)
    out_y = torch.full((B,), -9, dtype=torch.int32, device=DEV)
    counter = _i32(0)
    ok = dict(pad=2, flip_p=0.5, seed=1, stream_id=2)
    bad = [dict(ok, pad=AR.H), dict(ok, pad=AR.W + 3), dict(ok, pad=-1), dict(ok, flip_p=-0.01),
           dict(ok, flip_p=1.01), dict(ok, flip_p=float('nan'))]
    for kw in bad:
        with pytest.raises(KernelError):
            fn.gather_batch_aug(data, labels, sched, counter, out_x, out_y, **kw)
    # a row that is no whole number of 16-byte pixels vectors: 6 fp32 channels = 24 bytes a pixel
    data6 = torch.randn(8, AR.H, AR.W, 6, device=DEV)
    out6 = torch.full((B, AR.H, AR.W, 6), 9.0, device=DEV)
    with pytest.raises(KernelError):
        fn.gather_batch_aug(data6, labels, sched, counter, out6, out_y, **ok)
    # and the entry point itself with a row size that is not 16 * H * W * vpp
    from rafiki_amd.ops import _lib
    p = lambda t: t.data_ptr()      # noqa: E731
    for row_bytes, H, W, vpp in ((16 * AR.H * AR.W * 2 - 16, AR.H, AR.W, 2), (16 * AR.H * AR.W * 2, AR.W, AR.W, 2),
                                 (16 * AR.H * AR.W * 2, AR.H, AR.W, 1), (0, 0, AR.W, 2)):
        with pytest.raises(KernelError):
            _lib.call('rk_gather_batch_aug', p(data), row_bytes, p(labels), p(sched), p(counter), B, p(out_x),
                      p(out_y), None, 0, None, None, None, 1, 8, H, W, vpp, 2, 0.5, 1, 2, None,
                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((out_x == 9.0).all()) and bool((out6 == 9.0).all()) and bool((out_y == -9).all())
    fn.gather_batch_aug(data, labels, sched, counter, out_x, out_y, **ok)      # the same call, supported
    torch.cuda.synchronize()
    assert not bool((out_x == 9.0).any()) and bool((out_y == 0).all())


# ------------------------------------------------------------------------------------------- the engine
def _engine_data(eng, n=96, seed=7):
    gen = torch.Generator().manual_seed(seed)
    x = torch.zeros((n,) + tuple(eng.input_shape(1))[1:])
    x[..., :3] = torch.randn(x[..., :3].shape, generator=gen)
    data = x.to(eng.act_dtype)
    labels = torch.randint(0, 10, (n,), generator=gen, dtype=torch.int32)
    return data, labels


@pytest.mark.parametrize('dtype', ['bf16', 'fp32'])
def test_scheduled_graph_augments_per_epoch(dtype):
    """Two epochs of three replays of the captured step with augment = pad 2, flip 0.5: after every replay the
    static batch is the oracle's for that step's schedule row and that epoch, and one schedule gives different
    batches in epoch 0 and epoch 1.  augment_batch gives the same images, on the GPU and through the CPU twin."""
    from rafiki_amd.ops.augment import AUG_STREAM
    from rafiki_amd.engine.convnet import ConvNetEngine
    pad, flip_p, steps, B, n = 2, 0.5, 3, 32, 96
    eng = _engine(dtype, augment={'pad': pad, 'flip': flip_p})
    data, labels = _engine_data(eng)
    ddata, dlabels = data.to(DEV), labels.to(DEV)
    idx = torch.randint(0, n, (steps, B), generator=torch.Generator().manual_seed(1))
    eng.capture_scheduled(ddata, dlabels, steps, B)
    batches = {}
    for epoch in (0, 1):
        eng.set_schedule(idx.to(DEV), epoch=epoch)
        for s in range(steps):
            eng.replay()
            torch.cuda.synchronize()
            rows = idx[s].numpy()
            ref = AR.crop(data.float().numpy(), rows, *AR.draws(3, rows, epoch, pad, flip_p, AUG_STREAM))
            got = eng._static_x.float().cpu().numpy()
            assert np.array_equal(got, ref), (epoch, s)
            assert np.array_equal(eng._static_y.cpu().numpy(), labels.numpy()[rows]), (epoch, s)
            batches[epoch, s] = got
        assert int(eng._ctr.item()) == steps
    assert all(not np.array_equal(batches[0, s], batches[1, s]) for s in range(steps))
    # augment_batch: the same kernel over a one-row schedule, and the twin on a CPU engine of the same seed
    cpu = ConvNetEngine(num_classes=10, in_channels=3, image_size=16, cfg=(16, 'M', 32, 32, 'M'), fc_dims=(32,),
                        device='cpu', seed=3, dtype=dtype, augment={'pad': pad, 'flip': flip_p})
    assert tuple(cpu.input_shape(B)) == tuple(eng.input_shape(B))
    for epoch in (0, 1):
        out = torch.full(eng.input_shape(B), 9.0, dtype=eng.act_dtype, device=DEV)
        eng.augment_batch(ddata, idx[1].to(DEV), epoch, out)
        torch.cuda.synchronize()
        host = torch.full(cpu.input_shape(B), 9.0, dtype=data.dtype)
        cpu.augment_batch(data, idx[1], epoch, host)
        assert torch.equal(out.cpu(), host)
        assert np.array_equal(out.float().cpu().numpy(), batches[epoch, 1])


@pytest.mark.parametrize('dtype', ['bf16', 'fp32'])
def test_null_augmentation_trains_like_no_augmentation(dtype):
    """augment = pad 0, flip 0 runs the augmenting prologue and copies every image unchanged: after three
    replays from the same seed the master weights equal those of augment=None bit for bit."""
    steps, B = 3, 32
    masters = []
    for aug in (None, {'pad': 0, 'flip': 0.0}):
        eng = _engine(dtype, augment=aug)
        data, labels = _engine_data(eng)
        idx = torch.randint(0, 96, (steps, B), generator=torch.Generator().manual_seed(1)).to(DEV)
        eng.capture_scheduled(data.to(DEV), labels.to(DEV), steps, B)
        eng.set_schedule(idx, lr_scales=R.LR_SCALES[:steps], epoch=4)
        for _ in range(steps):
            eng.replay()
        torch.cuda.synchronize()
        masters.append(eng.flat.master.clone())
        assert (eng._aug_epoch is None) == (aug is None)
    assert torch.equal(masters[0], masters[1])
    assert bool(masters[0].isfinite().all())


@pytest.mark.parametrize('optimizer', ['sgd', 'adam'])
def test_model_loops_pass_their_epoch(optimizer, monkeypatch):
    """NativeImageClassifier.train on the GPU, two epochs: the scheduled graph (SGD) and the captured step fed
    by augment_batch (Adam) both train on the twin's batches for the epoch's permutation and number."""
    from rafiki_amd.engine.convnet import ConvNetEngine
    from rafiki_amd.models.image_classifier import NativeImageClassifier
    from rafiki_amd.ops import augment as A
    from rafiki_amd.parallel.context import TrialContext, use_context

    class Tiny(NativeImageClassifier):
        DEFAULT_IMAGE_SIZE = 16

        def _engine_kwargs(self, num_classes, channels, image_size):
            return dict(cfg=(16, 'M', 32, 32, 'M'), fc_dims=(32,), optimizer=optimizer, lr=1e-3, weight_decay=0.0)

    seen = []
    replay, step_graph = ConvNetEngine.replay, ConvNetEngine.step_graph

    def rec_replay(self):
        replay(self)
        seen.append(self._static_x.clone())

    def rec_step_graph(self, x, labels):
        seen.append(x.clone())
        step_graph(self, x, labels)
    monkeypatch.setattr(ConvNetEngine, 'replay', rec_replay)
    monkeypatch.setattr(ConvNetEngine, 'step_graph', rec_step_graph)
    uri = 'synthetic://image?n=128&size=16&channels=3&classes=10&seed=0'
    with use_context(TrialContext(device=torch.device(DEV))):
        m = Tiny(epochs=2, batch_size=32, image_size=16, augment='crop_flip', augment_pad=3, seed=9)
        m.train(uri)
        eng = m._engine
        assert (eng._sched_graph if optimizer == 'sgd' else eng._graph) is not None
        assert len(seen) == 8
        images, _, _ = m._load(uri)
        x_all = eng.prepare_inputs(images).cpu()
        gen = torch.Generator(device=DEV).manual_seed(9)
        for epoch in (0, 1):
            perm = torch.randperm(128, device=DEV, generator=gen).cpu()
            for b in range(4):
                idx = perm[b * 32:(b + 1) * 32]
                ref = A.apply(x_all, idx, *A.draws(9, idx, epoch, 3, 0.5))
                assert torch.equal(seen[4 * epoch + b].cpu(), ref), (epoch, b)
        assert isinstance(m.evaluate(uri), float)
        m.destroy()


def test_mlp_engine_refuses_augment():
    with pytest.raises(ValueError):
        _engine('fp32', cfg=(), augment={'pad': 1, 'flip': 0.5})
