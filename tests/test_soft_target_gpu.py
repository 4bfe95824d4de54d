"""The soft-target loss kernels (rk_softmax_xent_soft, rk_softmax_xent_f32_soft, rk_head_fwd_bwd_soft), the mixing
step prologue (rk_gather_batch_mix) and the engine and model paths built on them, against the oracles of
tests/soft_target_refs.py and tests/augment_refs.py (fp64 PyTorch, a Philox reference, pixel loops; nothing of
rafiki_amd)."""
import numpy as np
import pytest
import torch

import augment_refs as AR
import loss_optim_refs as R
import soft_target_refs as SR
from test_augment_gpu import _augmented_rows, _dataset, _engine_data
from test_head_gpu import rel
from test_loss_optim_gpu import _engine, _i32, _middle, _xent_check

pytestmark = pytest.mark.gpu

DEV = 'cuda'


@pytest.fixture(scope='module')
def fn():
    from rafiki_amd.ops import _lib, functional
    _lib.lib()  # loud failure if the native library is missing
    return functional


def _lam_dev(lam):
    return None if lam is None else torch.full((1,), lam, dtype=torch.float32, device=DEV)


def _mixed(lam, labels2, ncls):
    """The target really holds two labels: the hard-label reference must then lie far from the soft one."""
    return labels2 is not None and lam is not None and lam < 1.0 and ncls > 1


# ------------------------------------------------------------------------------------------- softmax-xent
def _soft_launch(variant, x, y, ncls, ldd, *, labels2, lam, eps, grad_scale):
    from rafiki_amd.ops import f32 as S, functional as F
    B = x.shape[0]
    dl = torch.full((B, ldd), 9.0, dtype=torch.bfloat16 if variant == 'bf16' else torch.float32, device=DEV)
    out = dict(dlogits=dl, loss_sum=torch.zeros(1, device=DEV), correct=_i32(0), counted=_i32(0))
    (F if variant == 'bf16' else S).softmax_xent_soft(
        x, y, ncls, labels2=labels2, lam=_lam_dev(lam), eps=eps, dlogits=dl, loss_sum=out['loss_sum'],
        correct=out['correct'], counted=out['counted'], grad_scale=grad_scale)
    return out


@pytest.mark.parametrize('padded', [False, True])
@pytest.mark.parametrize('ncls', SR.XENT_NCLS)
@pytest.mark.parametrize('variant', ['bf16', 'f32'])
def test_soft_softmax_xent_matches_fp64(variant, ncls, padded):
    """Every B of R.XENT_B, every (lam, eps) of SR.LAM_EPS, labels2 absent, given, and given with every third
    entry invalid (IGNORE, -1, ncls) where the row's own label may be valid; the padded inputs carry invalid own
    labels on every fourth row.  Bounds: the project's fixed ones through _xent_check (loss per row, fp32
    d(logits) per unit of scale, bf16 d(logits) relative; padding columns and invalid rows exactly zero);
    correct / counted exact.  Where the target holds two labels the hard-label fp64 gradient lies >= 10 bounds
    from the soft one (in both measures), so a kernel that ignored labels2 or lam fails; one that ignored eps is
    off by eps (1 - 1 / ncls) at the label, 5e3 fp32 bounds and >= 5 bf16 bounds.  (The loss is not held to a
    distance: the two losses differ by a signed amount per row, which can cancel over a batch.)  At lam 1, eps 0
    with labels2 given the gradient is the hard kernel's bit for bit."""
    from rafiki_amd.ops import f32 as S, functional as F
    worst = {}
    for B in R.XENT_B:
        logits, labels = R.xent_inputs(B, ncls, padded)
        gs = 1.0 / B
        x, y = logits.to(DEV), labels.to(DEV)
        seconds = {'none': None, 'given': SR.second_labels(labels, ncls, B),
                   'spoiled': SR.second_labels(labels, ncls, B, spoil_only_second=True)}
        hard_ref = R.xent_ref(logits, labels, ncls, grad_scale=gs)['dlogits']
        hard = torch.full((B, logits.shape[1]), 9.0, dtype=torch.bfloat16 if variant == 'bf16' else torch.float32,
                          device=DEV)
        (F if variant == 'bf16' else S).softmax_xent(x, y, ncls, dlogits=hard)
        for which, l2 in seconds.items():
            l2d = None if l2 is None else l2.to(DEV)
            for lam, eps in SR.LAM_EPS:
                tag = 'soft {} B={} ncls={} padded={} labels2={} lam={} eps={}'.format(variant, B, ncls, padded,
                                                                                      which, lam, eps)
                ref = SR.soft_xent_ref(logits, labels, ncls, labels2=l2, lam=lam, eps=eps, grad_scale=gs)
                out = _soft_launch(variant, x, y, ncls, logits.shape[1], labels2=l2d, lam=lam, eps=eps,
                                   grad_scale=None)
                torch.cuda.synchronize()
                got = {k: v.cpu() for k, v in out.items()}
                fig = _xent_check(tag, variant, got, ref, ncls, B, gs)
                print(tag, fig)
                assert int(got['counted'].item()) == ref['counted'], tag
                assert int(got['correct'].item()) == ref['correct'], tag
                for k, v in fig.items():
                    worst[k] = max(worst.get(k, 0.0), v)
                if _mixed(lam, l2, ncls) and ref['counted']:
                    away = (hard_ref - ref['dlogits']).abs().max().item()
                    assert away >= 10 * R.PROB_TOL * gs, (tag, away)
                    assert R.err(hard_ref, ref['dlogits']) >= 10 * R.BF16_REL, tag
                if (lam, eps) == (1.0, 0.0) and which == 'given':
                    assert torch.equal(out['dlogits'], hard), tag
        if padded and B >= 5:
            assert seconds['spoiled'][::3].tolist() != seconds['given'][::3].tolist()
    print('soft softmax {} ncls={} padded={} worst errors {}'.format(variant, ncls, padded, worst))


def test_soft_softmax_xent_refusals():
    """eps outside [0, 1) or NaN is a KernelError from the launcher, and nothing is launched."""
    from rafiki_amd.ops import f32 as S, functional as F
    from rafiki_amd.ops._lib import KernelError
    logits, labels = R.xent_inputs(5, 10, False)
    x, y = logits.to(DEV), labels.to(DEV)
    for mod, dt in ((F, torch.bfloat16), (S, torch.float32)):
        dl = torch.full((5, 10), 9.0, dtype=dt, device=DEV)
        loss = torch.full((1,), 2.5, device=DEV)
        for eps in (-0.01, 1.0, 1.5, float('nan'), float('inf')):
            with pytest.raises(KernelError):
                mod.softmax_xent_soft(x, y, 10, eps=eps, dlogits=dl, loss_sum=loss)
        with pytest.raises(ValueError):
            mod.softmax_xent_soft(x, y, 10, labels2=y[:3], dlogits=dl)
        with pytest.raises(ValueError):
            mod.softmax_xent_soft(x, y, 10, labels2=y, lam=torch.ones(1, dtype=torch.float64, device=DEV), dlogits=dl)
        torch.cuda.synchronize()
        assert bool((dl == 9.0).all()) and loss.item() == 2.5


# ------------------------------------------------------------------------------------------- fused head
@pytest.mark.parametrize('B,D,NC,ncls,gated', SR.HEAD_SHAPES)
def test_soft_head_matches_fp64(B, D, NC, ncls, gated):
    """rk_head_fwd_bwd_soft + rk_head_dw on its output, on the shapes, inputs, error measure and 1e-5 gate of
    tests/test_head_gpu.py, for every (lam, eps) of SR.LAM_EPS with labels2 absent and given.  With B > 2, row 1
    has an invalid own label and row 2 an invalid partner only: both rows give exactly zero.  Discrimination and
    bit identity as in the softmax test (against rk_head_fwd_bwd)."""
    from rafiki_amd.ops import f32 as S
    from rafiki_amd.ops._lib import KernelError
    g = torch.Generator().manual_seed(B + D)
    z = torch.randn(B, D, generator=g)
    if gated:
        z = torch.relu(z)
    w = torch.randn(NC, D, generator=g) * D ** -0.5
    w[ncls:] = 0.0
    b = torch.randn(NC, generator=g) * 0.1
    b[ncls:] = 0.0
    y = torch.randint(0, ncls, (B,), generator=g, dtype=torch.int32)
    y2 = SR.second_labels(y, ncls, B + D)
    if B > 2:
        y[1], y2[1], y2[2] = -1, -1, ncls
    zd, wd, bd, yd = z.to(DEV), w.to(DEV), b.to(DEV), y.to(DEV)
    z64, w64 = z.double(), w.double()
    logits = z64 @ w64.t()[:, :ncls] + b.double()[:ncls]

    def run(soft, **kw):
        out = dict(dlog=torch.full((B, NC), float('nan'), device=DEV), dz=torch.full((B, D), float('nan'), device=DEV),
                   loss=torch.zeros(1, device=DEV), corr=_i32(0), seen=_i32(0),
                   dw=torch.full((NC, D), float('nan'), device=DEV), db=torch.full((NC,), float('nan'), device=DEV),
                   dbh=torch.full((D,), float('nan'), device=DEV))
        (S.head_fwd_bwd_soft if soft else S.head_fwd_bwd)(
            zd, wd, bd, yd, ncls, dlogits=out['dlog'], dz=out['dz'], gated=gated, loss_sum=out['loss'],
            correct=out['corr'], counted=out['seen'], **kw)
        S.head_dw(zd, out['dlog'], out['dz'], dw=out['dw'], db=out['db'], dbh=out['dbh'])
        torch.cuda.synchronize()
        return out

    # the hard kernel takes labels alone, so its rows follow y's validity only
    hard = run(False)
    hard_ref = torch.zeros(B, NC, dtype=torch.float64)
    hard_ref[:, :ncls] = R.xent_ref(logits.float(), y, ncls, grad_scale=1.0 / B)['dlogits']
    for l2 in (None, y2):
        for lam, eps in SR.LAM_EPS:
            tag = (B, D, NC, ncls, l2 is not None, lam, eps)
            ref = SR.soft_xent_ref(logits, y, ncls, labels2=l2, lam=lam, eps=eps, grad_scale=1.0 / B)
            rd = torch.zeros(B, NC, dtype=torch.float64)
            rd[:, :ncls] = ref['dlogits']
            gz = rd @ w64
            if gated:
                gz = gz * (z64 > 0)
            out = run(True, labels2=None if l2 is None else l2.to(DEV), lam=_lam_dev(lam), eps=eps)
            fig = dict(dlog=rel(out['dlog'], rd), dz=rel(out['dz'], gz), dw=rel(out['dw'], rd.t() @ z64),
                       db=rel(out['db'], rd.sum(0)), dbh=rel(out['dbh'], gz.sum(0)))
            counted = max(1, ref['counted'])
            mean = ref['loss_sum'] / counted
            fig['loss'] = abs(out['loss'].item() / counted - mean) / max(1.0, mean)
            print('soft head', tag, fig)
            assert all(v < 1e-5 for v in fig.values()), (tag, fig)
            assert out['corr'].item() == ref['correct'] and out['seen'].item() == ref['counted'], tag
            assert torch.count_nonzero(out['dlog'][:, ncls:]) == 0, tag
            dead = ref['dlogits'].abs().sum(1) == 0
            assert torch.count_nonzero(out['dlog'].cpu()[dead]) == 0 and torch.count_nonzero(out['dz'].cpu()[dead]) == 0
            if B > 2:
                assert bool(dead[1]) and bool(dead[2]) == (l2 is not None)
            if _mixed(lam, l2, ncls):
                assert rel(hard_ref, rd) >= 10 * 1e-5, tag
            if (lam, eps) == (1.0, 0.0) and l2 is not None:
                same = torch.ones(B, dtype=torch.bool) if B <= 2 else ~dead | (SR.valid_labels(y.long(), ncls) == 0)
                assert torch.equal(out['dlog'].cpu()[same], hard['dlog'].cpu()[same]), tag
                assert torch.equal(out['dz'].cpu()[same], hard['dz'].cpu()[same]), tag
    for eps in (-0.01, 1.0, float('nan')):
        dlog = torch.full((B, NC), 9.0, device=DEV)
        with pytest.raises(KernelError):
            S.head_fwd_bwd_soft(zd, wd, bd, yd, ncls, eps=eps, dlogits=dlog, dz=torch.empty(B, D, device=DEV),
                                gated=gated)
        torch.cuda.synchronize()
        assert bool((dlog == 9.0).all())


# ------------------------------------------------------------------------------------------- mixing prologue
# (lam per step) and (box per step) tables: counters 0, 2, 3, 7 walk steps 0, 2, 0, 1, so each pair of tables
# reaches all of its values
LAM_TABLES = ((1.0, 0.0, 0.5), (0.7311, 1.0, 0.0))
BOX_TABLES = (('empty', 'pixel', 'corner'), ('whole', 'past', 'inverted'))
AUGS = (None, (2, 0.5, None), (2, 0.5, 5))      # (pad, flip_p, epoch) of the augmenting variants


def _two_images(fmt, h_sched, ctr, aug):
    """(a, p, ya, yb) of the oracle for step ctr: the primaries, and the partners = the batch rolled by one."""
    big, big_l = _dataset(fmt)
    idx = AR.clamp_rows(h_sched[ctr % AR.NSTEPS], AR.NROWS)
    if aug is None:
        rows = big[4:4 + AR.NROWS].float().numpy()
    else:
        rows = _augmented_rows(fmt, aug[0], aug[1], aug[2])
    lab = big_l[4:4 + AR.NROWS].numpy()
    pr = SR.partner(idx)
    return rows[idx], rows[pr], lab[idx], lab[pr]


@pytest.mark.parametrize('B', [1, 5, 64, 256])
@pytest.mark.parametrize('fmt', list(AR.FORMATS))
def test_gather_batch_mix_direct(fn, fmt, B):
    """rk_gather_batch_mix on its own, laid out as test_gather_batch_aug_direct: data, labels, sched, lr_table,
    lam_table and box_table are views into the middle of sentinel-filled buffers (the table sentinels are valid
    values, the wrong ones), so a wrong row, partner, step or box compares unequal and does not fault.  Plain and
    augmenting (pad 2, flip 0.5, epochs None and 5) gathers; boxes empty, one pixel, touching two borders, the
    whole image, reaching past the image (equal to its clamped form) and inverted (empty): bit-exact.  Blends:
    lam 1 and 0 bit-exact to the unmixed prologue's primaries / partners, else within SR.blend_bound of the fp64
    blend (BLEND_K = 4 fp32 roundings: 1 - lam, the two products, the sum; bf16 storage adds half an ulp)."""
    big, big_l = _dataset(fmt)
    C = big.shape[-1]
    bf16 = big.dtype == torch.bfloat16
    gen = torch.Generator().manual_seed(B)
    big_s = torch.full((2 + AR.NSTEPS + 6, B), 1, dtype=torch.int64)      # sentinel: a valid row, the wrong one
    big_s[2:2 + AR.NSTEPS] = torch.randint(2, AR.NROWS, (AR.NSTEPS, B), generator=gen)
    big_s[2:2 + AR.NSTEPS, 0] = torch.tensor([-1, AR.NROWS, -1])         # outside the dataset: read row 0
    big_s[2 + 1, B - 1] = AR.NROWS + 3
    big_t = torch.full((2 + AR.NSTEPS + 6,), 55.0)
    big_t[2:2 + AR.NSTEPS] = torch.tensor([1.0, 0.25, 0.5])
    big_lam = torch.full((2 + AR.NSTEPS + 6,), 0.25)
    big_box = torch.tensor([1, 2, 1, 2], dtype=torch.int32).repeat(2 + AR.NSTEPS + 6, 1)
    dbig, dl, ds, dt = big.to(DEV), big_l.to(DEV), big_s.to(DEV), big_t.to(DEV)
    dlam, dbox = big_lam.to(DEV), big_box.to(DEV)
    data, labels, sched, table = (_middle(dbig, 4, AR.NROWS), _middle(dl, 4, AR.NROWS), _middle(ds, 2, AR.NSTEPS),
                                  _middle(dt, 2, AR.NSTEPS))
    lam_table, box_table = _middle(dlam, 2, AR.NSTEPS), _middle(dbox, 2, AR.NSTEPS)
    h_sched = big_s[2:2 + AR.NSTEPS].numpy()
    out_x = torch.full((B, AR.H, AR.W, C), 9.0, dtype=big.dtype, device=DEV)
    out_y = torch.full((B,), -9, dtype=torch.int32, device=DEV)
    out_y2 = torch.full((B,), -9, dtype=torch.int32, device=DEV)
    lam_out = torch.full((1,), -1.0, device=DEV)
    big_z = torch.full((37 + 16,), float('nan'), dtype=torch.float64, device=DEV)
    zero = big_z[8:8 + 37]
    lr_out = torch.full((1,), -1.0, device=DEV)
    plain, plain_y = torch.empty_like(out_x), torch.empty_like(out_y)
    worst = 0.0

    def launch(kind, counter, aug, **kw):
        akw = {} if aug is None else dict(pad=aug[0], flip_p=aug[1], seed=AR.SEED, stream_id=AR.STREAM,
                                          epoch=None if aug[2] is None else _i32(aug[2]))
        fn.gather_batch_mix(data, labels, sched, counter, out_x, out_y, kind=kind, lam_table=lam_table,
                            box_table=box_table, out_y2=out_y2, lam_out=lam_out, **akw, **kw)
        torch.cuda.synchronize()

    def unmixed(counter, aug):
        if aug is None:
            fn.gather_batch(data, labels, sched, counter, plain, plain_y)
        else:
            fn.gather_batch_aug(data, labels, sched, counter, plain, plain_y, pad=aug[0], flip_p=aug[1], seed=AR.SEED,
                                stream_id=AR.STREAM, epoch=None if aug[2] is None else _i32(aug[2]))
        torch.cuda.synchronize()
        return plain

    for aug in AUGS:
        for kind, tables in (('mixup', LAM_TABLES), ('cutmix', BOX_TABLES)):
            for row in tables:
                if kind == 'mixup':
                    lam_table.copy_(torch.tensor(row))
                    boxes = [None] * 3
                else:
                    boxes = [SR.BOXES[n] for n in row]
                    box_table.copy_(torch.tensor(boxes, dtype=torch.int32))
                    lam_table.copy_(torch.tensor([0.75, 0.5, 0.125]))
                lams = lam_table.cpu().tolist()
                for ctr in (0, 2, 3, 7):        # 3 and 7 wrap to 0 and 1
                    s = ctr % AR.NSTEPS
                    counter = _i32(ctr)
                    out_x.fill_(9.0)
                    out_y.fill_(-9)
                    out_y2.fill_(-9)
                    lam_out.fill_(-1.0)
                    zero.fill_(float('nan'))
                    lr_out.fill_(-1.0)
                    launch(kind, counter, aug, zero=zero, lr_table=table, lr_out=lr_out)
                    a, p, ya, yb = _two_images(fmt, h_sched, ctr, aug)
                    what = (aug, kind, row, ctr)
                    got = out_x.float().cpu().numpy()
                    if kind == 'cutmix':
                        assert np.array_equal(got, SR.box_mix(a, p, boxes[s])), what
                        assert np.array_equal(got, SR.box_mix(a, p, SR.clamp_box(boxes[s], AR.H, AR.W))), what
                    elif lams[s] in (1.0, 0.0):
                        assert np.array_equal(got, a if lams[s] == 1.0 else p), what
                        um = unmixed(counter, aug)
                        assert torch.equal(out_x, um if lams[s] == 1.0 or B == 1 else um.roll(-1, 0)), what
                    else:
                        ref = SR.blend_mix(a, p, lams[s])
                        over = np.abs(got - ref) / SR.blend_bound(a, p, ref, bf16).clip(1e-300)
                        worst = max(worst, float(over.max()))
                        assert over.max() <= 1.0, (what, over.max())
                        if B > 1:
                            assert not np.array_equal(got, a) and not np.array_equal(got, p)
                    assert np.array_equal(out_y.cpu().numpy(), ya) and np.array_equal(out_y2.cpu().numpy(), yb), what
                    assert lam_out.item() == lams[s], what
                    assert lr_out.item() == big_t[2 + s].item(), what
                    assert int(counter.item()) == ctr      # no `done`: the counter is the caller's to advance
                    assert torch.count_nonzero(big_z[8:45]) == 0 and bool(big_z[:8].isnan().all()) and \
                        bool(big_z[45:].isnan().all())
    print('mix prologue {} B={} worst blend error / bound {:.3f}'.format(fmt, B, worst))
    # with `done` the last block advances the counter: three launches walk steps 1, 2, 0
    aug = AUGS[2]
    box_table.copy_(torch.tensor([SR.BOXES[n] for n in BOX_TABLES[0]], dtype=torch.int32))
    counter, done = _i32(1), _i32(0)
    lr_out.fill_(-1.0)
    for k in range(3):
        launch('cutmix', counter, aug, done=done)
        a, p, ya, yb = _two_images(fmt, h_sched, 1 + k, aug)
        assert np.array_equal(out_x.float().cpu().numpy(), SR.box_mix(a, p, SR.BOXES[BOX_TABLES[0][(1 + k) % 3]]))
        assert np.array_equal(out_y.cpu().numpy(), ya) and np.array_equal(out_y2.cpu().numpy(), yb)
        assert int(counter.item()) == 2 + k and int(done.item()) == 0
    assert lr_out.item() == -1.0                                  # no table: lr_out is left alone
    # a lam outside [0, 1] or NaN is clamped into it (NaN to 0) before it reaches the blend and the loss
    lam_table.copy_(torch.tensor([1.5, -0.5, float('nan')]))
    for ctr, want in ((0, 1.0), (1, 0.0), (2, 0.0)):
        launch('mixup', _i32(ctr), None)
        a, p, _, _ = _two_images(fmt, h_sched, ctr, None)
        assert lam_out.item() == want and np.array_equal(out_x.float().cpu().numpy(), a if want == 1.0 else p)
    lam_table.copy_(torch.tensor([0.75, 0.5, 0.125]))
    box_table.copy_(torch.tensor([SR.BOXES[n] for n in BOX_TABLES[1]], dtype=torch.int32))
    big_lam[2:2 + AR.NSTEPS] = torch.tensor([0.75, 0.5, 0.125])
    big_box[2:2 + AR.NSTEPS] = torch.tensor([SR.BOXES[n] for n in BOX_TABLES[1]], dtype=torch.int32)
    assert torch.equal(dbig.cpu(), big) and torch.equal(ds.cpu(), big_s)
    assert torch.equal(dl.cpu(), big_l) and torch.equal(dt.cpu(), big_t)
    assert torch.equal(dlam.cpu(), big_lam) and torch.equal(dbox.cpu(), big_box)


def test_gather_batch_mix_refusals(fn):
    """Null tables or outputs, an unknown kind, a bad geometry or probability: a KernelError (a short table: a
    ValueError from the wrapper) and nothing launched — the outputs keep their fill."""
    from rafiki_amd.ops import _lib
    from rafiki_amd.ops._lib import KernelError
    B = 4
    data = torch.randn(8, AR.H, AR.W, 8, device=DEV)
    labels = torch.zeros(8, dtype=torch.int32, device=DEV)
    sched = torch.zeros((2, B), dtype=torch.int64, device=DEV)
    out_x = torch.full((B, AR.H, AR.W, 8), 9.0, device=DEV)
    out_y = torch.full((B,), -9, dtype=torch.int32, device=DEV)
    out_y2 = torch.full((B,), -9, dtype=torch.int32, device=DEV)
    lam_out = torch.full((1,), -1.0, device=DEV)
    counter = _i32(0)
    ok = dict(kind='cutmix', lam_table=torch.ones(2, device=DEV),
              box_table=torch.zeros((2, 4), dtype=torch.int32, device=DEV), out_y2=out_y2, lam_out=lam_out)
    aug = dict(pad=2, flip_p=0.5, seed=1, stream_id=2)
    bad = [dict(ok, lam_table=None), dict(ok, box_table=None), dict(ok, out_y2=None), dict(ok, lam_out=None),
           dict(ok, **dict(aug, pad=AR.H)), dict(ok, **dict(aug, pad=-1)), dict(ok, **dict(aug, flip_p=1.01)),
           dict(ok, **dict(aug, flip_p=float('nan')))]
    for kw in bad:
        with pytest.raises(KernelError):
            fn.gather_batch_mix(data, labels, sched, counter, out_x, out_y, **kw)
    with pytest.raises(KernelError):
        fn.gather_batch_mix(data, None, sched, counter, out_x, out_y, **ok)
    with pytest.raises(KernelError):
        fn.gather_batch_mix(data, labels, sched, counter, out_x, None, **ok)
    for kw in (dict(ok, lam_table=torch.ones(1, device=DEV)),
               dict(ok, box_table=torch.zeros((1, 4), dtype=torch.int32, device=DEV)),
               dict(ok, lam_table=torch.ones(2, dtype=torch.float64, device=DEV)),
               dict(ok, out_y2=out_y2[:2])):
        with pytest.raises(ValueError):
            fn.gather_batch_mix(data, labels, sched, counter, out_x, out_y, **kw)
    with pytest.raises(ValueError):
        fn.gather_batch_mix(data, labels, sched, counter, out_x, out_y, **dict(ok, kind='cutout'))
    # a row that is no whole number of 16-byte pixel vectors: 6 fp32 channels = 24 bytes a pixel
    data6 = torch.randn(8, AR.H, AR.W, 6, device=DEV)
    out6 = torch.full((B, AR.H, AR.W, 6), 9.0, device=DEV)
    with pytest.raises(KernelError):
        fn.gather_batch_mix(data6, labels, sched, counter, out6, out_y, **ok)
    # and the entry point itself: a row size that is not 16 * H * W * vpp, an unknown kind, a pad without augment
    p = lambda t: t.data_ptr()      # noqa: E731
    rb = 16 * AR.H * AR.W * 2
    for row_bytes, H, W, vpp, augment, pad, kind in ((rb - 16, AR.H, AR.W, 2, 1, 2, 2), (rb, AR.W, AR.W, 2, 1, 2, 2),
                                                     (rb, AR.H, AR.W, 1, 1, 2, 2), (0, 0, AR.W, 2, 1, 2, 2),
                                                     (rb, AR.H, AR.W, 2, 1, 2, 0), (rb, AR.H, AR.W, 2, 1, 2, 3),
                                                     (rb, AR.H, AR.W, 2, 0, 2, 2)):
        with pytest.raises(KernelError):
            _lib.call('rk_gather_batch_mix', p(data), row_bytes, p(labels), p(sched), p(counter), B, p(out_x),
                      p(out_y), None, 0, None, None, None, 2, 8, H, W, vpp, augment, pad, 0.5 if augment else 0.0, 1,
                      2, None, kind, 0, p(ok['lam_table']), p(ok['box_table']), p(out_y2), p(lam_out),
                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((out_x == 9.0).all()) and bool((out6 == 9.0).all()) and bool((out_y == -9).all())
    assert bool((out_y2 == -9).all()) and lam_out.item() == -1.0
    fn.gather_batch_mix(data, labels, sched, counter, out_x, out_y, **ok, **aug)      # the same call, supported
    torch.cuda.synchronize()
    assert not bool((out_x == 9.0).any()) and bool((out_y == 0).all()) and bool((out_y2 == 0).all())
    assert lam_out.item() == 1.0


# ------------------------------------------------------------------------------------------- the engine
def _oracle_batch(data, labels, rows, kind, lam, box, epoch, seed, augment):
    """(x fp64-or-exact, y, y2) of one mixed batch through the oracles alone."""
    from rafiki_amd.ops.augment import AUG_STREAM
    host = data.float().numpy()
    pr = SR.partner(rows)
    if augment is None:
        a, p = host[rows], host[pr]
    else:
        a = AR.crop(host, rows, *AR.draws(seed, rows, epoch, augment['pad'], augment['flip'], AUG_STREAM))
        p = AR.crop(host, pr, *AR.draws(seed, pr, epoch, augment['pad'], augment['flip'], AUG_STREAM))
    lab = labels.numpy()
    x = SR.box_mix(a, p, box) if kind == 'cutmix' else SR.blend_mix(a, p, lam)
    return a, p, x, lab[rows], lab[pr]


@pytest.mark.parametrize('kind', ['mixup', 'cutmix'])
@pytest.mark.parametrize('dtype', ['bf16', 'fp32'])
def test_scheduled_graph_mixes_per_step_and_epoch(dtype, kind):
    """Two epochs of three replays of the captured step with mix on top of augment = pad 2, flip 0.5 and label
    smoothing: after every replay the static batch, y, y2 and lam are the oracle's for that step's plan row and
    that epoch; the plans of the two epochs differ.  mix_batch gives the same batch on the GPU and on a CPU
    engine of the same seed."""
    from rafiki_amd.engine.convnet import ConvNetEngine
    from rafiki_amd.ops import mix as M
    steps, B, n = 3, 32, 96
    augment = {'pad': 2, 'flip': 0.5}
    mix = {'kind': kind, 'alpha': 1.0, 'prob': 1.0}
    eng = _engine(dtype, augment=augment, mix=mix, label_smoothing=0.1)
    data, labels = _engine_data(eng)
    ddata, dlabels = data.to(DEV), labels.to(DEV)
    idx = torch.randint(0, n, (steps, B), generator=torch.Generator().manual_seed(1))
    eng.capture_scheduled(ddata, dlabels, steps, B)
    batches, plans = {}, {}
    for epoch in (0, 1):
        eng.set_schedule(idx.to(DEV), epoch=epoch)
        lam, box = plans[epoch] = M.plan(3, epoch, steps, kind, 1.0, 1.0, 16, 16)
        for s in range(steps):
            eng.replay()
            torch.cuda.synchronize()
            a, p, ref, ya, yb = _oracle_batch(data, labels, idx[s].numpy(), kind, lam[s], box[s], epoch, 3, augment)
            got = eng._static_x.float().cpu().numpy()
            if kind == 'cutmix':
                assert np.array_equal(got, ref), (epoch, s)
            else:
                assert (np.abs(got - ref) <= SR.blend_bound(a, p, ref, dtype == 'bf16')).all(), (epoch, s)
            assert np.array_equal(eng._static_y.cpu().numpy(), ya), (epoch, s)
            assert np.array_equal(eng._static_y2.cpu().numpy(), yb), (epoch, s)
            assert eng._lam.item() == lam[s], (epoch, s)
            batches[epoch, s] = eng._static_x.clone()
        assert int(eng._ctr.item()) == steps
        assert float(eng.loss_sum.item()) > 0 and bool(eng.flat.master.isfinite().all())
    assert not np.array_equal(plans[0][0], plans[1][0])
    assert all(not torch.equal(batches[0, s], batches[1, s]) for s in range(steps))
    cpu = ConvNetEngine(num_classes=10, in_channels=3, image_size=16, cfg=(16, 'M', 32, 32, 'M'), fc_dims=(32,),
                        device='cpu', seed=3, dtype=dtype, augment=augment, mix=mix, label_smoothing=0.1)
    for epoch in (0, 1):
        out = torch.full(eng.input_shape(B), 9.0, dtype=eng.act_dtype, device=DEV)
        oy = torch.full((B,), -9, dtype=torch.int32, device=DEV)
        eng.mix_batch(ddata, dlabels, idx[1].to(DEV), epoch, 1, out, oy)
        torch.cuda.synchronize()
        host = torch.full(cpu.input_shape(B), 9.0, dtype=data.dtype)
        hy = torch.full((B,), -9, dtype=torch.int32)
        cpu.mix_batch(data, labels, idx[1], epoch, 1, host, hy)
        assert torch.equal(out.cpu(), host) and torch.equal(oy.cpu(), hy)
        assert torch.equal(eng._static_y2.cpu(), cpu._static_y2) and eng._lam.item() == cpu._lam.item()
        assert torch.equal(out, batches[epoch, 1])


@pytest.mark.parametrize('kind', ['mixup', 'cutmix'])
@pytest.mark.parametrize('dtype', ['bf16', 'fp32'])
def test_unmixed_plan_trains_like_no_mix(dtype, kind):
    """mix with prob 0 (every lam 1, every box empty) and label_smoothing 0 runs the mixing prologue and the soft
    loss kernels and leaves, after three replays from the same seed, the master weights of an engine built
    without either, bit for bit."""
    steps, B = 3, 32
    masters = []
    for mix in (None, {'kind': kind, 'alpha': 1.0, 'prob': 0.0}):
        eng = _engine(dtype, mix=mix, label_smoothing=0.0)
        assert eng.soft == (mix is not None)
        data, labels = _engine_data(eng)
        idx = torch.randint(0, 96, (steps, B), generator=torch.Generator().manual_seed(1)).to(DEV)
        eng.capture_scheduled(data.to(DEV), labels.to(DEV), steps, B)
        eng.set_schedule(idx, lr_scales=R.LR_SCALES[:steps], epoch=4)
        for _ in range(steps):
            eng.replay()
        torch.cuda.synchronize()
        masters.append(eng.flat.master.clone())
        assert (eng._lam_table is None) == (mix is None)
        if mix is not None:
            assert bool((eng._lam_table == 1.0).all()) and not bool(eng._box_table.any()) and eng._lam.item() == 1.0
    assert torch.equal(masters[0], masters[1])
    assert bool(masters[0].isfinite().all())


@pytest.mark.parametrize('num_classes', [10, 40])
@pytest.mark.parametrize('kind', ['mixup', 'cutmix'])
def test_soft_gradient_matches_fp64_autograd(kind, num_classes):
    """fp32 engine, mix and smoothing on: after mix_batch + forward_backward the flat gradient is torch.autograd's
    through reference_loss in fp64 with the same labels2 / lam / smoothing, per parameter within the bound
    tests/test_engine_gpu.py::test_grads_match_reference holds the hard-label gradient to (relative Frobenius
    error < 0.12, cosine > 0.99; loss within 1e-2).  10 classes take the fused soft head (ncls_p 16), 40 classes
    (ncls_p 40, outside HEAD_NC) the unfused soft softmax."""
    from rafiki_amd.ops import f32 as S
    B = 64
    eng = _engine('fp32', num_classes=num_classes, mix={'kind': kind, 'alpha': 1.0, 'prob': 1.0},
                  label_smoothing=0.1)
    assert S.head_ok(eng.ncls_p, eng.d_last) == (num_classes == 10)
    data, _ = _engine_data(eng)
    labels = torch.randint(0, num_classes, (96,), generator=torch.Generator().manual_seed(2), dtype=torch.int32)
    idx = torch.randperm(96, generator=torch.Generator().manual_seed(1))[:B]
    x = torch.empty(eng.input_shape(B), device=DEV)
    y = torch.empty((B,), dtype=torch.int32, device=DEV)
    eng.mix_batch(data.to(DEV), labels.to(DEV), idx.to(DEV), 0, 2, x, y)
    eng.forward_backward(x, y)
    torch.cuda.synchronize()
    lam, y2 = eng._lam.item(), eng._static_y2.cpu()
    assert 0.0 < lam < 1.0 and not torch.equal(y2, y.cpu())
    fl = eng.flat
    params = {n: fl.w(n).detach().double().cpu().requires_grad_(True) for n in fl.names()}
    cpu = _engine('fp32', num_classes=num_classes, device='cpu')
    loss, _ = cpu.reference_loss(x.double().cpu(), y.cpu(), params, training=True, labels2=y2, lam=lam,
                                 smoothing=0.1)
    grads = torch.autograd.grad(loss, [params[n] for n in fl.names()])
    assert abs(eng.loss_sum.item() / B - loss.item()) < 1e-2 * max(1.0, loss.item())
    assert int(eng.seen.item()) == B
    for n, g in zip(fl.names(), grads):
        got = fl.g(n).double().cpu()
        fro = ((got - g).norm() / g.norm().clamp_min(1e-12)).item()
        cos = torch.nn.functional.cosine_similarity(got.flatten(), g.flatten(), 0).item()
        print('soft-grad-vs-fp64', kind, num_classes, n, fro, cos)
        assert fro < 0.12 and cos > 0.99, (n, fro, cos)


# ------------------------------------------------------------------------------------------- the model loops
@pytest.mark.parametrize('optimizer', ['sgd', 'adam'])
def test_model_loops_mix_their_batches(optimizer, monkeypatch):
    """NativeImageClassifier.train on the GPU, two epochs: the scheduled graph (SGD) and the captured step fed by
    mix_batch (Adam) both train on the twin's batches for each epoch's permutation and plan; evaluate takes no
    training step."""
    from rafiki_amd.engine.convnet import ConvNetEngine
    from rafiki_amd.models.image_classifier import NativeImageClassifier
    from rafiki_amd.ops import mix as M
    from rafiki_amd.parallel.context import TrialContext, use_context

    class Tiny(NativeImageClassifier):
        DEFAULT_IMAGE_SIZE = 16

        def _engine_kwargs(self, num_classes, channels, image_size):
            return dict(cfg=(16, 'M', 32, 32, 'M'), fc_dims=(32,), optimizer=optimizer, lr=1e-3, weight_decay=0.0)

    seen = []
    replay, step_graph = ConvNetEngine.replay, ConvNetEngine.step_graph

    def rec_replay(self):
        replay(self)
        seen.append((self._static_x.clone(), self._static_y.clone(), self._static_y2.clone(), self._lam.item()))

    def rec_step_graph(self, x, labels):
        seen.append((x.clone(), labels.clone(), self._static_y2.clone(), self._lam.item()))
        step_graph(self, x, labels)
    monkeypatch.setattr(ConvNetEngine, 'replay', rec_replay)
    monkeypatch.setattr(ConvNetEngine, 'step_graph', rec_step_graph)
    uri = 'synthetic://image?n=128&size=16&channels=3&classes=10&seed=0'
    with use_context(TrialContext(device=torch.device(DEV))):
        m = Tiny(epochs=2, batch_size=32, image_size=16, augment='crop_flip', augment_pad=3, mix='cutmix',
                 mix_prob=1.0, label_smoothing=0.1, seed=9)
        m.train(uri)
        eng = m._engine
        assert (eng._sched_graph if optimizer == 'sgd' else eng._graph) is not None
        assert eng.mix == {'kind': 'cutmix', 'alpha': 1.0, 'prob': 1.0} and eng.label_smoothing == 0.1
        assert len(seen) == 8
        images, labels, _ = m._load(uri)
        x_all = eng.prepare_inputs(images).cpu()
        y_all = torch.from_numpy(np.asarray(labels, dtype=np.int32))
        gen = torch.Generator(device=DEV).manual_seed(9)
        for epoch in (0, 1):
            perm = torch.randperm(128, device=DEV, generator=gen).cpu()
            lam, box = M.plan(9, epoch, 4, 'cutmix', 1.0, 1.0, 16, 16)
            for b in range(4):
                idx = perm[b * 32:(b + 1) * 32]
                ref = M.apply(x_all, idx, 'cutmix', lam[b], box[b], augment={'pad': 3, 'flip': 0.5}, seed=9,
                              epoch=epoch)
                x, y, y2, got_lam = seen[4 * epoch + b]
                assert torch.equal(x.cpu(), ref), (epoch, b)
                assert torch.equal(y.cpu(), y_all[idx]) and torch.equal(y2.cpu(), y_all[idx.roll(-1)]), (epoch, b)
                assert got_lam == lam[b], (epoch, b)
        assert isinstance(m.evaluate(uri), float)
        assert len(seen) == 8
        m.destroy()
