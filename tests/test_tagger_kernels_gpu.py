"""The entry points of csrc/kernels/tagger.hip (rk_tag_embed_fwd, rk_tag_embed_bwd, rk_tag_transpose,
rk_tag_add) and csrc/kernels/embed.hip (rk_embedding_fwd, rk_embedding_bwd, rk_embedding_bwd_ws), called raw
through _lib.call, against the references of tests/lstm_refs.py, which go through no kernel of this project.

These kernels move data, multiply by a dropout multiplier or sum rows in a fixed order, so the checks are
bit for bit: the dropout mask against the NumPy Philox twin of tests/loss_optim_refs.py, the embedding
gradients against a sequential fp32 sum in ascending token order (and against the fp64 index_add at
4 x that sum's own error), and rows that no token touches against the sentinel the output was prefilled with.
"""
import numpy as np
import pytest
import torch

import lstm_refs as L

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = 7.5


@pytest.fixture(scope='module')
def call():
    from rafiki_amd.ops import _lib
    _lib.lib()  # loud failure if the native library is missing
    return _lib.call


@pytest.fixture(scope='module')
def KernelError():
    from rafiki_amd.ops._lib import KernelError
    return KernelError


def _p(t):
    return None if t is None else t.data_ptr()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------- rk_tag_embed_fwd
def _tag_embed_fwd(call, ids, w, p, seed=0, step=None, with_mask=True, E=None):
    n, (V, EP) = len(ids), w.shape
    out = torch.full((n, EP), SENTINEL, device=DEV)
    mask = torch.full((n, EP), SENTINEL, device=DEV) if with_mask else None
    st = None if step is None else torch.tensor([step], dtype=torch.int32, device=DEV)
    ids_d, w_d = torch.as_tensor(ids, dtype=torch.int32).to(DEV), w.to(DEV)
    call('rk_tag_embed_fwd', _p(ids_d), _p(w_d), _p(out), _p(mask), n, EP if E is None else E, V, p, seed,
         L.DROP_STREAM, _p(st), _s())
    torch.cuda.synchronize()
    return out.cpu(), None if mask is None else mask.cpu()


@pytest.mark.parametrize('n,EP', [(1, 4), (51, 20), (257, 4)])     # n * EP / 4 = 1, 255, 257 threads
def test_tag_embed_fwd_mask_is_the_philox_stream(call, n, EP):
    V = 11
    g = _gen(n)
    w = torch.randn((V, EP), generator=g)
    ids = torch.randint(0, V, (n,), generator=g).tolist()
    for seed in L.PHILOX_SEEDS:
        for step in (None, 0, 5):
            for p in (0.3, 0.5):
                out, mask = _tag_embed_fwd(call, ids, w, p, seed, step)
                want = L.dropout_mask_ref(n, EP, p, seed, step)
                assert _bits_equal(mask, want), (seed, step, p)
                assert _bits_equal(out, L.embed_ref(w, ids) * want), (seed, step, p)
    # the step and the seed's high word reach the counter and the key
    a, b = L.dropout_mask_ref(257, 4, 0.5, L.PHILOX_SEEDS[0], 0), L.dropout_mask_ref(257, 4, 0.5, L.PHILOX_SEEDS[0], 5)
    c = L.dropout_mask_ref(257, 4, 0.5, L.PHILOX_SEEDS[0] & 0xFFFFFFFF, 0)
    assert not torch.equal(a, b) and not torch.equal(a, c)


def test_tag_embed_fwd_plain_gather_and_id_clamp(call):
    V, EP = 7, 8
    w = torch.randn((V, EP), generator=_gen(0)) + 3.0         # row 0 is not zero here: a clamp is visible
    ids = [0, 6, -1, V, 3, 3, 2 ** 31 - 1, -2 ** 31]
    out, _ = _tag_embed_fwd(call, ids, w, 0.0, with_mask=False)
    assert _bits_equal(out, L.embed_ref(w, ids))
    assert _bits_equal(out[2], w[0]) and _bits_equal(out[3], w[0])
    # p = 0 with a mask buffer: still a plain gather, the buffer is left alone
    out, mask = _tag_embed_fwd(call, ids, w, 0.0)
    assert _bits_equal(out, L.embed_ref(w, ids)) and (mask == SENTINEL).all()


def test_tag_embed_fwd_refusals(call, KernelError):
    w = torch.randn((5, 8), generator=_gen(1))
    for kw in (dict(p=0.0, E=6), dict(p=1.0), dict(p=-0.1), dict(p=0.3, with_mask=False)):
        with pytest.raises(KernelError):
            _tag_embed_fwd(call, [1, 2, 3], w, **kw)


# ------------------------------------------------------------------------------------------- rk_tag_embed_bwd
def _tag_batch():
    """[B, L] ids over V = 16: the padding id 0, a run of one token (5), a run of 70 (3), ids that never occur."""
    B, Ln, V = 10, 12, 16
    rng = np.random.default_rng(5)
    x = rng.choice([0, 1, 2, 7, 9, 15], size=(B, Ln))
    flat = x.reshape(-1)
    flat[rng.permutation(B * Ln)[:70]] = 3
    assert (flat == 3).sum() == 70
    flat[np.flatnonzero(flat != 3)[4]] = 5
    return x, V


@pytest.mark.parametrize('p', [0.0, 0.5])
@pytest.mark.parametrize('E', [4, 68])
def test_tag_embed_bwd_ordered_run_sums(call, E, p):
    from rafiki_amd.engine.tagger import pack_batch
    x, V = _tag_batch()
    n = x.size
    buf = pack_batch(x, None, 0, V)
    f = L.unpack(buf, n)
    assert f['nruns'] < n and -1 in f['uniq'] and 1 in np.diff(f['starts']) and 70 in np.diff(f['starts'])
    dy = torch.randn((n, E), generator=_gen(E))
    mask = L.dropout_mask_ref(n, E, p, 99, 2) if p > 0 else None
    dbuf = torch.from_numpy(buf).to(DEV)
    dw = torch.full((V, E), SENTINEL, device=DEV)
    dy_d, mask_d = dy.to(DEV), None if mask is None else mask.to(DEV)
    call('rk_tag_embed_bwd', _p(dbuf[2 * n:]), _p(dbuf[3 * n:]), _p(dbuf[4 * n:]), _p(dbuf[5 * n + 1:]), _p(dy_d),
         _p(mask_d), _p(dw), n, E, V, _s())      # maxruns = n > the run count
    torch.cuda.synchronize()
    dw = dw.cpu()
    seq = L.embed_bwd_seq32(f['ids'], dy, torch.full((V, E), SENTINEL), mask, skip=0)
    assert _bits_equal(dw, seq)
    used = sorted(set(f['ids']) - {0})
    rest = [v for v in range(V) if v not in used]
    assert 0 in rest and len(rest) > 1 and (dw[rest] == SENTINEL).all()
    ref = L.embed_bwd_ref(f['ids'], dy, V, mask, skip=0)
    e, tol = L.err(dw[used], ref[used]), L.TOL_FACTOR * L.err(seq[used], ref[used])
    print('tag_embed_bwd E={} p={}: err {:.3e}  tolerance {:.3e}'.format(E, p, e, tol))
    assert e <= tol


# ------------------------------------------------------------------------------------------- embed.hip
def _embedding_bwd(call, ids, dy, V, padding_idx, short=0):
    from rafiki_amd.ops import _lib
    n, E = dy.shape
    nbytes = int(_lib.lib().rk_embedding_bwd_ws(n))
    assert nbytes >= 16 * n + 256
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    dw = torch.full((V, E), SENTINEL, device=DEV)
    ids_d, dy_d = torch.as_tensor(ids, dtype=torch.int64).to(DEV), dy.to(DEV)
    call('rk_embedding_bwd', _p(ids_d), _p(dy_d), _p(dw), n, V, E, padding_idx, _p(ws), nbytes - short, _s())
    torch.cuda.synchronize()
    return dw.cpu()


@pytest.mark.parametrize('V', [1, 32, 33])       # the radix sort's bit count: 1, 5, 6
def test_embedding_bwd_ordered_run_sums(call, V):
    n, E = 200, 8
    g = _gen(V)
    ids = torch.randint(0, V, (n,), generator=g).tolist()
    if V > 1:
        ids = [v if v != 4 else 5 for v in ids]          # row 4: no token
        ids[7], ids[100], ids[150] = -3, V, V + 2          # out of range: row 0, like the forward's clamp
        ids[9] = V - 1
    dy = torch.randn((n, E), generator=g)
    cl = L.clamp_ids(ids, V).tolist()
    for pad in (-1, 0):
        dw = _embedding_bwd(call, ids, dy, V, pad)
        seq = L.embed_bwd_seq32(cl, dy, torch.zeros((V, E)), skip=None if pad < 0 else pad)
        assert _bits_equal(dw, seq), pad                  # every row written: zero where no token (or padding)
        ref = L.embed_bwd_ref(cl, dy, V, skip=None if pad < 0 else pad)
        assert L.err(dw, ref) <= L.TOL_FACTOR * L.err(seq, ref)
        if pad == 0:
            assert (dw[0] == 0).all()
        else:
            assert dw[0].abs().min() > 0
        if V > 1:
            assert (dw[4] == 0).all() and dw[V - 1].abs().min() > 0


def test_embedding_bwd_refusals(call, KernelError):
    dy = torch.randn((10, 8), generator=_gen(3))
    with pytest.raises(KernelError):
        _embedding_bwd(call, [1] * 10, dy, 4, -1, short=1)       # a workspace one byte short
    with pytest.raises(KernelError):
        _embedding_bwd(call, [1] * 10, dy[:, :6].contiguous(), 4, -1)


def test_embedding_fwd_gather(call, KernelError):
    V, E = 9, 12
    w = torch.randn((V, E), generator=_gen(4)) + 3.0
    w_d = w.to(DEV)
    for n in (1, 85, 86):                                         # n * E / 4 = 3, 255, 258 threads
        ids = torch.randint(0, V, (n,), generator=_gen(n)).tolist()
        ids[0] = -1
        ids[-1] = V if n > 1 else -1
        out = torch.full((n, E), SENTINEL, device=DEV)
        ids_d = torch.tensor(ids, dtype=torch.int64).to(DEV)
        call('rk_embedding_fwd', _p(ids_d), _p(w_d), _p(out), n, E, V, _s())
        torch.cuda.synchronize()
        assert _bits_equal(out, L.embed_ref(w, ids))
    out, ids_d = torch.full((2, 6), SENTINEL, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV)
    with pytest.raises(KernelError):
        call('rk_embedding_fwd', _p(ids_d), _p(w_d), _p(out), 2, 6, V, _s())


# ------------------------------------------------------------------------------------------- transpose, add
@pytest.mark.parametrize('G,R,C', [(2, 256, 64), (2, 512, 128), (3, 33, 31), (1, 1, 1)])
def test_tag_transpose(call, G, R, C):
    src = torch.randn((G, R, C), generator=_gen(R))
    dst = torch.full((G * R * C + 64,), SENTINEL, device=DEV)
    src_d = src.to(DEV)
    call('rk_tag_transpose', _p(src_d), _p(dst), G, R, C, _s())
    torch.cuda.synchronize()
    dst = dst.cpu()
    assert _bits_equal(dst[:G * R * C].view(G, C, R), src.transpose(1, 2).contiguous())
    assert (dst[G * R * C:] == SENTINEL).all()


@pytest.mark.parametrize('n', [1, 255, 257, 1025])
def test_tag_add(call, n):
    a, b = torch.randn(n, generator=_gen(n)), torch.randn(n, generator=_gen(n + 1))
    a_d, b_d = a.to(DEV), b.to(DEV)
    for bb, want in ((b, a + b), (None, a)):
        out = torch.full((n + 64,), SENTINEL, device=DEV)
        call('rk_tag_add', _p(a_d), _p(None if bb is None else b_d), _p(out), n, _s())
        torch.cuda.synchronize()
        out = out.cpu()
        assert _bits_equal(out[:n], want) and (out[n:] == SENTINEL).all()
    out = torch.full((64,), SENTINEL, device=DEV)
    call('rk_tag_add', _p(a_d), _p(b_d), _p(out), 0, _s())
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
