"""The CRF kernels (crf.hip), alone, in the tagger engine and in PyBiLstmCrf, against the torch Crf in fp64 (CPU)."""
import numpy as np
import pytest
import torch

from rafiki_amd.ops.crf import Crf
from rafiki_amd.ops import _lib
from rafiki_amd.ops.functional import _p, _s
from rafiki_amd.engine.tagger import TaggerEngine
from test_tagger_gpu import DEV, Net, _batch as _token_batch, _rel   # the tagger tests' net, batch maker, error measure

pytestmark = pytest.mark.gpu
# (NT, B, L, scale, a length-0 sentence): pad lanes and a partly filled block; a full wave; no transition; tiny; one
# tag; scores x 8 (path sums leave the fp32 range without the rescaling); a length-0 sentence
CASES = [(45, 5, 7, 1, False), (64, 33, 4, 1, False), (7, 3, 1, 1, False), (3, 1, 2, 1, False), (1, 3, 5, 1, False),
         (17, 9, 11, 8, False), (12, 6, 5, 1, True)]
LONG = [(5, 2, 256, 1, False), (5, 2, 257, 1, False)]   # Viterbi: the last L with backpointers in LDS, the first beyond


def _batch(NT, B, L, scale, zero):
    """An fp64 Crf with random fp32-exact scores, [B, L, NT] logits, tags, lens (one at full length, one 0 if ``zero``),
    and the kernels' device operands: padded time-major logits, trans, start, end, int32 lens, the workspace."""
    g = torch.Generator().manual_seed(NT * 1000 + B * 10 + L)
    crf = Crf(NT).double()
    for p in crf.parameters():
        p.data = (torch.randn(p.shape, generator=g) * scale).double()
    logits = (torch.randn(B, L, NT, generator=g) * scale).double()
    tags = torch.randint(0, NT, (B, L), generator=g)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[0] = L
    if zero:
        lens[2] = 0
    NTP = -(-NT // 4) * 4
    lg, tr, st, en = torch.zeros(L, B, NTP), torch.zeros(NTP, NTP), torch.zeros(NTP), torch.zeros(NTP)
    lg[:, :, :NT], tr[:NT, :NT], st[:NT], en[:NT] = logits.transpose(0, 1), crf.trans.data, crf.start.data, crf.end.data
    ws = torch.empty(int(_lib.lib().rk_crf_ws_bytes(L, B, NT)), dtype=torch.uint8, device=DEV)
    return crf, logits, tags, lens, [t.to(DEV) for t in (lg, tr, st, en, lens.int())] + [ws]


@pytest.mark.parametrize("NT,B,L,scale,zero", CASES)
def test_crf_nll_kernel_matches_fp64(NT, B, L, scale, zero):
    crf, logits, tags, lens, (lg, tr, st, en, dlens, ws) = _batch(NT, B, L, scale, zero)
    logits.requires_grad_()
    loss = crf.nll(logits, tags, lens)
    loss.backward()
    NTP = tr.shape[0]
    labels = tags.t().contiguous().int().to(DEV)
    inv = torch.tensor([1.0 / max(1, int(lens.sum()))], device=DEV)
    dlog, g_tr, g_st, g_en = (torch.full(s, float('nan'), device=DEV) for s in ((L, B, NTP), (NTP, NTP), (NTP,), (NTP,)))
    loss_sum = torch.zeros(4, device=DEV)
    _lib.call("rk_crf_nll", _p(lg), _p(tr), _p(st), _p(en), _p(labels), _p(dlens), L, B, NT, _p(inv), _p(dlog),
              _p(g_tr), _p(g_st), _p(g_en), _p(loss_sum), _p(ws), _s())
    dlog, g_tr, g_st, g_en = (t.cpu() for t in (dlog, g_tr, g_st, g_en))
    assert abs(float(loss_sum[0]) - loss.item()) < 1e-5 * max(1.0, abs(loss.item()))
    ref_tr = crf.trans.grad if crf.trans.grad is not None else torch.zeros(NT, NT)   # L = 1: no transition
    for name, got, ref in (('dlogits', dlog[:, :, :NT].transpose(0, 1), logits.grad), ('g_trans', g_tr[:NT, :NT], ref_tr),
                           ('g_start', g_st[:NT], crf.start.grad), ('g_end', g_en[:NT], crf.end.grad)):
        # one tag: every gradient is identically zero; fp64 autograd's own 1e-16 there is not the reference's scale
        ref = torch.where(ref.abs() < 1e-12, torch.zeros_like(ref), ref)
        assert _rel(got, ref) < 1e-5, (name, _rel(got, ref))
    if L == 1:
        assert not g_tr.any()
    steps = torch.arange(L)[:, None] < lens[None, :]                                   # [L, B]
    assert not dlog[~steps].any() and not dlog[:, :, NT:].any()
    assert not g_tr[NT:].any() and not g_tr[:, NT:].any() and not g_st[NT:].any() and not g_en[NT:].any()


@pytest.mark.parametrize("NT,B,L,scale,zero", CASES + LONG)
@torch.no_grad()
def test_crf_viterbi_kernel_finds_the_best_path(NT, B, L, scale, zero):
    crf, logits, _, lens, (lg, tr, st, en, dlens, ws) = _batch(NT, B, L, scale, zero)
    tags = torch.full((B, L), -7, dtype=torch.int32, device=DEV)
    _lib.call("rk_crf_viterbi", _p(lg), _p(tr), _p(st), _p(en), _p(dlens), L, B, NT, _p(tags), _p(ws), _s())
    got, best = tags.cpu().long(), crf.decode(logits, lens)
    for b, n in enumerate(lens.tolist()):
        assert (got[b, n:] == -1).all() and ((got[b, :n] >= 0) & (got[b, :n] < NT)).all()
        if n:
            s_got, s_best = (float(crf.start[y[0]] + crf.end[y[-1]] + logits[b, torch.arange(n), y].sum()
                                   + crf.trans[y[:-1], y[1:]].sum()) for y in (got[b, :n], best[b, :n]))
            assert abs(s_got - s_best) < 1e-5 * max(1.0, abs(s_best)), (b, s_got, s_best)


def _net(V, E, H, NT, p=0.0):
    net = Net(V, E, H, NT, p)
    net.crf = Crf(NT)
    with torch.no_grad():
        for q in net.crf.parameters():
            q.normal_()
    return net


@pytest.mark.parametrize("V,E,H,NT,B,L", [(50, 37, 51, 45, 5, 7), (64, 21, 100, 17, 9, 11)])
def test_tagger_crf_grads_match_fp64(V, E, H, NT, B, L):
    torch.manual_seed(0)
    net = _net(V, E, H, NT).to(DEV)
    eng = TaggerEngine(net, lr=0.01, dropout=0.0)
    x, y = _token_batch(np.random.default_rng(1), B, L, V, NT)
    eng.step(x, y, update=False, graph=False)
    torch.cuda.synchronize()
    g = eng.grads()
    ref = _net(V, E, H, NT).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in net.state_dict().items()})
    loss = ref.crf.nll(ref.out(ref.lstm(ref.emb(torch.from_numpy(x)))[0]), torch.from_numpy(y), (y != -100).sum(1))
    loss.backward()
    assert {k for k, _ in ref.named_parameters()} == set(g)
    for k, p in ref.named_parameters():
        assert _rel(g[k].cpu(), p.grad) < 1e-5, (k, _rel(g[k].cpu(), p.grad))
    assert abs(eng.take_loss() - loss.item()) < 1e-5 * max(1.0, abs(loss.item()))


def test_tagger_crf_graph_replay_matches_eager():
    """Captured and eager CRF steps leave bit-identical weights and Adam moments: the gradient fold is ordered."""
    torch.manual_seed(3)
    V, E, H, NT = 70, 37, 51, 45
    net = _net(V, E, H, NT).to(DEV)
    a = TaggerEngine(net, lr=0.01, dropout=0.2, seed=99)
    b = TaggerEngine(net, lr=0.01, dropout=0.2, seed=99)
    rng = np.random.default_rng(4)
    for B, L in [(5, 7), (3, 4), (5, 7), (5, 7), (3, 4), (8, 2), (5, 7)]:
        x, y = _token_batch(rng, B, L, V, NT)
        a.step(x, y, graph=True)
        b.step(x, y, graph=False)
    torch.cuda.synchronize()
    assert torch.equal(a.w, b.w) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
    a.close()


def test_pybilstmcrf_native_trains_unaligned_knobs():
    from rafiki_amd.models.pos_tagging import PyBiLstmCrf
    m = PyBiLstmCrf(epochs=3, word_embed_dims=37, word_rnn_hidden_size=51, word_dropout=0.01, learning_rate=0.05,
                    batch_size=32)
    m.train("synthetic://corpus?n=400&seed=0")
    assert m._engine is not None and m._engine.crf
    acc = m.evaluate("synthetic://corpus?n=100&seed=1")
    assert acc > 0.5, acc
    out = m.predict([["a", "b", "c"], ["d"]])
    assert [len(o) for o in out] == [3, 1] and all(0 <= t < m._tag_count for o in out for t in o)
