"""attn.hip called raw, the tagger engine's attention step and PyBiLstmAttn / PyBiLstmAttnCrf on the GPU.  Kernels: against
ops/attn.py's attention in fp64, tolerance TOL_FACTOR x the error of the same function in fp32 per output; the backward is
fed the forward kernel's ctx and lse, as the engine feeds it.  Engine: the yardstick of tests/test_charcnn_gpu.py."""
import functools

import numpy as np
import pytest
import torch

from lstm_refs import F32, F64, TOL_FACTOR, err
from test_charcnn_gpu import _chars, _within
from test_lstm_kernels_gpu import Out, _p, _s, call  # noqa: F401  (call: the fixture)
from test_tagger_gpu import DEV, _batch

pytestmark = pytest.mark.gpu
# (L, B, NH, dh, lens); the last one: 2400 (sentence, head) items, past the grid cap of 1024
CASES = [(1, 1, 1, 8, None), (7, 5, 2, 13, None), (17, 3, 4, 32, None), (40, 4, 1, 16, (40, 32, 16, 0)),
         (130, 2, 2, 16, None), (1, 300, 8, 8, None)]


@functools.lru_cache(maxsize=None)
def _case(L, B, NH, dh, lens):
    """qkv [B, L, 3 NH dh], dctx [B, L, NH dh], lens, and (ctx, lse, dqkv) of ops/attn.py in fp64 and in fp32."""
    from rafiki_amd.ops.attn import attention
    gen = torch.Generator().manual_seed(1000 * L + 10 * B + NH + dh)
    qkv, dctx = 1.5 * torch.randn((B, L, 3 * NH * dh), generator=gen), torch.randn((B, L, NH * dh), generator=gen)
    if lens is None:
        lens = torch.randint(1, L + 1, (B,), generator=gen)
        lens[0] = L
    lens, outs = torch.as_tensor(lens), []
    for dt in (F64, F32):
        x = qkv.to(dt).requires_grad_(True)
        ctx, lse = attention(x, lens, NH, with_lse=True)
        (ctx * dctx.to(dt)).sum().backward()
        outs.append((ctx.detach(), lse.detach(), x.grad))
    return qkv, dctx, lens, outs[0], outs[1]


def _tm(x, G, dh, DP):   # [B, L, G dh] -> the kernels' time-major [L, B, G, DP], zero-padded
    B, L, _ = x.shape
    out = torch.zeros((L, B, G, DP))
    out[..., :dh] = x.view(B, L, G, dh).transpose(0, 1)
    return out.to(DEV)


@pytest.mark.parametrize('L,B,NH,dh,lens', CASES)
def test_attn_kernels_match_fp64(call, L, B, NH, dh, lens):
    qkv, dctx, lens, ref, yard = _case(L, B, NH, dh, lens)
    DP, scale = (16 if dh <= 16 else 32), dh ** -0.5
    dq, dd, dl = _tm(qkv, 3 * NH, dh, DP), _tm(dctx, NH, dh, DP), lens.int().to(DEV)
    ctx, lse = Out((L, B, NH, DP), 64), Out((L, B, NH), 64)
    call('rk_attn_fwd', _p(dq), _p(dl), L, B, NH, DP, scale, _p(ctx.buf), _p(lse.buf), _s())
    runs = []
    for _ in range(2):
        g = Out((L, B, 3 * NH, DP), 64)
        call('rk_attn_bwd', _p(dq), _p(dl), _p(ctx.buf), _p(lse.buf), _p(dd), L, B, NH, DP, scale, _p(g.buf), _s())
        torch.cuda.synchronize()
        runs.append(g.get())
    assert torch.equal(*runs), 'two backward launches differ'
    c, s, g = ctx.get(), lse.get(), runs[0]
    dead = torch.arange(L)[:, None] >= lens[None, :]                                   # [L, B]
    assert all((t[dead] == 0).all() for t in (c, s, g)) and (c[..., dh:] == 0).all() and (g[..., dh:] == 0).all()
    got = [t[..., :dh].transpose(0, 1).reshape(B, L, -1) for t in (c, g)]
    rows = [('ctx', got[0], yard[0], ref[0]), ('lse', s.transpose(0, 1), yard[1], ref[1])]
    rows += [(k, a, y, r) for k, a, y, r in zip(('dq', 'dk', 'dv'), *(t.chunk(3, -1) for t in (got[1], yard[2], ref[2])))]
    _within('attn {}'.format((L, B, NH, dh)), [(k, err(a, r), TOL_FACTOR * err(y, r)) for k, a, y, r in rows])


class Net(torch.nn.Module):
    def __init__(self, V, E, H, NT, heads, dh, cell, crf, char):
        from rafiki_amd.ops.attn import SelfAttention
        super().__init__()
        self.emb = torch.nn.Embedding(V, E, padding_idx=0)
        if char:
            self.char_emb, self.char_conv = torch.nn.Embedding(40, 25, padding_idx=0), torch.nn.Conv1d(25, 30, 3, padding=1)
        setattr(self, cell, getattr(torch.nn, cell.upper())(E + (30 if char else 0), H, batch_first=True,
                                                             bidirectional=True))
        self.attn = SelfAttention(2 * H, heads, dh)
        self.out = torch.nn.Linear(2 * H, NT)
        if crf:
            from rafiki_amd.ops.crf import Crf
            self.crf = Crf(NT)
            for p in self.crf.parameters():
                p.data.normal_()

    def loss(self, x, chars, y):
        from rafiki_amd.ops.charcnn import char_features
        e, lens = self.emb(x), (y != -100).sum(1)
        if chars is not None:
            e = torch.cat([e, char_features(chars, self.char_emb, self.char_conv)], -1)
        lg = self.out(self.attn((self.gru if hasattr(self, 'gru') else self.lstm)(e)[0], lens))
        if hasattr(self, 'crf'):
            return self.crf.nll(lg, y, lens)
        return torch.nn.functional.cross_entropy(lg.reshape(-1, lg.shape[-1]), y.reshape(-1), ignore_index=-100)


def _cpu_grads(net, dims, x, ch, y, dtype):
    ref = Net(*dims).to(dtype)
    ref.load_state_dict({k: v.detach().cpu().to(dtype) for k, v in net.state_dict().items()})
    loss = ref.loss(torch.from_numpy(x), None if ch is None else torch.from_numpy(ch), torch.from_numpy(y))
    loss.backward()
    return {k: p.grad if p.grad is not None else torch.zeros_like(p) for k, p in ref.named_parameters()}, loss.item()


@pytest.mark.parametrize('E,H,NT,heads,dh,B,L,cell,crf,char',
                         [(37, 51, 45, 2, 13, 5, 7, cell, crf, False) for cell in ('lstm', 'gru') for crf in (False, True)]
                         + [(16, 100, 12, 4, 32, 17, 19, 'lstm', False, False), (37, 51, 45, 2, 13, 5, 7, 'gru', True, True)])
def test_attn_tagger_grads_match_fp64(E, H, NT, heads, dh, B, L, cell, crf, char):
    """The tightest slab is out.bias of the (16, 100, 12, 4, 32, 17, 19) case, tolerance 3.17e-07 (the fp32 net's own
    error there is 7.9e-08): the engine's logits carry 8e-09 of it, the softmax cross-entropy kernel and the column
    sum of d(logits) the rest, 2.88e-07 in all (ratio 0.91); the same net without the attention layer is at 0.71."""
    from rafiki_amd.engine.tagger import TaggerEngine
    torch.manual_seed(0)
    dims = (50, E, H, NT, heads, dh, cell, crf, char)
    net = Net(*dims).to(DEV)
    eng = TaggerEngine(net, lr=0.01, dropout=0.0)
    rng = np.random.default_rng(1)
    x, y = _batch(rng, B, L, 50, NT)
    ch = _chars(rng, x, 40) if char else None
    eng.step(x, y, update=False, graph=False, chars=ch)
    got = eng.grads()
    (ref, loss), (yard, _) = _cpu_grads(net, dims, x, ch, y, F64), _cpu_grads(net, dims, x, ch, y, F32)
    assert set(got) == set(ref)
    rows = []
    for k, r in ref.items():
        # q | k | v rows of the qkv weight apart; not of its bias: its k block is zero in exact arithmetic
        nb = 3 if k == 'attn.qkv.weight' else {'lstm': 4, 'gru.': 3}.get(k[:4], 1)
        rows += [('{}[{}]'.format(k, i), err(g, rr), TOL_FACTOR * err(yy, rr))
                 for i, (g, yy, rr) in enumerate(zip(got[k].cpu().chunk(nb), yard[k].chunk(nb), r.chunk(nb)))]
    _within('attn tagger {}'.format((E, H, NT, heads, dh, B, L, cell, crf, char)), rows)
    assert abs(eng.take_loss() - loss) < 1e-5 * max(1.0, abs(loss))


@pytest.mark.parametrize('cell,crf,char', [('lstm', False, False), ('gru', True, True)])
def test_attn_tagger_graph_replay_matches_eager(cell, crf, char):
    from rafiki_amd.engine.tagger import TaggerEngine
    torch.manual_seed(3)
    net = Net(70, 37, 51, 45, 2, 13, cell, crf, char).to(DEV)
    a, b = (TaggerEngine(net, lr=0.01, dropout=0.2, seed=99, clip_norm=1.0) for _ in range(2))
    rng = np.random.default_rng(4)
    for B, L in [(5, 7), (3, 4), (5, 7), (5, 7), (3, 4)]:
        x, y = _batch(rng, B, L, 70, 45)
        ch = _chars(rng, x, 40) if char else None
        a.step(x, y, graph=True, chars=ch)
        b.step(x, y, graph=False, chars=ch)
    assert len(a._graphs) == 2 and torch.equal(a.w, b.w) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
    a.close()


@pytest.mark.parametrize('name', ['PyBiLstmAttn', 'PyBiLstmAttnCrf'])
def test_pybilstmattn_native_trains_and_reloads(name):
    from rafiki_amd.models import pos_tagging
    knobs = dict(epochs=3, word_embed_dims=37, word_rnn_hidden_size=51, word_dropout=0.01, learning_rate=0.05,
                 batch_size=32, attn_heads=2, attn_head_dims=13)
    m = getattr(pos_tagging, name)(**knobs)
    m.train("synthetic://corpus?n=400&seed=0")
    assert m._engine is not None and m._engine.attn and m._engine.crf == name.endswith('Crf')
    assert m.evaluate("synthetic://corpus?n=100&seed=1") > 0.5
    m2 = getattr(pos_tagging, name)(**knobs)
    m2.load_parameters(m.dump_parameters())
    assert m2.predict([["a", "b", "c"], ["d"]]) == m.predict([["a", "b", "c"], ["d"]])
