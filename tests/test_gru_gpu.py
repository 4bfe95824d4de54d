"""gru.hip called raw, the tagger engine's GRU step and PyBiGru / PyBiGruCrf on the GPU.  Kernels: against gru_refs in
fp64, tolerance TOL_FACTOR x the fp32 yardstick's error per direction and gate block; the backward is fed the fp64
forward rounded to fp32; outputs NaN-filled with a canary tail (test_lstm_kernels_gpu.Out).  Engine: loss and grads()
against the fp64 torch net, tolerance from the same net in fp32 on the CPU, the GRU's entries per gate block; the loss,
one fp32 number whose yardstick can be exact by chance, gets the 1e-5 of tests/test_tagger_gpu.py."""
import functools
import math

import numpy as np
import pytest
import torch

import gru_refs as G
from lstm_refs import F32, TOL_FACTOR, err, ratio
from test_lstm_kernels_gpu import Out, _p, _s, call  # noqa: F401  (call: the fixture)
from test_tagger_gpu import DEV, _batch

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 5), (2, 16, 64), (5, 17, 51), (3, 33, 65), (4, 16, 128)]   # (T, B, H)


@functools.lru_cache(maxsize=None)
def case(T, B, H):
    """HP, fp32 gin, whh, bhh, dhout in the padded layout (units >= H zero), and the fp64 forward of them."""
    HP = 64 if H <= 64 else 128
    gen = torch.Generator().manual_seed(100 * H + 10 * T + B)
    live = (torch.arange(HP) < H).float()
    whh = (torch.rand((2, 3, HP, HP), generator=gen) * 2 - 1) * (2 / math.sqrt(H)) * live[:, None] * live
    bhh = (torch.rand((2, 3, HP), generator=gen) * 2 - 1) * live
    gin = 1.5 * torch.randn((T, B, 2, 3, HP), generator=gen) * live
    dhout = torch.randn((T, B, 2, HP), generator=gen) * live
    gin, whh, bhh = gin.view(T, B, 2, 3 * HP), whh.view(2, 3 * HP, HP), bhh.view(2, 3 * HP)
    return HP, gin, whh, bhh, dhout, G.fwd_run(gin, whh, bhh)


def _within(what, rows):
    lab, e, tol = max(rows, key=lambda r: ratio(r[1], r[2]))
    print('{}: worst slab {}: err {:.3e}  tolerance {:.3e}  ratio {:.3f}'.format(what, lab, e, tol, ratio(e, tol)))
    assert not [r for r in rows if not r[1] <= r[2]], (what, [r for r in rows if not r[1] <= r[2]][:8])


def _launch(call, name, shapes, B, HP, args):
    outs = [Out(sh, B * 2 * 3 * HP) for sh in shapes]
    keep = [a.to(DEV).contiguous() if torch.is_tensor(a) else a for a in args]
    call(name, *[_p(a) if torch.is_tensor(a) else a for a in keep], *[_p(o.buf) for o in outs], _s())
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize('T,B,H', SHAPES)
def test_gru_fwd32_matches_fp64(call, T, B, H):
    HP, gin, whh, bhh, _, ref = case(T, B, H)
    outs = _launch(call, 'rk_gru_fwd32', [(T, B, 2, HP), (T, B, 2, 3 * HP), (T, B, 2, HP)], B, HP,
                   (gin, whh, bhh, T, B, HP))
    got = [o.get() for o in outs]
    for name, g, y, r in zip(('hout', 'gsave', 'qsave'), got, G.fwd_run(gin, whh, bhh, F32), ref):
        _within('fwd {} {}'.format((T, B, H), name), G.slab_rows(g, y, r, HP))
    assert (got[0][..., H:] == 0).all()


@pytest.mark.parametrize('T,B,H', SHAPES)
def test_gru_bwd32_matches_fp64(call, T, B, H):
    HP, _, whh, _, dhout, fwd = case(T, B, H)
    saved = [x.float() for x in fwd]
    outs = _launch(call, 'rk_gru_bwd32', [(T, B, 2, 3 * HP)] * 2, B, HP,
                   (whh.transpose(1, 2), T, B, HP, dhout, *saved))
    ref, yard = G.bwd_run(whh, dhout, *saved), G.bwd_run(whh, dhout, *saved, dtype=F32)
    for name, o, y, r in zip(('dgin', 'dgh'), outs, yard, ref):
        _within('bwd {} {}'.format((T, B, H), name), G.slab_rows(o.get(), y, r, HP))
        assert (o.get().view(T, B, 2, 3, HP)[..., H:] == 0).all()


# ------------------------------------------------------------------------------------------- engine, models
class Net(torch.nn.Module):
    def __init__(self, V, E, H, NT, crf):
        super().__init__()
        self.emb = torch.nn.Embedding(V, E, padding_idx=0)
        self.gru = torch.nn.GRU(E, H, batch_first=True, bidirectional=True)
        self.out = torch.nn.Linear(2 * H, NT)
        if crf:
            from rafiki_amd.ops.crf import Crf
            self.crf = Crf(NT)
            for p in self.crf.parameters():
                p.data.normal_()

    def loss(self, x, y):
        lg = self.out(self.gru(self.emb(x))[0])
        if hasattr(self, 'crf'):
            return self.crf.nll(lg, y, (y != -100).sum(1))
        return torch.nn.functional.cross_entropy(lg.reshape(-1, lg.shape[-1]), y.reshape(-1), ignore_index=-100)


def _cpu_grads(net, dims, x, y, dtype):
    ref = Net(*dims).to(dtype)
    ref.load_state_dict({k: v.detach().cpu().to(dtype) for k, v in net.state_dict().items()})
    loss = ref.loss(torch.from_numpy(x), torch.from_numpy(y))
    loss.backward()
    return {k: p.grad if p.grad is not None else torch.zeros_like(p) for k, p in ref.named_parameters()}, loss.item()


@pytest.mark.parametrize('crf', [False, True])
@pytest.mark.parametrize('E,H,NT,B,L', [(37, 51, 45, 5, 7), (16, 100, 12, 17, 3), (37, 51, 45, 5, 1)])
def test_gru_tagger_grads_match_fp64(E, H, NT, B, L, crf):
    from rafiki_amd.engine.tagger import TaggerEngine
    torch.manual_seed(0)
    dims = (50, E, H, NT, crf)
    net = Net(*dims).to(DEV)
    eng = TaggerEngine(net, lr=0.01, dropout=0.0)
    x, y = _batch(np.random.default_rng(1), B, L, 50, NT)
    eng.step(x, y, update=False, graph=False)
    torch.cuda.synchronize()
    got = eng.grads()
    (ref, loss), (yard, _) = _cpu_grads(net, dims, x, y, torch.float64), _cpu_grads(net, dims, x, y, F32)
    assert set(got) == set(ref)
    rows = []
    for k, r in ref.items():
        n = 3 if k.startswith('gru.') else 1
        rows += [('{}[{}]'.format(k, i), err(g, rr), TOL_FACTOR * err(yy, rr))
                 for i, (g, yy, rr) in enumerate(zip(got[k].cpu().chunk(n), yard[k].chunk(n), r.chunk(n)))]
    _within('tagger {} crf={}'.format((E, H, NT, B, L), crf), rows)
    assert abs(eng.take_loss() - loss) < 1e-5 * max(1.0, abs(loss))


@pytest.mark.parametrize('crf', [False, True])
def test_gru_tagger_graph_replay_matches_eager(crf):
    from rafiki_amd.engine.tagger import TaggerEngine
    torch.manual_seed(3)
    net = Net(70, 37, 51, 45, crf).to(DEV)
    a, b = (TaggerEngine(net, lr=0.01, dropout=0.2, seed=99) for _ in range(2))
    rng = np.random.default_rng(4)
    for B, L in [(5, 7), (3, 4), (5, 7), (5, 7), (3, 4)]:
        x, y = _batch(rng, B, L, 70, 45)
        a.step(x, y, graph=True)
        b.step(x, y, graph=False)
    torch.cuda.synchronize()
    assert len(a._graphs) == 2
    assert torch.equal(a.w, b.w) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
    a.close()


@pytest.mark.parametrize('name', ['PyBiGru', 'PyBiGruCrf'])
def test_pybigru_native_trains_and_reloads(name):
    from rafiki_amd.models import pos_tagging
    knobs = dict(epochs=3, word_embed_dims=37, word_rnn_hidden_size=51, word_dropout=0.01, learning_rate=0.05,
                 batch_size=32)
    m = getattr(pos_tagging, name)(**knobs)
    m.train("synthetic://corpus?n=400&seed=0")
    assert m._engine is not None and m._engine.gru and m._engine.crf == name.endswith('Crf')
    acc = m.evaluate("synthetic://corpus?n=100&seed=1")
    assert acc > 0.5, acc
    queries = [["a", "b", "c"], ["d"]]
    m2 = getattr(pos_tagging, name)(**knobs)
    m2.load_parameters(m.dump_parameters())
    assert m2.predict(queries) == m.predict(queries)
