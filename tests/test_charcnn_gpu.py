"""charcnn.hip called raw, the tagger engine's char step and PyBiLstmChar / PyBiLstmCharCrf on the GPU.  Kernels: against
charcnn_refs in fp64, tolerance TOL_FACTOR x the fp32 yardstick's error per output; the backward is fed the fp64
forward's amax; outputs NaN-filled with a canary tail (test_lstm_kernels_gpu.Out).  Engine: loss and grads() against
the fp64 torch net, tolerance from the same net in fp32 on the CPU (the recurrence's entries per gate block), the loss
at the 1e-5 of tests/test_tagger_gpu.py."""
import numpy as np
import pytest
import torch

import charcnn_refs as R
from loss_optim_refs import philox_uniform
from lstm_refs import F32, TOL_FACTOR, err, ratio
from test_lstm_kernels_gpu import Out, _p, _s, call  # noqa: F401  (call: the fixture)
from test_tagger_gpu import DEV, _batch

pytestmark = pytest.mark.gpu
CASES = [(1, 16, 16), (5, 10, 20), (67, 25, 30), (4 * 128 + 3, 32, 64)]   # (n, Ec, F); 128: the grid cap


def _within(what, rows):
    for lab, e, tol in rows:
        print('{} {}: err {:.3e}  tolerance {:.3e}  ratio {:.3f}'.format(what, lab, e, tol, ratio(e, tol)))
    assert not [r for r in rows if not r[1] <= r[2]], (what, [r for r in rows if not r[1] <= r[2]])


def _fwd(call, c, p=0.0, seed=0, sid=0, step=None):
    n, FP = c['n'], c['FP']
    xc, mask = Out((n, FP), FP), Out((n, FP), FP)
    amax = torch.full((n * FP + FP,), -7, dtype=torch.int32, device=DEV)
    d = [c[k].to(DEV).contiguous() for k in ('chars', 'cemb', 'wc', 'bc')]
    call('rk_charcnn_fwd', *[_p(t) for t in d], n, c['EcP'], FP, c['CV'], p, seed, sid, _p(step) if step is not None
         else None, _p(xc.buf), _p(mask.buf) if p > 0 else None, _p(amax), _s())
    torch.cuda.synchronize()
    assert (amax[n * FP:] == -7).all()
    return xc.get(), (mask.get() if p > 0 else None), amax[:n * FP].view(n, FP).cpu()


@pytest.mark.parametrize('n,Ec,F', CASES)
def test_charcnn_fwd_matches_fp64(call, n, Ec, F):
    c = R.case(n, Ec, F)
    args = (c['chars'], c['cemb'], c['wc'], c['bc'])
    (ref, ramax, conv), (yard, _, _) = R.fwd(*args), R.fwd(*args, dtype=F32)
    xc, _, amax = _fwd(call, c)
    _within('fwd {}'.format((n, Ec, F)), [('xc', err(xc, ref), TOL_FACTOR * err(yard, ref))])
    lens = (c['chars'] != 0).sum(1)
    assert (xc[:, F:] == 0).all() and (xc[lens == 0] == 0).all() and (amax[lens == 0] == -1).all()
    top2 = conv.topk(2, 1).values                                    # margin of the winner over the runner-up
    clear = (top2[:, 0] - top2[:, 1] > 1e-4 * conv[conv.isfinite()].abs().max()) | (lens <= 1)[:, None]
    clear[c['ties']] = clear[:, F:] = True                           # exact ties (padded filters are all-zero ones):
    #                                                                  the first position, always
    assert (~clear).float().mean() <= 0.01, 'the reference leaves too many near-ties'
    assert (amax == ramax)[clear].all()


def test_charcnn_fwd_dropout_mask_is_philox(call):
    c, p, seed, sid = R.case(67, 25, 30), 0.3, 0x1234567, 0x6368
    step = torch.tensor([5], dtype=torch.int32, device=DEV)
    feat, _, _ = _fwd(call, c)
    xc, mask, _ = _fwd(call, c, p, seed, sid, step)
    keep = philox_uniform(67 * c['FP'], seed, sid, 5) >= np.float32(p)
    want = torch.from_numpy(np.where(keep, np.float32(1.0) / (np.float32(1.0) - np.float32(p)), np.float32(0)))
    assert torch.equal(mask.reshape(-1), want) and torch.equal(xc, feat * mask)


@pytest.mark.parametrize('n,Ec,F', CASES)
def test_charcnn_bwd_matches_fp64(call, n, Ec, F):
    c = R.case(n, Ec, F)
    EcP, FP, CV = c['EcP'], c['FP'], c['CV']
    amax = R.fwd(c['chars'], c['cemb'], c['wc'], c['bc'])[1]
    g = c['dxc'] * c['mask']
    ref, yard = R.bwd(c['chars'], c['cemb'], c['wc'], g, amax), R.bwd(c['chars'], c['cemb'], c['wc'], g, amax, F32)
    from rafiki_amd.ops import _lib
    ws = torch.empty(int(_lib.lib().rk_charcnn_ws_bytes(n, EcP, FP, CV)), dtype=torch.uint8, device=DEV)
    d = [c[k].to(DEV).contiguous() for k in ('chars', 'cemb', 'wc', 'dxc', 'mask')] + [amax.int().to(DEV)]
    runs = []
    for _ in range(2):
        outs = [Out((FP, 3, EcP), 64), Out((FP,), 64), Out((CV, EcP), 64)]
        call('rk_charcnn_bwd', *[_p(t) for t in d], n, EcP, FP, CV, *[_p(o.buf) for o in outs], _p(ws), _s())
        torch.cuda.synchronize()
        runs.append([o.get() for o in outs])
    dwc, dbc, dcemb = runs[0]
    assert all(torch.equal(a, b) for a, b in zip(*runs)), 'two launches differ'
    _within('bwd {}'.format((n, Ec, F)), [(k, err(got, r), TOL_FACTOR * err(y, r))
                                          for k, got, y, r in zip(('dwc', 'dbc', 'dcemb'), runs[0], yard, ref)])
    assert (dwc[F:] == 0).all() and (dwc[:, :, Ec:] == 0).all() and (dbc[F:] == 0).all() and (dcemb[:, Ec:] == 0).all()
    used = torch.zeros(CV, dtype=torch.bool)
    live = c['chars'].long()[c['chars'] < CV]
    used[live[live > 0]] = True
    assert (dcemb[~used] == 0).all()                                 # pad, absent and (never indexed) out-of-range ids


# ------------------------------------------------------------------------------------------- engine, models
class Net(torch.nn.Module):
    def __init__(self, V, E, H, NT, CV, Ec, F, cell, crf):
        super().__init__()
        self.emb = torch.nn.Embedding(V, E, padding_idx=0)
        self.char_emb = torch.nn.Embedding(CV, Ec, padding_idx=0)
        self.char_conv = torch.nn.Conv1d(Ec, F, 3, padding=1)
        rnn = getattr(torch.nn, cell.upper())(E + F, H, batch_first=True, bidirectional=True)
        setattr(self, cell, rnn)
        self.out = torch.nn.Linear(2 * H, NT)
        if crf:
            from rafiki_amd.ops.crf import Crf
            self.crf = Crf(NT)
            for p in self.crf.parameters():
                p.data.normal_()

    def loss(self, x, chars, y):
        from rafiki_amd.ops.charcnn import char_features
        rnn = self.gru if hasattr(self, 'gru') else self.lstm
        lg = self.out(rnn(torch.cat([self.emb(x), char_features(chars, self.char_emb, self.char_conv)], -1))[0])
        if hasattr(self, 'crf'):
            return self.crf.nll(lg, y, (y != -100).sum(1))
        return torch.nn.functional.cross_entropy(lg.reshape(-1, lg.shape[-1]), y.reshape(-1), ignore_index=-100)


def _chars(rng, x, CV):
    """[B, L, 16] uint8: a random word per token of x (none where x is padding), one id >= CV among them."""
    lens = rng.integers(1, 17, x.shape) * (x != 0)
    ch = rng.integers(2, CV, x.shape + (16,)) * (np.arange(16) < lens[..., None])
    ch[0, 0, 0] = CV + 1
    return ch.astype(np.uint8)


def _cpu_grads(net, dims, x, ch, y, dtype):
    ref = Net(*dims).to(dtype)
    ref.load_state_dict({k: v.detach().cpu().to(dtype) for k, v in net.state_dict().items()})
    loss = ref.loss(torch.from_numpy(x), torch.from_numpy(ch), torch.from_numpy(y))
    loss.backward()
    return {k: p.grad if p.grad is not None else torch.zeros_like(p) for k, p in ref.named_parameters()}, loss.item()


@pytest.mark.parametrize('crf', [False, True])
@pytest.mark.parametrize('cell', ['lstm', 'gru'])
@pytest.mark.parametrize('E,H,NT,Ec,F,B,L', [(37, 51, 45, 25, 30, 5, 7), (16, 100, 12, 10, 20, 17, 3)])
def test_char_tagger_grads_match_fp64(E, H, NT, Ec, F, B, L, cell, crf):
    from rafiki_amd.engine.tagger import TaggerEngine
    torch.manual_seed(0)
    dims = (50, E, H, NT, 40, Ec, F, cell, crf)
    net = Net(*dims).to(DEV)
    eng = TaggerEngine(net, lr=0.01, dropout=0.0)
    rng = np.random.default_rng(1)
    x, y = _batch(rng, B, L, 50, NT)
    ch = _chars(rng, x, 40)
    eng.step(x, y, update=False, graph=False, chars=ch)
    torch.cuda.synchronize()
    got = eng.grads()
    (ref, loss), (yard, _) = _cpu_grads(net, dims, x, ch, y, torch.float64), _cpu_grads(net, dims, x, ch, y, F32)
    assert set(got) == set(ref)
    rows = []
    for k, r in ref.items():
        nb = {'lstm': 4, 'gru.': 3}.get(k[:4], 1)
        rows += [('{}[{}]'.format(k, i), err(g, rr), TOL_FACTOR * err(yy, rr))
                 for i, (g, yy, rr) in enumerate(zip(got[k].cpu().chunk(nb), yard[k].chunk(nb), r.chunk(nb)))]
    _within('char tagger {} {} crf={}'.format((E, H, NT, Ec, F, B, L), cell, crf), rows)
    assert abs(eng.take_loss() - loss) < 1e-5 * max(1.0, abs(loss))


@pytest.mark.parametrize('cell,crf', [('lstm', False), ('gru', True)])
def test_char_tagger_graph_replay_matches_eager(cell, crf):
    from rafiki_amd.engine.tagger import TaggerEngine
    torch.manual_seed(3)
    net = Net(70, 37, 51, 45, 40, 25, 30, cell, crf).to(DEV)
    a, b = (TaggerEngine(net, lr=0.01, dropout=0.2, seed=99, clip_norm=1.0) for _ in range(2))
    rng = np.random.default_rng(4)
    for B, L in [(5, 7), (3, 4), (5, 7), (5, 7), (3, 4)]:
        x, y = _batch(rng, B, L, 70, 45)
        ch = _chars(rng, x, 40)
        a.step(x, y, graph=True, chars=ch)
        b.step(x, y, graph=False, chars=ch)
    torch.cuda.synchronize()
    assert len(a._graphs) == 2
    assert torch.equal(a.w, b.w) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
    a.close()


@pytest.mark.parametrize('name', ['PyBiLstmChar', 'PyBiLstmCharCrf'])
def test_pybilstmchar_native_trains_and_reloads(name):
    from rafiki_amd.models import pos_tagging
    knobs = dict(epochs=3, word_embed_dims=37, word_rnn_hidden_size=51, word_dropout=0.01, learning_rate=0.05,
                 batch_size=32, char_embed_dims=25, char_filters=30)
    m = getattr(pos_tagging, name)(**knobs)
    m.train("synthetic://corpus?n=400&seed=0")
    assert m._engine is not None and m._engine.char and m._engine.crf == name.endswith('Crf')
    acc = m.evaluate("synthetic://corpus?n=100&seed=1")
    assert acc > 0.5, acc
    queries = [["a", "b", "c"], ["d"]]
    m2 = getattr(pos_tagging, name)(**knobs)
    m2.load_parameters(m.dump_parameters())
    assert m2.predict(queries) == m.predict(queries)
