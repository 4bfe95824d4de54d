"""crf.hip at the places its structure can break: every tag count next to an instantiation edge (16 / 32 / 48 / 64),
reads outside the sentence, sentences of hundreds of tokens in the loss kernel, forbidden (-1e4) transitions, the
Viterbi backpointer addressing of all four waves in LDS and of every sentence in the workspace, the documented
tie-break (exact paths), the host-side argument checks, and the engine's decode / Adam / clip / workspace cache.
The reference is the torch Crf in fp64 on the CPU (tests/test_crf.py pins it to brute force).
"""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from rafiki_amd.ops.crf import Crf
from rafiki_amd.ops import _lib
from rafiki_amd.ops.functional import _p, _s
from rafiki_amd.engine.tagger import TaggerEngine
from crf_refs import FORBID, make_case, path_score, viterbi_first_max
from test_crf_gpu import _net                                        # Net with a randomly initialised Crf
from test_tagger_gpu import DEV, _batch as _token_batch, _rel      # the tagger tests' batch maker and error measure

pytestmark = pytest.mark.gpu
EBADARG = -1
NAN = float('nan')


# ------------------------------------------------------------------------------------------------ operands, launches
def _ntp(NT):
    return -(-NT // 4) * 4


def _ws(L, B, NT):
    """The kernels' workspace, every byte 0xFF: a float read before it is written is a NaN, a backpointer is 255."""
    return torch.full((int(_lib.lib().rk_crf_ws_bytes(L, B, NT)),), 0xFF, dtype=torch.uint8, device=DEV)


def _operands(c, poison=False, dev_lens=None):
    """Device operands of a case: padded time-major logits, trans, start, end, int32 lens, workspace.  poison: NaN in
    the logits of every t >= lens[b] and in the pad rows / columns of trans, start and end."""
    NT, B, L, NTP = c.NT, c.B, c.L, _ntp(c.NT)
    fill = NAN if poison else 0.0
    lg, tr, st, en = torch.zeros(L, B, NTP), torch.full((NTP, NTP), fill), torch.full((NTP,), fill), \
        torch.full((NTP,), fill)
    lg[:, :, :NT], tr[:NT, :NT], st[:NT], en[:NT] = c.logits.transpose(0, 1), c.crf.trans.data, c.crf.start.data, \
        c.crf.end.data
    if poison:
        lg[~(torch.arange(L)[:, None] < c.lens[None, :])] = NAN
    lens = c.lens if dev_lens is None else torch.as_tensor(dev_lens)
    return [t.to(DEV) for t in (lg, tr, st, en, lens.int())] + [_ws(L, B, NT)]


def _nll(c, ops, labels=None, inv=None):
    """rk_crf_nll into NaN-filled outputs: loss, d(logits) [L, B, NTP], g_trans, g_start, g_end (padded, on the CPU)."""
    lg, tr, st, en, dlens, ws = ops
    NTP = tr.shape[0]
    labels = (c.tags.t() if labels is None else labels.t()).contiguous().int().to(DEV)
    inv = torch.tensor([1.0 / max(1, int(c.lens.sum())) if inv is None else inv], device=DEV)
    out = [torch.full(s, NAN, device=DEV) for s in ((c.L, c.B, NTP), (NTP, NTP), (NTP,), (NTP,))]
    loss_sum = torch.zeros(4, device=DEV)
    _lib.call("rk_crf_nll", _p(lg), _p(tr), _p(st), _p(en), _p(labels), _p(dlens), c.L, c.B, c.NT, _p(inv),
              *(_p(o) for o in out), _p(loss_sum), _p(ws), _s())
    return [float(loss_sum[0])] + [o.cpu() for o in out]


def _viterbi(c, ops):
    lg, tr, st, en, dlens, ws = ops
    tags = torch.full((c.B, c.L), -7, dtype=torch.int32, device=DEV)
    _lib.call("rk_crf_viterbi", _p(lg), _p(tr), _p(st), _p(en), _p(dlens), c.L, c.B, c.NT, _p(tags), _p(ws), _s())
    return tags.cpu().long()


def _ref(c, dtype=torch.float64):
    """Crf.nll and its backward in ``dtype`` on the CPU: loss, then the four gradients in the kernel's order."""
    crf = Crf(c.NT).to(dtype)
    crf.load_state_dict({k: v.to(dtype) for k, v in c.crf.state_dict().items()})
    logits = c.logits.clone().to(dtype).requires_grad_()
    loss = crf.nll(logits, c.tags, c.lens)
    loss.backward()
    g_tr = crf.trans.grad if crf.trans.grad is not None else torch.zeros(c.NT, c.NT, dtype=dtype)
    return loss.item(), [logits.grad, g_tr, crf.start.grad, crf.end.grad]


NAMES = ('dlogits', 'g_trans', 'g_start', 'g_end')


def _unpadded(c, got):
    _, dlog, g_tr, g_st, g_en = got
    NT = c.NT
    return [dlog[:, :, :NT].transpose(0, 1), g_tr[:NT, :NT], g_st[:NT], g_en[:NT]]


def _check_nll(c, got, ref, gates=None):
    """The assertions of test_crf_gpu.py::test_crf_nll_kernel_matches_fp64, and every output finite.  gates: the bound
    of each gradient's error (1e-5 without)."""
    loss, grads = ref
    NT = c.NT
    assert all(bool(torch.isfinite(o).all()) for o in got[1:]) and math.isfinite(got[0])
    assert abs(got[0] - loss) < 1e-5 * max(1.0, abs(loss)), (got[0], loss)
    errs = [_rel(a, b) for a, b in zip(_unpadded(c, got), grads)]
    for k, name in enumerate(NAMES):
        assert errs[k] < (1e-5 if gates is None else gates[k]), (name, errs[k])
    _, dlog, g_tr, g_st, g_en = got
    steps = torch.arange(c.L)[:, None] < c.lens[None, :]                               # [L, B]
    assert not dlog[~steps].any() and not dlog[:, :, NT:].any()
    assert not g_tr[NT:].any() and not g_tr[:, NT:].any() and not g_st[NT:].any() and not g_en[NT:].any()
    return errs


def _check_paths(c, got, score_tol=1e-5):
    """-1 from lens[b] on, tags in range before, and the path's fp64 score is the best one's (Crf.decode in fp64)."""
    best = c.crf.decode(c.logits, c.lens)
    for b, n in enumerate(c.lens.tolist()):
        assert (got[b, n:] == -1).all() and ((got[b, :n] >= 0) & (got[b, :n] < c.NT)).all()
        if n:
            s_got, s_best = (path_score(c.crf, c.logits[b], y) for y in (got[b, :n], best[b, :n]))
            assert abs(s_got - s_best) < score_tol * max(1.0, abs(s_best)), (b, s_got, s_best)


def _first_max32(c):
    """The numpy first-maximum Viterbi in fp32: the kernel's additions one by one (no product, so nothing to fuse),
    hence its path bit for bit, ties included."""
    return torch.from_numpy(viterbi_first_max(*(p.detach().numpy().astype(np.float32) for p in
                                                (c.crf.trans, c.crf.start, c.crf.end)),
                                              c.logits.numpy().astype(np.float32), c.lens.tolist()))


# ------------------------------------------------------------------------- 1. loss and gradients at every instance edge
EDGE_NT = (2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)
# every tag count with a partly filled second block (B = 5: one live wave beside three dead ones) and with two full
# blocks and one more wave (B = 9); 63 and 64 also alone (B = 1) and as exactly one full block (B = 4); one tag count
# per instance there as well
EDGE_CASES = [(NT, B, L) for NT in EDGE_NT for B, L in ((5, 6), (9, 5))] + \
    [(NT, B, L) for NT in (63, 64) for B, L in ((1, 3), (4, 2))] + [(2, 1, 3), (16, 4, 2), (33, 1, 3), (48, 4, 2)]


@pytest.mark.parametrize("NT,B,L", EDGE_CASES)
def test_crf_nll_at_instance_edges(NT, B, L):
    c = make_case(NT, B, L, seed=1)
    assert c.lens[0] == L and (B == 1 or c.lens[B - 1] == 1)
    _check_nll(c, _nll(c, _operands(c)), _ref(c))


# -------------------------------------------------------------------------- 2. nothing outside the sentence is read
def _poison_lens(B, L, empty):
    g = torch.Generator().manual_seed(B * 10 + L)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[0], lens[B - 2] = L, 1
    if empty == 'first':      # wave 0 of block 0
        lens[0], lens[1] = 0, L
    elif empty == 'last':     # the last sentence of the batch
        lens[B - 1] = 0
    elif empty == 'block':    # the whole second block
        lens[4:8], lens[8] = 0, 1
    elif empty == 'overlong':  # sentences 0 and 1 at full length: the device gets more than L for them
        lens[1] = L
    return lens


POISON = [(17, 5, 6, -100, None), (17, 5, 6, 10 ** 6, None), (48, 9, 5, -100, None), (48, 9, 5, 10 ** 6, None),
          (63, 4, 2, -100, None), (63, 4, 2, 10 ** 6, None), (17, 5, 6, 10 ** 6, 'first'), (63, 4, 2, -100, 'last'),
          (48, 9, 5, 10 ** 6, 'block'), (17, 5, 6, -100, 'overlong')]


@pytest.mark.parametrize("NT,B,L,bad_label,variant", POISON)
def test_crf_kernels_read_nothing_outside_the_sentence(NT, B, L, bad_label, variant):
    """NaN logits from lens[b] on, NaN pad rows / columns of trans, start and end, labels no tag can have from lens[b]
    on, an all-0xFF workspace, NaN-filled outputs: the results are those of the clean operands."""
    c = make_case(NT, B, L, seed=2, lens=_poison_lens(B, L, variant))
    steps = torch.arange(L)[None, :] < c.lens[:, None]                                 # [B, L]
    c.logits = c.logits * steps[:, :, None]                                            # the reference gets zeros there
    dev_lens = None
    if variant == 'overlong':   # the kernels clamp a length to L
        dev_lens = c.lens.clone()
        dev_lens[0], dev_lens[1] = L + 3, 10 ** 6
        assert (dev_lens.clamp(max=L) == c.lens).all()
    labels = torch.where(torch.arange(L)[None, :] < c.lens[:, None], c.tags, torch.tensor(bad_label))
    _check_nll(c, _nll(c, _operands(c, poison=True, dev_lens=dev_lens), labels=labels), _ref(c))
    clean, dirty = _viterbi(c, _operands(c)), _viterbi(c, _operands(c, poison=True, dev_lens=dev_lens))
    assert torch.equal(clean, dirty)
    _check_paths(c, dirty)
    assert torch.equal(dirty, _first_max32(c))


# ------------------------------------------------------------------------------ 3. long sentences in the loss kernel
# (name, NT, B, L, keyword arguments of make_case)
LONG = [('random', 5, 5, 256, {}), ('random', 5, 5, 257, {}), ('random', 64, 3, 600, {}), ('random', 17, 2, 600, {}),
        ('forbid', 17, 2, 300, dict(forbid=True)), ('confident', 17, 2, 300, dict(confident=12.0))]


def _long_lens(B, L):
    g = torch.Generator().manual_seed(L)
    lens = torch.randint(L // 2, L + 1, (B,), generator=g)
    lens[0] = L
    return lens


@pytest.mark.parametrize("name,NT,B,L,kw", LONG, ids=['{}-{}-{}-{}'.format(*c[:4]) for c in LONG])
def test_crf_nll_long_sentences(name, NT, B, L, kw):
    """Gradients: within 4x the error of the same Crf.nll in torch fp32 on the CPU (1e-5 where that is smaller); the
    factor allows for the other summation order of the scaled-exp recursion.  Loss, one sentence per launch with
    inv = 1: |loss - fp64| <= (n + 2) * 2^-23 * max(|log Z|, |gold score|), two fp32 running sums of n + 2 terms with
    half an ulp of the partial sum per addition.

    Measured on an MI355X, kernel / torch fp32 per gradient, then the worst sentence's |loss - fp64| / its bound:
        case (NT, B, L)         dlogits          g_trans          g_start          g_end            loss
        random    5, 5, 256     8.7e-7 / 1.2e-4  1.8e-7 / 2.7e-5  2.4e-7 / 3.9e-5  1.2e-7 / 8.0e-6  1.6e-4 / 7.6e-3
        random    5, 5, 257     1.0e-6 / 1.1e-4  4.6e-7 / 6.4e-6  3.2e-7 / 2.3e-5  1.2e-7 / 9.0e-6  2.0e-4 / 1.9e-2
        random    64, 3, 600    2.4e-7 / 9.9e-5  3.2e-7 / 6.7e-5  2.1e-7 / 5.3e-5  6.1e-8 / 5.3e-5  6.4e-4 / 2.2e-1
        random    17, 2, 600    3.2e-7 / 3.9e-4  3.8e-7 / 2.6e-4  1.4e-7 / 2.6e-4  1.2e-7 / 2.5e-5  9.7e-4 / 1.7e-1
        forbid    17, 2, 300    5.3e-7 / 1.2e-4  4.0e-7 / 7.9e-5  6.2e-7 / 7.5e-5  3.1e-8 / 1.4e-5  2.3e-4 / 1.3e-2
        confident 17, 2, 300    1.8e-5 / 2.0e-2  1.9e-5 / 5.1e-2  4.6e-4 / 6.8e-1  7.8e-6 / 2.2e-3  4.4e-4 / 1.3e-1
    The confident model (gold emission + 12) leaves gradients of about 1e-5 of a token's, so both columns grow; its
    reported loss is a small difference of two sums of about 4000: the 300-token sentence gives 0.546387 against
    0.546825 in fp64, 8.0e-4 relative (docs/architecture.md states this figure).
    """
    c = make_case(NT, B, L, seed=3, lens=_long_lens(B, L), **kw)
    ref = _ref(c)
    e32 = [_rel(a, b) for a, b in zip(_ref(c, torch.float32)[1], ref[1])]
    gates = [max(4.0 * e, 1e-5) for e in e32]
    got = _nll(c, _operands(c))
    errs = [_rel(a, b) for a, b in zip(_unpadded(c, got), ref[1])]
    print('\ncrf long {} NT={} B={} L={}'.format(name, NT, B, L))
    for k, nm in enumerate(NAMES):
        print('  {:8s} kernel {:.3e}  torch fp32 {:.3e}  gate {:.3e}'.format(nm, errs[k], e32[k], gates[k]))
    rows = []
    for b in range(B):   # the loss of one sentence: a B = 1 launch with inv = 1
        n = int(c.lens[b])
        one = SimpleNamespace(NT=NT, B=1, L=L, crf=c.crf, logits=c.logits[b:b + 1], tags=c.tags[b:b + 1],
                              lens=c.lens[b:b + 1])
        loss = _nll(one, _operands(one), inv=1.0)[0]
        want = c.crf.nll(one.logits, one.tags, one.lens).item() * n                    # log Z - gold score
        gold = path_score(c.crf, c.logits[b], c.tags[b, :n])
        bound = (n + 2) * 2.0 ** -23 * max(abs(want + gold), abs(gold))
        rows.append((abs(loss - want), bound, abs(loss - want) / abs(want), loss, want, n))
        print('  sentence {} n={} loss {:.6f} fp64 {:.6f} |diff| {:.3e} bound {:.3e} rel {:.3e}'.format(
            b, n, loss, want, *rows[-1][:3]))
    _check_nll(c, got, ref, gates)
    for diff, bound, *_ in rows:
        assert diff <= bound, rows


# ----------------------------------------------------------------------------------------------- 4. hard constraints
@pytest.mark.parametrize("NT", [12, 33])
@pytest.mark.parametrize("gold", ['legal', 'forbidden'])
def test_crf_nll_with_forbidden_transitions(NT, gold):
    c = make_case(NT, 5, 9, seed=4, forbid=True)
    tr = c.crf.trans.data
    assert int((tr == FORBID).sum()) == ((NT - 1) * (NT - 2)) // 2 and int((c.crf.start.data == FORBID).sum()) == 2
    if gold == 'forbidden':   # sentence 0 (full length) takes a forbidden transition at its first step
        i, j = (tr == FORBID).nonzero()[0].tolist()
        c.tags[0, 0], c.tags[0, 1] = i, j
    used = torch.stack([tr[c.tags[b, t - 1], c.tags[b, t]] for b in range(5) for t in range(1, int(c.lens[b]))])
    assert bool((used == FORBID).any()) == (gold == 'forbidden')
    ref = _ref(c)
    assert (ref[0] > 100.0) == (gold == 'forbidden')
    _check_nll(c, _nll(c, _operands(c)), ref)


@pytest.mark.parametrize("NT", [12, 33])
@torch.no_grad()
def test_crf_viterbi_with_forbidden_transitions(NT):
    c = make_case(NT, 5, 9, seed=4, forbid=True)
    got = _viterbi(c, _operands(c))
    for b, n in enumerate(c.lens.tolist()):
        y = got[b, :n]
        assert float(c.crf.start[y[0]]) > -1e3
        assert n == 1 or bool((c.crf.trans[y[:-1], y[1:]] > -1e3).all())
    _check_paths(c, got)
    assert torch.equal(got, _first_max32(c))


# ---------------------------------------------------------------------------- 5. Viterbi: addressing and exact paths
def _viterbi_lens(B, L):
    """Every sentence at full length but one of length 1 (sentence 0) and a short one (sentence 1): waves 2 and 3 of
    block 0 and all waves of the later blocks write every backpointer row next to a neighbour that does the same."""
    lens = torch.full((B,), L)
    lens[0], lens[1] = 1, L // 3
    return lens


# L = 256: the last length with the backpointers in LDS, 4 * 256 * 64 bytes = all 64 KiB, waves 1..3 at their full
# offsets; L >= 257: in the workspace, sentences 2..8 at theirs
@pytest.mark.parametrize("NT,B,L", [(5, 9, 256), (64, 4, 256), (5, 9, 257), (64, 6, 257), (33, 5, 300)])
@torch.no_grad()
def test_crf_viterbi_backpointer_addressing(NT, B, L):
    c = make_case(NT, B, L, seed=5, lens=_viterbi_lens(B, L))
    got = _viterbi(c, _operands(c))
    _check_paths(c, got)
    assert torch.equal(got, _first_max32(c))


EXACT = [(NT, 9, L) for NT in (1, 16, 17, 48, 64) for L in (1, 2, 13)] + [(17, 9, 257)]


@pytest.mark.parametrize("NT,B,L", EXACT)
@torch.no_grad()
def test_crf_viterbi_exact_paths_and_tie_break(NT, B, L):
    """Small integer scores: every fp32 sum is exact and ties are frequent, so the path itself is pinned — strict '>'
    over ascending predecessors, the lowest of the tied final tags."""
    c = make_case(NT, B, L, seed=6, integer=True, lens=_viterbi_lens(B, L) if L > 13 else None)
    want = torch.from_numpy(viterbi_first_max(*(p.detach().numpy() for p in (c.crf.trans, c.crf.start, c.crf.end)),
                                              c.logits.numpy(), c.lens.tolist()))
    got = _viterbi(c, _operands(c))
    assert torch.equal(got, want)
    _check_paths(c, got)


# --------------------------------------------------------------------------- 6. argument checks (nothing is launched)
def test_crf_argument_checks():
    lib = _lib.lib()
    for L, B, NT in [(5, 3, 0), (5, 3, 65), (0, 3, 7), (5, 0, 7), (-1, 3, 7), (5, -1, 7)]:
        assert lib.rk_crf_ws_bytes(L, B, NT) == 0, (L, B, NT)
    shapes = [(L, B, NT) for NT, B, L in EDGE_CASES + EXACT] + [(L, B, NT) for _, NT, B, L, _ in LONG] + \
        [(256, 9, 5), (256, 4, 64), (257, 9, 5), (257, 6, 64), (300, 5, 33)]
    for L, B, NT in shapes:
        NTP = _ntp(NT)
        need = max(4 * (L * B * NTP + 2 * L * B + B * (NTP * NTP + 2 * NTP)), 64 * L * B)
        assert lib.rk_crf_ws_bytes(L, B, NT) >= need, (L, B, NT)

    c = make_case(5, 2, 257, seed=8)
    lg, tr, st, en, dlens, ws = _operands(c)
    labels = c.tags.t().contiguous().int().to(DEV)
    inv = torch.ones(1, device=DEV)
    NTP = tr.shape[0]
    outs = [torch.full(s, 3.0, device=DEV) for s in ((c.L, c.B, NTP), (NTP, NTP), (NTP,), (NTP,), (4,))]
    tags = torch.full((c.B, c.L), -7, dtype=torch.int32, device=DEV)

    def nll(L, B, NT, ws_):
        return lib.rk_crf_nll(_p(lg), _p(tr), _p(st), _p(en), _p(labels), _p(dlens), L, B, NT, _p(inv),
                              *(_p(o) for o in outs), _p(ws_), _s())

    def vit(L, B, NT, ws_):
        return lib.rk_crf_viterbi(_p(lg), _p(tr), _p(st), _p(en), _p(dlens), L, B, NT, _p(tags), _p(ws_), _s())
    for f in (nll, vit):
        assert f(c.L, c.B, 0, ws) == EBADARG and f(c.L, c.B, 65, ws) == EBADARG
        assert f(c.L, c.B, c.NT, None) == EBADARG        # the loss kernel always needs the workspace, Viterbi at 257
        assert f(0, c.B, c.NT, ws) == 0 and f(c.L, 0, c.NT, ws) == 0
    torch.cuda.synchronize()
    assert all(bool((o == 3.0).all()) for o in outs) and bool((tags == -7).all())      # nothing ran
    # at L = 256 the backpointers are in LDS: no workspace needed, and the result is that of a call with one
    c = make_case(5, 2, 256, seed=8)
    ops = _operands(c)
    with_ws = _viterbi(c, ops)
    assert _viterbi(c, ops[:5] + [None]).equal(with_ws)
    assert torch.equal(with_ws, _first_max32(c))


# --------------------------------------------------------------------------------------------------------- 7. engine
def _twin(net, V, E, H, NT):
    ref = _net(V, E, H, NT).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in net.state_dict().items()})
    return ref


def _twin_logits(ref, x):
    return ref.out(ref.lstm(ref.emb(torch.from_numpy(x)))[0])


@pytest.mark.parametrize("V,E,H,NT,B,L", [(50, 37, 51, 45, 5, 7), (64, 21, 100, 17, 9, 11)])
@torch.no_grad()
def test_tagger_decode_matches_fp64_twin(V, E, H, NT, B, L):
    """The engine's paths score as the fp64 twin's best paths do under the fp64 model (the engine's logits are fp32, so
    the paths themselves may differ at near-ties), and -1 from lens[b] on."""
    torch.manual_seed(10)
    net = _net(V, E, H, NT).to(DEV)
    eng = TaggerEngine(net, lr=0.01, dropout=0.0)
    x, y = _token_batch(np.random.default_rng(11), B, L, V, NT)
    lens = (y != -100).sum(1)
    got = eng.decode(x, lens)
    assert got.shape == (B, L) and got.dtype == np.int32
    ref = _twin(net, V, E, H, NT)
    logits = _twin_logits(ref, x)
    best = ref.crf.decode(logits, torch.from_numpy(lens))
    for b, n in enumerate(lens.tolist()):
        assert (got[b, n:] == -1).all() and ((got[b, :n] >= 0) & (got[b, :n] < NT)).all()
        s_got, s_best = (path_score(ref.crf, logits[b], np.asarray(p[b, :n])) for p in (got, best))
        assert abs(s_got - s_best) <= 1e-4 * max(1.0, abs(s_best)), (b, s_got, s_best)
        assert s_got <= s_best + 1e-12 * max(1.0, abs(s_best))


@pytest.mark.parametrize("clip", [False, True])
def test_tagger_crf_adam_step_matches_fp64(clip):
    """One Adam step of the native CRF tagger, without and with a binding clip, against the fp64 twin stepped by
    clip_grad_norm_ + torch.optim.Adam, with the bounds of test_tagger_gpu.py::test_tagger_adam_update_matches_fp64
    (moments 1e-6 relative, weights 1e-6 absolute); the norm counts the CRF's three segments."""
    torch.manual_seed(12)
    V, E, H, NT, B, L = 13, 5, 3, 5, 3, 4
    lr, betas, eps = 0.02, (0.9, 0.999), 1e-8
    net = _net(V, E, H, NT).to(DEV)
    ref = _twin(net, V, E, H, NT)
    x, y = _token_batch(np.random.default_rng(13), B, L, V, NT)
    lens = torch.from_numpy((y != -100).sum(1))
    ref.crf.nll(_twin_logits(ref, x), torch.from_numpy(y), lens).backward()
    first = math.sqrt(sum(float(p.grad.pow(2).sum()) for p in ref.parameters()))
    no_crf = math.sqrt(sum(float(p.grad.pow(2).sum()) for k, p in ref.named_parameters() if not k.startswith('crf.')))
    assert first > no_crf * (1 + 1e-3)                     # the CRF's gradients are a visible part of the norm
    cap = 0.5 * first if clip else None
    eng = TaggerEngine(net, lr=lr, dropout=0.0, betas=betas, eps=eps, clip_norm=cap)
    before = {k: v.clone() for k, v in eng._unpad(eng.w).items()}
    eng.step(x, y, graph=False)
    torch.cuda.synchronize()
    if clip:
        norm = float(torch.nn.utils.clip_grad_norm_(ref.parameters(), cap))
        st = eng.grad_stats()
        print('crf tagger norm', st['last_norm'], 'fp64', norm)
        assert norm == pytest.approx(first, rel=1e-12)
        assert abs(st['last_norm'] - norm) <= 1e-5 * norm
        assert (st['clipped'], st['skipped'], st['steps']) == (1, 0, 1)
    arena = float(eng.g.double().cpu().norm())             # the pad region holds no gradient
    assert abs(arena - first) <= 1e-5 * first
    opt = torch.optim.Adam(ref.parameters(), lr=lr, betas=betas, eps=eps)
    opt.step()
    w, m, v = eng._unpad(eng.w), eng._unpad(eng.m), eng._unpad(eng.v)
    assert set(w) == {k for k, _ in ref.named_parameters()}
    for k, p in ref.named_parameters():
        ew = float((w[k].double().cpu() - p.detach()).abs().max())
        em, ev = _rel(m[k].cpu(), opt.state[p]['exp_avg']), _rel(v[k].cpu(), opt.state[p]['exp_avg_sq'])
        print('  {:28s} w abs {:.3e}  m rel {:.3e}  v rel {:.3e}'.format(k, ew, em, ev))
        assert ew < 1e-6 and em < 1e-6 and ev < 1e-6, (k, ew, em, ev)
    for k in ('crf.trans', 'crf.start', 'crf.end'):
        assert bool((w[k] != before[k]).all()), k           # every entry has a gradient, and Adam's first step is lr
    eng.store_module(net)
    for k, shape in (('trans', (NT, NT)), ('start', (NT,)), ('end', (NT,))):
        p = getattr(net.crf, k)
        assert p.shape == shape and torch.equal(p.detach(), w['crf.' + k])
        assert torch.equal(p.detach(), eng.seg(eng.w, 'crf_' + k)[(slice(0, NT),) * len(shape)])
        assert float((p.detach().double().cpu() - getattr(ref.crf, k).detach()).abs().max()) < 1e-6


def test_tagger_crf_workspace_cache_reuse():
    """The (L, B)-keyed workspace of a shape seen before — here with every byte overwritten in between — gives the
    gradients of a fresh engine's first step on the same batch, bit for bit."""
    torch.manual_seed(14)
    V, E, H, NT = 50, 37, 51, 45
    net = _net(V, E, H, NT).to(DEV)
    eng = TaggerEngine(net, lr=0.01, dropout=0.0)
    rng = np.random.default_rng(15)
    batches = [_token_batch(rng, B, L, V, NT) for B, L in ((5, 7), (3, 4), (5, 7))]
    ptr = None
    for k, (x, y) in enumerate(batches):
        if k == 2:
            eng._crf_ws[(7, 5)].fill_(0xFF)
        eng.step(x, y, update=False, graph=False)
        if k == 0:
            ptr = eng._crf_ws[(7, 5)].data_ptr()
    torch.cuda.synchronize()
    assert set(eng._crf_ws) == {(7, 5), (4, 3)} and eng._crf_ws[(7, 5)].data_ptr() == ptr
    fresh = TaggerEngine(net, lr=0.01, dropout=0.0)
    fresh.step(*batches[2], update=False, graph=False)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(eng.g).all()) and torch.equal(eng.g, fresh.g)
    assert eng.take_loss() > 0.0
