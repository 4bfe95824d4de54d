"""The torch linear-chain CRF (rafiki_amd/ops/crf.py) against brute force over all paths, and PyBiLstmCrf on the CPU."""
import itertools

import numpy as np
import pytest
import torch

from rafiki_amd.ops.crf import Crf


@pytest.mark.parametrize("NT,L", [(3, 1), (3, 4), (2, 5)])
@torch.no_grad()
def test_crf_matches_brute_force(NT, L):
    torch.manual_seed(NT * 10 + L)
    crf = Crf(NT).double()
    for p in crf.parameters():
        p.data.normal_()
    lens = sorted({L, max(1, L - 2), 1}, reverse=True) + [0]
    B = len(lens)
    logits = torch.randn(B, L, NT, dtype=torch.float64)
    tags = torch.randint(0, NT, (B, L))
    total, best = 0.0, []
    for b, n in enumerate(lens):
        if n == 0:
            best.append([])
            continue
        paths = list(itertools.product(range(NT), repeat=n))

        def score(y):
            s = crf.start[y[0]] + crf.end[y[-1]] + sum(logits[b, t, y[t]] for t in range(n))
            return s + sum(crf.trans[y[t - 1], y[t]] for t in range(1, n))
        scores = torch.stack([score(y) for y in paths])
        total += float(torch.logsumexp(scores, 0) - score(tags[b, :n].tolist()))
        best.append(list(paths[int(scores.argmax())]))
    assert float(crf.nll(logits, tags, lens)) == pytest.approx(total / max(1, sum(lens)), rel=1e-12, abs=1e-12)
    dec = crf.decode(logits, lens)
    for b, n in enumerate(lens):
        assert dec[b, :n].tolist() == best[b] and (dec[b, n:] == -1).all()


@pytest.mark.parametrize("NT,B,L", [(1, 3, 4), (5, 9, 13), (17, 4, 30)])
@torch.no_grad()
def test_first_max_viterbi_matches_crf_decode(NT, B, L):
    """tests/crf_refs.py's numpy Viterbi (the GPU tests' exact-path reference): the paths of Crf.decode where no two
    paths tie (random fp64 scores), their scores where they do (integer scores), and the lowest tags on a full tie."""
    from crf_refs import make_case, path_score, viterbi_first_max
    for integer in (False, True):
        c = make_case(NT, B, L, seed=7, integer=integer)
        ops = [p.detach().numpy() for p in (c.crf.trans, c.crf.start, c.crf.end)] + [c.logits.numpy(), c.lens]
        got, ref = viterbi_first_max(*ops), c.crf.decode(c.logits, c.lens)
        assert got.dtype == np.int64 and got.shape == (B, L)
        for b, n in enumerate(c.lens.tolist()):
            assert (got[b, n:] == -1).all() and (ref[b, n:] == -1).all()
            if integer:   # every sum is exact, so the two best scores are equal whichever of the tied paths was taken
                assert path_score(c.crf, c.logits[b], got[b, :n]) == path_score(c.crf, c.logits[b], ref[b, :n])
            else:
                assert got[b, :n].tolist() == ref[b, :n].tolist()
        ops32 = [a.astype(np.float32) for a in ops[:4]] + [c.lens]
        if integer:       # the fp32 run of the same exact sums takes the same path
            assert (viterbi_first_max(*ops32) == got).all()
    zeros = viterbi_first_max(np.zeros((NT, NT)), np.zeros(NT), np.zeros(NT), np.zeros((2, L, NT)), [L, 0])
    assert (zeros[0] == 0).all() and (zeros[1] == -1).all()
    if NT >= 3:           # two tied predecessors (1 and 2) and two tied final tags (1 and 2): the lower of each
        tr, en = np.zeros((NT, NT)), np.zeros(NT)
        st = np.full(NT, -5.0)
        st[1] = st[2] = 0.0
        en[0] = -1.0
        assert viterbi_first_max(tr, st, en, np.zeros((1, 2, NT)), [2]).tolist() == [[1, 1]]


def test_pybilstmcrf_cpu_trains_predicts_and_reloads():
    from rafiki_amd.models.pos_tagging import PyBiLstmCrf
    knobs = dict(epochs=2, word_embed_dims=16, word_rnn_hidden_size=16, word_dropout=0.01, learning_rate=0.05,
                 batch_size=32)
    m = PyBiLstmCrf(**knobs)
    m.train("synthetic://corpus?n=200&seed=0")
    queries = [["a", "b", "c"], ["d"], ["e", "f", "g", "h", "i"]]
    out = m.predict(queries)
    assert [len(o) for o in out] == [3, 1, 5] and all(0 <= t < m._tag_count for o in out for t in o)
    params = m.dump_parameters()
    m2 = PyBiLstmCrf(**knobs)
    m2.load_parameters(params)
    assert m2.predict(queries) == out
    from rafiki_amd.models import ZOO
    assert ZOO['PyBiLstmCrf'] == ('pos_tagging.py', 'POS_TAGGING')
