"""The word encoder of ops/charcnn.py and PyBiLstmChar / PyBiLstmCharCrf on the torch path (CPU)."""
import numpy as np
import pytest
import torch

ACC_WORD, ACC_CHAR = 0.229, 0.616   # measured on the CPU: see test_char_features_tag_unseen_words_by_their_suffix


def test_encode_word_truncates_maps_unknowns_and_caps_the_vocabulary():
    from rafiki_amd.ops.charcnn import build_char_dict, encode_word
    d = build_char_dict(['abca', 'ab'])
    assert d == {'a': 2, 'b': 3, 'c': 4}                              # by frequency, 0 = pad and 1 = unknown kept free
    assert encode_word('cab?', d).tolist() == [4, 2, 3, 1] + [0] * 12
    long = encode_word('abababab' + 'x' * 9 + 'cccccccc', d)          # 25 characters: the first 8 and the last 8
    assert long.dtype == np.uint8 and long.tolist() == [2, 3] * 4 + [4] * 8
    big = build_char_dict([''.join(chr(0x400 + i) * (400 - i) for i in range(300))])
    assert len(big) == 254 and max(big.values()) == 255 and chr(0x400 + 254) not in big
    assert encode_word(chr(0x400 + 299), big).tolist() == [1] + [0] * 15


@pytest.mark.parametrize('name', ['PyBiLstmChar', 'PyBiLstmCharCrf'])
def test_pybilstmchar_trains_and_reloads_on_the_torch_path(name):
    from rafiki_amd.models import ZOO, pos_tagging
    cls = getattr(pos_tagging, name)
    knobs = dict(epochs=3, word_embed_dims=16, word_rnn_hidden_size=16, word_dropout=0.01, learning_rate=0.05,
                 batch_size=32, char_embed_dims=10, char_filters=20)
    m = cls(**knobs)
    m.train("synthetic://corpus?n=200&seed=0")
    assert m.evaluate("synthetic://corpus?n=50&seed=1") > 0.5
    queries = [["w1", "w20", "never-seen"], ["w3"]]
    m2 = cls(**knobs)
    m2.load_parameters(m.dump_parameters())
    assert m2.predict(queries) == m.predict(queries)
    assert ZOO[name] == ('pos_tagging.py', 'POS_TAGGING')
    assert {'char_embed_dims', 'char_filters'} <= set(cls.get_knob_config())


def test_char_features_tag_unseen_words_by_their_suffix(tmp_path):
    """Four tags, each decided by the word's three-letter suffix; the evaluation words share no stem with the
    training words, so PyBiLstm sees only the unknown id and can do no better than one tag for all.  Measured on the
    CPU: PyBiLstm 0.229, PyBiLstmChar 0.616 (ACC_WORD, ACC_CHAR); the bound is the midpoint of the two."""
    from rafiki_amd.model.dataset import write_corpus_zip
    from rafiki_amd.models.pos_tagging import PyBiLstm, PyBiLstmChar
    rng = np.random.default_rng(0)
    suffixes = ['ing', 'ely', 'ous', 'ment']

    def corpus(path, n, first):
        sents = []
        for _ in range(n):
            tags = rng.integers(0, 4, int(rng.integers(3, 9)))
            sents.append([[''.join(first[rng.integers(0, len(first), 4)]) + suffixes[t], int(t)] for t in tags])
        return write_corpus_zip(str(path), sents)

    train = corpus(tmp_path / 'train.zip', 300, np.array(list('abcdefghijkl')))
    test = corpus(tmp_path / 'test.zip', 60, np.array(list('mnopqrstuvwx')))
    knobs = dict(epochs=4, word_embed_dims=16, word_rnn_hidden_size=16, word_dropout=0.01, learning_rate=0.05,
                 batch_size=32)
    acc = {}
    for cls in (PyBiLstm, PyBiLstmChar):
        m = cls(**knobs, **({'char_embed_dims': 10, 'char_filters': 20} if cls is PyBiLstmChar else {}))
        torch.manual_seed(0)
        m.train(train)
        acc[cls.__name__] = m.evaluate(test)
    print(acc)
    assert acc['PyBiLstmChar'] > (ACC_WORD + ACC_CHAR) / 2, acc
