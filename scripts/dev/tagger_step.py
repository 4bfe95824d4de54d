"""Tagger training-step timing / kernel census (K18): PyBiLstm at E=37, H=51, 45 tags on the native
engine, batches of 32 sentences bucketed by length.  Prints one JSON line (ms/step, tokens/s).
``--crf`` times the BiLSTM-CRF step (the CRF loss / gradient kernel in place of the softmax cross-entropy),
``--gru`` the PyBiGru step (nn.GRU in place of nn.LSTM: the GRU recurrence kernels), ``--char`` the PyBiLstmChar step
(character-CNN word features beside the word embedding: the charcnn kernels; ``--Ec``, ``--F``, 60 characters),
``--attn`` the PyBiLstmAttn step (masked multi-head self-attention ahead of the output layer: the attn kernels;
``--heads``, ``--dh``).
Run under ``rocprofv3 --kernel-trace --stats`` for the step's kernel list."""
import argparse
import json
import time

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from rafiki_amd.engine.tagger import TaggerEngine


class Net(torch.nn.Module):
    def __init__(self, V, E, H, NT, gru=False, char=None, attn=None):
        super().__init__()
        self.emb = torch.nn.Embedding(V, E, padding_idx=0)
        if char:   # (CV, Ec, F)
            self.char_emb = torch.nn.Embedding(char[0], char[1], padding_idx=0)
            self.char_conv = torch.nn.Conv1d(char[1], char[2], 3, padding=1)
            E += char[2]
        if gru:
            self.gru = torch.nn.GRU(E, H, batch_first=True, bidirectional=True)
        else:
            self.lstm = torch.nn.LSTM(E, H, batch_first=True, bidirectional=True)
        if attn:   # (heads, head dims)
            from rafiki_amd.ops.attn import SelfAttention
            self.attn = SelfAttention(2 * H, *attn)
        self.out = torch.nn.Linear(2 * H, NT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--E', type=int, default=37)
    ap.add_argument('--H', type=int, default=51)
    ap.add_argument('--tags', type=int, default=45)
    ap.add_argument('--V', type=int, default=20000)
    ap.add_argument('--B', type=int, default=32)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--graph', type=int, default=1)
    ap.add_argument('--crf', action='store_true')
    ap.add_argument('--gru', action='store_true')
    ap.add_argument('--char', action='store_true')
    ap.add_argument('--Ec', type=int, default=25)
    ap.add_argument('--F', type=int, default=30)
    ap.add_argument('--attn', action='store_true')
    ap.add_argument('--heads', type=int, default=2)
    ap.add_argument('--dh', type=int, default=16)
    a = ap.parse_args()
    torch.manual_seed(0)
    CV = 60
    net = Net(a.V, a.E, a.H, a.tags, a.gru, (CV, a.Ec, a.F) if a.char else None,
              (a.heads, a.dh) if a.attn else None)
    if a.crf:
        from rafiki_amd.ops.crf import Crf
        net.crf = Crf(a.tags)
    net = net.cuda()
    eng = TaggerEngine(net, lr=0.05, dropout=0.1, seed=1)
    rng = np.random.default_rng(0)
    lengths = [8, 12, 16, 20, 24, 28, 32, 40]        # bucket lengths of a PTB-like corpus
    batches = []
    for L in lengths:
        x = rng.integers(1, a.V, (a.B, L))
        y = rng.integers(0, a.tags, (a.B, L))
        ch = None
        if a.char:                                    # word lengths 1..12, as English text has them
            ch = (rng.integers(2, CV, (a.B, L, 16)) * (np.arange(16) < rng.integers(1, 13, (a.B, L, 1)))).astype(np.uint8)
        batches.append((x, y, ch))
    for x, y, ch in batches * 2:                      # eager + capture per shape, then one replay
        eng.step(x, y, graph=bool(a.graph), chars=ch)
    torch.cuda.synchronize()
    eng.take_loss()
    t0 = time.perf_counter()
    toks = 0
    for i in range(a.steps):
        x, y, ch = batches[i % len(batches)]
        eng.step(x, y, graph=bool(a.graph), chars=ch)
        toks += x.size
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({'what': ('gru_' if a.gru else '') + ('char_' if a.char else '') + ('attn_' if a.attn else '')
                      + ('tagger_crf_step' if a.crf else 'tagger_step'),
                      'E': a.E, 'H': a.H, 'tags': a.tags, 'B': a.B, 'graph': a.graph,
                      'ms_per_step': round(1e3 * dt / a.steps, 4), 'tokens_per_s': round(toks / dt, 1),
                      'loss': eng.take_loss() / a.steps}))


if __name__ == '__main__':
    main()
