"""Character-level word features (the "CNN" of BiLSTM-CNN-CRF, Ma & Hovy 2016): the word encoder and the torch path.

A word is NCHAR = 16 character ids (uint8; 0 = padding, 1 = unknown character, then the training words' characters
by frequency, at most 256 ids in all); a longer word keeps its first 8 and last 8 characters.  ``char_features`` is
the network in torch: Embedding -> Conv1d(width 3, padding 1) -> max over the word's positions -> bias, with the
semantics of csrc/kernels/charcnn.hip (positions from the word's length on do not take part in the max, a token
without characters has all-zero features, ids outside the table read the zero padding row).  On the GPU in fp32 the
native tagger engine runs the fused kernels instead (engine/tagger.py); this is the CPU / bf16 / hidden > 128 path.
"""
from collections import Counter

import numpy as np

NCHAR = 16
MAX_IDS = 256
PAD, UNK = 0, 1


def build_char_dict(words) -> dict:
    """character -> id (2..255) of the characters of ``words``, the most frequent first (ties: first seen)."""
    counts = Counter(c for w in words for c in w)
    return {c: i + 2 for i, (c, _) in enumerate(counts.most_common(MAX_IDS - 2))}


def encode_word(word: str, char_dict: dict) -> np.ndarray:
    """[16] uint8 ids of a word: its characters as a prefix, zero-padded; beyond 16, the first 8 and the last 8."""
    if len(word) > NCHAR:
        word = word[:NCHAR // 2] + word[-(NCHAR // 2):]
    out = np.zeros(NCHAR, np.uint8)
    out[:len(word)] = [char_dict.get(c, UNK) for c in word]
    return out


def char_features(chars, emb, conv):
    """[..., F] features of chars [..., 16] (integer tensor) under emb = nn.Embedding(CV, Ec, padding_idx=0) and
    conv = nn.Conv1d(Ec, F, 3, padding=1)."""
    import torch
    import torch.nn.functional as F
    ids = chars.long().reshape(-1, NCHAR)
    n = (ids != 0).sum(1)
    valid = torch.arange(NCHAR, device=ids.device)[None, :] < n[:, None]
    ids = torch.where(ids < emb.num_embeddings, ids, torch.zeros_like(ids))
    x = emb(ids) * valid[..., None].to(emb.weight.dtype)
    c = F.conv1d(x.transpose(1, 2), conv.weight, None, padding=1)             # [N, F, 16]
    c = c.masked_fill(~valid[:, None, :], float('-inf')).max(2).values + conv.bias
    feat = torch.where((n > 0)[:, None], c, torch.zeros_like(c))
    return feat.reshape(chars.shape[:-1] + (-1,))
