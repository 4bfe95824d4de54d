"""Masked multi-head self-attention over a tagger's recurrent states (PyBiLstmAttn / PyBiLstmAttnCrf): the module, and
the computation in plain torch ops.  On the GPU in fp32 the native engine runs it on csrc/kernels/attn.hip
(engine/tagger.py); this file is the CPU / bf16 path and, in fp64, the reference of tests/test_attn_gpu.py."""
import math

import torch
import torch.nn as nn


def _live(lens, L: int, device) -> torch.Tensor:
    """[B, L] bool: position t of sentence b holds a token."""
    return torch.arange(L, device=device)[None, :] < torch.as_tensor(lens, device=device)[:, None]


def attention(qkv: torch.Tensor, lens, heads: int, with_lse: bool = False):
    """ctx [B, L, heads * dh] of qkv [B, L, 3 * heads * dh] (blocks q | k | v, each head-major): per sentence and
    head softmax(q k^T / sqrt(dh)) v over the keys j < lens[b].  Masked keys get exactly zero weight (fill, softmax,
    then a multiply by the key mask), so an empty sentence yields zeros and no NaN; query rows i >= lens[b] are zero
    as well.  with_lse: also lse [B, L, heads] = log sum_j exp(score), zero on those rows."""
    B, L, _ = qkv.shape
    dh = qkv.shape[-1] // (3 * heads)
    q, k, v = qkv.view(B, L, 3, heads, dh).permute(2, 0, 3, 1, 4)                      # each [B, heads, L, dh]
    live = _live(lens, L, qkv.device)
    keymask = live[:, None, None, :]
    s = ((q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(dh))).masked_fill(~keymask, -1e30)
    p = torch.softmax(s, -1) * keymask
    ctx = ((p @ v) * live[:, None, :, None]).transpose(1, 2).reshape(B, L, heads * dh)
    if not with_lse:
        return ctx
    return ctx, (torch.logsumexp(s, -1) * live[:, None, :]).transpose(1, 2)


class SelfAttention(nn.Module):
    """h + proj(attention(qkv(h))) over h [B, L, D]: every token reads every other token's state directly.  Positions
    past a sentence's length keep their h."""

    def __init__(self, dims: int, heads: int, head_dims: int):
        super().__init__()
        self.heads, self.head_dims = int(heads), int(head_dims)
        self.qkv = nn.Linear(dims, 3 * self.heads * self.head_dims)
        self.proj = nn.Linear(self.heads * self.head_dims, dims)

    def forward(self, h: torch.Tensor, lens) -> torch.Tensor:
        return h + self.proj(attention(self.qkv(h), lens, self.heads)) * _live(lens, h.shape[1], h.device)[..., None]
