"""Native BiLSTM tagger training step (PyBiLstm on the GPU).

Reference: examples/models/pos_tagging/PyBiLstm.py:185-235 (train loop: Adam, cross-entropy over the
padded batch), :249-268 (Embedding(V, E, padding_idx=0) -> Dropout -> BiLSTM(E, H) -> Linear(2H, tags)).

Every kernel of a step is in-tree (csrc/kernels): embedding gather fused with the Philox dropout mask
(tagger.hip), the input projection / output layer / all weight and data gradients on ``sgemm`` (f32.py
linear, linear_dx, linear_dw, colsum), the recurrence forward and BPTT as one persistent launch each
(lstm.hip), softmax cross-entropy with ignore_index and a device 1/#tokens scale (loss_optim.hip),
the embedding gradient as ordered run sums over host-sorted ids (tagger.hip), and one Adam launch
over a flat parameter arena (loss_optim.hip).

Layout: every extent is zero-padded once, in the arena, so any knob value stays on the in-tree
kernels — E and the tag count to multiples of 4 (16-B GEMM rows), the hidden size per gate block to
HP in {64, 128} (the recurrence kernels' tiles).  Padded rows / columns start at zero, receive
exactly zero gradient (zero activations in, zero upstream gradient out) and so stay zero under Adam:
the arena trains exactly the unpadded model.  nn.LSTM's two bias vectors are kept as two parameters
(each gets the full bias gradient), as torch's Adam sees them.

A step of a batch shape (L, B) is captured into a hipGraph the first time that shape is seen (after
an eager run that autotunes its GEMMs) and replayed afterwards; sentences are bucketed by length, so
the number of distinct shapes is the number of distinct bucket lengths.  Per step the host packs ids,
labels, the embedding-gradient runs and 1/#tokens into one int32 buffer and sends it with a single
async copy from pinned memory (double-buffered, so packing batch k+1 overlaps step k on the GPU).
The device step counter drives both Adam's bias corrections and the dropout stream, so replays draw
fresh masks.

A net with a ``crf`` attribute (ops/crf.py: PyBiLstmCrf) trains on the linear-chain CRF's sentence-level loss
instead: ``crf_trans`` / ``crf_start`` / ``crf_end`` follow ``b_out`` in the arena, ``rk_crf_nll`` (crf.hip) takes
the place of the softmax cross-entropy and writes d(logits) and the three CRF gradients, the batch carries its
sentence lengths, and ``decode`` runs Viterbi on the eval logits.  Without one, the arena layout, the launches and
the captured graphs are the softmax step's.

A net with a ``gru`` attribute (nn.GRU in place of ``lstm``: PyBiGru, PyBiGruCrf) takes the GRU step: three gate
blocks [r | z | n] in ``w_ih`` / ``w_hh`` / ``b_ih`` / ``b_hh``, the recurrence on gru.hip.  The candidate gate
multiplies W_hn h + b_hn by r, so the input projection carries b_ih alone and the kernel adds b_hh; BPTT returns
two gate-gradient matrices, dgin for W_ih, b_ih and the embedding, dgh for W_hh and b_hh.  Everything else (arena,
output layer, softmax or CRF loss, clip, Adam, graphs) is shared.

A net with ``char_emb`` (nn.Embedding(CV, Ec, padding_idx=0)) and ``char_conv`` (nn.Conv1d(Ec, F, 3, padding=1)) takes
the char step (PyBiLstmChar, PyBiLstmCharCrf; either cell, either loss): every token also carries 16 character ids,
``rk_charcnn_fwd`` (charcnn.hip) turns them into F word features (gather, width-3 convolution, max over the word's
positions, bias, dropout from a stream id of its own) and the recurrence's input is [x | xc].  The arena keeps the
input weights' columns E: as a segment of their own (``w_ihc``), so the word path is untouched: gin = x W_ih^T + b as
before, plus xc W_ihc^T.  ``char_emb`` (CV, EcP), ``char_w`` (FP, 3, EcP: K contiguous, torch's Conv1d.weight is
[F][Ec][3]), ``char_b`` and ``w_ihc`` follow the other segments; EcP in {16, 32}, FP a multiple of 16 up to 64.
``rk_charcnn_bwd`` writes the three char gradients into the gradient arena ahead of the clip sum and Adam.  Without
the char layers the arena layout, the launches and the graphs are as above.

A net with an ``attn`` attribute (ops/attn.py SelfAttention over the 2H recurrent states: PyBiLstmAttn, PyBiLstmAttnCrf;
either cell, either loss, with or without the char layers) takes the attention step between the recurrence and the
output layer: qkv = h W_qkv^T + b on ``S.linear``, ``rk_attn_fwd`` (attn.hip: masked softmax(q k^T / sqrt(dh)) v per
sentence and head, ctx and the log-sum-exp), h' = h + ctx W_o^T + b_o, and the output layer reads h'.  The backward
takes dh' from the output layer, W_o's gradients and dctx from it, ``rk_attn_bwd`` (d(qkv), P recomputed from the
log-sum-exp), W_qkv's gradients, and hands dh' + d(qkv) W_qkv to the BPTT kernel.  ``attn_wqkv`` (3 NH DP, 2, HP),
``attn_bqkv``, ``attn_wo`` (2, HP, NH DP) and ``attn_bo`` follow all other segments, the head dim zero-padded to DP in
{16, 32}; the batch carries its sentence lengths as for the CRF.  On rows past a sentence's length ctx is zero and the
engine's h' is h + b_o, where ops/attn.py keeps h: d(logits) is zero there, so the loss and every gradient agree, and
only ``logits()`` at padded positions differs between the two paths.  Without ``attn`` nothing above changes.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ..ops import _lib
from ..ops import f32 as S
from ..ops import graphs
from ..ops.functional import _p, _s
from .flat import GradClip, check_clip_norm

IGNORE = -100
_DROP_STREAM = 0x7a67   # Philox stream id of the tagger's dropout
_CHAR_STREAM = 0x6368   # and of the dropout on the char features
NCHAR = 16              # character ids a token carries (uint8, 0 = padding)


def _cdiv(a: int, b: int) -> int:
    return -(-a // b)


def pack_batch(x_bl: np.ndarray, y_bl, padding_idx: int = 0, vocab: Optional[int] = None, lens=None,
               chars=None) -> np.ndarray:
    """One batch as the int32 words the step reads: x_bl / y_bl are [B, L] (batch-first, like the
    reference's batches; labels IGNORE where no token).  Layout, with n = L*B tokens in time-major
    order (t, b): [ids n | labels n | perm n | run ids n | run starts n+1 | #runs | 1/#labelled as
    float bits].  perm is the stable argsort of the ids; run u covers perm[start[u]:start[u+1]] and
    has id uniq[u] (-1 for the padding id: no gradient).  With ``vocab``, ids outside [0, vocab) become
    the padding id, as the forward's gather treats them (no gradient row is written for them).  With ``lens``
    ([B] sentence lengths, read by the CRF and the attention steps) B more words follow; with ``chars`` ([B, L, 16]
    uint8 character ids, read by the char step) n * 4 more, the ids time-major [n][16]; without either, the layout is
    as above."""
    B, L = x_bl.shape
    n = B * L
    ids = np.ascontiguousarray(x_bl.T, dtype=np.int32).reshape(-1)
    if vocab is not None:
        ids = np.where((ids < 0) | (ids >= vocab), np.int32(padding_idx), ids)
    if y_bl is None:
        labels = np.full(n, IGNORE, np.int32)
    else:
        labels = np.ascontiguousarray(y_bl.T, dtype=np.int32).reshape(-1)
    perm = np.argsort(ids, kind='stable').astype(np.int32)
    s = ids[perm]
    starts = np.flatnonzero(np.diff(s)) + 1 if n > 1 else np.zeros(0, np.int64)
    starts = np.concatenate(([0], starts, [n])).astype(np.int32)
    uniq = s[starts[:-1]].astype(np.int32)
    uniq[uniq == padding_idx] = -1
    U = len(uniq)
    cnt = int((labels != IGNORE).sum())
    nl = 0 if lens is None else B
    out = np.zeros(5 * n + 3 + nl + (0 if chars is None else 4 * n), np.int32)
    out[0:n] = ids
    out[n:2 * n] = labels
    out[2 * n:3 * n] = perm
    out[3 * n:3 * n + U] = uniq
    out[4 * n:4 * n + U + 1] = starts
    out[5 * n + 1] = U
    out[5 * n + 2:5 * n + 3] = np.array([1.0 / max(1, cnt)], np.float32).view(np.int32)
    if lens is not None:
        out[5 * n + 3:5 * n + 3 + B] = lens
    if chars is not None:
        out[5 * n + 3 + nl:] = _chars_tm(chars, B, L).view(np.int32)
    return out


def _chars_tm(chars, B: int, L: int) -> np.ndarray:
    """[B, L, 16] uint8 character ids as time-major bytes [L * B * 16]."""
    c = np.asarray(chars)
    if c.shape != (B, L, NCHAR) or c.dtype != np.uint8:
        raise ValueError('chars must be uint8 [B, L, {}] (got {} {})'.format(NCHAR, c.dtype, c.shape))
    return np.ascontiguousarray(c.transpose(1, 0, 2)).reshape(-1)


class TaggerEngine:
    """Flat padded parameters + Adam state of one PyBiLstm ``Net`` (attributes emb, lstm or gru, out), and its
    training step on the in-tree kernels.  ``step`` takes batch-first numpy ids / labels.  ``clip_norm`` (None: off;
    > 0: the cap on the global gradient norm; inf: measure only): one sum-of-squares launch over the gradient arena
    right before the Adam launch, which reads the coefficient on the device — both inside the step's graph."""

    def __init__(self, net, lr: float, dropout: float, *, seed: int = 0, betas=(0.9, 0.999), eps=1e-8,
                 clip_norm: Optional[float] = None):
        dev = net.emb.weight.device
        assert dev.type == 'cuda', 'TaggerEngine runs on the GPU kernels'
        V, E = net.emb.weight.shape
        self.gru = hasattr(net, 'gru')   # the GRU cell (gru.hip) in place of the LSTM: three gate blocks
        cell = net.gru if self.gru else net.lstm
        H = cell.hidden_size
        NT = net.out.out_features
        if H > 128 or cell.num_layers != 1 or not cell.bidirectional:
            raise ValueError('TaggerEngine: one bidirectional layer of hidden <= 128 (got {})'.format(H))
        self.crf = hasattr(net, 'crf')   # a linear-chain CRF (ops/crf.py) in place of the per-token softmax
        if self.crf and NT > 64:
            raise ValueError('TaggerEngine: the CRF kernels take at most 64 tags (got {})'.format(NT))
        self.V, self.E, self.H, self.NT = V, E, H, NT
        self.char = hasattr(net, 'char_emb')   # character-CNN word features (charcnn.hip) beside the word embedding
        if self.char:
            CV, Ec = net.char_emb.weight.shape
            conv = net.char_conv
            F = conv.out_channels
            if conv.kernel_size != (3,) or conv.padding != (1,) or conv.in_channels != Ec or conv.bias is None:
                raise ValueError('TaggerEngine: char_conv must be Conv1d(Ec, F, 3, padding=1) with a bias')
            if not (CV <= 256 and Ec <= 32 and F <= 64 and net.char_emb.padding_idx == 0):
                raise ValueError('TaggerEngine: the char kernels take <= 256 characters, Ec <= 32, F <= 64, '
                                 'padding_idx 0 (got {}, {}, {})'.format(CV, Ec, F))
            if cell.input_size != E + F:
                raise ValueError('TaggerEngine: the cell\'s input must be [word | char] features')
            self.CV, self.Ec, self.F = CV, Ec, F
            self.EcP, self.FP = (16 if Ec <= 16 else 32), _cdiv(F, 16) * 16
        self.attn = hasattr(net, 'attn')   # masked multi-head self-attention (attn.hip) ahead of the output layer
        if self.attn:
            NH, dh = net.attn.heads, net.attn.head_dims
            if not (1 <= NH <= 8 and 1 <= dh <= 32):
                raise ValueError('TaggerEngine: the attention kernels take heads <= 8 and head_dims <= 32 '
                                 '(got {}, {})'.format(NH, dh))
            if net.attn.qkv.in_features != 2 * H or net.attn.proj.out_features != 2 * H:
                raise ValueError('TaggerEngine: attn must read and write the 2H recurrent states')
            self.NH, self.dh, self.DP = NH, dh, (16 if dh <= 16 else 32)
        self.EP, self.HP, self.NTP = _cdiv(E, 4) * 4, (64 if H <= 64 else 128), _cdiv(NT, 4) * 4
        self.padding_idx = net.emb.padding_idx if net.emb.padding_idx is not None else -1
        HP, EP, NTP = self.HP, self.EP, self.NTP
        NG = self.NG = 3 if self.gru else 4                              # gate blocks of HP units each
        shapes = [('emb', (V, EP)), ('w_ih', (2, NG * HP, EP)), ('w_hh', (2, NG * HP, HP)), ('b_ih', (2, NG * HP)),
                  ('b_hh', (2, NG * HP)), ('w_out', (NTP, 2 * HP)), ('b_out', (NTP,))]
        if self.crf:
            shapes += [('crf_trans', (NTP, NTP)), ('crf_start', (NTP,)), ('crf_end', (NTP,))]
        if self.char:
            shapes += [('char_emb', (self.CV, self.EcP)), ('char_w', (self.FP, 3, self.EcP)), ('char_b', (self.FP,)),
                       ('w_ihc', (2, NG * HP, self.FP))]
        if self.attn:
            AD = self.NH * self.DP
            shapes += [('attn_wqkv', (3 * AD, 2, HP)), ('attn_bqkv', (3 * AD,)), ('attn_wo', (2, HP, AD)),
                       ('attn_bo', (2, HP))]
        self._seg, o = {}, 0
        for k, sh in shapes:
            self._seg[k] = (o, sh)
            o += int(np.prod(sh))
        self.numel = o
        f = dict(device=dev, dtype=torch.float32)
        self.w, self.g, self.m, self.v = (torch.zeros(o, **f) for _ in range(4))
        self.ctr = torch.zeros(4, device=dev, dtype=torch.int32)       # [0]: steps taken (Adam t, dropout)
        self.loss_sum = torch.zeros(4, **f)                              # [0]: sum of batch-mean losses
        self.clip = None if check_clip_norm(clip_norm) is None else GradClip(self.g, clip_norm)
        self.whhT = torch.empty((2, HP, NG * HP), **f)
        self.bsum = None if self.gru else torch.empty(8 * HP, **f)       # the LSTM's b_ih + b_hh
        self.lr, self.p, self.seed = float(lr), float(dropout), int(seed) & ((1 << 63) - 1)
        self.betas, self.eps = betas, eps
        self.device = dev
        self._graphs, self._inbuf, self._pool = {}, {}, None
        self._crf_ws = {}                                                # (L, B) -> the CRF kernels' workspace
        self._char_ws = {}                                               # (L, B) -> rk_charcnn_bwd's workspace
        self._pinned, self._events, self._flip = [None, None], [None, None], 0
        self.load_module(net)

    # ------------------------------------------------------------------------ parameters
    def seg(self, t: torch.Tensor, k: str) -> torch.Tensor:
        o, sh = self._seg[k]
        return t[o:o + int(np.prod(sh))].view(sh)

    @torch.no_grad()
    def load_module(self, net):
        E, H, HP, NT, NG = self.E, self.H, self.HP, self.NT, self.NG
        self.w.zero_()
        self.seg(self.w, 'emb')[:, :E] = net.emb.weight.float()
        for d, suf in enumerate(('', '_reverse')):
            l = net.gru if self.gru else net.lstm
            w_ih = getattr(l, 'weight_ih_l0' + suf).float()
            self.seg(self.w, 'w_ih').view(2, NG, HP, self.EP)[d, :, :H, :E] = w_ih[:, :E].reshape(NG, H, E)
            if self.char:   # the columns E: multiply the char features
                self.seg(self.w, 'w_ihc').view(2, NG, HP, self.FP)[d, :, :H, :self.F] = \
                    w_ih[:, E:].reshape(NG, H, self.F)
            self.seg(self.w, 'w_hh').view(2, NG, HP, HP)[d, :, :H, :H] = \
                getattr(l, 'weight_hh_l0' + suf).float().view(NG, H, H)
            self.seg(self.w, 'b_ih').view(2, NG, HP)[d, :, :H] = getattr(l, 'bias_ih_l0' + suf).float().view(NG, H)
            self.seg(self.w, 'b_hh').view(2, NG, HP)[d, :, :H] = getattr(l, 'bias_hh_l0' + suf).float().view(NG, H)
        self.seg(self.w, 'w_out').view(self.NTP, 2, HP)[:NT, :, :H] = net.out.weight.float().view(NT, 2, H)
        self.seg(self.w, 'b_out')[:NT] = net.out.bias.float()
        if self.crf:
            self.seg(self.w, 'crf_trans')[:NT, :NT] = net.crf.trans.float()
            self.seg(self.w, 'crf_start')[:NT] = net.crf.start.float()
            self.seg(self.w, 'crf_end')[:NT] = net.crf.end.float()
        if self.char:
            Ec, F = self.Ec, self.F
            self.seg(self.w, 'char_emb')[:, :Ec] = net.char_emb.weight.float()
            self.seg(self.w, 'char_w')[:F, :, :Ec] = net.char_conv.weight.float().permute(0, 2, 1)   # [F][Ec][3]
            self.seg(self.w, 'char_b')[:F] = net.char_conv.bias.float()
        if self.attn:
            for k, v in self._attn_views(self.w).items():
                v.copy_(net.state_dict()[k].float().view(v.shape))

    def _attn_views(self, t: torch.Tensor) -> dict:
        """The unpadded regions of an arena's attention segments, by the module's parameter names (rows of qkv are
        (q | k | v, head, d), the 2H states are (direction, unit))."""
        NH, dh, DP, H, HP = self.NH, self.dh, self.DP, self.H, self.HP
        return {'attn.qkv.weight': self.seg(t, 'attn_wqkv').view(3, NH, DP, 2, HP)[:, :, :dh, :, :H],
                'attn.qkv.bias': self.seg(t, 'attn_bqkv').view(3, NH, DP)[:, :, :dh],
                'attn.proj.weight': self.seg(t, 'attn_wo').view(2, HP, NH, DP)[:, :H, :, :dh],
                'attn.proj.bias': self.seg(t, 'attn_bo')[:, :H]}

    def _unpad(self, t: torch.Tensor) -> dict:
        """Module-shaped views (copies) of an arena (weights or gradients)."""
        E, H, HP, NT, NG = self.E, self.H, self.HP, self.NT, self.NG
        cell = 'gru.' if self.gru else 'lstm.'
        out = {'emb.weight': self.seg(t, 'emb')[:, :E].clone(),
               'out.weight': self.seg(t, 'w_out').view(self.NTP, 2, HP)[:NT, :, :H].reshape(NT, 2 * H).clone(),
               'out.bias': self.seg(t, 'b_out')[:NT].clone()}
        if self.crf:
            out.update({'crf.trans': self.seg(t, 'crf_trans')[:NT, :NT], 'crf.start': self.seg(t, 'crf_start')[:NT],
                        'crf.end': self.seg(t, 'crf_end')[:NT]})
        if self.char:
            Ec, F = self.Ec, self.F
            out.update({'char_emb.weight': self.seg(t, 'char_emb')[:, :Ec],
                        'char_conv.weight': self.seg(t, 'char_w')[:F, :, :Ec].permute(0, 2, 1),
                        'char_conv.bias': self.seg(t, 'char_b')[:F]})
        if self.attn:
            AD = self.NH * self.dh
            shapes = {'attn.qkv.weight': (3 * AD, 2 * H), 'attn.qkv.bias': (3 * AD,), 'attn.proj.weight': (2 * H, AD),
                      'attn.proj.bias': (2 * H,)}
            out.update({k: v.reshape(shapes[k]) for k, v in self._attn_views(t).items()})
        for d, suf in enumerate(('', '_reverse')):
            w_ih = self.seg(t, 'w_ih').view(2, NG, HP, self.EP)[d, :, :H, :E].reshape(NG * H, E)
            if self.char:
                w_ihc = self.seg(t, 'w_ihc').view(2, NG, HP, self.FP)[d, :, :H, :self.F].reshape(NG * H, self.F)
                w_ih = torch.cat([w_ih, w_ihc], 1)
            out[cell + 'weight_ih_l0' + suf] = w_ih
            out[cell + 'weight_hh_l0' + suf] = self.seg(t, 'w_hh').view(2, NG, HP, HP)[d, :, :H, :H].reshape(NG * H, H)
            out[cell + 'bias_ih_l0' + suf] = self.seg(t, 'b_ih').view(2, NG, HP)[d, :, :H].reshape(NG * H)
            out[cell + 'bias_hh_l0' + suf] = self.seg(t, 'b_hh').view(2, NG, HP)[d, :, :H].reshape(NG * H)
        return {k: v.contiguous().clone() for k, v in out.items()}

    @torch.no_grad()
    def store_module(self, net):
        sd = net.state_dict()
        for k, v in self._unpad(self.w).items():
            sd[k].copy_(v.to(sd[k].dtype))

    def grads(self) -> dict:
        return self._unpad(self.g)

    def state(self) -> dict:
        return {'w': self.w.cpu(), 'm': self.m.cpu(), 'v': self.v.cpu(), 'ctr': self.ctr.cpu(), 'seed': self.seed}

    def load_state(self, st: dict):
        for k in ('w', 'm', 'v', 'ctr'):
            getattr(self, k).copy_(st[k])
        self.seed = int(st['seed'])

    # ------------------------------------------------------------------------ the step
    def _body(self, ib: torch.Tensor, L: int, B: int, update: bool = True):
        n, HP, EP, NTP = L * B, self.HP, self.EP, self.NTP
        dev, f, s = self.device, torch.float32, _s()
        ids, labels, perm = ib[0:n], ib[n:2 * n], ib[2 * n:3 * n]
        uniq, starts, nruns = ib[3 * n:4 * n], ib[4 * n:5 * n + 1], ib[5 * n + 1:5 * n + 2]
        inv = ib[5 * n + 2:5 * n + 3]
        W, G = self.w, self.g
        if update:   # t of Adam's bias corrections and the dropout stream's step
            _lib.call("rk_add_int", _p(self.ctr), 1, s)
        x = torch.empty((n, EP), device=dev, dtype=f)
        mask = torch.empty((n, EP), device=dev, dtype=f) if self.p > 0 else None
        _lib.call("rk_tag_embed_fwd", _p(ids), _p(self.seg(W, 'emb')), _p(x), _p(mask), n, EP, self.V, self.p,
                  self.seed, _DROP_STREAM, _p(self.ctr), s)
        self.last_mask = mask   # (tests: the dropout multipliers of the latest eager step, time-major rows)
        w_ih = self.seg(W, 'w_ih').view(2 * self.NG * HP, EP)
        xc = None
        if self.char:
            chars = ib[5 * n + 3 + (B if self.crf or self.attn else 0):]
            cmask = torch.empty((n, self.FP), device=dev, dtype=f) if self.p > 0 else None
            xc, amax = self._char_fwd(chars, n, self.p, self.seed, _CHAR_STREAM, self.ctr, cmask)
            self.last_char_mask = cmask
        hout, saved = self._recurrence_fwd(x, L, B, xc)
        h2 = hout.view(n, 2 * HP)
        w_out = self.seg(W, 'w_out')
        h2a = h2   # what the output layer reads
        if self.attn:
            dlens = ib[5 * n + 3:5 * n + 3 + B]
            h2a, qkv, ctx, lse = self._attn_fwd(h2, dlens, L, B)
        logits = S.linear(h2a, w_out, self.seg(W, 'b_out'))
        dlog = torch.empty((n, NTP), device=dev, dtype=f)
        if self.crf:   # loss, d(logits) and the three CRF gradients (into the arena, ahead of the clip sum and Adam)
            _lib.call("rk_crf_nll", _p(logits), _p(self.seg(W, 'crf_trans')), _p(self.seg(W, 'crf_start')),
                      _p(self.seg(W, 'crf_end')), _p(labels), _p(ib[5 * n + 3:5 * n + 3 + B]), L, B, self.NT, _p(inv),
                      _p(dlog), _p(self.seg(G, 'crf_trans')), _p(self.seg(G, 'crf_start')), _p(self.seg(G, 'crf_end')),
                      _p(self.loss_sum), _p(self._crf_workspace(L, B)), s)
        else:
            _lib.call("rk_softmax_xent_f32s", _p(logits), NTP, _p(labels), n, self.NT, IGNORE, _p(inv), _p(dlog), NTP,
                      _p(self.loss_sum), s)
        S.linear_dw(dlog, h2a, out=self.seg(G, 'w_out'))
        S.colsum(dlog, self.seg(G, 'b_out'))
        dh = S.linear_dx(dlog, w_out)
        if self.attn:   # dh is d(h'): the projection's gradients and dctx, the fused backward, then dh += dqkv W_qkv
            AD = self.NH * self.DP
            wqkv, wo = self.seg(W, 'attn_wqkv').view(3 * AD, 2 * HP), self.seg(W, 'attn_wo').view(2 * HP, AD)
            S.linear_dw(dh, ctx, out=self.seg(G, 'attn_wo').view(2 * HP, AD))
            S.colsum(dh, self.seg(G, 'attn_bo').view(-1))
            dctx = S.linear_dx(dh, wo)
            dqkv = torch.empty((n, 3 * AD), device=dev, dtype=f)
            _lib.call("rk_attn_bwd", _p(qkv), _p(dlens), _p(ctx), _p(lse), _p(dctx), L, B, self.NH, self.DP,
                      self.dh ** -0.5, _p(dqkv), s)
            S.linear_dw(dqkv, h2, out=self.seg(G, 'attn_wqkv').view(3 * AD, 2 * HP))
            S.colsum(dqkv, self.seg(G, 'attn_bqkv'))
            _lib.call("rk_tag_add", _p(dh), _p(S.linear_dx(dqkv, wqkv)), _p(dh), dh.numel(), s)
        GH = self.NG * HP
        _lib.call("rk_tag_transpose", _p(self.seg(W, 'w_hh')), _p(self.whhT), 2, GH, HP, s)
        dg = torch.empty((L, B, 2, GH), device=dev, dtype=f)       # d(gin): W_ih, b_ih, the embedding
        if self.gru:   # and d(W_hh h + b_hh), which differs in the candidate block (da_n * r)
            dgh = torch.empty((L, B, 2, GH), device=dev, dtype=f)
            _lib.call("rk_gru_bwd32", _p(self.whhT), L, B, HP, _p(dh), _p(hout), _p(saved[0]), _p(saved[1]), _p(dg),
                      _p(dgh), s)
        else:
            dgh = dg
            _lib.call("rk_lstm_bwd32", _p(self.whhT), L, B, HP, _p(dh), _p(saved[0]), _p(saved[1]), _p(dg), s)
        dg2, dgh2 = dg.view(n, 2 * GH), dgh.view(n, 2 * GH)
        S.linear_dw(dg2, x, out=self.seg(G, 'w_ih').view(2 * GH, EP))
        g_hh = self.seg(G, 'w_hh')
        if L > 1:   # h_{t-1} of the forward direction, h_{t+1} of the reverse one (zero initial state)
            S.linear_dw(dgh2[B:, :GH], h2[:-B, :HP], out=g_hh[0])
            S.linear_dw(dgh2[:-B, GH:], h2[B:, HP:], out=g_hh[1])
        else:
            _lib.call("rk_zero32", _p(g_hh), g_hh.numel(), s)
        S.colsum(dg2, self.seg(G, 'b_ih').view(-1))
        if self.gru:
            S.colsum(dgh2, self.seg(G, 'b_hh').view(-1))
        else:
            _lib.call("rk_tag_add", _p(self.seg(G, 'b_ih')), None, _p(self.seg(G, 'b_hh')), 8 * HP, s)
        if self.char:   # the char features' share of the input projection, then the fused char backward
            w_ihc = self.seg(W, 'w_ihc').view(2 * GH, self.FP)
            S.linear_dw(dg2, xc, out=self.seg(G, 'w_ihc').view(2 * GH, self.FP))
            gxc = S.linear_dx(dg2, w_ihc)
            _lib.call("rk_charcnn_bwd", _p(chars), _p(self.seg(W, 'char_emb')), _p(self.seg(W, 'char_w')), _p(gxc),
                      _p(cmask), _p(amax), n, self.EcP, self.FP, self.CV, _p(self.seg(G, 'char_w')),
                      _p(self.seg(G, 'char_b')), _p(self.seg(G, 'char_emb')), _p(self._char_workspace(L, B)), s)
        gx = S.linear_dx(dg2, w_ih)
        g_emb = self.seg(G, 'emb')
        _lib.call("rk_zero32", _p(g_emb), g_emb.numel(), s)
        _lib.call("rk_tag_embed_bwd", _p(perm), _p(uniq), _p(starts), _p(nruns), _p(gx), _p(mask), _p(g_emb), n, EP,
                  self.V, s)
        if update:
            b1, b2 = self.betas
            adam = (_p(self.w), None, _p(self.g), _p(self.m), _p(self.v), self.numel, self.lr, b1, b2, 1.0 - b1,
                    1.0 - b2, self.eps, 0.0, 0, 1.0, 1.0, 1.0, None, _p(self.ctr))
            if self.clip is None:
                _lib.call("rk_adam_step", *adam, s)
            else:
                partials, max_norm, stats = self.clip.reduce(self.g)
                _lib.call("rk_adam_step_clip", *adam, _p(partials), partials.numel(), max_norm, _p(stats), s)

    def _char_fwd(self, chars: torch.Tensor, n: int, p: float, seed: int, stream_id: int, ctr, cmask):
        """xc [n, FP] char features (dropout multipliers into cmask when p > 0) and amax [n, FP] of chars, the
        device words holding [n][16] uint8 ids."""
        xc = torch.empty((n, self.FP), device=self.device, dtype=torch.float32)
        amax = torch.empty((n, self.FP), device=self.device, dtype=torch.int32)
        _lib.call("rk_charcnn_fwd", _p(chars), _p(self.seg(self.w, 'char_emb')), _p(self.seg(self.w, 'char_w')),
                  _p(self.seg(self.w, 'char_b')), n, self.EcP, self.FP, self.CV, p, seed, stream_id, _p(ctr), _p(xc),
                  _p(cmask), _p(amax), _s())
        return xc, amax

    def _attn_fwd(self, h2: torch.Tensor, dlens: torch.Tensor, L: int, B: int):
        """h2' = h2 + W_o attention(W_qkv h2) of the states h2 [L * B, 2 HP] (dlens: device int32 [B] sentence
        lengths), and the three tensors the backward reads: qkv [n, 3 NH DP], ctx [n, NH DP], lse [n, NH]."""
        n, AD, HP, W, s = L * B, self.NH * self.DP, self.HP, self.w, _s()
        qkv = S.linear(h2, self.seg(W, 'attn_wqkv').view(3 * AD, 2 * HP), self.seg(W, 'attn_bqkv'))
        ctx = torch.empty((n, AD), device=self.device, dtype=torch.float32)
        lse = torch.empty((n, self.NH), device=self.device, dtype=torch.float32)
        _lib.call("rk_attn_fwd", _p(qkv), _p(dlens), L, B, self.NH, self.DP, self.dh ** -0.5, _p(ctx), _p(lse), s)
        h2a = S.linear(ctx, self.seg(W, 'attn_wo').view(2 * HP, AD), self.seg(W, 'attn_bo').view(-1))
        _lib.call("rk_tag_add", _p(h2), _p(h2a), _p(h2a), h2a.numel(), s)
        return h2a, qkv, ctx, lse

    def _recurrence_fwd(self, x: torch.Tensor, L: int, B: int, xc: Optional[torch.Tensor] = None):
        """Input projection and the recurrence of x [L * B, EP] (time-major rows; xc [L * B, FP]: the char features
        beside it): hout [L, B, 2, HP] and the two tensors the BPTT kernel reads back (LSTM: gates, cell states; GRU:
        gates, W_hn h + b_hn)."""
        HP, W, s = self.HP, self.w, _s()
        f = dict(device=self.device, dtype=torch.float32)
        GH = self.NG * HP
        w_ih = self.seg(W, 'w_ih').view(2 * GH, self.EP)
        hout = torch.empty((L, B, 2, HP), **f)
        gsave = torch.empty((L, B, 2, GH), **f)
        aux = torch.empty((L, B, 2, HP), **f)
        if self.gru:   # b_hh goes to the kernel: its candidate block sits inside the product with r
            gin = self._add_char(S.linear(x, w_ih, self.seg(W, 'b_ih').view(-1)), xc)
            _lib.call("rk_gru_fwd32", _p(gin), _p(self.seg(W, 'w_hh')), _p(self.seg(W, 'b_hh')), L, B, HP, _p(hout),
                      _p(gsave), _p(aux), s)
        else:
            _lib.call("rk_tag_add", _p(self.seg(W, 'b_ih')), _p(self.seg(W, 'b_hh')), _p(self.bsum), 8 * HP, s)
            gin = self._add_char(S.linear(x, w_ih, self.bsum), xc)
            _lib.call("rk_lstm_fwd32", _p(gin), _p(self.seg(W, 'w_hh')), L, B, HP, _p(hout), _p(gsave), _p(aux), s)
        return hout, (gsave, aux)

    def _add_char(self, gin: torch.Tensor, xc: Optional[torch.Tensor]) -> torch.Tensor:
        """gin += xc W_ihc^T (S.linear has no accumulate mode: a second GEMM and one elementwise pass)."""
        if xc is not None:
            ginc = S.linear(xc, self.seg(self.w, 'w_ihc').view(2 * self.NG * self.HP, self.FP))
            _lib.call("rk_tag_add", _p(gin), _p(ginc), _p(gin), gin.numel(), _s())
        return gin

    def _char_workspace(self, L: int, B: int) -> torch.Tensor:
        """rk_charcnn_bwd's workspace of a batch shape: allocated once per shape (step() asks before any capture)."""
        ws = self._char_ws.get((L, B))
        if ws is None:
            nbytes = int(_lib.lib().rk_charcnn_ws_bytes(L * B, self.EcP, self.FP, self.CV))
            ws = self._char_ws[(L, B)] = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=self.device)
        return ws

    def _need_chars(self, chars):
        if (chars is not None) != self.char:
            raise ValueError('chars ([B, L, 16] uint8) goes with a net that has char_emb / char_conv, and only with one')

    def _crf_workspace(self, L: int, B: int) -> torch.Tensor:
        """The CRF kernels' workspace of a batch shape: allocated once per shape (step() asks before any capture)."""
        ws = self._crf_ws.get((L, B))
        if ws is None:
            nbytes = int(_lib.lib().rk_crf_ws_bytes(L, B, self.NT))
            ws = self._crf_ws[(L, B)] = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=self.device)
        return ws

    def _upload(self, words: np.ndarray, key) -> torch.Tensor:
        """Async copy of a packed batch into the shape's device input buffer (pinned, double-buffered)."""
        k = self._flip
        self._flip ^= 1
        buf = self._pinned[k]
        if buf is None or buf.numel() < words.size:
            if self._events[k] is not None:
                self._events[k].synchronize()
            buf = self._pinned[k] = torch.empty(max(words.size, 1 << 16), dtype=torch.int32, pin_memory=True)
        elif self._events[k] is not None:
            self._events[k].synchronize()     # the copy that last read this buffer has run
        buf[:words.size].numpy()[:] = words
        dst = self._inbuf.get(key)
        if dst is None:
            dst = self._inbuf[key] = torch.empty(words.size, dtype=torch.int32, device=self.device)
        dst.copy_(buf[:words.size], non_blocking=True)
        ev = self._events[k] = torch.cuda.Event()
        ev.record()
        return dst

    def step(self, x_bl: np.ndarray, y_bl: np.ndarray, update: bool = True, graph: bool = True, chars=None):
        """One training step on a batch-first [B, L] batch (ids int, labels IGNORE-padded; chars [B, L, 16] uint8
        exactly when the net has the char layers)."""
        B, L = x_bl.shape
        key = (L, B)
        self._need_chars(chars)
        if self.char:
            self._char_workspace(L, B)
        # the CRF and the attention read sentence lengths: a sentence's labelled tokens are its first ones
        lens = (np.asarray(y_bl) != IGNORE).sum(1) if self.crf or self.attn else None
        ib = self._upload(pack_batch(x_bl, y_bl, self.padding_idx, self.V, lens, chars), key)
        g = self._graphs.get(key) if graph and update else None
        if g is not None:
            g.replay()
            return
        self._body(ib, L, B, update)
        if graph and update:
            # the eager run tuned this shape's GEMMs; capture for the next batches of this shape
            with graphs.LOCK:
                torch.cuda.current_stream().synchronize()
                if self._pool is None:
                    self._pool = torch.cuda.graph_pool_handle()
                cg = torch.cuda.CUDAGraph()
                with graphs.capture(cg, pool=self._pool):
                    self._body(ib, L, B, True)   # recorded, not run: the eager run above was this step
                self._graphs[key] = cg

    def take_loss(self) -> float:
        """Sum of the batch-mean losses since the last call (one host sync); also restarts the gradient-norm
        stats, so read grad_stats() first."""
        v = float(self.loss_sum[0].item())
        _lib.call("rk_zero32", _p(self.loss_sum), 4, _s())
        if self.clip is not None:
            self.clip.reset()
        return v

    def grad_stats(self) -> dict:
        """The gradient norms of the steps since the last take_loss() (one host sync): see GradClip.read."""
        if self.clip is None:
            raise RuntimeError('grad_stats needs clip_norm (float(\'inf\') measures without clipping)')
        return self.clip.read()

    # ------------------------------------------------------------------------ inference
    @torch.no_grad()
    def logits(self, x_bl: np.ndarray, chars=None, lens=None) -> torch.Tensor:
        """[B, L, tags] logits (eval: no dropout), eager on the same kernels.  lens ([B], read by the attention
        step): the sentence lengths, by default the count of non-padding ids."""
        B, L = x_bl.shape
        return self._logits_tm(x_bl, chars, lens).view(L, B, self.NTP)[:, :, :self.NT].transpose(0, 1)

    @torch.no_grad()
    def decode(self, x_bl: np.ndarray, lens, chars=None) -> np.ndarray:
        """[B, L] int32 tags of the CRF's best paths (-1 from lens[b] on): the eval forward, then Viterbi."""
        if not self.crf:
            raise RuntimeError('decode needs a net with a crf')
        B, L = x_bl.shape
        lg = self._logits_tm(x_bl, chars, lens)
        dlens = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).to(self.device)
        tags = torch.empty((B, L), device=self.device, dtype=torch.int32)
        _lib.call("rk_crf_viterbi", _p(lg), _p(self.seg(self.w, 'crf_trans')), _p(self.seg(self.w, 'crf_start')),
                  _p(self.seg(self.w, 'crf_end')), _p(dlens), L, B, self.NT, _p(tags), _p(self._crf_workspace(L, B)),
                  _s())
        return tags.cpu().numpy()

    def _logits_tm(self, x_bl: np.ndarray, chars=None, lens=None) -> torch.Tensor:
        """[L * B, NTP] logits, time-major rows t * B + b."""
        B, L = x_bl.shape
        self._need_chars(chars)
        n, HP, EP, dev, s = B * L, self.HP, self.EP, self.device, _s()
        ids = torch.from_numpy(np.ascontiguousarray(x_bl.T, dtype=np.int32).reshape(-1)).to(dev)
        x = torch.empty((n, EP), device=dev, dtype=torch.float32)
        _lib.call("rk_tag_embed_fwd", _p(ids), _p(self.seg(self.w, 'emb')), _p(x), None, n, EP, self.V, 0.0, 0, 0,
                  None, s)
        xc = None
        if self.char:
            xc, _ = self._char_fwd(torch.from_numpy(_chars_tm(chars, B, L)).to(dev), n, 0.0, 0, 0, None, None)
        hout, _ = self._recurrence_fwd(x, L, B, xc)
        h2 = hout.view(n, 2 * HP)
        if self.attn:
            if lens is None:
                lens = (np.asarray(x_bl) != self.padding_idx).sum(1)
            dlens = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).to(dev)
            h2 = self._attn_fwd(h2, dlens, L, B)[0]
        return S.linear(h2, self.seg(self.w, 'w_out'), self.seg(self.w, 'b_out'))

    def close(self):
        with graphs.quiesced():
            self._graphs.clear()
