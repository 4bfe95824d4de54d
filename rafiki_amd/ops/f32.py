"""fp32 tensor ops over the gfx950 kernels (``csrc/kernels/sgemm.hip`` + ``bnf.hip``) — the
reference-precision training path.  Every GEMM runs on v_mfma_f32_32x32x2_f32 (exact fp32 products,
fp32 accumulation); activations, gradients and BatchNorm are fp32.  The reference trains in fp32
everywhere (pg_gans.py:830,914; Keras defaults in TfFeedForward.py / TfVgg16.py).

Layouts (all device tensors contiguous):
  * activations  : NHWC fp32 ``[N, H, W, C]`` with C % 4 == 0 (the stem pads RGB to 4 channels)
  * conv weights : fp32 ``[Cout, kh, kw, Cin]`` (GEMM B operand ``[N][K]``, K = taps*Cin)
  * dense weights: fp32 ``[out, in]``

Every function launches on the current HIP stream and allocates only through the torch caching
allocator, so whole steps capture into one hipGraph.  Tile shape / LDS-ring depth / split-K are
picked per layer shape by the autotuner (``rafiki_amd.ops.autotune``) outside capture.
"""
from __future__ import annotations

import os
from functools import partial
from typing import NamedTuple, Optional

import torch

from . import _lib, autotune
from .functional import ACT_LRELU, ACT_NONE, ACT_RELU, _check_soft, bn_slots, cdiv, dropout_  # noqa: F401

KIND_CONV, KIND_WGRAD, KIND_DENSE, KIND_DENSE_DX, KIND_DENSE_DW = 0, 2, 3, 4, 5
F_RELU, F_BIAS, F_STATS, F_GATE, F_ACCUM, F_LRELU, F_BNB, F_BNP = 1, 2, 4, 8, 16, 32, 512, 1024
# block tiles (see rk_sgemm): 0-3 four-wave 2x2, 4 256x64 (4x1 waves), 5 256x128 / 6 128x256 (8 waves),
# 7 64x256 (1x4).  Tiles 4-7 exist for the conv kinds with C % 32 == 0 and the weight gradient.
TILES = [(128, 128), (128, 64), (64, 128), (64, 64), (256, 64), (256, 128), (128, 256), (64, 256),
         (64, 64), (128, 64), (64, 128)]   # 8-10: 1- / 2-wave tiles of 64x64 wave tiles (X6 candidates)
_NST3 = (0, 1, 2, 3, 4, 7)   # 3-stage rings: 4-wave tiles only (sgemm.hip s_launch)
_FEW_WAVE = (8, 9, 10)
NUM_CU = 256
# tile code + X6: the split-bf16 K loop of rk_sgemm (fp32-accurate products on the bf16 MFMA: every
# fp32 operand value = three bf16 pieces, six v_mfma_f32_32x32x16_bf16 per 16-deep chunk; see
# sgemm.hip).  RAFIKI_X6=0 keeps every GEMM on v_mfma_f32_32x32x2_f32.
X6 = 16
USE_X6 = os.environ.get('RAFIKI_X6', '1') != '0'


def tile_dims(t: int):
    """(BM, BN) of a tile code (X6 codes included)."""
    return TILES[t & 15]


def _p(t: Optional[torch.Tensor]):
    """Device pointer of a kernel operand; a host tensor here would be an illegal GPU access."""
    if t is None:
        return None
    if not t.is_cuda:
        raise ValueError('host tensor {} {} passed to a gfx950 kernel'.format(tuple(t.shape), t.dtype))
    return t.data_ptr()


def _nbytes(t):
    return t.untyped_storage().nbytes() - t.storage_offset() * t.element_size()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _check(t, name):
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError('{}: contiguous fp32 tensor required (got {} contiguous={})'.format(
            name, t.dtype, t.is_contiguous()))


def sgemm(kind, A, B, out, M, N, K, lda, ldb, ldc, *, tile=0, nst=2, splits=1, slab_stride=0, bias=None,
          stats=None, gate=None, H=1, W=1, C=4, taps=1, flags=0, alpha=1.0, slope=0.2):
    slot_mask = 0
    if stats is not None:
        assert stats.dtype == torch.float64 and stats.is_contiguous()
        slot_mask = stats.shape[0] - 1
    _lib.call("rk_sgemm", int(kind), int(tile), int(nst), _p(A), _p(B), _p(out), _p(bias), _p(stats), int(slot_mask),
              _p(gate), int(M), int(N), int(K), int(lda), int(ldb), int(ldc), int(H), int(W), int(C), int(taps),
              int(splits), int(slab_stride), int(flags), float(alpha), float(slope), _nbytes(A), _nbytes(B), _s())
    return out


# ------------------------------------------------------------------------------ config selection
def pick_tile(M: int, N: int) -> int:
    """Largest tile that still puts >= one block on every CU (else the tile with most blocks)."""
    best, best_blocks = 3, -1
    for t, (bm, bn) in enumerate(TILES[:4]):
        blocks = cdiv(M, bm) * cdiv(N, bn)
        waste = (cdiv(M, bm) * bm * cdiv(N, bn) * bn) / float(M * N)
        if waste > 1.3 and t != 3:
            continue
        if blocks >= NUM_CU:
            return t
        if blocks > best_blocks:
            best, best_blocks = t, blocks
    return best


def _cands(M, N, splittable=False, K=0, big=False):
    """(tile, nst, splits) configs: the heuristic first, then every tile x ring depth (``big``: also the
    256-wide tiles), plus split-K variants for grids that leave the chip idle."""
    t0 = pick_tile(M, N)
    out = [(t0, 2, 1)]
    tiles = range(8 if big else 4)
    for t in tiles:
        bm, bn = TILES[t]
        if t >= 4 and (cdiv(M, bm) * bm * cdiv(N, bn) * bn) / float(M * N) > 1.3:
            continue  # the big tiles only where they do not mostly compute padding
        for nst in ((2, 3) if t in _NST3 else (2,)):
            c = (t, nst, 1)
            if c not in out:
                out.append(c)
    if splittable:
        kt = cdiv(K, 32)
        for t in tiles:
            bm, bn = TILES[t]
            if t >= 4 and (cdiv(M, bm) * bm * cdiv(N, bn) * bn) / float(M * N) > 1.3:
                continue
            blocks = cdiv(M, bm) * cdiv(N, bn)
            for s in (2, 4, 8, 16, 32, 64, 128, 256):
                if s > kt // 2 or blocks * s > 8 * NUM_CU or s * M * N * 4 > (512 << 20):
                    continue
                if blocks * s < NUM_CU // 2:
                    continue
                s_eff = cdiv(kt, cdiv(kt, s))
                for nst in ((2, 3) if t in _NST3 else (2,)):
                    c = (t, nst, s_eff)
                    if c not in out:
                        out.append(c)
    if USE_X6:
        x6 = [(t + X6, nst, s) for (t, nst, s) in out]
        # the few-wave 64x64-wave-tile shapes, X6 only (their point is the split VALU per MFMA)
        for t in _FEW_WAVE:
            bm, bn = TILES[t]
            if (cdiv(M, bm) * bm * cdiv(N, bn) * bn) / float(M * N) > 1.3:
                continue
            x6.append((t + X6, 2, 1))
        out += x6
    return out


def _pick(key, cands, run, protect=()):
    """The tuned config for ``key``.  ``protect``: tensors the op accumulates into — a tuning sweep runs
    every candidate several times, so their contents are saved first and restored afterwards."""
    if not autotune.ENABLED:
        return cands[0]
    if protect and not autotune._valid(autotune.lookup(key), cands) and autotune.can_tune():
        saved = [t.clone() for t in protect]
        cfg = autotune.tune(key, cands, run)
        for t, v in zip(protect, saved):
            t.copy_(v)
        return cfg
    return autotune.tune(key, cands, run)


def _slots_flags(acc):
    return 0 if acc is None else acc.shape[0] - 1


def _act_flags(bias, act):
    return (F_BIAS if bias is not None else 0) | (F_RELU if act == ACT_RELU else F_LRELU if act == ACT_LRELU else 0)


def _sum_slabs(launch, out, splits, accumulate):
    """A weight gradient over ``splits`` K ranges: ``launch(dst, accumulate)`` computes out (+)= the product when
    splits == 1, else one raw slab of out's shape per split, which reduce_slabs sums into out."""
    if splits == 1:
        launch(out, bool(accumulate))
        return out
    slab = torch.empty((splits,) + tuple(out.shape), device=out.device, dtype=torch.float32)
    launch(slab, False)
    return reduce_slabs(slab, out, accumulate=accumulate)


def _gemm(cfg, launch, out, M, N, *, groups=1, ldc=None, accumulate=None, stats=None, bias=None, act=ACT_NONE,
          slope=0.2, alpha=1.0, gate=None, bias_rows=0):
    """One direct fp32 GEMM under cfg = (tile code, ring depth, K splits).  ``launch(dst, ldc, **kw)`` is the op's
    statement of it, an sgemm / sgemm_g / sgemm_grp call less where it writes and how: ``groups`` stacked [M][N]
    products into out, [groups * M][N] of row stride ``ldc`` (default N).  Its epilogue is ``accumulate`` (a weight
    gradient: out (+)= the product) or what sreduce_epi applies (bias, act, slope, alpha, gate, bias_rows), with
    ``stats`` (BN statistics, never split).  Unsplit, the epilogue rides in the kernel; split, the kernel writes raw
    slabs [splits][groups * M][N] and the combine (reduce_slabs / sreduce_epi) applies it."""
    tile, nst, s = cfg
    rows = groups * M
    split = dict(splits=s, slab_stride=rows * N) if s > 1 else {}
    if accumulate is not None:
        _sum_slabs(lambda dst, acc: launch(dst, N, tile=tile, nst=nst, flags=F_ACCUM if acc else 0, **split),
                   out, s, accumulate)
    elif s == 1:
        own = {k: v for k, v in (('gate', gate), ('stats', stats)) if v is not None}   # rk_sgemm's alone
        flags = _act_flags(bias, act) | (F_GATE if gate is not None else 0) | (F_STATS if stats is not None else 0)
        launch(out, ldc or N, tile=tile, nst=nst, bias=bias, flags=flags, slope=slope, alpha=alpha, **own)
    else:
        assert stats is None
        slab = torch.empty((s, rows, N), device=out.device, dtype=torch.float32)
        launch(slab, N, tile=tile, nst=nst, **split)
        sreduce_epi(slab, rows, N, out if out.dim() == 2 else out.view(rows, N), bias=bias, act=act, slope=slope,
                    alpha=alpha, gate=gate, bias_rows=bias_rows)


# ------------------------------------------------------------------------------------------ conv
# cfg[0] >= 0 is the direct implicit-GEMM kernel, cfg = (tile code, ring depth, K splits); cfg[0] < 0 names a
# route of CONV_ROUTES / WGRAD_ROUTES (the route table below), which also says what cfg[1:] hold.
# The Winograd weight sets those routes read are the rows of SET_KINDS, one per kind.
class SetKind(NamedTuple):
    """One kind of Winograd weight set of a 3x3 conv weight [Cout, 3, 3, Cin].  rows, cols = (Cout, Cin) for a
    forward kind and (Cin, Cout) for a data-gradient kind (the same conv on the flipped, transposed filters)."""
    name: str
    kwarg: str       # the keyword of conv_fwd / conv_dgrad it feeds
    dgrad: bool      # the data-gradient set of its family (else the forward set)
    family: int      # its kernel family: what rk_wino_weights_all reads in a block's fourth desc field
    entry: str       # the single-layer entry point: (w, forward set, data-gradient set, Cout, Cin, stream)
    size: object     # size(rows, cols): its floats of WinoWeights.buf
    view: object     # view(flat, rows, cols): the set as the conv takes it, of its flat fp32 slice
    unit: int        # the refresh table's offset unit per float (2: bf16 elements)
    offered: object  # offered(f4, hw, rows, cols): a layer with hw x hw maps (None: any) gets this kind
    padded: bool = False   # it has padding the transform never writes: its buffer starts zeroed


def _set_pair(fwd, dgrad, kwarg, *fields, **kw):
    """The forward and the data-gradient row of one family: they differ in name and ``dgrad`` only."""
    return SetKind(fwd, kwarg, False, *fields, **kw), SetKind(dgrad, kwarg, True, *fields, **kw)


def _f4_map(f4, hw):
    return bool(f4) and (hw is None or hw % 4 == 0)


SET_KINDS = (   # WinoWeights lays a layer's sets out in this order
    # F(2x2,3x3) fp32 sets [16][rows][cols]
    *_set_pair('u2', 'ut2', 'wino', 0, 'rk_wino_weights', lambda r, c: 16 * r * c,
               lambda flat, r, c: flat.view(16, r, c), 1, lambda f4, hw, r, c: True),
    # F(4x4,3x3) fp32 sets [36][rows][cols]: maps in multiples of 4
    *_set_pair('u4', 'ut4', 'wino4', 1, 'rk_wino4_weights', lambda r, c: 36 * r * c,
               lambda flat, r, c: flat.view(36, r, c), 1, lambda f4, hw, r, c: _f4_map(f4, hw)),
    # their X6 planes, bf16 [36][3][rows][cols] (54 floats per weight), where the pre-split PT path takes the shape
    *_set_pair('u4p', 'ut4p', 'wino4p', 2, 'rk_x6p_w4_weights', lambda r, c: 54 * r * c,
               lambda flat, r, c: flat.view(torch.bfloat16).view(36, 3, r, c), 2,
               lambda f4, hw, r, c: _f4_map(f4, hw) and (hw is None or wino4_ptx_ok(hw, hw, c, r))),
    # blocked sets of the UB fused kernels, flat (wino4b_numel): columns in multiples of 8, rows padded to 32
    *_set_pair('u4b', 'ut4b', 'wino4b', 3, 'rk_wino4b_weights', lambda r, c: wino4b_numel(r, c),
               lambda flat, r, c: flat, 1, lambda f4, hw, r, c: _f4_map(f4, hw) and c % 8 == 0, padded=True),
)
KIND = {k.name: k for k in SET_KINDS}
SET_KWARGS = tuple(k.kwarg for k in SET_KINDS if not k.dgrad)   # the weight-set kwargs of conv_fwd / conv_dgrad


def conv_sets(lazy, dgrad=False):
    """The weight-set kwargs of conv_fwd (``dgrad``: conv_dgrad) from ``lazy(kind)``: a callable producing
    the set of that kind, or None where the layer has none."""
    return {k.kwarg: lazy(k.name) for k in SET_KINDS if k.dgrad == bool(dgrad)}


def _set_dims(k, Cout, Cin):
    return (Cin, Cout) if k.dgrad else (Cout, Cin)


def wino_set(kind: str, w: torch.Tensor) -> torch.Tensor:
    """The ``kind`` set (a SET_KINDS name) of one conv weight [Cout, 3, 3, Cin], in a fresh buffer."""
    k = KIND[kind]
    Cout = w.shape[0]
    Cin = w.numel() // (9 * Cout)
    rows, cols = _set_dims(k, Cout, Cin)
    flat = (torch.zeros if k.padded else torch.empty)(k.size(rows, cols), device=w.device, dtype=torch.float32)
    out = k.view(flat, rows, cols)
    _lib.call(k.entry, _p(w), None if k.dgrad else _p(out), _p(out) if k.dgrad else None, Cout, Cin, _s())
    return out


def _offered(families, sets, taps, H, W, C, N, need):
    """(per route family: is it offered to this conv of C input / N output channels?, the candidates of those
    that are).  ``need``: the E_* options the call takes.  Computed once per call: the flags also go into its key."""
    on = [sets[f.weights] is not None and taps == 9 and not (need & ~f.also) and f.offer(H, W, C, N)
          for f in families]
    return on, [c for f, o in zip(families, on) if o for c in f.cfgs]


def _sets_key(sets, on):
    """The weight-set slots of a conv tune key: 'lazy' where the set is produced on demand (the candidate
    then times transform + conv), else whether its family is offered."""
    w2, w4, w4b, pt, ptx = on
    return (('lazy' if callable(sets[0]) else w2, 'lazy' if callable(sets[1]) else w4, pt,
             'lazy' if callable(sets[2]) else ptx) + (('b', 'lazy' if callable(sets[3]) else True),) * w4b)


def _run_route(r, x, sets, out, cfg, epi):
    u = sets[r.weights]
    r.kernel(x, u() if callable(u) else u, out=out, **SLOTS[r.slots](r, cfg), **epi)


def conv_fwd(x: torch.Tensor, w: torch.Tensor, *, taps: int = 9, stats_acc=None, bias=None, act=ACT_NONE,
             slope=0.2, out=None, wino=None, wino4=None, wino4p=None, wino4b=None, pro=None):
    """y = conv3x3(x, w) (stride 1, pad 1; taps=1: 1x1) [+bias][act]; with ``stats_acc`` (zeroed fp64
    [SL][2][Cout]) the per-channel (sum y, sum y^2) BatchNorm statistics ride in the epilogue.
    ``wino``: the layer's Winograd weights (WinoWeights.u), or a callable producing them (run only
    when a Winograd candidate runs, so the tuner times transform + conv) -> the fused F(2x2,3x3)
    kernels are more autotune candidates; ``wino4`` likewise for the F(4x4,3x3) kernels (WinoWeights.u4),
    ``wino4p`` the X6 weight planes (WinoWeights 'u4p') of the pre-split pre-transformed F(4x4) path,
    ``wino4b`` the blocked F(4x4) set ('u4b').
    ``pro``: normalise-on-load — x is the pre-BN output y of the previous conv, pro = its coeffs
    (bn_finalize): every candidate loads relu(y * scale + shift) (the F(4x4) kernels with blocked weights
    and the pre-transformed paths; see bn_on_load_ok)."""
    _check(x, 'conv_fwd x')
    Nb, H, W, Cin = x.shape
    Cout = w.shape[0]
    M, K = Nb * H * W, taps * Cin
    assert w.numel() == Cout * K, (w.shape, taps, Cin)
    if out is None:
        out = torch.empty((Nb, H, W, Cout), device=x.device, dtype=torch.float32)
    flags = _act_flags(bias, act) | (F_STATS if stats_acc is not None else 0)
    sets = (wino, wino4, wino4p, wino4b)
    epi = dict(bias=bias, stats=stats_acc, relu=act == ACT_RELU)
    need = 0
    if act == ACT_LRELU:   # rides (without statistics) only in the pre-transformed paths' epilogue: PG-GAN's D convs
        need, epi['lrelu'] = E_LRELU if stats_acc is None else E_DIRECT, slope
    if pro is not None:   # only the kernels that normalise on load are candidates
        assert bias is None and act == ACT_NONE and pro.shape == (4, Cin)
        need, epi['pro'], cands = E_PRO, pro, []
    else:
        cands = _cands(M, Cout, splittable=stats_acc is None and Cout % 4 == 0, K=K, big=Cin % 32 == 0)
    on, fused = _offered(CONV_FAMILIES, sets, taps, H, W, Cin, Cout, need)
    cands += fused
    if not cands:
        raise ValueError('conv_fwd(pro=...): no normalise-on-load kernel for this shape (see bn_on_load_ok)')

    def run(cfg):
        r = CONV_ROUTES.get(cfg[0])
        if r is not None:
            _run_route(r, x, sets, out, cfg, epi)
            return
        # split-K: small-M deep layers (inference at small batch: 4x4 maps, K = 9 x 512)
        _gemm(cfg, lambda dst, ldc, **kw: sgemm(KIND_CONV, x, w, dst, M, Cout, K, Cin, K, ldc, H=H, W=W, C=Cin,
                                                taps=taps, **kw),
              out, M, Cout, stats=stats_acc, bias=bias, act=act, slope=slope)
    cfg = _pick(('sf', M, Cout, K, H, W, Cin, taps, flags) + _sets_key(sets, on)
                + (('pro',) if pro is not None else ()), cands, run)
    if stats_acc is not None and autotune.can_tune():
        stats_acc.zero_()  # tuning runs accumulated into it
    run(cfg)
    return out


def conv_dgrad(dy: torch.Tensor, wt, *, taps: int = 9, out=None, gate=None, bnb=None, bnp=None,
               wino=None, wino4=None, cin=None, wino4p=None, wino4b=None):
    """dx = data gradient of a 3x3 conv as conv3x3(dy, wt) with wt = SConvWT.view() [Cin][taps*Cout]: the
    same routes as conv_fwd on the data-gradient sets (``wino``: WinoWeights.ut, ``wino4`` 'ut4', ``wino4p``
    'ut4p', ``wino4b`` 'ut4b').
    Epilogue options: ``gate`` (ReLU mask of the input activation), ``bnb = (y, coeffs, acc)`` (the input
    is BN+ReLU(y): mask + BN-backward sums into acc), ``bnp = (y, coeffs, acc)`` (the input is
    maxpool(BN+ReLU(y)), y at 2x resolution: routing + sums; dx stays the pooled gradient)."""
    _check(dy, 'conv_dgrad dy')
    Nb, H, W, Cout = dy.shape
    # wt / the sets may be callables (weights prepared per call, inside the timed candidate): then ``cin``
    Cin = cin if callable(wt) else wt.shape[0]
    M, K = Nb * H * W, taps * Cout
    assert callable(wt) or wt.numel() == Cin * K
    if out is None:
        out = torch.empty((Nb, H, W, Cin), device=dy.device, dtype=torch.float32)
    flags, bias, stats = F_GATE if gate is not None else 0, None, None
    if bnb is not None or bnp is not None:
        assert bnb is not None or (not (H & (H - 1)) and not (W & (W - 1))), 'pooled BN fusion needs power-of-two maps'
        flags, bias, stats, gate = _bn_bwd_epilogue(out, bnb, bnp)
    sets = (wino, wino4, wino4p, wino4b)
    epi = dict(bnb=bnb, bnp=bnp)
    on, fused = _offered(CONV_FAMILIES, sets, taps, H, W, Cout, Cin, E_DIRECT if flags & F_GATE else 0)
    cands = _cands(M, Cin, big=Cout % 32 == 0) + fused

    def run(cfg):
        r = CONV_ROUTES.get(cfg[0])
        if r is not None:
            _run_route(r, dy, sets, out, cfg, epi)
            return
        sgemm(KIND_CONV, dy, wt() if callable(wt) else wt, out, M, Cin, K, Cout, K, Cin, tile=cfg[0], nst=cfg[1],
              bias=bias, stats=stats, gate=gate, H=H, W=W, C=Cout, taps=taps, flags=flags)
    cfg = _pick(('sd', M, Cin, K, H, W, Cout, taps, flags) + _sets_key(sets, on), cands, run)
    if stats is not None and autotune.can_tune():
        stats.zero_()
    run(cfg)
    return out


def _lead_with_split(cands, M, N):
    """The split-K configs fill the chip: lead with the best-filling heuristic one."""
    split = [c for c in cands if c[2] > 1]
    if not split:
        return cands
    return [max(split, key=lambda c: min(cdiv(M, tile_dims(c[0])[0]) * cdiv(N, tile_dims(c[0])[1]) * c[2],
                                         2 * NUM_CU))] + cands


def conv_wgrad(dy: torch.Tensor, x: torch.Tensor, *, taps: int = 9, out=None, accumulate=False, xpro=None):
    """dW[co][tap][ci] (fp32 [Cout][taps*Cin]) = sum over pixels of dy[p][co] * x[shift_tap(p)][ci].
    ``xpro``: x is the pre-BN output of its producer and xpro that BN's coeffs (bn_finalize): the F(4x4)
    kernels normalise + ReLU it on load (the only candidates then; see bn_on_load_ok)."""
    _check(dy, 'conv_wgrad dy')
    _check(x, 'conv_wgrad x')
    Nb, H, W, Cout = dy.shape
    Cin = x.shape[-1]
    M, N, K = Cout, taps * Cin, Nb * H * W
    if out is None:
        out = torch.empty((Cout, N), device=dy.device, dtype=torch.float32)
    pro = {}
    if xpro is not None:
        assert taps == 9 and xpro.shape == (4, Cin)
        pro['xpro'] = xpro
    # per route its candidates for this problem ([]: not offered): they feed the candidate list and the key
    found = [r.offer(Nb, H, W, Cout, Cin) if taps == 9 and (xpro is None or r.also & E_PRO) else []
             for r in WGRAD_ROUTES.values()]
    cands = [] if pro else _lead_with_split(_cands(M, N, splittable=True, K=K, big=True), M, N)
    for f in found:
        cands = cands + f
    if not cands:
        raise ValueError('conv_wgrad(xpro=...): no normalise-on-load kernel for this shape (see bn_on_load_ok)')

    def run(cfg):
        r = WGRAD_ROUTES.get(cfg[0])
        if r is not None:
            r.kernel(dy, x, out, accumulate=accumulate, **SLOTS[r.slots](r, cfg), **pro)
            return
        _gemm(cfg, lambda dst, ldc, **kw: sgemm(KIND_WGRAD, dy, x, dst, M, N, K, Cout, Cin, ldc, H=H, W=W, C=Cin,
                                                taps=taps, **kw),
              out, M, N, accumulate=bool(accumulate))
    cfg = _pick(('sw', M, N, K, H, W, Cin, taps, bool(accumulate)) + tuple(bool(f) for f in found)
                + (('pro',) if pro else ()), cands, run, protect=(out,) if accumulate else ())
    run(cfg)
    return out


class SConvWT:
    """Flipped, transposed fp32 copies wt[ci][taps-1-t][co] = w[co][t][ci] of several conv weights living
    in one fp32 arena, refreshed by ONE rk_swt launch per step; with them the data gradient is a forward
    conv of dy on the forward kernels (``conv_dgrad``)."""

    def __init__(self, arena: torch.Tensor, weights, taps: int = 9):
        self.arena = arena
        meta, desc, self._views, off = [], [], [], 0
        for l, w in enumerate(weights):
            Cout = w.shape[0]
            Cin = w.numel() // (taps * Cout)
            so = (w.data_ptr() - arena.data_ptr()) // 4
            meta.append([so, off, Cout, Cin, taps])
            for t in range(taps):
                for co0 in range(0, Cout, 32):
                    for ci0 in range(0, Cin, 32):
                        desc.append([l, t, co0, ci0])
            self._views.append((off, Cin, Cout))
            off += (Cin * taps * Cout + 63) // 64 * 64
        dev = arena.device
        self.taps = taps
        self.buf = torch.zeros(max(off, 64), dtype=torch.float32, device=dev)
        self.meta = torch.tensor(meta, dtype=torch.int64, device=dev)
        self.desc = torch.tensor(desc, dtype=torch.int32, device=dev)

    _fresh = False

    def refresh(self):
        _lib.call("rk_swt", _p(self.arena), _p(self.buf), _p(self.desc), self.desc.shape[0], _p(self.meta), _s())
        self._fresh = True

    def begin_step(self):
        """The weights change every step: the next lazy() read refreshes (one launch) first."""
        self._fresh = False

    def lazy(self, l: int):
        """Callable view for conv_dgrad's direct candidates: the refresh launch runs only in steps whose
        tuned data gradients use the direct kernel (Winograd ones read WinoWeights instead)."""
        def get():
            if not self._fresh:
                self.refresh()
            return self.view(l)
        return get

    def view(self, l: int) -> torch.Tensor:
        off, Cin, Cout = self._views[l]
        return self.buf[off:off + Cin * self.taps * Cout].view(Cin, self.taps * Cout)


# -------------------------------------------------------------------- Winograd F(2x2, 3x3) convs
WF_RELU, WF_BIAS, WF_STATS, WF_LRELU, WF_BNB, WF_BNP, WF_POOL = 1, 2, 4, 8, 512, 1024, 2048
WINO = os.environ.get('RAFIKI_WINOGRAD', '1') != '0'


def wino_ok(H: int, W: int, C: int) -> bool:
    """Shapes the fused Winograd kernel takes: stride-1 3x3, even maps, C % 8 == 0."""
    return WINO and H % 2 == 0 and W % 2 == 0 and C % 8 == 0 and C > 0


def wino_weights(w: torch.Tensor, u: torch.Tensor, ut: Optional[torch.Tensor] = None):
    """u [16][Cout][Cin] = G g G^T of w [Cout][9*Cin]; ut [16][Cin][Cout]: the data-gradient set."""
    Cout = w.shape[0]
    Cin = w.numel() // (9 * Cout)
    assert u.numel() == 16 * Cout * Cin and (ut is None or ut.numel() == 16 * Cout * Cin)
    _lib.call("rk_wino_weights", _p(w), _p(u), _p(ut), Cout, Cin, _s())
    return u, ut


def wino_u(w: torch.Tensor) -> torch.Tensor:
    """Forward Winograd weights [16][Cout][Cin] of one conv weight [Cout, 3, 3, Cin] (fresh buffer)."""
    return wino_set('u2', w)


def wino_ut(w: torch.Tensor) -> torch.Tensor:
    """Data-gradient Winograd weights [16][Cin][Cout] of one conv weight [Cout, 3, 3, Cin]."""
    return wino_set('ut2', w)


def _bn_bwd_epilogue(out, bnb, bnp):
    """(flags, bias, stats, gate) of a data gradient into a BN+ReLU layer, ``bnb`` = (y, coeffs, acc), or into
    maxpool(BN+ReLU(y)) with y at 2x resolution, ``bnp``: gate = y, bias = BN scale | shift, the sums go to acc.
    The flag is F_BNB / F_BNP, the same bits as WF_BNB / WF_BNP."""
    y, coeffs, stats = bnb if bnb is not None else bnp
    Nb, H, W, N = out.shape
    assert y.shape == (out.shape if bnb is not None else (Nb, 2 * H, 2 * W, N))
    assert stats.dtype == torch.float64 and stats.shape[-1] == N
    return F_BNB if bnb is not None else F_BNP, coeffs[2:4].reshape(-1).contiguous(), stats, y


def _wino_epilogue(out, bias, stats, relu, bnb, bnp):
    """(flags, bias, stats, gate) of a Winograd conv's epilogue: bias / ReLU / BN statistics, or with ``bnb``
    / ``bnp`` = (y, coeffs, acc) the BN-backward forms of conv_dgrad (gate = y, bias = BN scale | shift)."""
    flags = (WF_BIAS if bias is not None else 0) | (WF_RELU if relu else 0) | (WF_STATS if stats is not None else 0)
    gate = None
    if bnb is not None or bnp is not None:
        flags, bias, stats, gate = _bn_bwd_epilogue(out, bnb, bnp)
    if stats is not None:
        assert stats.dtype == torch.float64 and stats.is_contiguous() and stats.shape[-1] == out.shape[-1]
    return flags, bias, stats, gate


def _pro(pro):
    """A kernel's nullable normalise-on-load argument: scale [C], shift [C] of the BN coeffs [4][C], or NULL."""
    return None if pro is None else _p(pro[2])


def _fused_conv(name, variant, x, u, out, oshape, *, bias=None, stats=None, relu=False, bnb=None, bnp=None,
                pool=False, grp=(1, 0, 0, 0, 0), tail=()):
    """What wino_conv, wino4_conv and their _grp forms share: ``out`` (allocated if None) of shape ``oshape``, the
    epilogue flags and the call of the fused entry point ``name``.  grp = (groups, gx, gu, gy, gbias); ``tail``:
    what the entry point takes between those and the stream (rk_wino4_conv_grp: pro)."""
    Nb, H, W, C = x.shape[-4:]
    if out is None:
        out = torch.empty(oshape, device=x.device, dtype=torch.float32)
    assert out.shape == oshape and out.is_contiguous()
    flags, bias, stats, gate = _wino_epilogue(out, bias, stats, relu, bnb, bnp)
    _lib.call(name, _p(x), _p(u), _p(out), _p(bias), _p(stats), _slots_flags(stats), _p(gate), Nb, H, W, C, oshape[-1],
              flags | (WF_POOL if pool else 0), int(variant), *grp, *tail, _s())
    return out


def _grp_conv(name, variant, P, x, u, out, bias, relu, pool, tail=()):
    """The _grp forms: G convs in one grid, x [G, Nb, H, W, C] (or shared [Nb, H, W, C]), u [G, P, N, C]."""
    G, _, N, C = u.shape
    shared = x.dim() == 4
    Nb, H, W, Cx = x.shape[-4:]
    assert Cx == C and (shared or x.shape[0] == G) and u.is_contiguous() and x.is_contiguous()
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    grp = (G, 0 if shared else Nb * H * W * C, P * N * C, Nb * Ho * Wo * N, N if bias is not None else 0)
    return _fused_conv(name, variant, x, u, out, (G, Nb, Ho, Wo, N), bias=bias, relu=relu, pool=pool, grp=grp,
                       tail=tail)


def _wino2_entry(variant):
    """(entry point, its variant) of F(2x2) variant 0-5: 2-5 are the small-wave-tile kernels of winograd4.hip
    (small grids)."""
    return ("rk_wino2s_conv_grp", variant - 2) if variant >= 2 else ("rk_wino_conv_grp", variant)


def wino_conv(x: torch.Tensor, u: torch.Tensor, *, out=None, bias=None, stats=None, relu=False, bnb=None, bnp=None,
              variant=0):
    """y = conv3x3(x, w) (stride 1, pad 1) from u = wino_weights(w): x [Nb, H, W, C] fp32 NHWC.
    ``stats``: fp64 BN slots (sum y, sum y^2); ``bnb`` / ``bnp`` = (y, coeffs, acc) as in conv_dgrad."""
    _check(x, 'wino_conv x')
    Nb, H, W, C = x.shape
    N = u.shape[1]
    assert u.shape == (16, N, C) and u.is_contiguous(), (u.shape, x.shape)
    return _fused_conv(*_wino2_entry(variant), x, u, out, (Nb, H, W, N), bias=bias, stats=stats, relu=relu, bnb=bnb,
                       bnp=bnp)


# ----------------------------------------------------------------- Winograd F(4x4, 3x3) forward
WINO4 =os.environ.get('RAFIKI_WINOGRAD4', '1') != '0'


def wino4_ok(H: int, W: int, C: int) -> bool:
    """Shapes the fused F(4x4,3x3) kernel takes: stride-1 3x3, maps in multiples of 4, C % 8 == 0."""
    return WINO and WINO4 and H % 4 == 0 and W % 4 == 0 and C % 8 == 0 and C > 0


# normalise-on-load (the non-pooled BN + ReLU blocks of the fp32 engine): RAFIKI_BN_ON_LOAD=0 materialises
# every BN output instead
BN_ON_LOAD = os.environ.get('RAFIKI_BN_ON_LOAD', '1') != '0'


def bn_on_load_ok(Nb: int, H: int, W: int, Cin: int, Cout: int) -> bool:
    """Whether a 3x3 conv of Cin -> Cout channels on [Nb, H, W] can take its input as the previous conv's
    pre-BN output (conv_fwd(pro=...) with blocked F(4x4) weights, conv_wgrad(xpro=...))."""
    # Cin <= 512: the fused forward stages the 2 x Cin coefficients in 4 KiB of LDS (W4_PRO_MAXC)
    return (BN_ON_LOAD and wino4_ok(H, W, Cin) and Cin % 4 == 0 and Cin <= 512
            and bool(_wino4_wgrad_cands(Nb, H, W, Cout, Cin) or _wino4_pt_cands(Nb, H, W, Cout, Cin)))


def wino4_u(w: torch.Tensor) -> torch.Tensor:
    """Forward F(4x4) weights [36][Cout][Cin] of one conv weight [Cout, 3, 3, Cin] (fresh buffer)."""
    return wino_set('u4', w)


def wino4_ut(w: torch.Tensor) -> torch.Tensor:
    """Data-gradient F(4x4) weights [36][Cin][Cout] (flipped, transposed filters) of w [Cout, 3, 3, Cin]."""
    return wino_set('ut4', w)


# blocked F(4x4) sets: the weights as the fused kernel's LDS stage image, one contiguous 36-KiB block per 32
# output channels x 8 input channels (rk_wino4b_weights / WinoWeights 'u4b' / 'ut4b'; variants 3-5 of wino4_conv)
def wino4b_numel(N: int, C: int) -> int:
    """Floats of a blocked F(4x4) set with N output rows (padded to 32) and C input columns."""
    return 36 * cdiv(N, 32) * 32 * C


def wino4b_u(w: torch.Tensor, dgrad: bool = False) -> torch.Tensor:
    """Blocked F(4x4) set (forward, or the data-gradient one) of one conv weight [Cout, 3, 3, Cin]."""
    return wino_set('ut4b' if dgrad else 'u4b', w)


def wino4_conv(x: torch.Tensor, u: torch.Tensor, *, out=None, bias=None, stats=None, relu=False, bnb=None, bnp=None,
               variant=0, n_out=None, pro=None):
    """y = conv3x3(x, w) (stride 1, pad 1) by F(4x4,3x3) from u = wino4_u(w); options as wino_conv.
    Variants 3-5 take the blocked set (wino4b_u / WinoWeights 'u4b'), flat, with ``n_out`` (default: out's) channels.
    ``pro``: normalise-on-load — x is the pre-BN output of the previous conv and pro its BN coeffs [4][C]
    (bn_finalize): the kernel loads relu(x * scale + shift) (blocked variants 3-5, no bias / activation)."""
    _check(x, 'wino4_conv x')
    Nb, H, W, C = x.shape
    if variant >= 3:
        N = int(out.shape[-1] if n_out is None else n_out)
        assert u.dim() == 1 and u.numel() == wino4b_numel(N, C) and u.is_contiguous(), (u.shape, N, C)
    else:
        N = u.shape[1]
        assert u.shape == (36, N, C) and u.is_contiguous(), (u.shape, x.shape)
    if pro is not None:
        assert variant >= 3 and bias is None and not relu and bnb is None and bnp is None
        assert pro.shape == (4, C) and pro.is_contiguous()
    return _fused_conv("rk_wino4_conv_grp", variant, x, u, out, (Nb, H, W, N), bias=bias, stats=stats, relu=relu,
                       bnb=bnb, bnp=bnp, tail=(_pro(pro),))


# largest map the pre-transformed paths are offered on: 8 with the f32 GEMM (they lost on 16x16 maps,
# profiles/wgrad4_variants_r3.jsonl); with the X6 GEMM loop their batched GEMM is 1.1-1.3x faster, so the
# tuner also weighs them on 16x16 and 32x32 maps
PT_MAX_HW = int(os.environ.get('RAFIKI_PT_MAX_HW', '32' if USE_X6 else '8'))


def wino4_pt_ok(H, W, C, N):
    """Deep maps (<= 8x8), where the fused kernels re-transform each input window once per output-channel
    block: there the transform-once + grouped-GEMM path is a tuner candidate."""
    return (WINO and WINO4 and H % 4 == 0 and W % 4 == 0 and H <= PT_MAX_HW and W <= PT_MAX_HW and C % 4 == 0
            and C >= 32
            and N >= 32)


def _pt_cfgs(route_id):
    """(id, sgemm tile, nst) of a pre-transformed path: the four-wave tiles x ring depths on the f32 and the X6
    K loop, and the few-wave X6 tiles."""
    return tuple((route_id, t + x, n) for x in ((0, X6) if USE_X6 else (0,)) for t in (0, 1, 2, 3)
                 for n in ((2, 3) if t in _NST3 else (2,))) + \
        (tuple((route_id, t + X6, 2) for t in _FEW_WAVE) if USE_X6 else ())


def wino4_conv_pt(x: torch.Tensor, u: torch.Tensor, *, out=None, bias=None, stats=None, relu=False, bnb=None,
                  bnp=None, tile=0, nst=2, splits=1, lrelu=None, pro=None):
    """wino4_conv through position-major buffers: V = B^T x B [36][T][C] (one launch), Y'[q] = V[q] u[q]^T
    as one 36-group sgemm, then A^T Y' A with the same epilogues (bias / ReLU / BN statistics / BNB / BNP;
    ``lrelu`` = slope: bias + leaky ReLU, the PG-GAN discriminator's conv epilogue).
    With bf16 X6 planes u [36][3][N][C] (WinoWeights 'u4p' / 'ut4p') the input transform writes V as planes
    too and the GEMM is the pre-split X6 one (x6p_gemm; ``tile`` / ``nst`` are its configs)."""
    _check(x, 'wino4_conv_pt x')
    Nb, H, W, C = x.shape
    planes = u.dtype == torch.bfloat16   # u4p / ut4p X6 planes [36][3][N][C]
    N = u.shape[-2]
    assert u.shape == ((36, 3, N, C) if planes else (36, N, C)) and u.is_contiguous() and H % 4 == 0 and W % 4 == 0, \
        (u.shape, x.shape)
    if out is None:
        out = torch.empty((Nb, H, W, N), device=x.device, dtype=torch.float32)
    assert out.shape == (Nb, H, W, N) and out.is_contiguous()
    flags, bias, stats, gate = _wino_epilogue(out, bias, stats, relu, bnb, bnp)
    if lrelu is not None:
        assert flags in (0, WF_BIAS)
        flags |= WF_LRELU
    T = Nb * (H // 4) * (W // 4)
    if pro is not None:   # normalise-on-load in the input transform (pro = the producer's BN coeffs [4][C])
        assert pro.shape == (4, C) and pro.is_contiguous()
    if planes:   # pre-split X6: V planes [36][3][T][C] once, then the plane GEMM (no split in the K loop)
        splits = x6p_splits(C, splits)
        # Y' tile-major [T][36][N]: the output transform reads each tile's 36 positions as one run
        yt = torch.empty((splits, T, 36, N), device=x.device, dtype=torch.float32)
        v = torch.empty((36, 3, T, C), device=x.device, dtype=torch.bfloat16)
        _lib.call("rk_x6p_w4_input", _p(x), _p(v), Nb, H, W, C, _pro(pro), _s())
        x6p_gemm(v, u, yt, T, N, C, groups=36, tile=tile, nst=nst, splits=splits, row_major_groups=True)
    else:
        splits = 1
        yt = torch.empty((36, T, N), device=x.device, dtype=torch.float32)
        v = torch.empty((36, T, C), device=x.device, dtype=torch.float32)
        _lib.call("rk_wino4_pt_input", _p(x), _p(v), Nb, H, W, C, _pro(pro), _s())
        sgemm_grp(KIND_DENSE, v, u, yt, T, N, C, C, C, N, 36, T * C, N * C, T * N, tile=tile, nst=nst)
    _lib.call("rk_wino4_pt_conv_out", _p(yt), _p(out), _p(bias), _p(stats), _slots_flags(stats), _p(gate),
              Nb, H, W, N, flags, splits, 36 * T * N, int(planes), float(0.0 if lrelu is None else lrelu), _s())
    return out


def wino4_conv_grp(x, u, *, out=None, bias=None, relu=False, variant=0, pool=False):
    """k F(4x4) convs in one grid: x [G, Nb, H, W, C] (or shared [Nb, H, W, C]), u [G, 36, N, C].
    ``pool`` (with bias + relu): the 2x2 max-pool from the epilogue, out [G, Nb, H/2, W/2, N]."""
    assert not pool or (bias is not None and relu)
    return _grp_conv("rk_wino4_conv_grp", variant, 36, x, u, out, bias, relu, pool, tail=(None,))


def _wino4_wgrad_cands(Nb, H, W, Cout, Cin):
    """Split-K choices of rk_wino4_wgrad (variant 0: 32 co x 32 ci blocks, 1: 64 co x 32 ci, 2: 32 x 32
    software-pipelined over two LDS stages): 128..4096
    blocks, >= 4 chunks of 8 tiles per block, slabs <= 256 MiB.  cfg = (WINO4_WGRAD, variant, splits)."""
    if not (WINO and WINO4 and H % 4 == 0 and W % 4 == 0 and Cin >= 8 and Cout >= 16):
        return []
    nt = Nb * (H // 4) * (W // 4)
    if nt >= (1 << 22) or 4 * Nb * H * W * max(Cin, Cout) >= 0x7fffffff:
        return []
    out = []
    for v, bco in ((0, 32), (1, 64)):   # 2 (software-pipelined) measured 1.2-1.3x slower, wino4_variants_r5
        if v == 1 and Cout < 64:
            continue
        base = cdiv(Cout, bco) * cdiv(Cin, 32)
        for s in (1, 2, 4, 8, 16, 32, 64, 128, 256):
            tps = cdiv(cdiv(nt, s), 8) * 8
            s_eff = cdiv(nt, tps)
            if tps < 32 or base * s_eff > 4096 or (s_eff > 1 and s_eff * 9 * Cout * Cin * 4 > (256 << 20)):
                continue
            if base * s_eff < 128 and s != 1:
                continue
            c = (WINO4_WGRAD, v, s_eff)
            if c not in out:
                out.append(c)
    return out


def wino4_wgrad(dy: torch.Tensor, x: torch.Tensor, out: torch.Tensor, *, splits=1, accumulate=False, variant=0,
                xpro=None):
    """out [Cout][9*Cin] (+)= weight gradient of a 3x3 stride-1 conv by F(4x4,3x3); splits > 1: per-split
    slabs summed by reduce_slabs.  ``xpro``: x is pre-BN, normalised + ReLU'd on load (variants 0 / 1)."""
    _check(dy, 'wino4_wgrad dy')
    _check(x, 'wino4_wgrad x')
    Nb, H, W, Cout = dy.shape
    Cin = x.shape[-1]
    assert x.shape[:3] == dy.shape[:3] and out.numel() == Cout * 9 * Cin and out.is_contiguous()
    assert xpro is None or (xpro.shape == (4, Cin) and xpro.is_contiguous() and variant in (0, 1))
    return _sum_slabs(lambda dst, acc: _lib.call("rk_wino4_wgrad", _p(dy), _p(x), _p(dst), Nb, H, W, Cout, Cin,
                                                 int(splits), int(acc), int(variant), _pro(xpro), _s()),
                      out, splits, accumulate)


def _wino4_pt_cands(Nb, H, W, Cout, Cin):
    """The pre-transformed F(4x4) weight gradient (transform once, 36 GEMMs as one split-K sgemm) on
    maps of <= 8x8, where the fused kernels' redundant per-block transforms dominate (VGG-small batch
    256: 8x8x256x256 84.8 vs 101.7 us, 4x4x512x512 76.4 vs 96.3; it loses on 16x16 maps,
    profiles/wgrad4_variants_r3.jsonl)."""
    if not (WINO and WINO4 and H % 4 == 0 and W % 4 == 0 and H <= PT_MAX_HW and W <= PT_MAX_HW and Cin % 4 == 0
            and Cout % 4 == 0 and Cin >= 32 and Cout >= 32):
        return []
    T = Nb * (H // 4) * (W // 4)
    if T % 32 or 36 * T * max(Cin, Cout) * 4 >= (1 << 31) or 36 * Cout * Cin * 4 > (512 << 20):
        return []
    return list(_pt_cfgs(WINO4_WGRAD_PT))


def wino4_wgrad_pt(dy: torch.Tensor, x: torch.Tensor, out: torch.Tensor, *, accumulate=False, tile=0, nst=2,
                   planes=False, splits=1, xpro=None):
    """out [Cout][9*Cin] (+)= the F(4x4,3x3) weight gradient through position-major transformed buffers:
    M [36][T][Cout], V [36][T][Cin] (one transform launch each), dU[q] = M[q]^T V[q] as ONE sgemm with
    36 K-splits (slab q = dU[q]), then dW = G^T dU G.  ``planes``: the operands as X6 planes transposed to
    K-inner ([36][3][C][T]) and the 36 GEMMs as one grouped pre-split X6 launch (x6p_gemm configs)."""
    _check(dy, 'wino4_wgrad_pt dy')
    _check(x, 'wino4_wgrad_pt x')
    Nb, H, W, Cout = dy.shape
    Cin = x.shape[-1]
    T = Nb * (H // 4) * (W // 4)
    assert H % 4 == 0 and W % 4 == 0 and T % 32 == 0 and x.shape[:3] == dy.shape[:3], (dy.shape, x.shape)
    assert out.numel() == Cout * 9 * Cin and out.is_contiguous()
    assert xpro is None or (not planes and xpro.shape == (4, Cin) and xpro.is_contiguous())
    if planes:   # pre-split X6: M^T / V^T planes [36][3][C][T] (K = tiles inner), 36-group plane GEMM
        splits = x6p_splits(T, splits)
        du = torch.empty((splits, 36, Cout, Cin), device=dy.device, dtype=torch.float32)
        m = torch.empty((36, 3, Cout, T), device=dy.device, dtype=torch.bfloat16)
        v = torch.empty((36, 3, Cin, T), device=dy.device, dtype=torch.bfloat16)
        _lib.call("rk_x6p_w4_wgrad_transform", _p(dy), _p(x), _p(m), _p(v), Nb, H, W, Cout, Cin, _s())
        x6p_gemm(m, v, du, Cout, Cin, T, groups=36, tile=tile, nst=nst, splits=splits)
    else:
        splits = 1
        du = torch.empty((36, Cout, Cin), device=dy.device, dtype=torch.float32)
        m = torch.empty((36 * T, Cout), device=dy.device, dtype=torch.float32)
        v = torch.empty((36 * T, Cin), device=dy.device, dtype=torch.float32)
        _lib.call("rk_wino4_pt_transform", _p(dy), _p(x), _p(m), _p(v), Nb, H, W, Cout, Cin, _pro(xpro), _s())
        sgemm(KIND_DENSE_DW, m, v, du, Cout, Cin, 36 * T, Cout, Cin, Cin, tile=tile, nst=nst, splits=36,
              slab_stride=Cout * Cin)
    _lib.call("rk_wino4_pt_output", _p(du), _p(out), Cout, Cin, int(bool(accumulate)), splits, 36 * Cout * Cin, _s())
    return out


# ---------------------------------------------------------------- pre-split X6 GEMMs (x6p.hip)
# The X6 products with the operands split into bf16 planes ONCE by their producers (the Winograd
# transforms) instead of after every LDS read inside the K loop: the pre-transformed F(4x4) paths on
# planes are autotune candidates next to their fp32-operand sgemm forms.  RAFIKI_X6P=0 turns them off.
USE_X6P = USE_X6 and os.environ.get('RAFIKI_X6P', '1') != '0'
# tiles 9-12: warp-specialised (2x2 compute waves + 4 loader waves that alone issue the LDS-DMA pieces)
XP_TILES = ((128, 128), (128, 64), (64, 128), (64, 64), (64, 64), (128, 64), (64, 128), (256, 128), (128, 256),
            (128, 128), (128, 64), (64, 128), (64, 64))
XP_NST3 = (0, 1, 2, 3, 4, 5, 6, 9, 10, 11, 12)   # tiles 7-8 (8 waves, 72 KiB per stage) ring 2 stages only
# (tile, nst, splits) of the x6p GEMM: every tile x ring depth unsplit; the big tiles also with 2 / 4 K-splits
# (the 4x4-map GEMMs have T = 256 rows: 288 blocks of 128x128 for 256 CUs; the slabs are summed by the
# output transforms that read Y' / dU anyway)
_XP_CFGS = tuple((t, n, 1) for t in range(len(XP_TILES)) for n in ((2, 3) if t in XP_NST3 else (2,))) + \
    tuple((t, 2, s) for t in (0, 1, 2, 7, 8) for s in (2, 4)) + tuple((t, 3, s) for t in (9, 10, 11) for s in (2, 4))


def x6p_pack(tile: int, nst: int) -> int:
    """One config slot for an x6p GEMM's (tile, ring depth): the 'x6p code' of the PTX and dense routes."""
    return 4 * tile + nst


def x6p_unpack(code: int):
    return code // 4, code % 4


def x6p_split(src: torch.Tensor, out=None) -> torch.Tensor:
    """bf16 X6 planes [3][rows][cols] (hi, mid, lo; x = hi + mid + lo) of an fp32 [rows][cols] matrix."""
    _check(src, 'x6p_split src')
    rows, cols = src.shape
    if out is None:
        out = torch.empty((3, rows, cols), dtype=torch.bfloat16, device=src.device)
    _lib.call("rk_x6p_split", _p(src), _p(out), rows, cols, cols, cols, rows * cols, _s())
    return out


def x6p_split_t(src: torch.Tensor, ldd: Optional[int] = None, out=None) -> torch.Tensor:
    """bf16 X6 planes [3][cols][ldd] of the TRANSPOSE of an fp32 [rows][cols] matrix (row stride any), the
    plane columns rows .. ldd-1 zero (ldd: rows rounded up to 32, the x6p GEMM's K granularity)."""
    rows, cols = src.shape
    assert src.dtype == torch.float32 and src.stride(1) == 1, (src.dtype, src.stride())
    ldd = ldd or cdiv(rows, 32) * 32
    if out is None:
        out = torch.empty((3, cols, ldd), dtype=torch.bfloat16, device=src.device)
    _lib.call("rk_x6p_split_t", _p(src), _p(out), rows, cols, src.stride(0), ldd, cols * ldd, _s())
    return out


def x6p_gemm(A: torch.Tensor, B: torch.Tensor, out: torch.Tensor, M: int, N: int, K: int, *, groups: int = 1,
             tile: int = 0, nst: int = 2, accumulate: bool = False, splits: int = 1,
             row_major_groups: bool = False) -> torch.Tensor:
    """out[g] (+)= A[g] . B[g]^T for g < groups: A bf16 planes [G][3][M][K], B [G][3][N][K] (contiguous),
    out fp32 [G][M][N] (``row_major_groups``: [M][G][N]); K % 32 == 0.  splits > 1: out is [splits][...] raw
    split-K partial sums."""
    assert A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16 and A.is_contiguous() and B.is_contiguous()
    assert A.numel() == groups * 3 * M * K and B.numel() == groups * 3 * N * K
    assert out.numel() == splits * groups * M * N and not (accumulate and splits > 1)
    ldc, gsc = (groups * N, N) if row_major_groups else (N, M * N)
    _lib.call("rk_x6p_gemm", int(tile), int(nst), _p(A), _p(B), _p(out), M, N, K, K, K, ldc, M * K, N * K, 3 * M * K,
              3 * N * K, gsc, int(groups), int(bool(accumulate)), int(splits), groups * M * N, _nbytes(A),
              _nbytes(B), _s())
    return out


def x6p_splits(K: int, s: int) -> int:
    """The effective split count of ``s`` requested splits over K (every split gets >= one 32-deep K-tile)."""
    nk = K // 32
    per = cdiv(nk, max(1, s))
    return cdiv(nk, per)


def wino4_u4p(w: torch.Tensor, dgrad: bool = False) -> torch.Tensor:
    """X6 planes of the F(4x4) weights of one conv weight [Cout, 3, 3, Cin] (fresh buffer): forward set
    [36][3][Cout][Cin] (WinoWeights 'u4p'), ``dgrad``: the data-gradient set [36][3][Cin][Cout] ('ut4p')."""
    return wino_set('ut4p' if dgrad else 'u4p', w)


def wino4_ptx_ok(H, W, C, N):
    """Shapes the plane path of the pre-transformed F(4x4) conv takes (K = C channels, % 32)."""
    return USE_X6P and wino4_pt_ok(H, W, C, N) and C % 32 == 0


def _wino4_ptx_wgrad_cands(Nb, H, W, Cout, Cin):
    """The plane path of the pre-transformed F(4x4) weight gradient: K = T tiles (% 32)."""
    if not (USE_X6P and _wino4_pt_cands(Nb, H, W, Cout, Cin)):
        return []
    T = Nb * (H // 4) * (W // 4)
    if T % 32 or 108 * T * max(Cin, Cout) >= (1 << 31):
        return []
    return [(WINO4_WGRAD_PTX, x6p_pack(t, n), x6p_splits(T, s)) for t, n, s in _XP_CFGS]


def _wino_wgrad_cands(Nb, H, W, Cout, Cin):
    """Split-K choices of rk_wino_wgrad that fill the chip: 128..4096 blocks, >= 8 chunks of 8 tiles per
    block, slabs <= 256 MiB."""
    if not (WINO and H % 2 == 0 and W % 2 == 0 and Cin >= 8 and Cout >= 16):
        return []
    nt = Nb * (H // 2) * (W // 2)
    if nt >= (1 << 22) or 4 * Nb * H * W * max(Cin, Cout) >= 0x7fffffff:
        return []
    base = cdiv(Cout, 64) * cdiv(Cin, 64)
    out = []
    for s in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512):
        tps = cdiv(cdiv(nt, s), 8) * 8
        s_eff = cdiv(nt, tps)
        if tps < 64 or base * s_eff > 4096 or (s_eff > 1 and s_eff * 9 * Cout * Cin * 4 > (256 << 20)):
            continue
        if base * s_eff < 128 and s != 1:
            continue
        c = (WINO_WGRAD, 0, s_eff)
        if c not in out:
            out.append(c)
    return out


def wino_wgrad(dy: torch.Tensor, x: torch.Tensor, out: torch.Tensor, *, splits=1, accumulate=False):
    """out [Cout][9*Cin] (+)= weight gradient of a 3x3 stride-1 conv by F(2x2,3x3); splits > 1: per-split
    slabs summed by reduce_slabs."""
    _check(dy, 'wino_wgrad dy')
    _check(x, 'wino_wgrad x')
    Nb, H, W, Cout = dy.shape
    Cin = x.shape[-1]
    assert x.shape[:3] == dy.shape[:3] and out.numel() == Cout * 9 * Cin and out.is_contiguous()
    return _sum_slabs(lambda dst, acc: _lib.call("rk_wino_wgrad", _p(dy), _p(x), _p(dst), Nb, H, W, Cout, Cin,
                                                 int(splits), int(acc), _s()),
                      out, splits, accumulate)


def wino_conv_grp(x, u, *, out=None, bias=None, relu=False, variant=0, pool=False):
    """k Winograd convs in one grid: x [G, Nb, H, W, C] (or [Nb, H, W, C] shared), u [G, 16, N, C],
    bias [G, N] -> out [G, Nb, H, W, N].  ``pool`` (with bias + relu, variants >= 2): the 2x2 max-pool of
    the output from the epilogue, out [G, Nb, H/2, W/2, N]."""
    H, W = x.shape[-3:-1]
    assert not pool or (bias is not None and relu and variant >= 2 and H % 2 == 0 and W % 2 == 0)
    return _grp_conv(*_wino2_entry(variant), 16, x, u, out, bias, relu, pool)


# ------------------------------------------------------------------------------- the route table
# Every autotune candidate with cfg[0] < 0 is one row below; the dispatchers (conv_fwd, conv_dgrad, conv_wgrad,
# conv_fwd_grp) look the row up by cfg[0] and call its kernel wrapper.  A data gradient is the same conv on the
# transposed weight set with another epilogue, so forward and data gradient share the conv rows.
class Route(NamedTuple):
    id: int            # cfg[0]
    name: str
    slots: str         # what cfg[1], cfg[2] hold: a key of SLOTS, the decoder into the wrapper's kwargs
    kernel: object     # the wrapper: conv kernel(x, u, out=, **slots, **epilogue); wgrad kernel(dy, x, out, ...)
    offer: object      # conv: offer(H, W, C, N) -> the shape fits (C input, N output channels);
    #                    weight gradient: offer(Nb, H, W, Cout, Cin) -> its candidates ([]: not offered)
    cfgs: tuple = ()   # conv: its candidates, in the order the tuner sees them
    family: str = ''   # conv rows of one family share weight set, predicate and options: offered together
    weights: int = 0   # conv: the weight set it reads, an index into SET_KWARGS
    variant: int = 0   # 'fixed' rows: the kernel's variant argument
    also: int = 0      # E_* options it carries beyond bias / ReLU / BN statistics / BNB / BNP
    grp: object = None   # its grouped launcher (conv_fwd_grp), if it has one
    pool: bool = False   # ... whose epilogue can write the 2x2 max-pool


E_LRELU, E_PRO, E_DIRECT = 1, 2, 4   # leaky-ReLU epilogue, normalise-on-load; E_DIRECT: no row carries it
SLOTS = {   # what cfg[1], cfg[2] of a row's candidates hold -> the keyword arguments of its wrapper they become
    'fixed: 0, 1': lambda r, cfg: {'variant': r.variant},
    '0, K splits': lambda r, cfg: {'splits': cfg[2]},
    'kernel variant, K splits': lambda r, cfg: {'variant': cfg[1], 'splits': cfg[2]},
    'sgemm tile code, ring depth': lambda r, cfg: {'tile': cfg[1], 'nst': cfg[2]},
    'x6p code, K splits': lambda r, cfg: dict(zip(('tile', 'nst'), x6p_unpack(cfg[1])), splits=cfg[2]),
}
_SGEMM, _X6P = 'sgemm tile code, ring depth', 'x6p code, K splits'


def _fused(id, name, variant, kernel, **kw):
    return Route(id, name, 'fixed: 0, 1', kernel, cfgs=((id, 0, 1),), variant=variant, **kw)


_F2 = dict(family='f2', weights=0, offer=lambda H, W, C, N: wino_ok(H, W, C), grp=wino_conv_grp)
_F4 = dict(family='f4', weights=1, offer=lambda H, W, C, N: wino4_ok(H, W, C), grp=wino4_conv_grp, pool=True)
_F4B = dict(family='f4b', weights=3, offer=_F4['offer'], also=E_PRO)
WINO4_PT, WINO4_PTX = -14, -15
WINO_WGRAD, WINO4_WGRAD, WINO4_WGRAD_PT, WINO4_WGRAD_PTX = -3, -7, -13, -16
WINO4_PTX_CFGS = tuple((WINO4_PTX, x6p_pack(t, n), s) for t, n, s in _XP_CFGS) if USE_X6P else ()
CONV_ROUTES = {r.id: r for r in (
    # fused F(2x2,3x3): rk_wino_conv_grp (variants 0 / 1) and the 16x16-wave-tile kernels of winograd4.hip (2-5)
    _fused(-1, 'F(2x2) 4-wave 64x32', 0, wino_conv, **_F2),
    _fused(-2, 'F(2x2) 8-wave 64x64', 1, wino_conv, **_F2),
    _fused(-8, 'F(2x2) 4-wave 32x32', 2, wino_conv, pool=True, **_F2),
    _fused(-9, 'F(2x2) 2-wave 16x32', 3, wino_conv, pool=True, **_F2),
    _fused(-10, 'F(2x2) 8-wave 64x32', 4, wino_conv, pool=True, **_F2),
    # software-pipelined over two LDS stages: wins the 4x4-map layers
    _fused(-12, 'F(2x2) 8-wave 64x32 two-stage', 5, wino_conv, pool=True, **_F2),
    # fused F(4x4,3x3), rk_wino4_conv_grp.  Its software-pipelined variant 2 (4-wave 32x32 over two LDS stages, one
    # wave per SIMD) measured 1.3-1.5x slower than these on every VGG-small layer
    # (profiles/winograd_variants_r2e.jsonl) and has no row: it stays callable as wino4_conv(variant=2) /
    # wino4_wgrad(variant=2) for tests/test_winograd4_gpu.py
    _fused(-5, 'F(4x4) 8-wave 64 tiles x 32 channels', 0, wino4_conv, **_F4),
    _fused(-6, 'F(4x4) 4-wave 32 x 32', 1, wino4_conv, **_F4),
    # the same kernel on the blocked sets (wino4b_numel); the only fused rows that normalise on load
    _fused(-17, 'F(4x4) blocked, 8-wave tile of -5', 3, wino4_conv, **_F4B),
    _fused(-18, 'F(4x4) blocked, 4-wave tile of -6', 4, wino4_conv, **_F4B),
    _fused(-19, 'F(4x4) blocked, warp-specialised (4 compute + 4 loader waves, two LDS stages)', 5, wino4_conv, **_F4B),
    # pre-transformed F(4x4) (wino4_conv_pt): on the fp32 set through sgemm_grp, on the X6 planes through x6p_gemm
    Route(WINO4_PT, 'F(4x4) pre-transformed', _SGEMM, wino4_conv_pt, cfgs=_pt_cfgs(WINO4_PT), family='pt',
          weights=1, offer=lambda H, W, C, N: wino4_ok(H, W, C) and wino4_pt_ok(H, W, C, N), also=E_LRELU | E_PRO),
    Route(WINO4_PTX, 'F(4x4) pre-transformed, X6 planes', _X6P, wino4_conv_pt, cfgs=WINO4_PTX_CFGS,
          family='ptx', weights=2, offer=lambda H, W, C, N: wino4_ptx_ok(H, W, C, N), also=E_LRELU | E_PRO),
)}
# weight gradients: every row's candidates depend on the problem, so ``offer`` returns them
WGRAD_ROUTES = {r.id: r for r in (
    Route(WINO_WGRAD, 'F(2x2) weight gradient', '0, K splits', wino_wgrad, _wino_wgrad_cands),
    Route(WINO4_WGRAD, 'F(4x4) weight gradient', 'kernel variant, K splits', wino4_wgrad, _wino4_wgrad_cands,
          also=E_PRO),
    Route(WINO4_WGRAD_PT, 'F(4x4) pre-transformed weight gradient', _SGEMM, wino4_wgrad_pt, _wino4_pt_cands,
          also=E_PRO),
    Route(WINO4_WGRAD_PTX, 'F(4x4) pre-transformed weight gradient, X6 planes', _X6P,
          partial(wino4_wgrad_pt, planes=True), _wino4_ptx_wgrad_cands),
)}


def _family(name):
    """One conv family as a single row (what a dispatcher evaluates once per call): its first row with the
    candidates of all its rows."""
    rows = [r for r in CONV_ROUTES.values() if r.family == name]
    shared = [(r.weights, r.offer, r.also, r.grp) for r in rows]
    assert shared.count(shared[0]) == len(rows), name
    return rows[0]._replace(name=name, cfgs=tuple(c for r in rows for c in r.cfgs))


CONV_FAMILIES = tuple(_family(n) for n in ('f2', 'f4', 'f4b', 'pt', 'ptx'))   # the order _sets_key reads
GRP_FAMILIES = CONV_FAMILIES[:2]   # the ones with grouped launchers


class WinoWeights:
    """Winograd-domain weights of several 3x3 convs whose fp32 weights live in one arena: per layer every
    kind of set (SET_KINDS) the layer is offered, the data-gradient kinds with ``dgrad=True``, in one buffer.

    ``refresh()`` transforms every LIVE set in one launch per weight update.  The convs take
    the sets through ``lazy(kind, l)`` callables, which the autotuned conv calls only when a Winograd
    candidate of that kind runs: a set that is not fresh this step is transformed on demand (always
    correct), and ``end_step()`` narrows the live sets to the ones the tuned convs actually used, so a
    step pays only for the transforms it needs (outside graph capture; the captured step replays the
    narrowed refresh)."""

    KINDS = tuple(k.name for k in SET_KINDS)

    def __init__(self, arena: torch.Tensor, weights, dgrad=True, f4=None, hw=None):
        """hw[l]: the layer's map size (F(4x4) sets only where it is a multiple of 4; None: every layer)."""
        self.arena = arena
        self.weights = list(weights)
        self.dgrad = dgrad
        f4 = WINO4 if f4 is None else f4
        self._layers, self._sets, off = [], {}, 0
        for l, w in enumerate(self.weights):
            Cout = w.shape[0]
            Cin = w.numel() // (9 * Cout)
            so = (w.data_ptr() - arena.data_ptr()) // 4
            assert 0 <= so and so + w.numel() <= arena.numel() and w.is_contiguous()
            self._layers.append((so, Cout, Cin))
            for k in SET_KINDS:
                rows, cols = _set_dims(k, Cout, Cin)
                if (dgrad or not k.dgrad) and k.offered(f4, None if hw is None else hw[l], rows, cols):
                    self._sets[(k.name, l)] = (off, k.size(rows, cols))
                    off += k.size(rows, cols)
        self.buf = torch.zeros(max(off, 1), dtype=torch.float32, device=arena.device)
        self._tables = {}
        self.live = frozenset(self._sets)
        self._fresh = set()
        self._used = set()
        self._prepare(self.live)

    def _prepare(self, live):
        """The table rk_wino_weights_all transforms the ``live`` sets by, (desc, meta, nblocks), or None for no
        set.  meta has one row per (family, layer) with a live set: (weight offset in the arena, forward set's
        offset in buf or -1, data-gradient set's or -1, Cout, Cin); desc one row per 32 x 32 filter block of
        it: (meta row, co0, ci0, family)."""
        if live not in self._tables:
            desc, meta = [], []
            for fam in sorted({k.family for k in SET_KINDS}):
                for l, (so, Cout, Cin) in enumerate(self._layers):
                    offs = {k.dgrad: k.unit * self._sets[(k.name, l)][0]
                            for k in SET_KINDS if k.family == fam and (k.name, l) in live}
                    if not offs:
                        continue
                    desc += [[len(meta), co0, ci0, fam] for co0 in range(0, Cout, 32) for ci0 in range(0, Cin, 32)]
                    meta.append([so, offs.get(False, -1), offs.get(True, -1), Cout, Cin])
            dev = self.arena.device
            self._tables[live] = (torch.tensor(desc, dtype=torch.int32, device=dev).reshape(-1),
                                  torch.tensor(meta, dtype=torch.int64, device=dev).reshape(-1),
                                  len(desc)) if desc else None
        return self._tables[live]

    def refresh(self):
        """Every live set of every family in ONE launch (rk_wino_weights_all)."""
        table = self._prepare(self.live)
        if table is not None:
            desc, meta, nb = table
            _lib.call("rk_wino_weights_all", _p(self.arena), _p(self.buf), _p(desc), nb, _p(meta), _s())
        self._fresh = set(self.live)

    def end_step(self):
        """Narrow the live sets to the ones this step's convs used (no-op inside graph capture)."""
        used, self._used = frozenset(self._used), set()
        if not used or used == self.live:
            return
        try:
            capturing = torch.cuda.is_current_stream_capturing()
        except Exception:
            capturing = False
        if not capturing:
            self._prepare(used)
            self.live = used

    def _view(self, kind, l):
        off, n = self._sets[(kind, l)]
        return KIND[kind].view(self.buf[off:off + n], *_set_dims(KIND[kind], *self._layers[l][1:]))

    def _ensure(self, kind, l):
        if (kind, l) not in self._fresh:   # not refreshed this step: transform this layer's set now
            k = KIND[kind]
            so, Cout, Cin = self._layers[l]
            w = self.arena[so:so + 9 * Cout * Cin]
            v = _p(self._view(kind, l))
            _lib.call(k.entry, _p(w), None if k.dgrad else v, v if k.dgrad else None, Cout, Cin, _s())
            self._fresh.add((kind, l))
        self._used.add((kind, l))
        return self._view(kind, l)

    def has(self, kind, l):
        return (kind, l) in self._sets

    def lazy(self, kind, l):
        """Callable returning the fresh set (or None when the layer has no such set)."""
        if (kind, l) not in self._sets:
            return None
        return lambda: self._ensure(kind, l)

    def conv_sets(self, l, dgrad=False):
        """Layer l's lazy sets as the weight-set kwargs of conv_fwd (``dgrad``: of conv_dgrad)."""
        return conv_sets(lambda kind: self.lazy(kind, l), dgrad)

    def u(self, l):
        return self._view('u2', l)

    def ut(self, l):
        assert self.dgrad
        return self._view('ut2', l)

    def u4(self, l):
        return self._view('u4', l) if ('u4', l) in self._sets else None

    def ut4(self, l):
        return self._view('ut4', l) if ('ut4', l) in self._sets else None

    def u4p(self, l):
        return self._view('u4p', l) if ('u4p', l) in self._sets else None


# ----------------------------------------------------------------------------------------- dense
# Pre-split X6 dense candidates (cfg = (XP_DENSE, x6p tile * 4 + nst, splits)): both operands split into bf16
# planes by one pass each (x6p_split / x6p_split_t, inside the timed candidate), then the x6p GEMM — its K
# loop is LDS reads + MFMAs only, where the sgemm X6 loop re-splits every fragment after its LDS read and runs
# VALU-bound (the PG-GAN dense layers: 512 x 8192 at mb 512, profiles/pg_gan_lod3_f32_kernels_r5.txt); the
# bias / activation / gate epilogue and the split-K combine ride in sreduce_epi / reduce_slabs
XP_DENSE = -21
XPD_MIN_MACS = 1 << 28   # GEMM size below which the split passes cannot pay (VGG / MLP heads, tiny layers)
XPD_CFGS = tuple((XP_DENSE, x6p_pack(t, n), s) for t in (0, 1, 2, 3) for n in (2, 3) for s in (1, 2, 4)) + \
    tuple((XP_DENSE, x6p_pack(t, 2), s) for t in (7, 8) for s in (1, 2, 4)) if USE_X6P else ()


def _xpd(cfg):
    return cfg[0] == XP_DENSE


def _offer_xpd(key, cands, macs, fits=True):
    """(key, candidates) of a dense op, with the pre-split X6 candidates where the GEMM is big enough to pay for
    the split passes and ``fits`` them (the op's own conditions): the key then says so."""
    if fits and macs >= XPD_MIN_MACS:
        return key + ('xp',), cands + list(XPD_CFGS)
    return key, cands


def _xp_gemm_into(A, B, M, N, K, code, s, out=None, accumulate=False):
    """x6p GEMM of planes A [3][M][K] . B [3][N][K]^T: into ``out`` (s == 1) or a fresh [s][M][N] slab."""
    s = x6p_splits(K, s)
    tile, nst = x6p_unpack(code)
    if s == 1 and out is not None:
        x6p_gemm(A, B, out, M, N, K, tile=tile, nst=nst, accumulate=accumulate)
        return out, 1
    slab = torch.empty((s, M, N), device=A.device, dtype=torch.float32)
    x6p_gemm(A, B, slab, M, N, K, tile=tile, nst=nst, splits=s)
    return slab, s


def linear(x: torch.Tensor, w: torch.Tensor, bias=None, *, act=ACT_NONE, slope=0.2, out=None, alpha=1.0):
    """out = act(alpha * x @ w.T + bias), fp32; small-M layers autotune split-K + a fused combine."""
    M, K = x.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty((M, N), device=x.device, dtype=torch.float32)
    epi = dict(bias=bias, act=act, slope=slope, alpha=alpha)

    def run(cfg):
        if _xpd(cfg):
            slab, _ = _xp_gemm_into(x6p_split(x), x6p_split(w), M, N, K, cfg[1], cfg[2])
            sreduce_epi(slab, M, N, out, **epi)
            return
        _gemm(cfg, lambda dst, ldc, **kw: sgemm(KIND_DENSE, x, w, dst, M, N, K, x.stride(0), w.stride(0), ldc, **kw),
              out, M, N, ldc=out.stride(0), **epi)
    key, cands = _offer_xpd(('sl', M, N, K, act, bias is not None, float(alpha)),
                            _cands(M, N, splittable=N % 4 == 0 and out.stride(0) % 4 == 0, K=K), M * N * K,
                            K % 32 == 0 and x.is_contiguous() and w.is_contiguous())
    run(_pick(key, cands, run))
    return out


def linear_dx(dy: torch.Tensor, w: torch.Tensor, *, gate=None, out=None):
    """dx[M][in] = dy[M][out] @ w[out][in], optionally gated (dx = 0 where gate <= 0)."""
    M, Nout = dy.shape
    Nin = w.shape[1]
    if out is None:
        out = torch.empty((M, Nin), device=dy.device, dtype=torch.float32)

    def run(cfg):
        if _xpd(cfg):
            slab, _ = _xp_gemm_into(x6p_split(dy), x6p_split_t(w), M, Nin, Nout, cfg[1], cfg[2])
            sreduce_epi(slab, M, Nin, out, gate=gate)
            return
        _gemm(cfg, lambda dst, ldc, **kw: sgemm(KIND_DENSE_DX, dy, w, dst, M, Nin, Nout, dy.stride(0), w.stride(0),
                                                ldc, **kw),
              out, M, Nin, ldc=out.stride(0), gate=gate)
    key, cands = _offer_xpd(('sx', M, Nin, Nout, gate is not None), _cands(M, Nin, splittable=Nin % 4 == 0, K=Nout),
                            M * Nin * Nout, Nout % 32 == 0 and dy.is_contiguous() and w.is_contiguous())
    run(_pick(key, cands, run))
    return out


def linear_dw(dy: torch.Tensor, x: torch.Tensor, *, out=None, accumulate=False):
    """dw[out][in] = dy[M][out]^T @ x[M][in] (fp32)."""
    M, Nout = dy.shape
    Nin = x.shape[1]
    if out is None:
        out = torch.empty((Nout, Nin), device=dy.device, dtype=torch.float32)

    def run(cfg):
        if _xpd(cfg):
            Mp = cdiv(M, 32) * 32
            res, k = _xp_gemm_into(x6p_split_t(dy, Mp), x6p_split_t(x, Mp), Nout, Nin, Mp, cfg[1], cfg[2],
                                   out=out if out.is_contiguous() else None, accumulate=accumulate)
            if k > 1 or res is not out:
                reduce_slabs(res, out, accumulate=accumulate)
            return
        _gemm(cfg, lambda dst, ldc, **kw: sgemm(KIND_DENSE_DW, dy, x, dst, Nout, Nin, M, dy.stride(0), x.stride(0),
                                                ldc, **kw),
              out, Nout, Nin, accumulate=bool(accumulate))
    key, cands = _offer_xpd(('sdw', M, Nout, Nin, bool(accumulate)), _cands(Nout, Nin, splittable=True, K=M),
                            Nout * Nin * M)
    run(_pick(key, cands, run, protect=(out,) if accumulate else ()))
    return out


def sreduce_epi(slab, M, N, out, *, bias=None, act=ACT_NONE, slope=0.2, alpha=1.0, gate=None, bias_rows=0):
    """out = act(alpha * sum_s slab[s] + bias) (gated); bias_rows > 0: row block g uses bias[g]."""
    _lib.call("rk_sreduce_epi", _p(slab), slab.shape[0], int(M), int(N), _p(bias), int(act), float(slope),
              float(alpha), _p(gate), 0 if gate is None else gate.stride(0), _p(out), out.stride(0), int(bias_rows),
              _s())
    return out


def reduce_slabs(slab, out, *, accumulate=False, scale=1.0):
    from .functional import reduce_slabs as _rs
    return _rs(slab, out, accumulate=accumulate, scale=scale)


def lrelu_gate(gy: torch.Tensor, y: torch.Tensor, slope: float, out=None):
    """gy * (y > 0 ? 1 : slope) (fp32, contiguous, same shape)."""
    _check(gy, 'lrelu_gate gy')
    _check(y, 'lrelu_gate y')
    assert gy.shape == y.shape
    if out is None:
        out = torch.empty_like(gy)
    _lib.call("rk_lrelu_gate_f32", _p(gy), _p(y), _p(out), gy.numel(), float(slope), _s())
    return out


def lrelu_gate_colsum(gy: torch.Tensor, y: torch.Tensor, slope: float, acc=None):
    """(g, colsum(g)) with g = lrelu_gate(gy, y, slope) in one pass; gy / y [..., C] fp32.  ``acc`` (fp32
    [C]): the column sum is added into it instead (returns (g, acc))."""
    _check(gy, 'lrelu_gate_colsum gy')
    _check(y, 'lrelu_gate_colsum y')
    assert gy.shape == y.shape
    Cc = gy.shape[-1]
    R = gy.numel() // Cc
    g = torch.empty_like(gy)
    chunks = _colsum_chunks(R, Cc) if Cc % 4 == 0 else 1
    part = torch.empty((chunks, Cc), device=gy.device, dtype=torch.float32)
    _lib.call("rk_lrelu_gate_colsum_f32", _p(gy), _p(y), _p(g), R, Cc, float(slope), _p(part), chunks, _s())
    if acc is not None:
        assert acc.shape == (Cc,) and acc.dtype == torch.float32 and acc.is_contiguous()
        if Cc % 4:   # odd width (the slab fold takes whole float4s)
            return g, acc.add_(part.sum(0))
        return g, reduce_slabs(part, acc, accumulate=True)
    if chunks == 1:
        return g, part[0]
    out = torch.empty(Cc, device=gy.device, dtype=torch.float32)
    return g, reduce_slabs(part, out)


def _colsum_chunks(R, Cc):
    """Row chunks of the column-sum kernels: ~2 blocks per CU over the column blocks (256 columns per
    block on the vectorised path, C % 4 == 0; 64 otherwise), >= 64 rows per chunk."""
    cols = min(Cc // 4, 64) * 4 if Cc % 4 == 0 else 64
    return max(1, min(cdiv(R, 64), cdiv(2 * NUM_CU, cdiv(Cc, cols))))


def colsum(x2d, out, *, accumulate=False):
    """out[c] (+)= sum_r x2d[r, c] (fp32).  Tall inputs split the rows over ~2 blocks per CU, then fold
    the partial rows with reduce_slabs."""
    R, Cc = x2d.shape
    chunks = _colsum_chunks(R, Cc)
    if chunks == 1:
        _lib.call("rk_colsum_f32", _p(x2d), R, Cc, x2d.stride(0), _p(out), int(accumulate), 1, _s())
        return out
    part = torch.empty((chunks, Cc), device=x2d.device, dtype=torch.float32)
    _lib.call("rk_colsum_f32", _p(x2d), R, Cc, x2d.stride(0), _p(part), 0, chunks, _s())
    if Cc % 4:   # the slab fold takes whole float4s; an odd width (not on the engines' padded paths) folds here
        s = part.sum(0)
        return out.add_(s) if accumulate else out.copy_(s)
    return reduce_slabs(part, out, accumulate=accumulate)


# -------------------------------------------------------------------------------------- batchnorm
def bn_fwd(y, acc, count, gamma, beta, eps, running_mean=None, running_var=None, momentum=0.1, *, pool=False,
           act=ACT_RELU, slope=0.2, coeffs=None, out=None):
    """Train-mode BN (+act, +2x2 max-pool) from the fp64 slot sums ``acc`` [SL][2][C]; writes coeffs
    [4][C] = mean, rstd, scale, shift (for backward).  Returns (out, coeffs)."""
    Nb, H, W, C = y.shape
    if coeffs is None:
        coeffs = torch.empty((4, C), device=y.device, dtype=torch.float32)
    if out is None:
        shape = (Nb, H // 2, W // 2, C) if pool else (Nb, H, W, C)
        out = torch.empty(shape, device=y.device, dtype=torch.float32)
    _lib.call("rk_bnf_fwd", _p(y), _p(acc), acc.shape[0], float(count), _p(gamma), _p(beta), float(eps),
              _p(running_mean), _p(running_var), float(momentum), None, None, _p(coeffs), _p(out), Nb, H, W, C,
              int(pool), int(act), float(slope), _s())
    return out, coeffs


def bn_finalize(y, acc, count, gamma, beta, eps, running_mean=None, running_var=None, momentum=0.1, *, coeffs=None):
    """The coefficient half of bn_fwd (one block): coeffs [4][C] = mean, rstd, scale, shift and the
    running-statistics update, no output pass — the consumer conv normalises + ReLUs y on its loads
    (conv_fwd(pro=coeffs), conv_wgrad(xpro=coeffs))."""
    Nb, H, W, C = y.shape
    if coeffs is None:
        coeffs = torch.empty((4, C), device=y.device, dtype=torch.float32)
    _lib.call("rk_bnf_fwd", _p(y), _p(acc), acc.shape[0], float(count), _p(gamma), _p(beta), float(eps),
              _p(running_mean), _p(running_var), float(momentum), None, None, _p(coeffs), None, Nb, H, W, C,
              0, int(ACT_RELU), 0.2, _s())
    return coeffs


def bn_eval(y, scale, shift, *, pool=False, act=ACT_RELU, slope=0.2, out=None):
    Nb, H, W, C = y.shape
    if out is None:
        shape = (Nb, H // 2, W // 2, C) if pool else (Nb, H, W, C)
        out = torch.empty(shape, device=y.device, dtype=torch.float32)
    _lib.call("rk_bnf_fwd", _p(y), None, 0, 1.0, None, None, 0.0, None, None, 0.0, _p(scale), _p(shift), None, _p(out),
              Nb, H, W, C, int(pool), int(act), float(slope), _s())
    return out


def col_stats(a2d, acc, b2d=None):
    """fp64 slot 0 of ``acc`` += per-column (sum a, sum a*b) (b = a when None)."""
    R, C = a2d.shape
    _lib.call("rk_bnf_colstats", _p(a2d), _p(b2d), R, C, _p(acc), _s())
    return acc


_BWD_BLOCKS = 1024   # grid cap of the BN-backward reduce (8 passes of pixel rows per block)


def bn_bwd(dout, y, coeffs, gamma, acc, *, pool=False, act=ACT_RELU, slope=0.2, dgamma=None, dbeta=None, dy=None,
           accumulate=False, reduced=False, count=None):
    """Backward of out = pool?(act(BN(y))).  ``acc``: zeroed fp64 [SL][2][C] for (sum dz, sum dz*y);
    ``reduced``: the producer of dout already accumulated them (conv_dgrad(bnb=/bnp=...)).
    ``count`` (default the pixel count): ``inf`` with unit coefficients drops the normalisation terms
    (dy = the act mask / pool routing of dout; ``dbeta`` = sum dz, a bias gradient)."""
    Nb, H, W, C = y.shape
    s = _s()
    if not reduced:
        if C <= 1024 and not (C & (C - 1)):
            npix = dout.numel() // C
            # 8 passes of 256 / (C / 4) pixel rows per block (2 passes: 4x the slot atomics, measured slower)
            blocks = max(1, min(_BWD_BLOCKS, cdiv(npix, max(1, 256 // (C // 4)) * 8)))
            _lib.call("rk_bnf_bwd_reduce", _p(dout), _p(y), _p(coeffs), _p(acc), acc.shape[0], blocks, Nb, H, W, C,
                      int(pool), int(act), float(slope), s)
        elif not pool and act == ACT_NONE:
            col_stats(dout.reshape(-1, C), acc, y.reshape(-1, C))
        else:
            raise ValueError('bn_bwd: unsupported channel count {} for pool/act'.format(C))
    if dy is None:
        dy = torch.empty_like(y)
    _lib.call("rk_bnf_bwd_apply", _p(dout), _p(y), _p(coeffs), _p(acc), acc.shape[0],
              float(Nb * H * W) if count is None else float(count), _p(gamma),
              _p(dgamma), _p(dbeta), int(accumulate), _p(dy), Nb, H, W, C, int(pool), int(act), float(slope), s)
    return dy


# ----------------------------------------------------------------------------------- loss / misc
def softmax_xent(logits, labels, ncls, *, dlogits=None, probs=None, loss_sum=None, correct=None, counted=None,
                 ignore_index=-100, grad_scale=None):
    B = logits.shape[0]
    if grad_scale is None:
        grad_scale = 1.0 / max(1, B)
    if dlogits is not None:
        _check(dlogits, 'softmax_xent dlogits')
    _lib.call("rk_softmax_xent_f32", _p(logits), logits.stride(0), _p(labels), B, ncls, ignore_index,
              float(grad_scale), _p(dlogits), 0 if dlogits is None else dlogits.stride(0), _p(probs), _p(loss_sum),
              _p(correct), _p(counted), _s())


def softmax_xent_soft(logits, labels, ncls, *, labels2=None, lam=None, eps=0.0, dlogits=None, loss_sum=None,
                      correct=None, counted=None, ignore_index=-100, grad_scale=None):
    """``functional.softmax_xent_soft`` with fp32 d(logits)."""
    B = logits.shape[0]
    if grad_scale is None:
        grad_scale = 1.0 / max(1, B)
    if dlogits is not None:
        _check(dlogits, 'softmax_xent_soft dlogits')
    _check_soft(labels2, lam, labels)
    _lib.call("rk_softmax_xent_f32_soft", _p(logits), logits.stride(0), _p(labels), _p(labels2), _p(lam), float(eps),
              B, ncls, ignore_index, float(grad_scale), _p(dlogits), 0 if dlogits is None else dlogits.stride(0),
              _p(loss_sum), _p(correct), _p(counted), _s())


HEAD_NC = (8, 16, 32)


def head_ok(ncls_p: int, D: int) -> bool:
    """Shapes the fused classifier head (csrc/kernels/head.hip) takes."""
    return ncls_p in HEAD_NC and D % 32 == 0 and D > 0


def head_fwd_bwd(z, w, bias, labels, ncls, *, dlogits, dz, gated, loss_sum=None, correct=None, counted=None,
                 grad_scale=None):
    """Output layer + softmax cross-entropy + its data gradient in one launch: z [B][D] -> dlogits [B][NC]
    ((softmax - onehot) * grad_scale), dz [B][D] = dlogits W (gated by z > 0 when ``gated``)."""
    _check(z, 'head z')
    B, D = z.shape
    NC = w.shape[0]
    assert w.shape == (NC, D) and dlogits.shape == (B, NC) and dz.shape == (B, D)
    _lib.call("rk_head_fwd_bwd", _p(z), B, D, _p(w), _p(bias), NC, _p(labels), int(ncls),
              float(1.0 / max(1, B) if grad_scale is None else grad_scale), _p(dlogits), _p(dz), int(bool(gated)),
              _p(loss_sum), _p(correct), _p(counted), _s())


def head_fwd_bwd_soft(z, w, bias, labels, ncls, *, labels2=None, lam=None, eps=0.0, dlogits, dz, gated,
                      loss_sum=None, correct=None, counted=None, grad_scale=None):
    """``head_fwd_bwd`` against the soft target of ``softmax_xent_soft`` (labels2 / lam / eps as there)."""
    _check(z, 'head z')
    B, D = z.shape
    NC = w.shape[0]
    assert w.shape == (NC, D) and dlogits.shape == (B, NC) and dz.shape == (B, D)
    _check_soft(labels2, lam, labels)
    _lib.call("rk_head_fwd_bwd_soft", _p(z), B, D, _p(w), _p(bias), NC, _p(labels), _p(labels2), _p(lam), float(eps),
              int(ncls), float(1.0 / max(1, B) if grad_scale is None else grad_scale), _p(dlogits), _p(dz),
              int(bool(gated)), _p(loss_sum), _p(correct), _p(counted), _s())


def head_dw(z, dlogits, dz, *, dw, db=None, dbh=None):
    """dw [NC][D] = dlogits^T z, db = colsum(dlogits), dbh = colsum(dz) (the hidden layer's bias gradient)."""
    B, D = z.shape
    NC = dlogits.shape[1]
    _lib.call("rk_head_dw", _p(z), _p(dlogits), _p(dz), B, D, NC, _p(dw), _p(db), _p(dbh), _s())


def pack_nhwc(images, cpad=4, scale=1.0, shift=0.0, out=None, nhwc=False, idx=None):
    """uint8/float32 NCHW (``nhwc``: NHWC) -> fp32 NHWC with channels padded to ``cpad``, x*scale+shift.
    ``idx`` (int32 [n], device): pack images[idx] (the minibatch gather in the same pass)."""
    if nhwc:
        Nb, H, W, Cc = images.shape
    else:
        Nb, Cc, H, W = images.shape
    nsrc = Nb
    if idx is not None:
        assert idx.dtype == torch.int32 and idx.is_cuda and idx.dim() == 1
        idx = idx.contiguous()
        Nb = idx.numel()
    if out is None:
        out = torch.empty((Nb, H, W, cpad), device=images.device, dtype=torch.float32)
    is_u8 = 1 if images.dtype == torch.uint8 else 0
    if not is_u8 and images.dtype != torch.float32:
        images = images.float()
    _lib.call("rk_pack_nhwc_f32", _p(images.contiguous()), is_u8 | (2 if nhwc else 0), Nb, Cc, H, W, cpad,
              float(scale), float(shift), _p(out), _p(idx), nsrc, _s())
    return out


# ------------------------------------------------------------------- stride-2 gather convolutions
# The PG-GAN resampling convs as one family closed under differentiation:
#   S2(x, W)  : y[o]  = sum_t W[t] x[2o + d_t]       (4x4 taps d_t in {-1..2}^2, stride 2)
#   S2T(z, W) : x'[p] = sum_{o,t: 2o + d_t = p} W[t]^T z[o]    (its adjoint: the 2x transposed conv)
#   S2W(x, g) : dW[t] = sum_o g[o] x[2o + d_t]^T   (weight gradient)
# with W [Co][16][Ci] (tap t = 4(dy+1) + dx+1).  conv3x3 + 2x2 box downscale (_conv2d_downscale2d,
# pg_gans.py:1053-1059) is S2 with box-summed weights; upscale2d + conv3x3 (_upscale2d_conv2d,
# pg_gans.py:1032-1039) is S2T with box-summed flipped weights — both at 1/2.25 of the MACs of the
# full-resolution conv and without any materialised 2x tensor.
def _tap_word(vals):
    w = 0
    for t, v in enumerate(vals):
        w |= (int(v) + 1 & 3) << (2 * t)
    return w


def _par_d(r, u):
    return (0 if u == 0 else 2) if r == 0 else (1 if u == 0 else -1)


_S2_TPY = _tap_word([t // 4 - 1 for t in range(16)])
_S2_TPX = _tap_word([t % 4 - 1 for t in range(16)])
# S2T parity group g = 2 ry + rx, tap t4 = 2u + v: source offset (r - d) / 2 of the matching S2 tap
_S2T_TPY = [_tap_word([(g >> 1) - _par_d(g >> 1, t4 >> 1) >> 1 for t4 in range(4)]) for g in range(4)]
_S2T_TPX = [_tap_word([(g & 1) - _par_d(g & 1, t4 & 1) >> 1 for t4 in range(4)]) for g in range(4)]
_S2T_OYX = sum(((g >> 1) | ((g & 1) << 1)) << (2 * g) for g in range(4))


def _u32x4(vals):
    import ctypes
    v = list(vals) + [0] * (4 - len(vals))
    return (ctypes.c_uint * 4)(*v)


def sgemm_g(kind, A, B, out, M, N, K, lda, ldb, ldc, H, W, C, Ho, Wo, stride, ntaps, tpy, tpx, *, groups=1, oyx=0,
            os_=1, gstride_b=0, tile=0, nst=2, splits=1, slab_stride=0, bias=None, flags=0, alpha=1.0, slope=0.2):
    _lib.call("rk_sgemm_g", int(kind), int(tile), int(nst), _p(A), _p(B), _p(out), _p(bias), int(M), int(N), int(K),
              int(lda), int(ldb), int(ldc), int(H), int(W), int(C), int(Ho), int(Wo), int(stride), int(ntaps),
              int(groups), _u32x4(tpy), _u32x4(tpx), int(oyx), int(os_), int(gstride_b), int(splits),
              int(slab_stride), int(flags), float(alpha), float(slope), _nbytes(A), _nbytes(B), _s())
    return out


def s2_conv(x, W, *, bias=None, act=ACT_NONE, slope=0.2, out=None):
    """S2: x [N, H, W, Ci] -> [N, H/2, W/2, Co] with W [Co, 16*Ci] (+bias, act)."""
    _check(x, 's2_conv x')
    Nb, H, Wd, Ci = x.shape
    Co = W.shape[0]
    assert W.numel() == Co * 16 * Ci and H % 2 == 0 and Wd % 2 == 0, (W.shape, x.shape)
    Ho, Wo = H // 2, Wd // 2
    M, K = Nb * Ho * Wo, 16 * Ci
    if out is None:
        out = torch.empty((Nb, Ho, Wo, Co), device=x.device, dtype=torch.float32)
    flags = _act_flags(bias, act)

    def run(cfg):
        _gemm(cfg, lambda dst, ldc, **kw: sgemm_g(6, x, W, dst, M, Co, K, Ci, K, ldc, H, Wd, Ci, Ho, Wo, 2, 16,
                                                  [_S2_TPY], [_S2_TPX], **kw),
              out, M, Co, bias=bias, act=act, slope=slope)
    run(_pick(('s2f', M, Co, K, H, Wd, Ci, flags), _cands(M, Co, splittable=Co % 4 == 0, K=K), run))
    return out


def s2t_weights(W, Co, Ci):
    """W [Co, 16*Ci] -> the 4 parity groups' [Ci][4 taps * Co] B operands of S2T."""
    out = torch.empty((4, Ci, 4 * Co), device=W.device, dtype=torch.float32)
    _lib.call("rk_s2t_weights", _p(W), _p(out), int(Co), int(Ci), _s())
    return out


def s2t_conv(z, W, *, bias=None, act=ACT_NONE, slope=0.2, out=None, wr=None):
    """S2T: z [N, h, w, Co] -> [N, 2h, 2w, Ci] (the adjoint of S2 with the same W [Co, 16*Ci]):
    four output-parity GEMMs of 4 taps each in ONE launch (grid = 4 parity groups x tiles)."""
    _check(z, 's2t_conv z')
    Nb, h, w, Co = z.shape
    Ci = W.numel() // (16 * Co)
    assert W.numel() == Co * 16 * Ci
    if wr is None:
        wr = s2t_weights(W, Co, Ci)
    M, K = Nb * h * w, 4 * Co
    if out is None:
        out = torch.empty((Nb, 2 * h, 2 * w, Ci), device=z.device, dtype=torch.float32)
    flags = _act_flags(bias, act)

    def run(cfg):
        _gemm(cfg, lambda dst, ldc, **kw: sgemm_g(6, z, wr, dst, M, Ci, K, Co, K, ldc, h, w, Co, h, w, 1, 4, _S2T_TPY,
                                                  _S2T_TPX, groups=4, oyx=_S2T_OYX, os_=2, gstride_b=Ci * K, **kw),
              out, M, Ci, groups=4, bias=bias, act=act, slope=slope)
    run(_pick(('s2t', M, Ci, K, h, w, Co, flags), _cands(M, Ci, splittable=Ci % 4 == 0, K=K), run))
    return out


def s2_wgrad(x, g, *, out=None):
    """S2W: dW [Co, 16*Ci] = sum_o g[o] (x) x[2o + d_t]; x [N, H, W, Ci], g [N, H/2, W/2, Co]."""
    _check(x, 's2_wgrad x')
    _check(g, 's2_wgrad g')
    Nb, H, Wd, Ci = x.shape
    Co = g.shape[-1]
    Ho, Wo = H // 2, Wd // 2
    assert g.shape == (Nb, Ho, Wo, Co), (g.shape, x.shape)
    M, N, K = Co, 16 * Ci, Nb * Ho * Wo
    if out is None:
        out = torch.empty((Co, N), device=x.device, dtype=torch.float32)

    def run(cfg):
        _gemm(cfg, lambda dst, ldc, **kw: sgemm_g(7, g, x, dst, M, N, K, Co, Ci, ldc, H, Wd, Ci, Ho, Wo, 2, 16,
                                                  [_S2_TPY], [_S2_TPX], **kw),
              out, M, N, accumulate=False)
    run(_pick(('s2w', M, N, K, H, Wd, Ci), _lead_with_split(_cands(M, N, splittable=True, K=K), M, N), run))
    return out


# ------------------------------------------------------------------------------------ resampling
def upscale2x(x, scale=1.0, out=None):
    """nearest 2x upscale of NHWC fp32 / bf16 (times ``scale``)."""
    Nb, H, W, Cc = x.shape
    if out is None:
        out = torch.empty((Nb, 2 * H, 2 * W, Cc), device=x.device, dtype=x.dtype)
    _lib.call("rk_resample2x", 0, int(x.dtype == torch.bfloat16), _p(x.contiguous()), _p(out), Nb, H, W, Cc,
              float(scale), _s())
    return out


def downscale2x(x, scale=0.25, out=None):
    """``scale`` x 2x2 sum of NHWC fp32 / bf16 (0.25: the box-filter downscale2d)."""
    Nb, H, W, Cc = x.shape
    if out is None:
        out = torch.empty((Nb, H // 2, W // 2, Cc), device=x.device, dtype=x.dtype)
    _lib.call("rk_resample2x", 1, int(x.dtype == torch.bfloat16), _p(x.contiguous()), _p(out), Nb, H, W, Cc,
              float(scale), _s())
    return out


def conv_wt(w, taps=9):
    """w [Cout, taps*Cin] -> [Cin, taps*Cout] flipped transposed weights: conv_dgrad(dy, conv_wt(w)) is the
    data gradient of conv_fwd(x, w) (one LDS-tiled transpose launch; the autograd path's per-call
    equivalent of SConvWT)."""
    Cout = w.shape[0]
    Cin = w.numel() // (taps * Cout)
    out = torch.empty((Cin, taps * Cout), device=w.device, dtype=torch.float32)
    _lib.call("rk_wflip_t", _p(w.contiguous()), _p(out), int(Cout), int(Cin), int(taps), _s())
    return out


# ------------------------------------------------------------------------------ grouped GEMMs
# k same-shape problems per launch (rk_sgemm_grp): the k models of an inference ensemble run each layer
# as ONE kernel (k x the workgroups of one model: small-batch layers fill the chip, launches / k).
def sgemm_grp(kind, A, B, out, M, N, K, lda, ldb, ldc, groups, gstride_a, gstride_b, gstride_o, gstride_bias=0, *,
              tile=0, nst=2, splits=1, slab_stride=0, bias=None, flags=0, alpha=1.0, slope=0.2, H=1, W=1, C=4,
              taps=1):
    _lib.call("rk_sgemm_grp", int(kind), int(tile), int(nst), _p(A), _p(B), _p(out), _p(bias), int(M), int(N), int(K),
              int(lda), int(ldb), int(ldc), int(H), int(W), int(C), int(taps), int(splits), int(slab_stride),
              int(flags), float(alpha), float(slope), _nbytes(A), _nbytes(B), int(groups), int(gstride_a),
              int(gstride_b), int(gstride_o), int(gstride_bias), _s())
    return out


def _grp_run(kind, A, B, out, M, N, K, lda, ldb, G, gsa, key, *, bias=None, act=ACT_NONE, slope=0.2, geo=None,
             fused=None):
    """Autotuned grouped launch: out [G, M, N]; split-K slabs [s, G*M, N] combined by sreduce_epi with
    per-group bias.  ``fused`` = (candidates, weight sets, epilogue): the grouped rows of CONV_ROUTES."""
    geo = geo or {}

    def gemm(dst, ldc, splits=1, **kw):
        # gstride_bias: a split launch takes no bias (its combine finds group g's by ``bias_rows``)
        return sgemm_grp(kind, A, B, dst, M, N, K, lda, ldb, ldc, G, gsa, N * K, M * N, N if splits == 1 else 0,
                         splits=splits, **geo, **kw)

    def run(cfg):
        if cfg[0] in CONV_ROUTES:
            _run_grp_route(cfg, A, fused[1], out, fused[2])
            return
        _gemm(cfg, gemm, out, M, N, groups=G, bias=bias, act=act, slope=slope, bias_rows=M)
    cands = [c for c in _cands(M * G, N, splittable=N % 4 == 0, K=K) if (c[0] & 15) < 4 or (c[0] & 15) in _FEW_WAVE]
    if fused is not None:
        cands.extend(fused[0])
    run(_pick(key, cands, run))
    return out


def _run_grp_route(cfg, x, sets, out, epi):
    r = CONV_ROUTES[cfg[0]]
    r.grp(x, sets[r.weights], out=out, variant=r.variant, **epi)


def conv_fwd_grp_pool_ok(H, W, Cin, wino, wino4):
    """conv_fwd_grp(pool=True) has a fused candidate for this shape (F(4x4) or the small-tile F(2x2))."""
    return any(_offered(GRP_FAMILIES, (wino, wino4), 9, H, W, Cin, 0, 0)[0])


def conv_fwd_grp(x, W, *, bias=None, act=ACT_NONE, slope=0.2, out=None, wino=None, wino4=None, pool=False):
    """k convs in one launch: x [G, Nb, H, W, Cin] (or [Nb, H, W, Cin] shared by every group),
    W [G, Cout, taps*Cin], bias [G, Cout] -> [G, Nb, H, W, Cout] (3x3 stride-1 or 1x1).
    ``wino``: stacked Winograd weights [G, 16, Cout, Cin] -> grouped fused F(2x2,3x3) candidates;
    ``wino4``: [G, 36, Cout, Cin] -> grouped F(4x4,3x3) candidates.  ``pool`` (bias + ReLU): the 2x2
    max-pool written by the fused kernels' epilogue -> [G, Nb, H/2, W/2, Cout] (only they are candidates;
    see conv_fwd_grp_pool_ok)."""
    G, Cout, K = W.shape
    shared = x.dim() == 4
    Nb, H, Wd, Cin = x.shape[-4:]
    taps = K // Cin
    assert taps in (1, 9) and K == taps * Cin and (shared or x.shape[0] == G), (x.shape, W.shape)
    _check(x, 'conv_fwd_grp x')
    M = Nb * H * Wd
    if pool:
        return _conv_fwd_grp_pooled(x, W, bias, act, out, wino, wino4)
    if out is None:
        out = torch.empty((G, Nb, H, Wd, Cout), device=x.device, dtype=torch.float32)
    (w2, w4), cfgs = _offered(GRP_FAMILIES, (wino, wino4), taps, H, Wd, Cin, Cout,
                              0 if act in (ACT_NONE, ACT_RELU) else E_DIRECT)
    assert not w2 or (wino.shape == (G, 16, Cout, Cin) and wino.is_contiguous())
    assert not w4 or (wino4.shape == (G, 36, Cout, Cin) and wino4.is_contiguous())
    fused = (cfgs, (wino, wino4), dict(bias=bias, relu=act == ACT_RELU)) if cfgs else None
    return _grp_run(0, x, W, out, M, Cout, K, Cin, K, G, 0 if shared else M * Cin,
                    ('sfg', G, M, Cout, K, H, Wd, Cin, shared, bias is not None, act, w2, w4), bias=bias,
                    act=act, slope=slope, geo=dict(H=H, W=Wd, C=Cin, taps=taps), fused=fused)


def _conv_fwd_grp_pooled(x, W, bias, act, out, wino, wino4):
    G, Cout, K = W.shape
    Nb, H, Wd, Cin = x.shape[-4:]
    assert bias is not None and act == ACT_RELU and K == 9 * Cin and H % 2 == 0 and Wd % 2 == 0
    if out is None:
        out = torch.empty((G, Nb, H // 2, Wd // 2, Cout), device=x.device, dtype=torch.float32)
    sets = (wino, wino4)
    w2, w4 = _offered(GRP_FAMILIES, sets, 9, H, Wd, Cin, Cout, 0)[0]
    # the F(4x4) rows lead: the first candidate is what a capture uses on a tune miss
    cands = [c for fam, o in (('f4', w4), ('f2', w2)) if o
             for r in CONV_ROUTES.values() if r.family == fam and r.pool for c in r.cfgs]
    if not cands:
        raise ValueError('conv_fwd_grp(pool=True): no fused candidate (see conv_fwd_grp_pool_ok)')
    epi = dict(bias=bias, relu=True, pool=True)

    def run(cfg):
        _run_grp_route(cfg, x, sets, out, epi)
    run(_pick(('sfgp', G, Nb * H * Wd, Cout, K, H, Wd, Cin, x.dim() == 4, w2, w4), cands, run))
    return out


def linear_grp(x, w, bias=None, *, act=ACT_NONE, slope=0.2, out=None):
    """k dense layers in one launch: x [G, M, K] (or [M, K] shared), w [G, N, K], bias [G, N] -> [G, M, N]."""
    G, N, K = w.shape
    shared = x.dim() == 2
    M = x.shape[-2]
    _check(x, 'linear_grp x')
    if out is None:
        out = torch.empty((G, M, N), device=x.device, dtype=torch.float32)
    return _grp_run(3, x, w, out, M, N, K, K, K, G, 0 if shared else M * K,
                    ('slg', G, M, N, K, shared, bias is not None, act), bias=bias, act=act, slope=slope)


def bn_eval_grp(y, scale, shift, *, pool=False, act=ACT_RELU, slope=0.2, out=None):
    """eval BN(+act, +2x2 max-pool) of G stacked batches y [G, Nb, H, W, C] with per-group scale / shift [G, C]."""
    G, Nb, H, W, C = y.shape
    if out is None:
        out = torch.empty((G, Nb, H // 2 if pool else H, W // 2 if pool else W, C), device=y.device,
                          dtype=torch.float32)
    _lib.call("rk_bnf_eval_grp", _p(y), _p(scale.contiguous()), _p(shift.contiguous()), _p(out), G, Nb, H, W, C,
              int(pool), int(act), float(slope), _s())
    return out
