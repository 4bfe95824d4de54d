"""fp64 references, an fp32 yardstick and input sets for the BiLSTM recurrence (csrc/kernels/lstm.hip), the
embedding kernels (csrc/kernels/embed.hip) and the tagger's side kernels (csrc/kernels/tagger.hip), shared by
tests/test_lstm_refs.py (CPU: the references against fp64 torch.nn.LSTM autograd, and how far a wrong formula
moves them), tests/test_lstm_kernels_gpu.py and tests/test_tagger_kernels_gpu.py (the kernels against them).

Nothing here calls a kernel of this project.  Everything is in the kernels' own layouts, so the raw entry
points can be fed directly (HP hidden units per direction, gate blocks [i | f | g | o] of HP each):

    gin   [T][B][2][4HP]  input projection incl. both biases      whh   [2][4HP][HP]
    hout  [T][B][2][HP]                                           csave [T][B][2][HP]
    gsave [T][B][2][4HP]  activated gates                         dhout [T][B][2][HP]     dgin [T][B][2][4HP]

The functions take the dtype they are asked for.  float64 is the reference.  float32 is the yardstick: every
operation in fp32, exp(x) as exp2(fl(x * log2 e)) (what the fast exp intrinsic computes, and where it loses
accuracy as |x| grows), sigmoid and tanh in the kernels' algebraic form.

Error measure: err(a, ref) = max |a - ref| / max |ref| of loss_optim_refs, taken slab by slab: per direction
and per gate block, in the teacher-forced checks also per timestep, so one wrong gate, direction or step is
not diluted by the rest.  Tolerance of a slab: TOL_FACTOR * e_ref, e_ref the yardstick's error against fp64
on the same inputs and the same slab.  Both errors share the slab's max |ref|, so the rule is the same
whether it is read relatively or absolutely.  No tolerance is taken from a kernel's output.
"""
import functools
import math

import numpy as np
import torch

from loss_optim_refs import PHILOX_SEEDS, SENSITIVITY, TOL_FACTOR, err, philox_uniform  # noqa: F401

F64, F32 = torch.float64, torch.float32
LOG2E = 1.4426950408889634
DROP_STREAM = 0x7a67      # the Philox stream id of the tagger's dropout (engine/tagger.py)


def bf16(x):
    """x rounded to nearest even onto bfloat16, in the dtype of x."""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


# ------------------------------------------------------------------------------------------- arithmetic
def _exp(x):
    return torch.exp(x) if x.dtype == F64 else torch.exp2(x * LOG2E)


def sigm(x):
    if x.dtype == F64:
        return torch.sigmoid(x)
    return 1.0 / (1.0 + _exp(-x))


def tanh(x):
    if x.dtype == F64:
        return torch.tanh(x)
    e = _exp(-2.0 * x.abs())
    t = (1.0 - e) / (1.0 + e)
    return torch.where(x < 0, -t, t)


def dot(a, w, init=None, order='mm'):
    """init + a [B, K] . w [N, K]^T.  order 'mm': the library's matmul, init added last.  'asc': init first,
    then one term after the other in ascending k (a zero term changes nothing, so zero padding is exact)."""
    if order == 'mm':
        r = a @ w.t()
        return r if init is None else init + r
    r = torch.zeros((a.shape[0], w.shape[0]), dtype=a.dtype) if init is None else init.clone()
    for k in range(a.shape[1]):
        r = r + a[:, k:k + 1] * w[None, :, k]
    return r


# ------------------------------------------------------------------------------------------- forward
FWD_WRONG = ('rev_forwards', 'no_carry', 'gate_order', 'dir0_weights')
BWD_WRONG = ('no_dc_carry', 'ct_for_cp', 'cp_first_nonzero', 'no_rec', 'w_untransposed', 'og_slope')


def fwd_step(gin_t, h_prev, c_prev, whh_d, wrong=None, order='mm'):
    """One cell step of one direction: gin_t [B, 4HP], h_prev / c_prev [B, HP], whh_d [4HP, HP] ->
    (activated gates [B, 4HP], c [B, HP], h [B, HP])."""
    HP = h_prev.shape[-1]
    a = dot(h_prev, whh_d, gin_t, order)
    ai, af, ag, ao = a.split(HP, -1)
    if wrong == 'gate_order':          # blocks read as i, f, o, g
        ag, ao = ao, ag
    i, f, g, o = sigm(ai), sigm(af), tanh(ag), sigm(ao)
    c = i * g if wrong == 'no_carry' else f * c_prev + i * g
    h = o * tanh(c)
    return torch.cat([i, f, g, o], -1), c, h


def fwd_run(gin, whh, dtype=F64, round_op=None, forced=None, wrong=None, order='mm'):
    """Both directions over the whole sequence (direction 1 walks t = T-1 .. 0) -> (hout, gsave, csave).
    round_op: applied to the recurrent operand h_{t-1} (bf16 for the bf16 kernels' model).
    forced = (hout_k, csave_k): teacher forcing, every step starts from round_op(hout_k) and csave_k of the
    step before it (zero at each direction's first step) instead of from this function's own state."""
    T, B, _, G4 = gin.shape
    HP = G4 // 4
    gin, whh = gin.to(dtype), whh.to(dtype)
    hout = torch.zeros((T, B, 2, HP), dtype=dtype)
    csave = torch.zeros((T, B, 2, HP), dtype=dtype)
    gsave = torch.zeros((T, B, 2, G4), dtype=dtype)
    for d in range(2):
        w = whh[0 if wrong == 'dir0_weights' else d]
        ts = list(range(T)) if d == 0 or wrong == 'rev_forwards' else list(range(T - 1, -1, -1))
        h = c = torch.zeros((B, HP), dtype=dtype)
        for s, t in enumerate(ts):
            if forced is not None and s > 0:
                h, c = forced[0][ts[s - 1], :, d].to(dtype), forced[1][ts[s - 1], :, d].to(dtype)
            hop = round_op(h) if round_op is not None else h
            g, c, h = fwd_step(gin[t, :, d], hop, c, w, wrong, order)
            hout[t, :, d], gsave[t, :, d], csave[t, :, d] = h, g, c
    return hout, gsave, csave


# ------------------------------------------------------------------------------------------- backward
def bwd_run(whh, dhout, gsave, csave, rec=None, dtype=F64, round_op=None, wrong=None, order='mm'):
    """BPTT from the saved gates and cell states -> dgin [T][B][2][4HP], the formulas of lstm.hip's header:
        dh = dhout_t + dgates_next . W_hh            dc_t = dc_carry + dh * o * (1 - tanh(c_t)^2)
        dao = dh * tanh(c_t) * o (1 - o)   dai = dc_t * g * i (1 - i)   dag = dc_t * i * (1 - g^2)
        daf = dc_t * c_{t-1} * f (1 - f)   dc_carry = dc_t * f
    with c_{t-1} = 0 at each direction's first forward step.  rec [T][B][2][4HP]: the recurrent operand of
    every step (the step that follows time t in BPTT order reads rec[t]) instead of this function's own dgates;
    round_op: applied to the own dgates when they are the operand."""
    T, B, _, G4 = gsave.shape
    HP = G4 // 4
    whh, dhout, gsave, csave = (x.to(dtype) for x in (whh, dhout, gsave, csave))
    dgin = torch.zeros((T, B, 2, G4), dtype=dtype)
    for d in range(2):
        w = whh[d]
        wt = (w.reshape(HP, G4) if wrong == 'w_untransposed' else w.t()).contiguous()      # [HP, 4HP]
        ts = list(range(T - 1, -1, -1)) if d == 0 else list(range(T))
        dc = torch.zeros((B, HP), dtype=dtype)
        dg = None
        for s, t in enumerate(ts):
            tp = t - 1 if d == 0 else t + 1          # the forward's previous step
            dh = dhout[t, :, d]
            if s > 0 and wrong != 'no_rec':
                if rec is not None:
                    opnd = rec[ts[s - 1], :, d].to(dtype)
                else:
                    opnd = round_op(dg) if round_op is not None else dg
                dh = dh + dot(opnd, wt, None, order)
            i, f, g, o = gsave[t, :, d].split(HP, -1)
            ct = csave[t, :, d]
            if 0 <= tp < T:
                cp = ct if wrong == 'ct_for_cp' else csave[tp, :, d]
            else:
                cp = ct if wrong == 'cp_first_nonzero' else torch.zeros_like(ct)
            th = tanh(ct)
            dct = dh * o * (1.0 - th * th)
            if wrong != 'no_dc_carry':
                dct = dc + dct
            dao = dh * th * (1.0 - th * th) if wrong == 'og_slope' else dh * th * o * (1.0 - o)
            dai = dct * g * i * (1.0 - i)
            dag = dct * i * (1.0 - g * g)
            daf = dct * cp * f * (1.0 - f)
            dc = dct * f
            dg = torch.cat([dai, daf, dag, dao], -1)
            dgin[t, :, d] = dg
    return dgin


# ------------------------------------------------------------------------------------------- slabs
def slabs(x, HP, per_t=False):
    """[(label, view)] of x [T][B][2][q * HP]: one slab per direction and gate block (and timestep)."""
    out = []
    for d in range(2):
        for q in range(x.shape[-1] // HP):
            v = x[:, :, d, q * HP:(q + 1) * HP]
            lab = 'd{}'.format(d) + ('' if x.shape[-1] == HP else ' gate ' + 'ifgo'[q])
            if per_t:
                out += [('{} t{}'.format(lab, t), v[t]) for t in range(x.shape[0])]
            else:
                out.append((lab, v))
    return out


def slab_ratios(got, yard, ref, HP, per_t=False):
    """[(label, kernel error, tolerance)] slab by slab: tolerance = TOL_FACTOR * err(yardstick, ref)."""
    out = []
    for (lab, g), (_, y), (_, r) in zip(slabs(got, HP, per_t), slabs(yard, HP, per_t), slabs(ref, HP, per_t)):
        out.append((lab, err(g, r), TOL_FACTOR * err(y, r)))
    return out


def ratio(e, tol):
    return 0.0 if e == 0.0 else (math.inf if tol == 0.0 else e / tol)


# ------------------------------------------------------------------------------------------- cases
LSTM_HP = (64, 128)
LSTM_TB = ((1, 1), (2, 16), (3, 17), (5, 33))
LSTM_FAMILIES = ('fp32', 'bf16')
EXTREME_TB = (3, 5)


@functools.lru_cache(maxsize=None)
def recurrence_case(HP, T, B, family, extreme=False):
    """fp32 gin, whh (bf16 values for the bf16 family), dhout of one case; every unit live, the two directions
    different.  extreme: +-30 and +-100 among the gin entries (the exp argument overflows there)."""
    gen = torch.Generator().manual_seed(1000 * HP + 10 * T + B + (7 if family == 'bf16' else 0) + (3 if extreme else 0))
    a = 2.0 / math.sqrt(HP)
    whh = (torch.rand((2, 4 * HP, HP), generator=gen) * 2 - 1) * a
    if family == 'bf16':
        whh = bf16(whh)
    gin = 1.5 * torch.randn((T, B, 2, 4 * HP), generator=gen)
    dhout = torch.randn((T, B, 2, HP), generator=gen)
    if extreme:
        flat = gin.view(-1)
        idx = torch.randperm(flat.numel(), generator=gen)[:flat.numel() // 8]
        vals = torch.tensor([30.0, -30.0, 100.0, -100.0])
        flat[idx] = vals[torch.arange(idx.numel()) % 4]
    return gin, whh, dhout


def recurrence_cases():
    out = [(HP, T, B, False) for HP in LSTM_HP for T, B in LSTM_TB]
    return out + [(HP,) + EXTREME_TB + (True,) for HP in LSTM_HP]


@functools.lru_cache(maxsize=None)
def saved_state(HP, T, B, family, extreme=False):
    """(gsave, csave) as fp32: the fp64 reference forward of the case (with the bf16 h operand for the bf16
    family), rounded.  The backward kernels are fed these, so their check does not depend on a forward kernel."""
    gin, whh, _ = recurrence_case(HP, T, B, family, extreme)
    _, gs, cs = fwd_run(gin, whh, F64, round_op=bf16 if family == 'bf16' else None)
    return gs.float(), cs.float()


# ------------------------------------------------------------------------------------------- whole BiLSTM
def lstm_params(lstm):
    """(w_ih [2, 4H, E], w_hh [2, 4H, H], b_ih [2, 4H], b_hh [2, 4H]) of a one-layer bidirectional nn.LSTM."""
    s = ('', '_reverse')
    return tuple(torch.stack([getattr(lstm, n + '_l0' + x).detach() for x in s])
                 for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh'))


PARAM_NAMES = ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0')


def pad_units(x, H, HP, axis_blocks):
    """Zero-pad each of the axis_blocks gate blocks of x's last axis from H to HP."""
    sh = x.shape[:-1]
    out = torch.zeros(sh + (axis_blocks, HP), dtype=x.dtype)
    out[..., :H] = x.reshape(sh + (axis_blocks, H))
    return out.reshape(sh + (axis_blocks * HP,))


def bilstm_ref(x, params, gy, dtype=F64, HP=None, round_op=None, order='mm'):
    """y [B, T, 2H] and the gradients of sum(y * gy) for x [B, T, E] through the functions above, every
    operation in dtype: dict y, dx, and the eight nn.LSTM parameter gradients by name.  HP: run in the
    kernels' padded layout (gate blocks and hidden units zero-padded to HP) and cut the result back."""
    w_ih, w_hh, b_ih, b_hh = (p.to(dtype) for p in params)
    x, gy = x.to(dtype), gy.to(dtype)
    B, T, E = x.shape
    H = w_hh.shape[-1]
    P = H if HP is None else HP
    w_ih_p = pad_units(w_ih.transpose(1, 2), H, P, 4).transpose(1, 2)                      # [2, 4P, E]
    w_hh_p = torch.zeros((2, 4 * P, P), dtype=dtype)
    w_hh_p[:, :, :H] = pad_units(w_hh.transpose(1, 2), H, P, 4).transpose(1, 2)
    xt = x.transpose(0, 1)                                                                 # [T, B, E]
    gin = pad_units(torch.einsum('tbe,dge->tbdg', xt, w_ih) + (b_ih + b_hh), H, P, 4)     # [T, B, 2, 4P]
    hout, gsave, csave = fwd_run(gin, w_hh_p, dtype, round_op=round_op, order=order)
    dh = torch.zeros((T, B, 2, P), dtype=dtype)
    dh[..., :H] = gy.transpose(0, 1).reshape(T, B, 2, H)
    dg = bwd_run(w_hh_p, dh, gsave, csave, dtype=dtype, round_op=round_op, order=order)
    hp = torch.zeros_like(hout)
    hp[1:, :, 0], hp[:-1, :, 1] = hout[:-1, :, 0], hout[1:, :, 1]
    dw_ih = torch.einsum('tbdg,tbe->dge', dg, xt).reshape(2, 4, P, E)[:, :, :H].reshape(2, 4 * H, E)
    dw_hh = torch.einsum('tbdg,tbdh->dgh', dg, hp).reshape(2, 4, P, P)[:, :, :H, :H].reshape(2, 4 * H, H)
    db = dg.sum((0, 1)).reshape(2, 4, P)[:, :, :H].reshape(2, 4 * H)
    out = dict(y=hout[..., :H].reshape(T, B, 2 * H).transpose(0, 1),
               dx=torch.einsum('tbdg,dge->tbe', dg, w_ih_p).transpose(0, 1), padded=(hout, gsave, csave, dg))
    for d, suf in enumerate(('', '_reverse')):
        out['weight_ih_l0' + suf], out['weight_hh_l0' + suf] = dw_ih[d], dw_hh[d]
        out['bias_ih_l0' + suf] = out['bias_hh_l0' + suf] = db[d]
    return out


def torch_lstm_ref(x, lstm, gy):
    """The same dict from fp64 nn.LSTM autograd (lstm: a float64 module)."""
    x = x.double().clone().requires_grad_(True)
    lstm.zero_grad()
    y = lstm(x)[0]
    (y * gy.double()).sum().backward()
    out = dict(y=y.detach(), dx=x.grad)
    out.update({k: p.grad for k, p in lstm.named_parameters()})
    return out


PADDED_H = (1, 63, 65, 127)
PADDED_T = (1, 3)
PADDED_E = (8, 6)        # 8: the in-tree GEMMs; 6: rows that are no multiple of 16 bytes, torch's addmm
PADDED_B = 3


@functools.lru_cache(maxsize=None)
def padded_case(H, T, E, B=PADDED_B):
    """(fp64 nn.LSTM, x [B, T, E], gy [B, T, 2H]); the weights are nn.LSTM's own U(-1/sqrt(H), 1/sqrt(H))."""
    torch.manual_seed(100 * H + 10 * T + E)
    lstm = torch.nn.LSTM(E, H, batch_first=True, bidirectional=True).double()
    with torch.no_grad():
        for p in lstm.parameters():          # fp32 values: what the GPU module will hold
            p.copy_(p.float().double())
    return lstm, torch.randn(B, T, E), torch.randn(B, T, 2 * H)


# ------------------------------------------------------------------------------------------- embedding
def clamp_ids(ids, V):
    ids = np.asarray(ids).astype(np.int64)
    return np.where((ids < 0) | (ids >= V), 0, ids)


def embed_ref(w, ids):
    """w[ids] with ids outside [0, V) reading row 0."""
    return w[torch.from_numpy(clamp_ids(ids, w.shape[0]))]


def dropout_mask_ref(n, EP, p, seed, step=None):
    """fp32 [n, EP]: 1 / (1 - p) where the uniform of element i (word i % 4 of Philox counter i / 4, stream
    DROP_STREAM, the step) is >= p, else 0, all in fp32."""
    p32 = np.float32(p)
    keep = np.float32(1.0) / (np.float32(1.0) - p32)
    u = philox_uniform(n * EP, seed, DROP_STREAM, step)
    return torch.from_numpy(np.where(u >= p32, keep, np.float32(0.0)).astype(np.float32).reshape(n, EP))


def embed_bwd_ref(ids, dy, V, mask=None, skip=None):
    """fp64 dW [V, E] = index_add of dy (* mask) by id; ids in skip contribute nothing."""
    g = dy.double() if mask is None else dy.double() * mask.double()
    ids = torch.as_tensor(np.asarray(ids).astype(np.int64))
    keep = torch.ones_like(ids, dtype=torch.bool) if skip is None else ids != skip
    return torch.zeros((V, dy.shape[1]), dtype=F64).index_add_(0, ids[keep], g[keep])


def embed_bwd_seq32(ids, dy, dw, mask=None, skip=None):
    """dw (fp32, changed in place and returned): each row some token touches becomes the fp32 sum of its
    tokens' dy (* mask) rows, added one by one in ascending token order from 0; other rows keep what they held."""
    dyn = dy.numpy() if mask is None else (dy.numpy() * mask.numpy()).astype(np.float32)
    out = dw.numpy()
    seen = set()
    for i, v in enumerate(np.asarray(ids).tolist()):
        if skip is not None and v == skip:
            continue
        if v not in seen:
            out[v] = 0.0
            seen.add(v)
        out[v] = out[v] + dyn[i]
    return dw


def pack_ref(x_bl, y_bl, padding_idx=0, vocab=None, ignore=-100):
    """engine.tagger.pack_batch by a plain loop: dict ids, labels, perm, uniq, starts, nruns, inv (fp32)."""
    B, L = len(x_bl), len(x_bl[0])
    ids, labels = [], []
    for t in range(L):
        for b in range(B):
            v = int(x_bl[b][t])
            if vocab is not None and not 0 <= v < vocab:
                v = padding_idx
            ids.append(v)
            labels.append(ignore if y_bl is None else int(y_bl[b][t]))
    perm = sorted(range(len(ids)), key=lambda i: ids[i])     # Python's sort is stable
    uniq, starts = [], []
    for k, i in enumerate(perm):
        if k == 0 or ids[i] != ids[perm[k - 1]]:
            uniq.append(-1 if ids[i] == padding_idx else ids[i])
            starts.append(k)
    starts.append(len(ids))
    cnt = sum(1 for v in labels if v != ignore)
    return dict(ids=ids, labels=labels, perm=perm, uniq=uniq, starts=starts, nruns=len(uniq),
                inv=np.float32(1.0 / max(1, cnt)))


def unpack(buf, n):
    """The fields of a pack_batch buffer of n tokens, cut to the run count."""
    U = int(buf[5 * n + 1])
    return dict(ids=buf[0:n].tolist(), labels=buf[n:2 * n].tolist(), perm=buf[2 * n:3 * n].tolist(),
                uniq=buf[3 * n:3 * n + U].tolist(), starts=buf[4 * n:4 * n + U + 1].tolist(), nruns=U,
                inv=buf[5 * n + 2:5 * n + 3].view(np.float32)[0],
                slack=np.concatenate([buf[3 * n + U:4 * n], buf[4 * n + U + 1:5 * n + 1]]))
