"""fp64 reference and fp32 yardstick of the GRU recurrence (csrc/kernels/gru.hip) in the kernels' own layouts, gate
blocks [r | z | n] of HP each; nothing here calls a kernel of this project.  float64 is the reference; float32 is the
yardstick, with lstm_refs' fast-exp sigmoid and tanh.  Error and tolerance: lstm_refs' rule, slab by slab.

    gin [T][B][2][3HP] (b_ih only)   whh [2][3HP][HP]   bhh [2][3HP]   hout, qsave, dhout [T][B][2][HP]
    gsave (activated r, z, n), dgin, dgh [T][B][2][3HP]
"""
import torch

from lstm_refs import F64, TOL_FACTOR, err, sigm, tanh


def fwd_run(gin, whh, bhh, dtype=F64):
    """Both directions over the whole sequence (direction 1 walks t = T-1 .. 0) -> (hout, gsave, qsave)."""
    T, B, _, G3 = gin.shape
    HP = G3 // 3
    gin, whh, bhh = gin.to(dtype), whh.to(dtype), bhh.to(dtype)
    hs, gs, qs = ([[None, None] for _ in range(T)] for _ in range(3))
    for d in range(2):
        h = torch.zeros((B, HP), dtype=dtype)
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            ar, az, an = gin[t, :, d].split(HP, -1)
            gr, gz, q = (h @ whh[d].t() + bhh[d]).split(HP, -1)
            r, z = sigm(ar + gr), sigm(az + gz)
            n = tanh(an + r * q)
            h = (1.0 - z) * n + z * h
            hs[t][d], gs[t][d], qs[t][d] = h, torch.cat([r, z, n], -1), q
    return tuple(torch.stack([torch.stack(x, 1) for x in v]) for v in (hs, gs, qs))


def bwd_run(whh, dhout, hout, gsave, qsave, dtype=F64):
    """BPTT from the saved forward -> (dgin, dgh), the formulas of gru.hip's header."""
    T, B, _, HP = hout.shape
    whh, dhout, hout, gsave, qsave = (x.to(dtype) for x in (whh, dhout, hout, gsave, qsave))
    dgin, dgh = torch.zeros_like(gsave), torch.zeros_like(gsave)
    for d in range(2):
        rec = torch.zeros((B, HP), dtype=dtype)
        for t in (range(T - 1, -1, -1) if d == 0 else range(T)):
            tp = t - 1 if d == 0 else t + 1          # the forward's previous step
            hp = hout[tp, :, d] if 0 <= tp < T else torch.zeros((B, HP), dtype=dtype)
            r, z, n = gsave[t, :, d].split(HP, -1)
            dh = dhout[t, :, d] + rec
            dan = dh * (1.0 - z) * (1.0 - n * n)
            daz = dh * (hp - n) * z * (1.0 - z)
            dar = dan * qsave[t, :, d] * r * (1.0 - r)
            dgin[t, :, d], dgh[t, :, d] = torch.cat([dar, daz, dan], -1), torch.cat([dar, daz, dan * r], -1)
            rec = dh * z + dgh[t, :, d] @ whh[d]
    return dgin, dgh


def slab_rows(got, yard, ref, HP):
    """[(label, kernel error, tolerance)] per direction and gate block: tolerance = TOL_FACTOR * err(yardstick, ref)."""
    return [('d{} {}'.format(d, 'rzn'[g] if got.shape[-1] > HP else 'h'), err(got[:, :, d, s], ref[:, :, d, s]),
             TOL_FACTOR * err(yard[:, :, d, s], ref[:, :, d, s]))
            for d in range(2) for g in range(got.shape[-1] // HP) for s in [slice(g * HP, (g + 1) * HP)]]
