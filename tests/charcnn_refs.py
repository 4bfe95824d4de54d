"""fp64 reference and fp32 yardstick of the character-CNN word features (csrc/kernels/charcnn.hip) in the kernels' own
padded layouts; nothing here calls a kernel of this project.  The formula is written out: gather, unfold of the three
taps, one matmul, masked max with the first-index rule (no conv1d).  dtype float64 is the reference, float32 the
yardstick; tolerance per output = TOL_FACTOR * err(yardstick, reference).

    chars uint8 [n][16]   cemb [CV][EcP]   wc [FP][3][EcP]   bc [FP]   xc, mask, dxc [n][FP]   amax int [n][FP]
"""
import functools

import torch

from lstm_refs import F64

C = 16
LENS = (0, 1, 2, 15, 16)


@functools.lru_cache(maxsize=None)
def case(n, Ec, F):
    """One case's fp32 inputs, padded (extents beyond Ec / F zero).  Tokens 0..4 have the lengths LENS; token 3 is one
    repeated character (exact ties), token 4 carries an id >= CV; n = 1 is the single word "aa"."""
    gen = torch.Generator().manual_seed(1000 * n + 10 * Ec + F)
    EcP, FP, CV = (16 if Ec <= 16 else 32), -(-F // 16) * 16, 40
    lens = torch.randint(1, C + 1, (n,), generator=gen)
    chars = torch.randint(2, CV, (n, C), generator=gen)
    if n == 1:
        lens[0], chars[0] = 2, 7
    else:
        lens[:5] = torch.tensor(LENS)
        chars[3] = 7
        chars[4, 1] = CV + 3
    chars = (chars * (torch.arange(C)[None] < lens[:, None])).to(torch.uint8)
    le, lf = (torch.arange(EcP) < Ec).float(), (torch.arange(FP) < F).float()
    cemb = torch.randn((CV, EcP), generator=gen) * le
    cemb[0] = 0
    wc = torch.randn((FP, 3, EcP), generator=gen) / (3 * Ec) ** 0.5 * le * lf[:, None, None]
    bc = torch.randn(FP, generator=gen) * lf
    dxc = torch.randn((n, FP), generator=gen) * lf
    mask = (torch.rand((n, FP), generator=gen) >= 0.3).float() / 0.7
    return dict(n=n, Ec=Ec, F=F, EcP=EcP, FP=FP, CV=CV, chars=chars, cemb=cemb, wc=wc, bc=bc, dxc=dxc, mask=mask,
                ties=[0] if n == 1 else [3])


def _window(chars, cemb, dtype):
    """Xp [n][18][EcP] (rows 0 and 17 the zero padding), live [n][16], the clamped ids, len [n]."""
    ids = chars.long()
    n = (ids != 0).sum(1)
    live = (torch.arange(C)[None] < n[:, None]) & (ids < cemb.shape[0])
    idc = torch.where(live, ids, torch.zeros_like(ids))
    x = cemb.to(dtype)[idc] * live[..., None].to(dtype)
    return torch.nn.functional.pad(x, (0, 0, 1, 1)), live, idc, n


def fwd(chars, cemb, wc, bc, dtype=F64):
    """(feat [n][FP], amax [n][FP] (-1 for an empty token), conv [n][16][FP] with -inf from the word's length on)."""
    xp, _, _, n = _window(chars, cemb, dtype)
    unf = torch.cat([xp[:, k:k + C] for k in range(3)], -1)                       # [n][16][3 EcP], tap-major
    conv = unf @ wc.to(dtype).reshape(wc.shape[0], -1).t()
    conv = conv.masked_fill((torch.arange(C)[None] >= n[:, None])[..., None], float('-inf'))
    top = conv.max(1, keepdim=True).values
    amax = torch.where(conv == top, torch.arange(C)[None, :, None], C).min(1).values   # the first position
    some = (n > 0)[:, None]
    feat = torch.where(some, top[:, 0] + bc.to(dtype), torch.zeros((), dtype=dtype))
    return feat, torch.where(some, amax, -1), conv


def bwd(chars, cemb, wc, g, amax, dtype=F64):
    """(dwc, dbc, dcemb) of g = dxc * mask [n][FP] at the winning positions amax."""
    xp, live, idc, _ = _window(chars, cemb, dtype)
    wc = wc.to(dtype)
    g = g.to(dtype) * (amax >= 0)
    a = amax.clamp_min(0)
    dxp = torch.zeros_like(xp)
    dwc = torch.zeros_like(wc)
    for k in range(3):
        rows = (a + k)[..., None].expand(-1, -1, xp.shape[-1])                    # window row of X[amax + k - 1]
        dwc[:, k] = torch.einsum('nf,nfe->fe', g, xp.gather(1, rows))
        dxp.scatter_add_(1, rows, g[..., None] * wc[None, :, k])
    dx = dxp[:, 1:C + 1] * live[..., None].to(dtype)
    dcemb = torch.zeros(cemb.shape, dtype=dtype).index_add_(0, idc.reshape(-1), dx.reshape(-1, dx.shape[-1]))
    return dwc, g.sum(0), dcemb
