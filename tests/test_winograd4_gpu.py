"""Fused Winograd F(4x4,3x3) fp32 conv (csrc/kernels/winograd4.hip) vs fp64 PyTorch references.

F(4x4,3x3)'s transforms have coefficients up to 8 (A^T) and 5 (B^T), so its fp32 round-off is about
ten times F(2x2)'s (profiles/winograd_error_r2.jsonl); the gate is 3e-5 relative Frobenius error,
against ~1e-6 measured."""
import math

import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TOL = 3e-5
# 0 / 1: 8- / 4-wave tiles; 2: 4-wave two-stage (not a tuner candidate, kept exercised); 3 / 4: 0 / 1 on the
# blocked weight sets (wino4b_u); 5: warp-specialised two-stage kernel on the blocked sets
VARIANTS = [0, 1, 2, 3, 4, 5]


def _u4(S, w2, variant, dgrad=False):
    if variant >= 3:
        return S.wino4b_u(w2, dgrad=dgrad)
    return S.wino4_ut(w2) if dgrad else S.wino4_u(w2)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def _conv_ref(x_nhwc, w_ohwi):
    return TF.conv2d(x_nhwc.double().permute(0, 3, 1, 2), w_ohwi.double().permute(0, 3, 1, 2),
                     padding=1).permute(0, 2, 3, 1)


def _w2(w):
    return w.to(DEV).reshape(w.shape[0], -1).contiguous()


@pytest.mark.parametrize("N,H,W,Cin,Cout", [
    (2, 8, 8, 16, 32), (3, 4, 12, 24, 40), (4, 32, 32, 64, 64), (8, 4, 4, 512, 512), (2, 4, 4, 8, 72),
    (5, 16, 16, 128, 128), (1, 12, 20, 8, 8), (3, 8, 8, 256, 96)])
@pytest.mark.parametrize("variant", VARIANTS)
def test_wino4_fwd_and_stats(N, H, W, Cin, Cout, variant):
    from rafiki_amd.ops import f32 as S
    x = _rand(N, H, W, Cin, seed=1)
    w = _rand(Cout, 3, 3, Cin, seed=2, scale=1.0 / math.sqrt(9 * Cin))
    u = _u4(S, _w2(w), variant)
    acc = torch.zeros((S.bn_slots(Cout), 2, Cout), dtype=torch.float64, device=DEV)
    y = S.wino4_conv(x.to(DEV), u, stats=acc, variant=variant, n_out=Cout)
    torch.cuda.synchronize()
    ref = _conv_ref(x, w)
    assert rel(y, ref) < TOL
    s = acc.sum(0).cpu()
    r = ref.reshape(-1, Cout)
    assert rel(s[0], r.sum(0)) < TOL and rel(s[1], (r * r).sum(0)) < TOL


@pytest.mark.parametrize("variant", [0, 4])
def test_wino4_bias_relu(variant):
    from rafiki_amd.ops import f32 as S
    x = _rand(3, 8, 8, 32, seed=3)
    w = _rand(48, 3, 3, 32, seed=4, scale=0.1)
    b = _rand(48, seed=5)
    y = S.wino4_conv(x.to(DEV), _u4(S, _w2(w), variant), bias=b.to(DEV), relu=True, variant=variant, n_out=48)
    torch.cuda.synchronize()
    assert rel(y, torch.relu(_conv_ref(x, w) + b.double())) < TOL
    # bias without ReLU (the runtime-flag instantiation: no-BN blocks followed by a max-pool)
    y = S.wino4_conv(x.to(DEV), _u4(S, _w2(w), variant), bias=b.to(DEV), variant=variant, n_out=48)
    torch.cuda.synchronize()
    assert rel(y, _conv_ref(x, w) + b.double()) < TOL


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(4, 8, 8, 64, 128), (2, 16, 16, 64, 64), (8, 4, 4, 512, 256),
                                            (2, 4, 8, 24, 16)])
@pytest.mark.parametrize("variant", VARIANTS)
def test_wino4_dgrad_from_flipped_set(N, H, W, Cin, Cout, variant):
    """dx = conv(dy, flip(w)^T) from the ut set."""
    from rafiki_amd.ops import f32 as S
    x = _rand(N, H, W, Cin, seed=6)
    w = _rand(Cout, 3, 3, Cin, seed=7, scale=0.1)
    dy = _rand(N, H, W, Cout, seed=8)
    dx = S.wino4_conv(dy.to(DEV), _u4(S, _w2(w), variant, dgrad=True), variant=variant, n_out=Cin)
    torch.cuda.synchronize()
    xd = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    out = TF.conv2d(xd, w.double().permute(0, 3, 1, 2), padding=1)
    (gx,) = torch.autograd.grad(out, xd, dy.double().permute(0, 3, 1, 2))
    assert rel(dx, gx.permute(0, 2, 3, 1)) < TOL


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("H", [8, 4])
def test_wino4_dgrad_bn_epilogues_match_direct(pool, variant, H):
    """The BNB / BNP epilogues give the same dx and BN-backward sums as the direct kernel's."""
    from rafiki_amd.ops import f32 as S
    N, W, Cin, Cout = 4, H, 64, 128
    Hy, Wy = (2 * H, 2 * W) if pool else (H, W)
    y = _rand(N, Hy, Wy, Cin, seed=17) + 0.2
    gamma, beta = torch.ones(Cin) * 1.3, _rand(Cin, seed=18) * 0.1
    acc = torch.zeros((S.bn_slots(Cin), 2, Cin), dtype=torch.float64, device=DEV)
    S.col_stats(y.to(DEV).view(-1, Cin), acc)
    _, coeffs = S.bn_fwd(y.to(DEV), acc, N * Hy * Wy, gamma.to(DEV), beta.to(DEV), 1e-5, pool=pool, act=1)
    w = _rand(Cout, 3, 3, Cin, seed=19, scale=0.05)
    arena = w.reshape(-1).to(DEV).contiguous()
    wt = S.SConvWT(arena, [arena.view(Cout, 3, 3, Cin)])
    wt.refresh()
    ut = _u4(S, _w2(w), variant, dgrad=True)
    dyo = _rand(N, H, W, Cout, seed=20).to(DEV)
    acc_w, acc_d = torch.zeros_like(acc), torch.zeros_like(acc)
    key = 'bnp' if pool else 'bnb'
    d_w = S.wino4_conv(dyo, ut, variant=variant, n_out=Cin, **{key: (y.to(DEV), coeffs, acc_w)})
    d_d = S.conv_dgrad(dyo, wt.view(0), **{key: (y.to(DEV), coeffs, acc_d)})
    torch.cuda.synchronize()
    assert rel(d_w, d_d) < TOL
    assert rel(acc_w.sum(0), acc_d.sum(0)) < TOL


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_wino4_conv_grouped(shared, variant):
    """k convs in one grid (the serving ensemble's layers) == k separate convs."""
    from rafiki_amd.ops import f32 as S
    G, Nb, H, Cin, Cout = 3, 5, 8, 32, 48
    x = (_rand(Nb, H, H, Cin, seed=40) if shared else _rand(G, Nb, H, H, Cin, seed=40)).to(DEV)
    w = [_rand(Cout, 3, 3, Cin, seed=41 + g, scale=0.1) for g in range(G)]
    u = torch.stack([S.wino4_u(_w2(wg)) for wg in w]).contiguous()
    b = _rand(G, Cout, seed=45).to(DEV)
    y = S.wino4_conv_grp(x, u, bias=b, relu=True, variant=variant)
    torch.cuda.synchronize()
    for g in range(G):
        xg = x if shared else x[g]
        ref = torch.relu(_conv_ref(xg.cpu(), w[g]) + b[g].double().cpu())
        assert rel(y[g], ref) < TOL


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(4, 8, 8, 64, 128), (2, 32, 32, 64, 64), (16, 4, 4, 256, 512),
                                            (3, 4, 12, 24, 40), (2, 4, 4, 16, 16)])
@pytest.mark.parametrize("splits", [1, 2, 5])
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_wino4_wgrad(N, H, W, Cin, Cout, splits, variant):
    from rafiki_amd.ops import f32 as S
    x = _rand(N, H, W, Cin, seed=30)
    dy = _rand(N, H, W, Cout, seed=31)
    nt = N * (H // 4) * (W // 4)
    tps = -(-(-(-nt // splits)) // 8) * 8
    s_eff = -(-nt // tps)
    dw = torch.empty(Cout, 9 * Cin, device=DEV)
    S.wino4_wgrad(dy.to(DEV), x.to(DEV), dw, splits=s_eff, variant=variant)
    prev = _rand(Cout, 9 * Cin, seed=32).to(DEV)
    acc = prev.clone()
    S.wino4_wgrad(dy.to(DEV), x.to(DEV), acc, splits=s_eff, accumulate=True, variant=variant)
    torch.cuda.synchronize()
    wd = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    out = TF.conv2d(x.double().permute(0, 3, 1, 2), wd, padding=1)
    (gw,) = torch.autograd.grad(out, wd, dy.double().permute(0, 3, 1, 2))
    ref = gw.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin)
    assert rel(dw, ref) < TOL
    assert rel(acc, ref + prev.double().cpu()) < TOL


def test_wino_weights_live_sets_and_on_demand_transform():
    """WinoWeights narrows its per-step refresh to the sets the convs used; a set outside the live
    group is transformed on demand, so every lazy() read sees the current weights."""
    from rafiki_amd.ops import f32 as S
    shapes = [(64, 32), (16, 64), (40, 24)]
    arena = torch.zeros(sum(co * 9 * ci for co, ci in shapes) + 5, device=DEV)
    ws, off = [], 5
    for k, (co, ci) in enumerate(shapes):
        w = arena[off:off + co * 9 * ci].view(co, 9 * ci)
        w.copy_(_rand(co, 9 * ci, seed=50 + k).to(DEV))
        ws.append(w)
        off += co * 9 * ci
    ww = S.WinoWeights(arena, ws, hw=[8, 6, 4])
    assert not ww.has('u4', 1) and ww.has('ut4', 2)
    ww.refresh()
    for l, w in enumerate(ws):
        assert torch.equal(ww.lazy('u2', l)(), S.wino_u(w))
        assert torch.equal(ww.lazy('ut2', l)(), S.wino_ut(w))
        if ww.has('u4', l):
            assert torch.equal(ww.lazy('u4', l)(), S.wino4_u(w))
            assert torch.equal(ww.lazy('ut4', l)(), S.wino4_ut(w))
    ww.end_step()
    # a step that only uses layer 0's F(4x4) forward set and layer 2's F(2x2) gradient set
    ww.refresh()
    ww.lazy('u4', 0)()
    ww.lazy('ut2', 2)()
    ww.end_step()
    assert ww.live == frozenset({('u4', 0), ('ut2', 2)})
    for w in ws:
        w.mul_(-0.5).add_(0.25)
    ww.refresh()
    torch.cuda.synchronize()
    assert torch.equal(ww.u4(0), S.wino4_u(ws[0]))
    assert torch.equal(ww.ut(2), S.wino_ut(ws[2]))
    assert not torch.equal(ww.u(1), S.wino_u(ws[1]))          # not live: stale until asked for
    assert torch.equal(ww.lazy('u2', 1)(), S.wino_u(ws[1]))   # on-demand transform
    assert torch.equal(ww.lazy('ut4', 2)(), S.wino4_ut(ws[2]))


def test_wino_weights_every_kind_matches_its_producer_and_blocked_sets_are_permutations():
    """Every kind of set a layer has (planes and blocked sets included) comes out of the one-launch refresh,
    and out of the on-demand transform of a set that is not live, bit-equal to the stand-alone producer's;
    a blocked set is its plain set permuted by w4b_index (winograd4.hip), zero in the rows padded up to 32.
    (40, 24) @ 4 has partial 32-blocks both ways and padded rows in both blocked sets."""
    from rafiki_amd.ops import f32 as S
    producers = {'u2': S.wino_u, 'ut2': S.wino_ut, 'u4': S.wino4_u, 'ut4': S.wino4_ut, 'u4p': S.wino4_u4p,
                 'ut4p': lambda w: S.wino4_u4p(w, dgrad=True), 'u4b': S.wino4b_u,
                 'ut4b': lambda w: S.wino4b_u(w, dgrad=True)}
    shapes = [(64, 32), (16, 64), (40, 24)]
    arena = torch.zeros(sum(co * 9 * ci for co, ci in shapes) + 5, device=DEV)
    ws, off = [], 5
    for k, (co, ci) in enumerate(shapes):
        w = arena[off:off + co * 9 * ci].view(co, 9 * ci)
        w.copy_(_rand(co, 9 * ci, seed=70 + k).to(DEV))
        ws.append(w)
        off += co * 9 * ci
    ww = S.WinoWeights(arena, ws, hw=[8, 6, 4])
    have = sorted(ww.live)
    assert {k for k, l in have if l == 0} == set(producers) and {k for k, l in have if l == 1} == {'u2', 'ut2'}
    assert {k for k, l in have if l == 2} == {'u2', 'ut2', 'u4', 'ut4', 'u4b', 'ut4b'}
    ww.refresh()
    for kind, l in have:
        assert torch.equal(ww._view(kind, l), producers[kind](ws[l])), (kind, l)

    def blocked_index(rows, cols):
        pos, r, c = torch.meshgrid(torch.arange(36), torch.arange(rows), torch.arange(cols), indexing='ij')
        return ((((r >> 5) * (cols >> 3) + (c >> 3)) * 36 + pos) * 32 + (r & 31)) * 8 + ((c & 7) ^ ((((r & 31) >> 2) & 3) << 1))
    for (plain, blocked), l in [(kk, l) for kk in (('u4', 'u4b'), ('ut4', 'ut4b')) for l in (0, 2)]:
        u, ub = ww._view(plain, l).cpu(), ww._view(blocked, l).cpu()
        _, rows, cols = u.shape
        assert (rows, cols) == (shapes[l] if plain == 'u4' else shapes[l][::-1])
        idx = blocked_index(rows, cols).reshape(-1)
        assert ub.shape == (S.wino4b_numel(rows, cols),) and idx.unique().numel() == idx.numel()
        assert torch.equal(ub[idx], u.reshape(-1)), (blocked, l)
        rest = torch.ones(ub.numel(), dtype=torch.bool)
        rest[idx] = False
        assert int(rest.sum()) == 36 * (-rows % 32) * cols and not ub[rest].any(), (blocked, l)
    # narrow to two sets, change the weights: a set outside the live group is transformed on demand
    ww.end_step()
    ww.refresh()
    ww.lazy('u4', 0)()
    ww.lazy('ut2', 2)()
    ww.end_step()
    assert ww.live == frozenset({('u4', 0), ('ut2', 2)})
    for w in ws:
        w.mul_(-0.5).add_(0.25)
    ww.refresh()
    assert torch.equal(ww.lazy('u4p', 0)(), S.wino4_u4p(ws[0]))
    assert torch.equal(ww.lazy('ut4b', 2)(), S.wino4b_u(ws[2], dgrad=True))


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(16, 8, 8, 64, 128), (32, 4, 4, 256, 128), (8, 16, 16, 32, 64),
                                            (64, 4, 4, 40, 36)])   # (16x16 works too; the tuner skips it)
@pytest.mark.parametrize("tile", [0, 3, 16, 19])   # 16, 19: the X6 K loop
def test_wino4_wgrad_pretransformed(N, H, W, Cin, Cout, tile):
    """Pre-transformed F(4x4) weight gradient (transform launch + 36-split sgemm + output transform)."""
    from rafiki_amd.ops import f32 as S
    x = _rand(N, H, W, Cin, seed=40)
    dy = _rand(N, H, W, Cout, seed=41)
    dw = torch.empty(Cout, 9 * Cin, device=DEV)
    S.wino4_wgrad_pt(dy.to(DEV), x.to(DEV), dw, tile=tile)
    prev = _rand(Cout, 9 * Cin, seed=42).to(DEV)
    acc = prev.clone()
    S.wino4_wgrad_pt(dy.to(DEV), x.to(DEV), acc, accumulate=True, tile=tile)
    torch.cuda.synchronize()
    wd = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    out = TF.conv2d(x.double().permute(0, 3, 1, 2), wd, padding=1)
    (gw,) = torch.autograd.grad(out, wd, dy.double().permute(0, 3, 1, 2))
    ref = gw.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin)
    assert rel(dw, ref) < TOL
    assert rel(acc, ref + prev.double().cpu()) < TOL


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(8, 4, 4, 512, 512), (3, 8, 8, 256, 96), (16, 8, 8, 64, 128),
                                            (5, 4, 8, 40, 36)])
@pytest.mark.parametrize("tile", [0, 3, 16, 19])   # 16, 19: the X6 K loop
def test_wino4_conv_pretransformed_fwd_stats_bias_relu(N, H, W, Cin, Cout, tile):
    """Pre-transformed F(4x4) conv (input transform + 36-group sgemm + output transform) vs fp64."""
    from rafiki_amd.ops import f32 as S
    x = _rand(N, H, W, Cin, seed=50)
    w = _rand(Cout, 3, 3, Cin, seed=51, scale=1.0 / math.sqrt(9 * Cin))
    u = S.wino4_u(_w2(w))
    acc = torch.zeros((S.bn_slots(Cout), 2, Cout), dtype=torch.float64, device=DEV)
    y = S.wino4_conv_pt(x.to(DEV), u, stats=acc, tile=tile)
    b = _rand(Cout, seed=52)
    yb = S.wino4_conv_pt(x.to(DEV), u, bias=b.to(DEV), relu=True, tile=tile)
    torch.cuda.synchronize()
    ref = _conv_ref(x, w)
    assert rel(y, ref) < TOL
    s = acc.sum(0).cpu()
    r = ref.reshape(-1, Cout)
    assert rel(s[0], r.sum(0)) < TOL and rel(s[1], (r * r).sum(0)) < TOL
    assert rel(yb, torch.relu(ref + b.double())) < TOL


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("H", [8, 4])
def test_wino4_conv_pretransformed_bn_epilogues(pool, H):
    """BNB / BNP data-gradient epilogues of the pre-transformed conv == the fused kernel's."""
    from rafiki_amd.ops import f32 as S
    N, W, Cin, Cout = 4, H, 64, 128
    Hy, Wy = (2 * H, 2 * W) if pool else (H, W)
    y = _rand(N, Hy, Wy, Cin, seed=57) + 0.2
    gamma, beta = torch.ones(Cin) * 1.3, _rand(Cin, seed=58) * 0.1
    acc = torch.zeros((S.bn_slots(Cin), 2, Cin), dtype=torch.float64, device=DEV)
    S.col_stats(y.to(DEV).view(-1, Cin), acc)
    _, coeffs = S.bn_fwd(y.to(DEV), acc, N * Hy * Wy, gamma.to(DEV), beta.to(DEV), 1e-5, pool=pool, act=1)
    w = _rand(Cout, 3, 3, Cin, seed=59, scale=0.05)
    ut = S.wino4_ut(_w2(w))
    dyo = _rand(N, H, W, Cout, seed=60).to(DEV)
    acc_f, acc_p = torch.zeros_like(acc), torch.zeros_like(acc)
    key = 'bnp' if pool else 'bnb'
    d_f = S.wino4_conv(dyo, ut, **{key: (y.to(DEV), coeffs, acc_f)})
    d_p = S.wino4_conv_pt(dyo, ut, **{key: (y.to(DEV), coeffs, acc_p)})
    torch.cuda.synchronize()
    assert rel(d_p, d_f) < TOL
    assert rel(acc_p.sum(0), acc_f.sum(0)) < TOL


# ------------------------------------------------------------------------- what the launchers refuse
# The entry points called directly, on valid tiny tensors (Nb = 1, H = W = 4, C = 8, N = 32 unless the case says
# otherwise): every refused call returns its status (-1 RK_EBADARG, -2 RK_EUNSUPPORTED) before any launch.
def _pro_vec(C):
    """Identity normalise-on-load coefficients: scale [C] = 1, shift [C] = 0."""
    return torch.cat([torch.ones(C), torch.zeros(C)]).to(DEV)


def _fwd_call(S, name, *, H=4, C=8, N=32, flags=0, variant=0, groups=1, bias=False, stats=False, pro=False):
    """(arguments, outputs, the other tensors behind the arguments) of rk_wino4_conv_grp / rk_wino2s_conv_grp:
    ``groups`` convs, each with its own x, u (sized as the blocked set, the largest form), y and bias."""
    Nb, W = 1, 4
    x = _rand(groups, Nb, H, W, C, seed=70).abs().to(DEV)
    u = _rand(groups, S.wino4b_numel(N, C), seed=71, scale=0.1).to(DEV)
    y = torch.zeros(groups, Nb, H, W, N, device=DEV)
    b = _rand(groups, N, seed=72).to(DEV) if bias else None
    acc = torch.zeros((S.bn_slots(N), 2, N), dtype=torch.float64, device=DEV) if stats else None
    p = _pro_vec(C) if pro else None
    args = [S._p(x), S._p(u), S._p(y), S._p(b), S._p(acc), S._slots_flags(acc), None, Nb, H, W, C, N, flags, variant,
            groups, x[0].numel(), u[0].numel(), y[0].numel(), N if bias else 0]
    if name == 'rk_wino4_conv_grp':
        args.append(S._p(p))
    return args + [S._s()], [y], (x, u, b, acc, p)


def _wgrad_call(S, *, splits=1, accumulate=0, variant=0, xpro=False):
    Nb, H, W, Co, Ci = 2, 4, 4, 16, 16   # two tiles
    dy, x = _rand(Nb, H, W, Co, seed=73).to(DEV), _rand(Nb, H, W, Ci, seed=74).abs().to(DEV)
    out = torch.zeros(splits, Co, 9 * Ci, device=DEV)
    p = _pro_vec(Ci) if xpro else None
    return [S._p(dy), S._p(x), S._p(out), Nb, H, W, Co, Ci, splits, accumulate, variant, S._p(p), S._s()], \
        [out], (dy, x, p)


def _pt_transform_call(S, *, Co=8, Ci=8, xpro=False):
    dy, x = _rand(1, 4, 4, Co, seed=75).to(DEV), _rand(1, 4, 4, Ci, seed=76).abs().to(DEV)
    m, v = torch.zeros(36, 1, Co, device=DEV), torch.zeros(36, 1, Ci, device=DEV)
    p = _pro_vec(Ci) if xpro else None
    return [S._p(dy), S._p(x), S._p(m), S._p(v), 1, 4, 4, Co, Ci, S._p(p), S._s()], [m, v], (dy, x, p)


def _pt_input_call(S, *, C=8, planes=False, pro=False):
    """rk_wino4_pt_input (v [36][T][C] fp32) / rk_x6p_w4_input (``planes``: v [36][3][T][C] bf16), T = 1."""
    x = _rand(1, 4, 4, C, seed=77).abs().to(DEV)
    v = torch.zeros(36, 3, 1, C, dtype=torch.bfloat16, device=DEV) if planes else torch.zeros(36, 1, C, device=DEV)
    p = _pro_vec(C) if pro else None
    return [S._p(x), S._p(v), 1, 4, 4, C, S._p(p), S._s()], [v], (x, p)


_W4, _W2S = 'rk_wino4_conv_grp', 'rk_wino2s_conv_grp'
_REFUSALS = {
    'conv4 H = 6': (-1, lambda S: (_W4, _fwd_call(S, _W4, H=6))),
    'conv4 WF_STATS, null stats': (-1, lambda S: (_W4, _fwd_call(S, _W4, flags=S.WF_STATS))),
    'conv4 WF_BIAS, null bias': (-1, lambda S: (_W4, _fwd_call(S, _W4, flags=S.WF_BIAS))),
    'conv4 groups = 2, WF_STATS': (-2, lambda S: (_W4, _fwd_call(S, _W4, groups=2, flags=S.WF_STATS, stats=True))),
    'conv4 variant 6': (-1, lambda S: (_W4, _fwd_call(S, _W4, variant=6))),
    'conv4 WF_POOL alone': (-2, lambda S: (_W4, _fwd_call(S, _W4, flags=S.WF_POOL))),
    'conv4 pro, variant 0': (-2, lambda S: (_W4, _fwd_call(S, _W4, pro=True))),
    'conv4 pro, bias + relu': (-2, lambda S: (_W4, _fwd_call(S, _W4, pro=True, variant=3, bias=True,
                                                             flags=S.WF_BIAS | S.WF_RELU))),
    'conv4 pro, C = 520': (-2, lambda S: (_W4, _fwd_call(S, _W4, pro=True, variant=3, C=520))),
    'conv4 pro, groups = 2': (-2, lambda S: (_W4, _fwd_call(S, _W4, pro=True, variant=3, groups=2))),
    'conv2s variant 4': (-1, lambda S: (_W2S, _fwd_call(S, _W2S, variant=4))),
    'wgrad splits = 2, accumulate': (-1, lambda S: ('rk_wino4_wgrad', _wgrad_call(S, splits=2, accumulate=1))),
    # 2 tiles in chunks of 8 per split: one split holds both, the second is empty
    'wgrad empty split': (-1, lambda S: ('rk_wino4_wgrad', _wgrad_call(S, splits=2))),
    'wgrad xpro, variant 2': (-2, lambda S: ('rk_wino4_wgrad', _wgrad_call(S, variant=2, xpro=True))),
    'pt_transform Co = 6': (-2, lambda S: ('rk_wino4_pt_transform', _pt_transform_call(S, Co=6))),
    'pt_input C = 6': (-2, lambda S: ('rk_wino4_pt_input', _pt_input_call(S, C=6))),
    'x6p_w4_input C = 6': (-2, lambda S: ('rk_x6p_w4_input', _pt_input_call(S, C=6, planes=True))),
}


@pytest.mark.parametrize("case", list(_REFUSALS))
def test_wino4_launchers_refuse(case):
    from rafiki_amd.ops import _lib
    from rafiki_amd.ops import f32 as S
    status, build = _REFUSALS[case]
    name, (args, _outs, _keep) = build(S)
    with pytest.raises(_lib.KernelError, match=r'{} failed with status {}$'.format(name, status)):
        _lib.call(name, *args)


_ACCEPTS = {
    'rk_wino4_conv_grp': lambda S, pro: _fwd_call(S, _W4, variant=3, pro=pro),
    'rk_wino4_wgrad': lambda S, pro: _wgrad_call(S, xpro=pro),
    'rk_wino4_pt_transform': lambda S, pro: _pt_transform_call(S, xpro=pro),
    'rk_wino4_pt_input': lambda S, pro: _pt_input_call(S, pro=pro),
    'rk_x6p_w4_input': lambda S, pro: _pt_input_call(S, planes=True, pro=pro),
}


@pytest.mark.parametrize("name", list(_ACCEPTS))
def test_wino4_merged_entry_points_take_pro_or_null(name):
    """Each merged entry point runs with pro = NULL and with pro given.  x >= 0 and pro is the identity (scale 1,
    shift 0), so relu(x * 1 + 0) == x exactly and both calls compute the same thing: the transforms (one
    kernel, pro a run-time pointer) to the bit, the conv and the weight gradient within this file's gate."""
    from rafiki_amd.ops import _lib
    from rafiki_amd.ops import f32 as S
    outs = []
    for pro in (False, True):
        args, written, _keep = _ACCEPTS[name](S, pro)
        _lib.call(name, *args)
        torch.cuda.synchronize()
        outs.append([t.float() for t in written])
    for a, b in zip(*outs):
        assert b.abs().sum().item() > 0
        if name in ('rk_wino4_conv_grp', 'rk_wino4_wgrad'):
            assert rel(a, b) < TOL
        else:
            assert torch.equal(a, b)
