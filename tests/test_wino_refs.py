"""The references of tests/wino_refs.py are anchored (they are the convolution), their tolerances are bounds, the
exact sets stay below 2^24, and the judge of tests/test_wino_fused_gpu.py bites: wrong kernels written as mutants of
the reference are rejected on every sweep shape they apply to.  The weight-gradient kernels' fp32-reciprocal tile
decode is checked in full.  CPU only."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import sgemm_refs as G
import wino_refs as R

F64, F32 = torch.float64, torch.float32
MOS = (2, 4)
CASES = [(MO, s) for MO in MOS for s in R.shapes(MO)]
IDS = lambda v: '-'.join(map(str, v)) if isinstance(v, tuple) else str(v)   # noqa: E731


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _rand(seed, shape, scale=1.0):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed), dtype=F64) * scale


def _rejected(*a, **kw):
    try:
        R.judge('mutant', *a, **kw)
    except AssertionError:
        return True
    return False


def _rejected_sums(*a):
    try:
        R.judge_sums('mutant', *a)
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------- anchor
@pytest.mark.parametrize('MO,shape', CASES, ids=IDS)
def test_references_are_the_convolution(MO, shape):
    """fused_conv on G g G^T, its data-gradient form and fused_wgrad (1, 2 and 4 splits summed) against fp64
    conv2d / autograd."""
    Nb, H, W, C, N = shape
    x, w, dy = _rand(1, (Nb, H, W, C)), _rand(2, (N, 9, C), (9 * C) ** -0.5), _rand(3, (Nb, H, W, N))
    xd = _nchw(x).clone().requires_grad_(True)
    wd = w.reshape(N, 3, 3, C).permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = TF.conv2d(xd, wd, padding=1)
    gx, gw = torch.autograd.grad(y, (xd, wd), _nchw(dy))
    got = R.fused_conv(x, R.transform_weights(w, MO), MO)
    assert (got - y.detach().permute(0, 2, 3, 1)).abs().max() < 1e-12
    got = R.fused_conv(dy, R.transform_weights(w, MO, dgrad=True), MO)
    assert (got - gx.permute(0, 2, 3, 1)).abs().max() < 1e-12
    ref = gw.permute(0, 2, 3, 1).reshape(N, 9, C)
    for splits in (1, 2, 4):
        if R.wgrad_splits(Nb * (H // MO) * (W // MO), splits) is None:
            continue
        slabs, tiles = R.fused_wgrad(dy, x, MO, splits)
        assert len(tiles) == splits and sum(tiles) == Nb * (H // MO) * (W // MO)
        assert (slabs.sum(0) - ref).abs().max() < 1e-12 * Nb * H * W


@pytest.mark.parametrize('MO,shape', CASES, ids=IDS)
def test_normalise_on_load_reference(MO, shape):
    Nb, H, W, C, N = shape
    x, w = _rand(4, (Nb, H, W, C)), _rand(5, (N, 9, C), (9 * C) ** -0.5)
    pro = R.draw_pro('random', 6, C)
    assert bool((pro[0] > 0).any() and (pro[0] < 0).any() and (pro[1] > 0).any() and (pro[1] < 0).any())
    xn = (x * pro[0] + pro[1]).clamp_min(0)
    y = TF.conv2d(_nchw(xn), w.reshape(N, 3, 3, C).permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1)
    assert (R.fused_conv(x, R.transform_weights(w, MO), MO, pro=pro) - y).abs().max() < 1e-12
    a, _ = R.fused_wgrad(_rand(7, (Nb, H, W, N)), x, MO, pro=pro)
    b, _ = R.fused_wgrad(_rand(7, (Nb, H, W, N)), xn, MO)
    assert (a - b).abs().max() < 1e-12 * Nb * H * W


def test_blocked_layout_is_a_permutation_with_zero_padding():
    for rows, cols in ((40, 24), (8, 8), (72, 8), (32, 512)):
        idx = R.blocked_index(rows, cols).reshape(-1)
        assert idx.unique().numel() == idx.numel() and int(idx.max()) < R.blocked_numel(rows, cols)
        U = _rand(8, (36, rows, cols)) + 3.0
        ub = R.to_blocked(U)
        assert torch.equal(ub[idx], U.reshape(-1)) and int((ub == 0).sum()) == 36 * (-rows % 32) * cols


# -------------------------------------------------------------------------- the tolerances are bounds
@pytest.mark.parametrize('MO,shape', CASES, ids=IDS)
def test_hard_tolerance_dominates_the_fp32_yardstick(MO, shape):
    """|yardstick - ref| <= n 2^-23 S on every element of the conv (plain and normalise-on-load), of the weight
    gradient and of the weight transform."""
    Nb, H, W, C, N = shape
    for pro in (False, True):
        x, U, p = R.conv_problem('random', MO, shape, pro)
        ref = R.fused_conv(x, U, MO, pro=p)
        S = R.fused_conv(x, U, MO, pro=p, absval=True)
        yard = R.fused_conv(x.to(F32), U.to(F32), MO, pro=p).to(F64)
        assert bool(((yard - ref).abs() <= R.n_fwd(MO, C, pro=pro) * R.U32 * S).all())
        assert (yard - ref).abs().max() > 0
    dy, x = R.wgrad_problem('random', MO, shape)
    for splits in (1, 2):
        if R.wgrad_splits(Nb * (H // MO) * (W // MO), splits) is None:
            continue
        ref, tiles = R.fused_wgrad(dy, x, MO, splits)
        S, _ = R.fused_wgrad(dy, x, MO, splits, absval=True)
        yard = R.fused_wgrad(dy.to(F32), x.to(F32), MO, splits)[0].to(F64)
        for s, t in enumerate(tiles):
            assert bool(((yard[s] - ref[s]).abs() <= R.n_wgrad(MO, t) * R.U32 * S[s]).all())
    w = R.draw_w('random', 9, N, C)
    for dgrad in (False, True):
        ref = R.transform_weights(w, MO, dgrad)
        S = R.transform_weights(w, MO, dgrad, absval=True)
        yard = R.transform_weights(w, MO, dgrad, dtype=F32).to(F64)
        assert bool(((yard - ref).abs() <= R.N_WEIGHTS[MO] * R.U32 * S).all())


# ------------------------------------------------------------------------------------ the exact sets
@pytest.mark.parametrize('MO,shape', CASES, ids=IDS)
def test_exact_sets_stay_below_2_24(MO, shape):
    """S < 2^24 on every element, with the bias and under normalise-on-load; the reference is integer-valued.
    F(2x2) weight gradient: in units of 1/4 (G^T halves twice)."""
    Nb, H, W, C, N = shape
    bias = R.draw_bias('exact', 11, N)
    for pro in (False, True):
        x, U, p = R.conv_problem('exact', MO, shape, pro)
        ref = R.fused_conv(x, U, MO, pro=p)
        S = R.fused_conv(x, U, MO, pro=p, absval=True) + bias.abs()
        assert R.exact_ok(S) and torch.equal(ref, ref.round()) and bool((U == U.round()).all())
        # the statistics' fp32 partial sums: sum v exact on both, sum v^2 on F(2x2) only (judge_sums knows)
        assert R.sums_exact(ref + bias, MO) == (True, MO == 2)
        assert float(ref.abs().max()) > 0
    dy, x = R.wgrad_problem('exact', 2, R.shapes(2)[R.shapes(MO).index(shape)])
    S, _ = R.fused_wgrad(dy, x, 2, absval=True)
    ref, _ = R.fused_wgrad(dy, x, 2)
    assert R.exact_ok(S + 6.0, 0.25) and torch.equal(ref * 4, (ref * 4).round())


@pytest.mark.parametrize('shape', R.shapes(2), ids=IDS)
def test_exact_w_is_exact_for_f2x2_only(shape):
    Nb, H, W, C, N = shape
    w = R.draw_w('exact_w', 12, N, C)
    for dgrad in (False, True):
        U = R.transform_weights(w, 2, dgrad)
        assert torch.equal(U, U.round()) and torch.equal(U, R.transform_weights(w, 2, dgrad, dtype=F32).to(F64))
    U4 = R.transform_weights(w, 4)
    assert not torch.equal(U4, G.f32r(U4)), 'F(4x4): G holds 1/6 and 1/24, the set is no fp32 set'


def test_gates_are_exact_decisions():
    """BNB / BNP gates: y * scale + shift is exact in fp32 on every element (the cap on excluded elements is 0) and
    the BNB draw has elements exactly on the threshold."""
    on_threshold = 0
    for MO, shape in CASES:
        Nb, H, W, C, N = shape
        scale, shift = G.draw_scale_shift(21, N)
        y = G.draw_decision(22, (Nb * H * W, N))
        y2 = G.draw_pool_y(23, Nb, H, W, N, scale)
        assert G.decisions_inexact(y, scale, shift) == 0 and G.decisions_inexact(y2, scale, shift) == 0
        z = y * scale + shift
        on_threshold += int((z == 0).sum())
        assert not bool(((z != 0) & (z.abs() < 2.0 ** -20)).any())
        gate = G.draw_gate(24, (Nb * H * W, N))
        assert not bool(((gate != 0) & (gate.abs() < 2.0 ** -20)).any())
    assert on_threshold > 0


# --------------------------------------------------------------------------------------------- bite
def _applies(mutant, MO, shape, tb):
    Nb, H, W, C, N = shape
    T = Nb * (H // MO) * (W // MO)
    return {'border_neighbour': Nb >= 3, 'drop_tile_block': T > tb and T % tb != 0, 'drop_last_chunk': True,
            'double_chunk': (C // 8) % 2 == 1, 'at_coeff': True, 'at_slight': True,
            'skip_channel': N % 16 != 0}[mutant]


FWD_MUTANTS = ('border_neighbour', 'drop_tile_block', 'drop_last_chunk', 'double_chunk', 'at_coeff', 'at_slight',
               'skip_channel')


@pytest.mark.parametrize('mode', ('exact', 'random'))
@pytest.mark.parametrize('MO,shape', CASES, ids=IDS)
def test_forward_mutants_are_rejected(MO, shape, mode):
    """Every wrong forward kernel, on every shape it applies to and against each tile-block size the kernels use,
    is rejected by the judge; the true reference passes it."""
    Nb, H, W, C, N = shape
    x, U, _ = R.conv_problem(mode, MO, shape)
    ref = R.fused_conv(x, U, MO)
    tol = R.n_fwd(MO, C) * R.U32 * R.fused_conv(x, U, MO, absval=True)
    yard = R.fused_conv(x.to(F32), U.to(F32), MO).to(F64) if mode == 'random' else None
    R.judge('reference', yard if mode == 'random' else ref, ref, tol, mode, yard, MO=MO)
    seen = 0
    for mutant in FWD_MUTANTS:
        for tb in ((16, 32, 64) if mutant == 'drop_tile_block' else (64,)):
            if not _applies(mutant, MO, shape, tb):
                continue
            bad = R.fused_conv(x, U, MO, mutant=mutant, tile_block=tb)
            assert _rejected(bad, ref, tol, mode, yard, MO=MO), (mutant, tb)
            seen += 1
    assert seen >= 3


def test_every_forward_mutant_applies_somewhere():
    for mutant in FWD_MUTANTS:
        for MO in MOS:
            assert any(_applies(mutant, MO, s, tb) for s in R.shapes(MO) for tb in (16, 32, 64)), (mutant, MO)
    for MO in MOS:      # blocks of 16, 32 and 64 tiles each meet a partial last block after a full one
        for tb in (16, 32, 64):
            assert any(_applies('drop_tile_block', MO, s, tb) for s in R.shapes(MO))


@pytest.mark.parametrize('MO,shape', CASES, ids=IDS)
def test_the_old_frobenius_gate_accepts_a_slightly_wrong_output_transform(MO, shape):
    """A^T[MO - 1][3] off by 2^-16 of itself at one in-tile position: inside the older tests' whole-tensor gate
    (1e-5 for F(2x2), 3e-5 for F(4x4)), rejected by the judge (per in-tile position against the yardstick)."""
    Nb, H, W, C, N = shape
    x, U, _ = R.conv_problem('random', MO, shape)
    ref = R.fused_conv(x, U, MO)
    tol = R.n_fwd(MO, C) * R.U32 * R.fused_conv(x, U, MO, absval=True)
    yard = R.fused_conv(x.to(F32), U.to(F32), MO).to(F64)
    bad = G.f32r(R.fused_conv(x, U, MO, mutant='at_slight'))
    assert R.frobenius(bad, ref) < R.OLD_GATE[MO]
    assert _rejected(bad, ref, tol, 'random', yard, MO=MO)


@pytest.mark.parametrize('mode', ('exact', 'random'))
@pytest.mark.parametrize('MO,shape', CASES, ids=IDS)
def test_dgrad_without_the_flip_is_rejected(MO, shape, mode):
    Nb, H, W, C, N = shape
    dy = R.draw_x(mode, 31, (Nb, H, W, N))
    w = R.draw_w('random', 32, N, C) if mode == 'random' else R.ints(32, (N, 9, C), -1, 1) * 24.0
    ref = R.fused_conv(dy, R.transform_weights(w, MO, dgrad=True), MO)
    bad = R.fused_conv(dy, R.transform_weights(w, MO, dgrad=True, mutant='noflip'), MO)
    tol = R.n_fwd(MO, N) * R.U32 * R.fused_conv(dy, R.transform_weights(w, MO, dgrad=True), MO, absval=True)
    yard = R.fused_conv(dy.to(F32), R.transform_weights(w, MO, dgrad=True).to(F32), MO).to(F64)
    assert _rejected(bad, ref, tol, mode, yard, MO=MO)
    # and the transform itself, element by element under its own bound
    u, ub = R.transform_weights(w, MO, dgrad=True), R.transform_weights(w, MO, dgrad=True, mutant='noflip')
    assert _rejected(ub, u, R.N_WEIGHTS[MO] * R.U32 * R.transform_weights(w, MO, dgrad=True, absval=True), mode)


def _stats_case(mode, MO, shape, bias):
    Nb, H, W, C, N = shape
    x, U, _ = R.conv_problem(mode, MO, shape)
    acc, S = R.fused_conv(x, U, MO), R.fused_conv(x, U, MO, absval=True)
    r = G.epilogue(acc.reshape(-1, N), S.reshape(-1, N), R.n_fwd(MO, C), bias=bias, stats=True)
    return r


@pytest.mark.parametrize('mode', ('exact', 'random'))
@pytest.mark.parametrize('MO,shape', CASES, ids=IDS)
def test_a_statistic_that_counts_a_masked_tile_is_rejected(MO, shape, mode):
    """A tile past the end of a partial tile block holds zero accumulators, so bias alone: counting one adds MO^2
    b and MO^2 b^2 per channel.  Rejected against the fp64 sums on the exact set (they must be equal) and against the
    sums of the output itself on both sets."""
    Nb, H, W, C, N = shape
    bias = R.draw_bias(mode, 41, N)
    r = _stats_case(mode, MO, shape, bias)
    extra = torch.stack([MO * MO * bias, MO * MO * bias * bias])
    own, own_tol = R.own_sums(r['out'], MO)
    R.judge_sums('reference', r['sums'], own, own_tol, mode, r['out'], MO)
    assert _rejected_sums(r['sums'] + extra, own, own_tol, mode, r['out'], MO)
    if mode == 'exact':
        assert _rejected_sums(r['sums'] + extra, r['sums'], r['sums_tol'], mode, r['out'], MO)


@pytest.mark.parametrize('MO', MOS)
def test_the_old_frobenius_gate_accepts_a_miscounted_statistic(MO):
    """One channel with bias 1 among channels with a large bias (64 on F(4x4)'s 1200 pixels, 256 on F(2x2)'s 300):
    the masked tile's MO^2 ones vanish in the old tests' norm over all channels; the exact set's sums must be equal,
    so the judge rejects them."""
    shape = R.shapes(MO)[2]
    N = shape[-1]
    bias = torch.full((N,), 64.0 if MO == 4 else 256.0, dtype=F64)
    bias[N - 1] = 1.0
    r = _stats_case('exact', MO, shape, bias)
    assert R.sums_exact(r['out'], MO)[0]
    extra = torch.zeros(2, N, dtype=F64)
    extra[:, N - 1] = MO * MO
    bad = r['sums'] + extra
    assert R.frobenius(bad[0], r['sums'][0]) < R.OLD_GATE[MO] and R.frobenius(bad[1], r['sums'][1]) < R.OLD_GATE[MO]
    own, own_tol = R.own_sums(r['out'], MO)
    assert _rejected_sums(bad, own, own_tol, 'exact', r['out'], MO)
    assert _rejected_sums(bad, r['sums'], r['sums_tol'], 'exact', r['out'], MO)


@pytest.mark.parametrize('mode', ('exact', 'random'))
@pytest.mark.parametrize('MO,shape', CASES, ids=IDS)
def test_pool_and_padding_mutants_are_rejected(MO, shape, mode):
    Nb, H, W, C, N = shape
    x, U, _ = R.conv_problem(mode, MO, shape)
    acc, S = R.fused_conv(x, U, MO), R.fused_conv(x, U, MO, absval=True)
    bias = R.draw_bias(mode, 51, N)
    ref, tol = R.pooled(acc, S, R.n_fwd(MO, C), bias)
    bad, _ = R.pooled(acc, S, R.n_fwd(MO, C), bias, mutant='pool_shift')
    yard = None
    if mode == 'random':
        yard = R.pool2(G.f32r(R.fused_conv(x.to(F32), U.to(F32), MO).to(F64) + bias).clamp_min(0))
        R.judge('reference', yard, ref, tol, mode, yard, MO=MO // 2)
    if W > 2:       # a 2-wide map has one window per row: shifting it (cyclically) changes nothing
        assert _rejected(bad, ref, tol, mode, yard, MO=MO // 2)
    # the padding normalised to relu(shift) instead of staying zero
    x, U, pro = R.conv_problem(mode, MO, shape, pro=True)
    ref = R.fused_conv(x, U, MO, pro=pro)
    tol = R.n_fwd(MO, C, pro=True) * R.U32 * R.fused_conv(x, U, MO, pro=pro, absval=True)
    yard = R.fused_conv(x.to(F32), U.to(F32), MO, pro=pro).to(F64) if mode == 'random' else None
    assert _rejected(R.fused_conv(x, U, MO, pro=pro, mutant='pad_relu_shift'), ref, tol, mode, yard, MO=MO)


@pytest.mark.parametrize('MO,shape', CASES, ids=IDS)
def test_weight_gradient_mutants_are_rejected(MO, shape):
    """One split a chunk short; the border row read from the neighbouring image; padding normalised."""
    Nb, H, W, Ci, Co = shape
    T = Nb * (H // MO) * (W // MO)
    dy, x = R.wgrad_problem('random', MO, shape)
    pro = R.draw_pro('random', 61, Ci)
    for splits in (1, 2, 4):
        if R.wgrad_splits(T, splits) is None:
            continue
        ref, tiles = R.fused_wgrad(dy, x, MO, splits)
        S, _ = R.fused_wgrad(dy, x, MO, splits, absval=True)
        yard = R.fused_wgrad(dy.to(F32), x.to(F32), MO, splits)[0].to(F64)
        muts = ['split_short'] + (['border_neighbour'] if Nb >= 3 else [])
        for mutant in muts:
            bad, _ = R.fused_wgrad(dy, x, MO, splits, mutant=mutant)
            rej = [_rejected(bad[s], ref[s], R.n_wgrad(MO, t) * R.U32 * S[s], 'random', yard[s], layout='wgrad')
                   for s, t in enumerate(tiles)]
            assert any(rej), (mutant, splits)
        for s, t in enumerate(tiles):
            R.judge('reference', yard[s], ref[s], R.n_wgrad(MO, t) * R.U32 * S[s], 'random', yard[s], layout='wgrad')
    ref, tiles = R.fused_wgrad(dy, x, MO, pro=pro)
    S, _ = R.fused_wgrad(dy, x, MO, pro=pro, absval=True)
    bad, _ = R.fused_wgrad(dy, x, MO, pro=pro, mutant='pad_relu_shift')
    yard = R.fused_wgrad(dy.to(F32), x.to(F32), MO, pro=pro)[0].to(F64)
    assert _rejected(bad[0], ref[0], R.n_wgrad(MO, T, pro=True) * R.U32 * S[0], 'random', yard[0], layout='wgrad')


# ---------------------------------------------------------------------------------- expected_status
def test_expected_status_of_the_launchers():
    s4, s2 = (1, 4, 4, 8, 32), (1, 2, 2, 8, 32)
    e = R.expected_status
    assert e('rk_wino4_conv_grp', 0, s4) == 0 and e('rk_wino4_conv_grp', 6, s4) == -1
    assert e('rk_wino4_conv_grp', 0, (1, 6, 4, 8, 32)) == -1 and e('rk_wino4_conv_grp', 0, (1, 4, 4, 12, 32)) == -1
    assert e('rk_wino4_conv_grp', 0, s4, flags=R.STATS) == -1 and e('rk_wino4_conv_grp', 0, s4, flags=R.BIAS) == -1
    assert e('rk_wino4_conv_grp', 0, s4, flags=R.BNB, stats=True, gate=True) == -1
    assert e('rk_wino4_conv_grp', 0, s4, flags=R.STATS, stats=True, groups=2) == -2
    assert e('rk_wino4_conv_grp', 0, s4, flags=R.POOL) == -2 and e('rk_wino4_conv_grp', 0, s4, flags=R.POOLED, bias=True) == 0
    assert e('rk_wino4_conv_grp', 0, s4, pro=True) == -2 and e('rk_wino4_conv_grp', 3, s4, pro=True) == 0
    assert e('rk_wino4_conv_grp', 3, s4, pro=True, flags=R.BIAS | R.RELU, bias=True) == -2
    assert e('rk_wino4_conv_grp', 3, (1, 4, 4, 520, 32), pro=True) == -2 and e('rk_wino4_conv_grp', 3, s4, pro=True, groups=2) == -2
    assert e('rk_wino2s_conv_grp', 4, s2) == -1 and e('rk_wino2s_conv_grp', 3, s2) == 0
    assert e('rk_wino_conv_grp', 2, s2) == -1 and e('rk_wino_conv_grp', 1, s2, flags=R.POOLED, bias=True) == -2
    assert e('rk_wino_conv_grp', 0, (1, 3, 2, 8, 32)) == -1
    w = (2, 4, 4, 16, 16)
    assert e('rk_wino4_wgrad', 0, w) == 0 and e('rk_wino4_wgrad', 0, w, splits=2) == -1
    assert e('rk_wino4_wgrad', 0, w, splits=2, accumulate=True) == -1 and e('rk_wino4_wgrad', 3, w) == -1
    assert e('rk_wino4_wgrad', 2, w, pro=True) == -2 and e('rk_wino4_wgrad', 1, w, pro=True) == 0
    assert e('rk_wino_wgrad', 0, (5, 6, 10, 8, 72), splits=4) == 0 and e('rk_wino_wgrad', 0, (1, 3, 2, 8, 8)) == -1
    assert e('rk_wino4_wgrad', 0, (1 << 12, 128, 128, 8, 8)) == -2


# ------------------------------------------------------------------------------------------- decode
def test_the_fp32_reciprocal_tile_decode_is_exact_below_2_22_tiles():
    """(int)((t + 0.5f) * (1.0f / d)) == t // d for every t < 2^22: d = 1..299 and a spread of larger divisors up
    to 2^22 - 1 (powers of two and their neighbours, primes, the largest values)."""
    t = np.arange(1 << 22, dtype=np.int64)
    big = sorted({v for k in range(8, 22) for v in ((1 << k) - 1, 1 << k, (1 << k) + 1)}
                 | {300, 337, 1000, 1023, 4099, 65521, 100003, 1000003, 3000017, (1 << 22) - 3, (1 << 22) - 1})
    for d in list(range(1, 300)) + big:
        got = R.decode(t, d)
        bad = np.nonzero(got != t // d)[0]
        assert bad.size == 0, 'd = {}: first mismatch at t = {} ({} != {})'.format(d, bad[0], got[bad[0]], bad[0] // d)
