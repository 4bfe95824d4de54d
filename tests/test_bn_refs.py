"""tests/bn_refs.py on the CPU: its fp64 formulas against torch's batch_norm + activation + max_pool2d under
autograd (1e-12), and how far each plausible wrong formula moves an output that tests/test_bn_gpu.py compares,
measured on that file's own inputs against the tolerance it applies there (>= 10 x).  Also: every case's inputs
leave no decision (sign of z, window argmax) inside the guard band, and bn_slots() is a power of two."""
import pytest
import torch
import torch.nn.functional as TF

import bn_refs as B
from loss_optim_refs import err

F64, F32 = B.F64, B.F32
ANCHOR = 1e-12


# ------------------------------------------------------------------------------------------- anchor
def _torch_bn(c, pool, act):
    y = c.y.double().permute(0, 3, 1, 2).requires_grad_(True)
    g, b = c.gamma.double().requires_grad_(True), c.beta.double().requires_grad_(True)
    rm, rv = c.rm.double().clone(), c.rv.double().clone()
    z = TF.batch_norm(y, rm, rv, g, b, training=True, momentum=c.momentum, eps=c.eps)
    a = torch.relu(z) if act == B.ACT_RELU else TF.leaky_relu(z, B.SLOPE) if act == B.ACT_LRELU else z
    out = TF.max_pool2d(a, 2) if pool else a
    gy, gg, gb = torch.autograd.grad(out, [y, g, b], c.dout[pool].double().permute(0, 3, 1, 2))
    return out.detach().permute(0, 2, 3, 1), gy.permute(0, 2, 3, 1), gg, gb, rm, rv


@pytest.mark.parametrize('act', B.ACTS)
@pytest.mark.parametrize('pool', [False, True])
@pytest.mark.parametrize('shape', B.ANCHOR_SHAPES)
def test_formulas_match_torch_autograd(shape, pool, act):
    """stats -> finalize -> fwd / bwd in fp64 (coefficients unrounded) against autograd, ties included: the
    zero-gamma channel (every z == 0) and the constant channel (every window four equal values)."""
    for hyper in (0, 1):
        c = B.Case('f32', shape, hyper)
        s, q = B.stats(c.y)
        mean, rstd, scale, shift, rm, rv = B.finalize(s, q, c.count, c.gamma, c.beta, c.eps, c.rm, c.rv, c.momentum)
        out = B.fwd(c.y, scale, shift, pool, act)
        dy, dg, db = B.bwd(c.dout[pool], c.y, mean, rstd, scale, shift, c.gamma, c.count, pool, act)
        for name, got, ref in zip(('out', 'dy', 'dgamma', 'dbeta', 'rm', 'rv'), (out, dy, dg, db, rm, rv),
                                  _torch_bn(c, pool, act)):
            assert err(got, ref) <= ANCHOR, (name, err(got, ref))
        sums = B.bwd_sums(c.dout[pool], c.y, scale, shift, pool, act)
        assert err(sums[0], db) <= ANCHOR
        dy2, _, _ = B.bwd(c.dout[pool], c.y, mean, rstd, scale, shift, c.gamma, c.count, pool, act, sums=sums)
        assert torch.equal(dy, dy2)


@pytest.mark.parametrize('shape', B.ANCHOR_SHAPES)
def test_eval_formulas_match_torch(shape):
    c = B.Case('f32', shape)
    scale, shift = B.eval_coeffs(c.gamma, c.beta, c.rm, c.rv, c.eps)
    ref = TF.batch_norm(c.y.double().permute(0, 3, 1, 2), c.rm.double(), c.rv.double(), c.gamma.double(),
                        c.beta.double(), training=False, eps=c.eps).permute(0, 2, 3, 1)
    assert err(B.fwd(c.y, scale, shift, False, B.ACT_NONE), ref) <= ANCHOR
    ones, zeros = torch.ones_like(c.gamma), torch.zeros_like(c.beta)
    for a, b in zip(B.eval_coeffs(None, None, c.rm, c.rv, c.eps), B.eval_coeffs(ones, zeros, c.rm, c.rv, c.eps)):
        assert torch.equal(a, b)


def test_window_order_and_edges():
    x = torch.arange(2 * 5 * 3 * 2, dtype=F64).reshape(2, 5, 3, 2)
    w = B.windows(x)
    assert w.shape == (2, 2, 1, 2, 4)
    assert w[1, 1, 0, 1].tolist() == [x[1, 2, 0, 1], x[1, 2, 1, 1], x[1, 3, 0, 1], x[1, 3, 1, 1]]
    back = B.unwindow(w, 5, 3)
    assert torch.equal(back[:, :4, :2], x[:, :4, :2]) and not back[:, 4].any() and not back[:, :, 2].any()


def test_tables_sum_to_their_input():
    sums = torch.randn(2, 24, dtype=F64, generator=torch.Generator().manual_seed(1)) * 100
    sums[0, 3] = 0.0
    for SL in (1, 2, 3, 4, 5, 8):
        t = B.split_slots(sums, SL, SL)
        assert t.shape == (SL, 2, 24) and (SL == 1 or bool((t[:, sums != 0] < 0).any()))
    for R in B.ROW_COUNTS:
        t, ref = B.split_rows(sums, R, R)
        assert t.dtype == F32 and t.shape == (R, 2, 24) and err(ref, sums) < 1e-6


# ------------------------------------------------------------------------------------------- guard band
@pytest.mark.parametrize('kind,shape', [('bf16', s) for s in B.BF16_SHAPES + tuple(B.ROW_SHAPE + (C,) for C in
                                                                                B.ROW_CHANNELS)] +
                         [('f32', s) for s in B.F32_SHAPES])
def test_no_decision_inside_the_guard_band(kind, shape):
    c = B.case(kind, shape)
    assert bool((c.y[..., B.CONST] == B.CONST_Y).all()) and c.gamma[B.ZERO] == 0 and c.gamma[B.BIG] == -8
    assert bool((c.gamma < 0).any()) and c.coeffs[2, B.ZERO] == 0 and c.coeffs[3, B.ZERO] == 0
    m, v = c.y[..., B.OFF].double().mean(), c.y[..., B.OFF].double().var()
    assert 4 < m / v.sqrt() < 16                                         # mean = 8 std, up to the draw
    for pool in B.pools_of(shape):
        for act in B.acts_of(shape):
            assert B.ambiguous(c.y, c.coeffs[2], c.coeffs[3], pool, act) == 0, (pool, act)


@pytest.mark.parametrize('i', range(len(B.LARGE)))
def test_no_decision_inside_the_guard_band_large(i):
    c, pool = B.large_case(i), B.LARGE[i][1]
    assert B.ambiguous(c.y, c.coeffs[2], c.coeffs[3], pool, B.ACT_RELU) == 0


def test_guard_band_counts_what_it_should():
    y = torch.tensor([1.0, 1.0 + 2.0 ** -22, -3.0, 1.0, 1.0, 1.0, -2.0, -3.0]).reshape(2, 2, 2, 1)
    one, zero = torch.ones(1), torch.zeros(1)
    assert B.ambiguous(y, one, zero, True, B.ACT_NONE) == 1              # window 0: two near-equal maxima
    assert B.ambiguous(y, one, zero, False, B.ACT_RELU) == 0
    assert B.ambiguous(y, one, -one, False, B.ACT_RELU) == 5             # z = 0 or 2^-22 at five positions
    assert B.ambiguous(y, zero, zero, True, B.ACT_RELU) == 0             # scale 0: z == shift in any precision
    assert B.ambiguous(-y.abs(), one, zero, True, B.ACT_RELU) == 0       # all clamped to exactly 0


# ------------------------------------------------------------------------------------------- bn_slots
def test_bn_slots_is_a_power_of_two():
    """The conv epilogues and the reduce kernels pick a slot with block & (SL - 1)."""
    from rafiki_amd.ops.functional import bn_slots
    for C in range(4, 2049, 4):
        n = bn_slots(C)
        assert 1 <= n <= 8 and n & (n - 1) == 0, (C, n)
        assert n <= max(1, 512 // C) < 2 * n or n == 8
    assert [bn_slots(C) for C in (8, 16, 32, 64, 128, 256, 512, 1024, 2048)] == [8, 8, 8, 8, 4, 2, 1, 1, 1]
    assert [bn_slots(C) for C in (72, 80, 96, 136, 168)] == [4, 4, 4, 2, 2]


# ------------------------------------------------------------------------------------------- sensitivity
def _wrong_bwd(c, pool, act, knob=None, slope=B.SLOPE):
    """B.bwd on the case's fed coefficients with one thing wrong (knob None: nothing, equal to B.bwd)."""
    y, dout, g = c.y.double(), c.dout[pool].double(), c.gamma.double()
    mean, rstd, scale, shift = c.coeffs.double()
    N, H, W, C = c.shape
    Ho, Wo = H // 2, W // 2
    z = y * scale + shift
    d = B.act_d(z, act, slope)
    if knob == 'ge0' and act != B.ACT_NONE:
        d = torch.where(z >= 0, torch.ones_like(z), torch.full_like(z, slope if act == B.ACT_LRELU else 0.0))
    if knob == 'no_slope' and act == B.ACT_LRELU:
        d = B.act_d(z, B.ACT_RELU)
    if pool:
        key = B.windows({'route_on_z': z, 'route_on_y': y}.get(knob, B.act_f(z, act, slope)))
        is_max = key == key.amax(-1, keepdim=True)
        cs = is_max.to(torch.int8).cumsum(-1)
        sel = is_max & (cs == (cs[..., -1:] if knob == 'last_max' else 1))
        dz = B.unwindow(sel.double() * B.windows(d), H, W) * B.spread(dout, H, W)
    else:
        dz = d * dout
    s0 = dz.reshape(-1, C).sum(0)
    s1 = (dz * ((y - mean) * rstd if knob == 'xhat_sum' else y)).reshape(-1, C).sum(0)
    count = N * Ho * Wo if knob == 'pooled_count' and pool else c.count
    dg, db = rstd * (s1 - mean * s0), s0
    k1, k2 = g * rstd, -g * rstd * rstd * dg / count
    k3 = -g * rstd * db / count + (k2 * mean if knob == 'k3_sign' else -k2 * mean)
    dy = k1 * dz + k2 * y + k3
    if pool and knob in ('edge_zero', 'edge_k1dout'):
        edge = torch.ones((N, H, W, 1), dtype=torch.bool)
        edge[:, :2 * Ho, :2 * Wo] = False
        hh, ww = (torch.arange(H) // 2).clamp_max(Ho - 1), (torch.arange(W) // 2).clamp_max(Wo - 1)
        near = dout[:, hh][:, :, ww]                   # the nearest window's gradient
        dy = torch.where(edge, torch.zeros_like(dy) if knob == 'edge_zero' else k1 * near + k2 * y + k3, dy)
    return dy, dg, db


def _bwd_refs(c, pool, act, slope=B.SLOPE):
    ref, r32, _, floor = B.bwd_refs(c.dout[pool], c.y, c.coeffs, c.gamma, c.count, pool, act, slope)
    return ref, (r32, floor)


def _moved(c, wrong, ref, ref32):
    """Does the wrong result leave the GPU test's tolerance of any output by the sensitivity factor?"""
    hits = {}
    ref32, floor = ref32
    for name, w, r, r32, fl in zip(('dy', 'dgamma', 'dbeta'), wrong, ref, ref32, floor):
        delta = (w - r).abs()
        if name == 'dy' and c.kind == 'bf16':
            tol = B.tol_bf16(r32, r)
            hits[name] = bool(((delta >= B.SENSITIVITY * tol) & (delta > 0)).any())
        else:
            tol, _ = B.tol_f32(r32, r, floor=fl)
            dc = delta.reshape(-1, r.shape[-1]).amax(0)
            hits[name] = bool(((dc >= B.SENSITIVITY * tol) & (dc > 0)).any())
    return hits


ODD_BF16, ODD_F32 = (3, 5, 3, 24), (2, 7, 6, 32)
# knob -> the (kind, shape, pool, act) of test_bn_gpu.py that must show it.  An input that cannot show a knob is
# named in the comment and left out.
BWD_KNOBS = {
    # ties exist only in the constant channel (dy moves to another position) and in the zero-gamma channel
    # (k1 = 0: dy cannot move; sum dz*y moves unless ReLU makes dz = 0 there)
    'last_max': [('bf16', (4, 8, 8, 64), True, a) for a in B.ACTS] + [('f32', (4, 8, 8, 64), True, a) for a in B.ACTS],
    'route_on_y': [('bf16', (4, 8, 8, 64), True, B.ACT_RELU), ('f32', (2, 4, 4, 4), True, B.ACT_NONE),
                   ('bf16', ODD_BF16, True, B.ACT_LRELU)],
    # z == 0 exactly happens only in the zero-gamma channel (beta = 0): dgamma / dbeta leave 0 there; no other
    # channel and no ACT_NONE case can show it
    'ge0': [('bf16', (4, 8, 8, 64), False, B.ACT_RELU), ('f32', (4, 8, 8, 64), True, B.ACT_RELU),
            ('f32', (2, 4, 4, 4), False, B.ACT_LRELU), ('bf16', (2, 4, 4, 8), True, B.ACT_LRELU)],
    'no_slope': [('bf16', (4, 8, 8, 64), p, B.ACT_LRELU) for p in (False, True)] +
                [('f32', (2, 7, 6, 32), p, B.ACT_LRELU) for p in (False, True)],
    # only the odd maps have an edge
    'edge_zero': [('bf16', ODD_BF16, True, a) for a in B.ACTS] + [('f32', ODD_F32, True, a) for a in B.ACTS] +
                 [('bf16', (2, 2, 7, 40), True, B.ACT_RELU), ('f32', (2, 2, 7, 16), True, B.ACT_RELU)],
    'edge_k1dout': [('bf16', ODD_BF16, True, a) for a in B.ACTS] + [('f32', ODD_F32, True, a) for a in B.ACTS] +
                   [('bf16', (2, 2, 7, 40), True, B.ACT_RELU), ('f32', (2, 2, 7, 16), True, B.ACT_RELU)],
    'k3_sign': [('bf16', (4, 8, 8, 64), p, B.ACT_RELU) for p in (False, True)] +
               [('f32', (4, 8, 8, 64), p, B.ACT_NONE) for p in (False, True)],
    # without pooling the two counts are the same number
    'pooled_count': [('bf16', (4, 8, 8, 64), True, B.ACT_RELU), ('f32', (4, 8, 8, 64), True, B.ACT_LRELU),
                     ('bf16', ODD_BF16, True, B.ACT_NONE)],
    'xhat_sum': [('bf16', (4, 8, 8, 64), False, B.ACT_RELU), ('f32', (4, 8, 8, 64), True, B.ACT_RELU),
                 ('bf16', (37, 1, 1, 784), False, B.ACT_NONE), ('f32', (5, 1, 1, 1536), False, B.ACT_NONE)],
}


@pytest.mark.parametrize('knob', list(BWD_KNOBS))
def test_wrong_backward_leaves_the_tolerance(knob):
    for kind, shape, pool, act in BWD_KNOBS[knob]:
        c = B.case(kind, shape)
        ref, ref32 = _bwd_refs(c, pool, act)
        for a, b in zip(_wrong_bwd(c, pool, act), ref):
            assert err(a, b) <= ANCHOR                               # the copy itself is right
        hits = _moved(c, _wrong_bwd(c, pool, act, knob), ref, ref32)
        assert any(hits.values()), (knob, kind, shape, pool, act, hits)


def test_routing_on_z_is_wrong_only_for_a_decreasing_activation():
    """max act(z) and max z sit at the same position whenever act is non-decreasing, and where ReLU flattens a
    whole window to 0 the routed gradient is 0 wherever it goes: with slope >= 0 'routing on z' is not a
    different function, negative gamma or not, so no case of test_bn_gpu.py with slope 0.2 can tell them apart
    (asserted here).  A negative slope makes act(z) non-monotone and the two differ: the (4, 8, 8, 64) cases
    with slope -0.2 show it, and test_bn_gpu.py runs them."""
    for kind in ('bf16', 'f32'):
        c = B.case(kind, (4, 8, 8, 64))
        for act in B.ACTS:
            for a, b in zip(_wrong_bwd(c, True, act, 'route_on_z'), _wrong_bwd(c, True, act)):
                assert torch.equal(a, b)
        slope = B.NEG_SLOPE
        assert B.ambiguous(c.y, c.coeffs[2], c.coeffs[3], True, B.ACT_LRELU, slope) == 0
        ref, ref32 = _bwd_refs(c, True, B.ACT_LRELU, slope)
        hits = _moved(c, _wrong_bwd(c, True, B.ACT_LRELU, 'route_on_z', slope), ref, ref32)
        assert hits['dy'] and (hits['dgamma'] or hits['dbeta']), hits


def _fin_tols(c, sums):
    args = (sums[0], sums[1], c.count, c.gamma, c.beta, c.eps, c.rm, c.rv, c.momentum)
    ref, r32 = B.finalize(*args, dtype=F64), B.finalize(*[a.to(F32) if torch.is_tensor(a) else a for a in args],
                                                        dtype=F32)
    return ref, [B.tol_f32(a, b)[0] for a, b in zip(r32, ref)]


@pytest.mark.parametrize('kind,shape', [('bf16', (2, 4, 4, 8)), ('bf16', (4, 8, 8, 64)), ('f32', (2, 4, 4, 4)),
                                        ('f32', (4, 8, 8, 64)), ('f32', (9, 32, 32, 256))])
def test_wrong_running_statistics_leave_the_tolerance(kind, shape):
    """Biased running variance: the move is momentum * var / (count - 1), so it shrinks with the pixel count; it
    clears the margin at every count up to the 256 of (4, 8, 8, 64).  At the 9216 pixels of (9, 32, 32, 256)
    with momentum 0.01 it is 1e-6 of var, inside fp32's own error: that case cannot show it and is checked for
    the swapped momentum only."""
    c = B.case(kind, shape)
    ref, tols = _fin_tols(c, c.sums)
    mean, var = ref[0], (c.sums[1] / c.count - ref[0] ** 2).clamp_min(0)
    m = c.momentum
    biased = (1 - m) * c.rv.double() + m * var
    swapped = m * c.rm.double() + (1 - m) * mean, m * c.rv.double() + (1 - m) * var * c.count / (c.count - 1)
    if c.count <= 256:
        assert bool(((biased - ref[5]).abs() >= B.SENSITIVITY * tols[5]).any())
    assert bool(((swapped[0] - ref[4]).abs() >= B.SENSITIVITY * tols[4]).any())
    assert bool(((swapped[1] - ref[5]).abs() >= B.SENSITIVITY * tols[5]).any())


@pytest.mark.parametrize('SL', [2, 3, 4, 5, 8])
def test_reading_only_slot_0_leaves_the_tolerance(SL):
    for kind, shape in (('bf16', (4, 8, 8, 64)), ('f32', (4, 8, 8, 64))):
        c = B.case(kind, shape)
        ref, tols = _fin_tols(c, c.sums)
        table = B.split_slots(c.sums, SL, SL)
        wrong = B.finalize(table[0, 0], table[0, 1], c.count, c.gamma, c.beta, c.eps, c.rm, c.rv, c.momentum)
        for w, r, t in zip(wrong, ref, tols):
            assert bool(((w - r).abs() >= B.SENSITIVITY * t).any())
        bsums = B.bwd_sums(c.dout[True], c.y, c.coeffs[2], c.coeffs[3], True, B.ACT_RELU)
        ref, ref32 = _bwd_refs(c, True, B.ACT_RELU)
        co = c.coeffs
        wrong = B.bwd(c.dout[True], c.y, co[0], co[1], co[2], co[3], c.gamma, c.count, True, B.ACT_RELU,
                      sums=B.split_slots(bsums, SL, SL)[0])
        assert all(_moved(c, wrong, ref, ref32).values())
