"""The fp32 dispatcher's routes, pinned on the CPU (no GPU, no kernel library).

``rafiki_amd/ops/f32.py`` turns every conv / dense call into a tune key, a candidate list of
``(tile, nst, splits)`` configs and a ``run(cfg)`` that launches kernels.  A mistake there passes wrong
arguments to a kernel, so this test records, for one call per entry of the shipped tune seed plus a few
hand-written ones, what the dispatcher offers and what every candidate would launch:

* ``_lib.call`` is replaced by a recorder, device pointers by ``'P'`` / ``None``, the stream by 0, and the
  tuning seam ``f32._pick`` by a function that keeps ``(key, cands, run)``; the operands are ``meta`` tensors;
* per case the key must equal the seed key, the shipped pick must be one of the candidates, and the SHA-1
  of the candidate list and of the launch traces of EVERY candidate (kernel name, every scalar argument,
  which pointers are null) must equal ``tests/golden/f32_routes.json``.

``python tests/test_f32_routes.py --record`` rewrites the golden file.  To see what changed after a
mismatch: ``--dump FILE`` at the commit that recorded the golden writes every candidate's full trace, and
``--diff FILE`` at the new commit prints, per differing case, the key and the first differing candidate with
its new trace.
"""
import ctypes
import glob
import hashlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from rafiki_amd.ops import _lib, autotune, functional  # noqa: E402
from rafiki_amd.ops import f32 as S  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'f32_routes.json')
# the one shipped gfx950 seed, whatever source hash keys it (tests/test_tune_seed.py checks the name)
(SEED,) = glob.glob(os.path.join(autotune.SHIPPED_DIR, 'gfx950-s*.json'))
F64, BF16 = torch.float64, torch.bfloat16


def t(*shape, dt=torch.float32):
    return torch.empty(shape, dtype=dt, device='meta')


def _set(flag, make):
    """A weight set as the key names it: 'lazy' -> a callable, True -> a tensor, False -> None."""
    return make if flag == 'lazy' else make() if flag else None


def call_from_key(k):
    """The dispatcher call a seed key was recorded from (the key layouts invert exactly)."""
    fam = k[0]
    if fam in ('sf', 'sd'):
        _, M, N, K, H, W, C, taps, flags, w2, w4, pt, ptx = k[:13]
        rest = k[13:]
        Nb = M // (H * W)
        b = next((r[1] for r in rest if isinstance(r, tuple) and r[0] == 'b'), False)
        # the input channels are C; the set shapes are [.., out channels N, C]
        sets = dict(wino=_set(w2, lambda: t(16, N, C)), wino4=_set(w4 or pt, lambda: t(36, N, C)),
                    wino4p=_set(ptx, lambda: t(36, 3, N, C, dt=BF16)), wino4b=_set(b, lambda: t(S.wino4b_numel(N, C))))
        if fam == 'sf':
            act = S.ACT_RELU if flags & 1 else S.ACT_LRELU if flags & 32 else S.ACT_NONE
            S.conv_fwd(t(Nb, H, W, C), t(N, taps * C), taps=taps, stats_acc=t(8, 2, N, dt=F64) if flags & 4 else None,
                       bias=t(N) if flags & 2 else None, act=act, pro=t(4, C) if 'pro' in rest else None, **sets)
        else:
            kw = {}
            if flags == S.F_BNB:
                kw['bnb'] = (t(Nb, H, W, N), t(4, N), t(8, 2, N, dt=F64))
            elif flags == S.F_BNP:
                kw['bnp'] = (t(Nb, 2 * H, 2 * W, N), t(4, N), t(8, 2, N, dt=F64))
            elif flags == S.F_GATE:
                kw['gate'] = t(Nb, H, W, N)
            S.conv_dgrad(t(Nb, H, W, C), lambda: t(N, taps * C), taps=taps, cin=N, **sets, **kw)
    elif fam == 'sw':
        _, Cout, N, K, H, W, Cin, taps, acc = k[:9]
        Nb = K // (H * W)
        S.conv_wgrad(t(Nb, H, W, Cout), t(Nb, H, W, Cin), taps=taps, out=t(Cout, taps * Cin), accumulate=acc,
                     xpro=t(4, Cin) if 'pro' in k else None)
    elif fam in ('sfg', 'sfgp'):
        if fam == 'sfg':
            _, G, M, Cout, K, H, W, Cin, shared, hb, act, w2, w4 = k
        else:
            _, G, M, Cout, K, H, W, Cin, shared, w2, w4 = k
            hb, act = True, S.ACT_RELU
        Nb = M // (H * W)
        S.conv_fwd_grp(t(Nb, H, W, Cin) if shared else t(G, Nb, H, W, Cin), t(G, Cout, K),
                       bias=t(G, Cout) if hb else None, act=act, wino=t(G, 16, Cout, Cin) if w2 else None,
                       wino4=t(G, 36, Cout, Cin) if w4 else None, pool=fam == 'sfgp')
    elif fam == 'sl':
        _, M, N, K, act, hb, alpha = k[:7]
        S.linear(t(M, K), t(N, K), t(N) if hb else None, act=act, alpha=alpha)
    elif fam == 'sx':
        _, M, Nin, Nout, g = k[:5]
        S.linear_dx(t(M, Nout), t(Nout, Nin), gate=t(M, Nin) if g else None)
    elif fam == 'sdw':
        _, M, Nout, Nin, acc = k[:5]
        S.linear_dw(t(M, Nout), t(M, Nin), out=t(Nout, Nin), accumulate=acc)
    elif fam == 'slg':
        _, G, M, N, K, shared, hb, act = k
        S.linear_grp(t(M, K) if shared else t(G, M, K), t(G, N, K), t(G, N) if hb else None, act=act)
    else:
        raise AssertionError('seed key family {!r} cannot be inverted into a call: teach this test'.format(fam))


def _extra_cases():
    """Hand-written calls the seed does not hold: the stride-2 family at PG-GAN lod-0 shapes (16 x 32x32 x
    512 <-> 16x16) and every dispatcher at Nb=8, H=W=8, Cin=32, Cout=64, the smallest shape at which every
    conv route id is offered."""
    Nb, H, Ci, Co = 8, 8, 32, 64
    x, w, dy = (lambda: t(Nb, H, H, Ci)), (lambda: t(Co, 9 * Ci)), (lambda: t(Nb, H, H, Co))

    def fsets(lazy=False):
        mk = dict(wino=lambda: t(16, Co, Ci), wino4=lambda: t(36, Co, Ci), wino4p=lambda: t(36, 3, Co, Ci, dt=BF16),
                  wino4b=lambda: t(S.wino4b_numel(Co, Ci)))
        return mk if lazy else {k: f() for k, f in mk.items()}

    def dsets(lazy=False):
        mk = dict(wino=lambda: t(16, Ci, Co), wino4=lambda: t(36, Ci, Co), wino4p=lambda: t(36, 3, Ci, Co, dt=BF16),
                  wino4b=lambda: t(S.wino4b_numel(Ci, Co)))
        return dict(mk if lazy else {k: f() for k, f in mk.items()}, cin=Ci)

    def acc(C):
        return t(8, 2, C, dt=F64)
    G = 3
    return [
        ('s2/conv', lambda: S.s2_conv(t(16, 32, 32, 512), t(512, 16 * 512), bias=t(512), act=S.ACT_LRELU)),
        ('s2/tconv', lambda: S.s2t_conv(t(16, 16, 16, 512), t(512, 16 * 512), bias=t(512), act=S.ACT_LRELU)),
        ('s2/wgrad', lambda: S.s2_wgrad(t(16, 32, 32, 512), t(16, 16, 16, 512))),
        ('fwd/plain', lambda: S.conv_fwd(x(), w(), **fsets())),
        ('fwd/lazy', lambda: S.conv_fwd(x(), w(), **fsets(True))),
        ('fwd/stats', lambda: S.conv_fwd(x(), w(), stats_acc=acc(Co), **fsets(True))),
        ('fwd/bias_relu', lambda: S.conv_fwd(x(), w(), bias=t(Co), act=S.ACT_RELU, **fsets(True))),
        ('fwd/bias_lrelu', lambda: S.conv_fwd(x(), w(), bias=t(Co), act=S.ACT_LRELU, slope=0.1, **fsets(True))),
        ('fwd/pro', lambda: S.conv_fwd(x(), w(), stats_acc=acc(Co), pro=t(4, Ci), **fsets(True))),
        ('fwd/1x1', lambda: S.conv_fwd(x(), t(Co, Ci), taps=1, bias=t(Co), **fsets())),
        ('fwd/no_sets', lambda: S.conv_fwd(x(), w(), bias=t(Co))),
        ('dgrad/plain', lambda: S.conv_dgrad(dy(), t(Ci, 9 * Co), **dsets())),
        ('dgrad/lazy', lambda: S.conv_dgrad(dy(), lambda: t(Ci, 9 * Co), **dsets(True))),
        ('dgrad/bnb', lambda: S.conv_dgrad(dy(), lambda: t(Ci, 9 * Co), bnb=(x(), t(4, Ci), acc(Ci)), **dsets(True))),
        ('dgrad/bnp', lambda: S.conv_dgrad(dy(), lambda: t(Ci, 9 * Co), bnp=(t(Nb, 2 * H, 2 * H, Ci), t(4, Ci), acc(Ci)),
                                           **dsets(True))),
        ('dgrad/gate', lambda: S.conv_dgrad(dy(), lambda: t(Ci, 9 * Co), gate=x(), **dsets(True))),
        ('wgrad/plain', lambda: S.conv_wgrad(dy(), x())),
        ('wgrad/accumulate', lambda: S.conv_wgrad(dy(), x(), out=t(Co, 9 * Ci), accumulate=True)),
        ('wgrad/xpro', lambda: S.conv_wgrad(dy(), x(), xpro=t(4, Ci))),
        ('wgrad/1x1', lambda: S.conv_wgrad(dy(), x(), taps=1)),
        ('grp/conv', lambda: S.conv_fwd_grp(t(G, Nb, H, H, Ci), t(G, Co, 9 * Ci), bias=t(G, Co), act=S.ACT_RELU,
                                            wino=t(G, 16, Co, Ci), wino4=t(G, 36, Co, Ci))),
        ('grp/conv_shared', lambda: S.conv_fwd_grp(x(), t(G, Co, 9 * Ci), wino=t(G, 16, Co, Ci))),
        ('grp/conv_direct', lambda: S.conv_fwd_grp(x(), t(G, Co, 9 * Ci), bias=t(G, Co), act=S.ACT_LRELU)),
        ('grp/conv_pool', lambda: S.conv_fwd_grp(t(G, Nb, H, H, Ci), t(G, Co, 9 * Ci), bias=t(G, Co), act=S.ACT_RELU,
                                                 wino=t(G, 16, Co, Ci), wino4=t(G, 36, Co, Ci), pool=True)),
        ('grp/conv_pool_f2', lambda: S.conv_fwd_grp(t(G, Nb, 6, 6, Ci), t(G, Co, 9 * Ci), bias=t(G, Co),
                                                    act=S.ACT_RELU, wino=t(G, 16, Co, Ci), pool=True)),
        ('grp/linear', lambda: S.linear_grp(t(G, 64, 96), t(G, 40, 96), t(G, 40), act=S.ACT_RELU)),
        ('dense/fwd', lambda: S.linear(t(512, 1024), t(1024, 1024), t(1024), act=S.ACT_LRELU)),
        ('dense/dx', lambda: S.linear_dx(t(512, 1024), t(1024, 1024), gate=t(512, 1024))),
        ('dense/dw', lambda: S.linear_dw(t(500, 1024), t(500, 1024), out=t(1024, 1024), accumulate=True)),
        ('dense/small', lambda: S.linear(t(8, 32), t(10, 32), t(10))),
    ]


def _plain(a):
    return list(a) if isinstance(a, ctypes.Array) else a


def compute():
    """{case id: (seed key or None, shipped pick or None, key, cands, [trace lines of each candidate])}."""
    trace, grab = [], {}

    def pick(key, cands, run, protect=()):
        grab['kcr'] = (key, list(cands), run)
        return cands[0]

    def ptr(x):
        return None if x is None else 'P'
    with open(SEED) as f:
        seed = {autotune._tup(json.loads(k)): autotune._tup(v) for k, v in json.load(f).items()}
    cases = [('seed:' + hashlib.sha1(json.dumps(k).encode()).hexdigest()[:12], k, v,
              (lambda k=k: call_from_key(k))) for k, v in seed.items()]
    cases += [(name, None, None, fn) for name, fn in _extra_cases()]
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        for mod in (S, functional):
            mp.setattr(mod, '_p', ptr)
            mp.setattr(mod, '_s', lambda: 0)
        mp.setattr(_lib, 'call', lambda name, *a: trace.append(json.dumps([name] + [_plain(x) for x in a])))
        mp.setattr(S, '_pick', pick)
        for cid, skey, pick_, fn in cases:
            grab.clear()
            fn()
            key, cands, run = grab['kcr']
            lines = []
            for c in cands:
                del trace[:]
                run(c)
                lines.append(list(trace))
            assert cid not in out, cid
            out[cid] = (skey, pick_, key, cands, lines)
    return out


def digests(case):
    _, _, _, cands, lines = case
    h = hashlib.sha1()
    for c, ls in zip(cands, lines):
        h.update((json.dumps(c) + '\n' + '\n'.join(ls) + '\n').encode())
    return [hashlib.sha1(json.dumps(cands).encode()).hexdigest(), h.hexdigest()]


@pytest.fixture(scope='module')
def routes():
    return compute()


def test_every_seed_key_reproduces_and_its_pick_is_offered(routes):
    seeded = {cid: c for cid, c in routes.items() if c[0] is not None}
    assert len(seeded) == 408
    for cid, (skey, pick, key, cands, _) in seeded.items():
        assert key == skey, (skey, key)
        assert autotune._valid(pick, cands), (skey, pick)


def test_every_conv_route_id_is_offered_at_the_small_shape(routes):
    ids = {c[0] for cid in ('fwd/plain', 'wgrad/plain') for c in routes[cid][3] if c[0] < 0}
    assert ids == {-1, -2, -8, -9, -10, -12, -5, -6, -17, -18, -19, -14, -15, -3, -7, -13, -16}
    assert {c[0] for c in routes['dense/fwd'][3] if c[0] < 0} == {-21}


def test_candidates_and_launches_match_the_golden(routes):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(routes)
    bad = []
    for cid, case in routes.items():
        got = digests(case)
        if got != golden[cid]:
            what = 'candidates' if got[0] != golden[cid][0] else 'launches'
            print('{}: {} differ\n  key   {}\n  cands {}'.format(cid, what, case[2], case[3]))
            bad.append(cid)
    assert not bad, '{} of {} cases differ (see --dump / --diff in the module docstring): {}'.format(
        len(bad), len(routes), bad[:8])


def test_conv_sets_pass_each_kind_under_its_kwarg():
    from rafiki_amd.ops import autograd
    assert S.conv_sets(lambda kind: kind) == dict(wino='u2', wino4='u4', wino4p='u4p', wino4b='u4b')
    assert S.conv_sets(lambda kind: kind, dgrad=True) == dict(wino='ut2', wino4='ut4', wino4p='ut4p', wino4b='ut4b')
    w = t(8, 9 * 8)
    for dgrad in (False, True):   # the autograd layer: lazy producers, no blocked set, nothing for a 1x1 conv
        sets = autograd._wino_sets(w, w, 9, dgrad=dgrad)
        assert sets.pop('wino4b') is None and sorted(sets) == ['wino', 'wino4', 'wino4p']
        assert all(callable(v) for v in sets.values())
    assert autograd._wino_sets(w, w, 1) == {}


def _main(argv):
    routes = compute()
    if argv[:1] == ['--record']:
        os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
        with open(GOLDEN, 'w') as f:
            json.dump({cid: digests(c) for cid, c in routes.items()}, f, indent=0, sort_keys=True)
        print('{} cases, {} candidates -> {}'.format(len(routes), sum(len(c[3]) for c in routes.values()), GOLDEN))
    elif argv[:1] == ['--dump'] and len(argv) == 2:
        with open(argv[1], 'w') as f:
            json.dump({cid: [c[2], c[3], c[4]] for cid, c in routes.items()}, f)
    elif argv[:1] == ['--diff'] and len(argv) == 2:
        with open(argv[1]) as f:
            old = json.load(f)
        for cid, (_, _, key, cands, lines) in routes.items():
            okey, ocands, olines = old.get(cid, (None, [], []))
            new = [key, [list(c) for c in cands], lines]
            if json.loads(json.dumps(new)) == [okey, ocands, olines]:
                continue
            print('{}\n  key  {}\n  was  {}'.format(cid, key, okey))
            for i, c in enumerate(cands):
                if i >= len(ocands) or list(c) != ocands[i] or lines[i] != olines[i]:
                    print('  candidate {} {} (was {})'.format(i, c, ocands[i] if i < len(ocands) else None))
                    print('\n'.join('    new ' + ln for ln in lines[i]))
                    if i < len(olines):
                        print('\n'.join('    old ' + ln for ln in olines[i]))
                    break
            else:
                print('  {} candidates now, {} before'.format(len(cands), len(ocands)))
    else:
        sys.exit('usage: test_f32_routes.py --record | --dump FILE | --diff FILE')


if __name__ == '__main__':
    _main(sys.argv[1:])
