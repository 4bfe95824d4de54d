"""WinoWeights' buffer layout and refresh tables, pinned on the CPU (no GPU, no kernel library).

``rafiki_amd/ops/f32.py`` lays every Winograd weight set of a network out in one buffer and describes the
per-step transform launch (``rk_wino_weights_all``) by two tables: ``desc`` (one row per 32 x 32 filter block)
and ``meta`` (one row per layer and kernel family).  A mistake there makes the kernel write a set to the wrong
place, so this test records, for three networks and two live groups each:

* ``buf.numel()``, every ``(kind, layer) -> (offset, numel)`` and every view's shape and dtype;
* for the refresh launch, ``nblocks`` and the SHA-1 of the ``desc`` and of the ``meta`` bytes;

and compares them to ``tests/golden/wino_tables.json``.  The kernel launcher is replaced by a recorder that
keeps the tensors it is handed, as in test_wino_weights_logic.py.

``python tests/test_wino_tables.py --record`` rewrites the golden file.
"""
import hashlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from rafiki_amd.ops import f32 as S  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'wino_tables.json')
VGG = [(64, 8, 32), (64, 64, 32), (128, 64, 16), (128, 128, 16), (256, 128, 8), (256, 256, 8), (512, 256, 4),
       (512, 512, 4)]   # (Cout, Cin, hw) of the VGG-small training blocks
ODD = [(64, 32, 8), (16, 64, 6), (40, 24, 4)]   # the layers of test_wino_weights_logic.py
CONFIGS = {'vgg/dgrad': (VGG, True), 'vgg/fwd': (VGG, False), 'odd': (ODD, True)}
NARROW = (('u4', 0), ('ut2', 2))   # the group test_wino_weights_logic.py narrows to (those the network has)


def _sha(t):
    return hashlib.sha1(t.contiguous().numpy().tobytes()).hexdigest()


def _refresh(ww, calls):
    del calls[:]
    ww.refresh()
    (name, args), = calls
    assert name == 'rk_wino_weights_all'
    arena, buf, desc, nb, meta, _ = args
    assert arena is ww.arena and buf is ww.buf and desc.dtype == torch.int32 and meta.dtype == torch.int64
    return {'nblocks': int(nb), 'desc': _sha(desc), 'meta': _sha(meta)}


def compute():
    assert S.WINO and S.WINO4 and S.USE_X6P
    calls, out = [], {}
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(S._lib, 'call', lambda name, *a: calls.append((name, a)) or 0)
        mp.setattr(S, '_s', lambda: None)
        mp.setattr(S, '_p', lambda t: t)   # host tensors: the recorder keeps the tables themselves
        mp.setattr(torch.cuda, 'is_current_stream_capturing', lambda: False)
        for cid, (layers, dgrad) in CONFIGS.items():
            arena = torch.zeros(sum(co * 9 * ci for co, ci, _ in layers) + 3)
            ws, off = [], 3
            for co, ci, _ in layers:
                ws.append(arena[off:off + co * 9 * ci].view(co, 9 * ci))
                off += co * 9 * ci
            ww = S.WinoWeights(arena, ws, dgrad=dgrad, hw=[hw for _, _, hw in layers])
            sets = sorted(ww._sets, key=lambda kl: ww._sets[kl][0])
            rec = {'numel': ww.buf.numel(),
                   'sets': {'{}:{}'.format(*kl): list(ww._sets[kl]) for kl in sets},
                   'views': {'{}:{}'.format(*kl): [list(ww._view(*kl).shape), str(ww._view(*kl).dtype)] for kl in sets},
                   'refresh': {'full': _refresh(ww, calls)}}
            ww.end_step()
            narrow = [kl for kl in NARROW if ww.has(*kl)]
            for kl in narrow:
                ww.lazy(*kl)()
            ww.end_step()
            assert ww.live == frozenset(narrow)
            rec['refresh']['narrowed'] = dict(_refresh(ww, calls), live=['{}:{}'.format(*kl) for kl in narrow])
            out[cid] = rec
    return out


def test_layout_and_refresh_tables_match_the_golden():
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = json.loads(json.dumps(compute()))
    assert sorted(got) == sorted(golden)
    for cid in got:
        for field in ('numel', 'sets', 'views', 'refresh'):
            assert got[cid][field] == golden[cid][field], (cid, field)


if __name__ == '__main__':
    if sys.argv[1:] != ['--record']:
        sys.exit('usage: test_wino_tables.py --record')
    with open(GOLDEN, 'w') as f:
        json.dump(compute(), f, indent=1, sort_keys=True)
        f.write('\n')
    print('{} networks -> {}'.format(len(CONFIGS), GOLDEN))
