"""The ctypes binding table (rafiki_amd/ops/_lib.py) against the C declarations it binds (CPU).

ctypes converts each argument by its ``_SIGS`` row, not by the C prototype: a row that says ``c_int`` where the
launcher takes ``long long`` truncates a stride or byte count without any error.  So every ``extern "C"``
definition in csrc/kernels/*.hip is parsed here and compared with its row position by position.
"""
import ctypes as C
import re
from pathlib import Path

from rafiki_amd.ops import _lib

KERNELS = Path(__file__).resolve().parent.parent / 'csrc' / 'kernels'
# rk_* entry points that Python does not bind (called from another translation unit)
UNBOUND = {'rk_lrelu_gate_colsum4_f32'}
SCALARS = {'int': C.c_int, 'long long': C.c_longlong, 'unsigned': C.c_uint, 'unsigned int': C.c_uint,
           'unsigned long long': C.c_ulonglong, 'float': C.c_float, 'double': C.c_double}
_DEF = re.compile(r'extern\s+"C"\s+([\w\s]+?)\s*\b(rk_\w+)\s*\(([^)]*)\)\s*\{')


def _param_type(param):
    """'const float* x' -> 'pointer', 'long long gx' -> 'long long' (the parameter's name dropped)."""
    if '*' in param:
        return 'pointer'
    words = param.split()
    assert len(words) >= 2, param
    return ' '.join(w for w in words[:-1] if w != 'const')


def _declared():
    """[(name, return type, [parameter types])] of every extern "C" rk_* definition, duplicates kept."""
    out = []
    for src in sorted(KERNELS.glob('*.hip')):
        for ret, name, params in _DEF.findall(src.read_text()):
            params = [p.strip() for p in params.split(',')] if params.strip() not in ('', 'void') else []
            out.append((name, ' '.join(ret.split()), [_param_type(p) for p in params]))
    return out


def _matches(ctype, decl):
    if decl == 'pointer':
        return ctype is C.c_void_p or (isinstance(ctype, type) and issubclass(ctype, C._Pointer))
    return ctype is SCALARS.get(decl)   # a spelling that is not in SCALARS matches nothing


def _bound():
    """name -> (restype, argtypes) of everything lib() binds."""
    rows = {name: (C.c_int, args) for name, args in _lib._SIGS.items()}
    assert not set(rows) & set(_lib._RESTYPES)
    rows.update(_lib._RESTYPES)
    return rows


def test_parser_finds_the_entry_points():
    names = [d[0] for d in _declared()]
    assert len(names) >= len(_lib._SIGS), (len(names), len(_lib._SIGS))
    assert not [n for n in set(names) if names.count(n) > 1]


def test_every_binding_matches_its_declaration():
    decls = {}
    for name, ret, params in _declared():
        decls.setdefault(name, []).append((ret, params))
    bad = []
    for name, (restype, argtypes) in _bound().items():
        if len(decls.get(name, ())) != 1:
            bad.append('{}: defined {} times'.format(name, len(decls.get(name, ()))))
            continue
        ret, params = decls[name][0]
        if restype is not SCALARS.get(ret):
            bad.append('{}: returns {}, bound as {}'.format(name, ret, restype.__name__))
        if len(params) != len(argtypes):
            bad.append('{}: {} parameters, {} argtypes'.format(name, len(params), len(argtypes)))
            continue
        bad += ['{}: parameter {} is {}, bound as {}'.format(name, i, d, t.__name__)
                for i, (t, d) in enumerate(zip(argtypes, params)) if not _matches(t, d)]
    assert not bad, '\n'.join(bad)


def test_every_unbound_entry_point_is_listed():
    declared = {d[0] for d in _declared()}
    assert declared - set(_bound()) == UNBOUND
