"""bench.py's command line: a plain run measures the headline only (``--full`` adds the other phases) and
``--dump-outputs DIR`` writes the last timed step's arrays as float32 / float64 ``.npy`` files."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def bench():
    spec = importlib.util.spec_from_file_location('rafiki_bench_cli', os.path.join(ROOT, 'bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_full_and_dump_are_off_by_default(bench, monkeypatch):
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '7', '--warmup', '2'])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--full', '--dump-outputs', 'somewhere'])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == 'somewhere'


def test_dump_outputs_writes_float_arrays(bench, tmp_path):
    arrays = {'w': torch.arange(6, dtype=torch.float32).reshape(2, 3),
              'count': torch.tensor([5], dtype=torch.int32),
              'half': torch.tensor([0.5, -1.25], dtype=torch.bfloat16),
              'wide': torch.tensor([1.0 + 2.0 ** -40], dtype=torch.float64)}
    d = str(tmp_path / 'out')
    assert bench.dump_outputs(d, arrays) == sorted(arrays)
    assert sorted(os.listdir(d)) == sorted(n + '.npy' for n in arrays)
    w = np.load(os.path.join(d, 'w.npy'))
    assert w.dtype == np.float32 and w.shape == (2, 3) and np.array_equal(w, np.arange(6).reshape(2, 3))
    c = np.load(os.path.join(d, 'count.npy'))
    assert c.dtype == np.float32 and c.tolist() == [5.0]
    h = np.load(os.path.join(d, 'half.npy'))
    assert h.dtype == np.float32 and h.tolist() == [0.5, -1.25]
    wide = np.load(os.path.join(d, 'wide.npy'))
    assert wide.dtype == np.float64 and wide[0] == 1.0 + 2.0 ** -40


def test_dump_outputs_samples_the_same_elements_within_the_budget(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_BUDGET_BYTES', 4096)
    big = torch.arange(10000, dtype=torch.float32).reshape(100, 100)
    arrays = {'big': big, 'small': torch.tensor([1.0, 2.0, 3.0])}
    got = []
    for sub in ('a', 'b'):
        d = str(tmp_path / sub)
        bench.dump_outputs(d, arrays)
        got.append({n: np.load(os.path.join(d, n + '.npy')) for n in arrays})
    a, b = got
    assert a['small'].tolist() == [1.0, 2.0, 3.0]
    assert a['big'].dtype == np.float32 and a['big'].ndim == 1
    assert sum(v.nbytes for v in a.values()) <= 4096
    assert a['big'].size == 4096 // 2 // 4                     # an equal share of the budget
    assert np.all(np.diff(a['big']) > 0) and a['big'].max() < 10000   # distinct elements, in order
    assert np.array_equal(a['big'], b['big'])                   # the same sample in every run


@pytest.mark.gpu
def test_plain_bench_run_measures_the_headline_only_and_dumps(tmp_path):
    d = str(tmp_path / 'dump')
    env = dict(os.environ, WORKDIR_PATH=str(tmp_path / 'workdir'))
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1',
                        '--dataset-size', '2048', '--dump-outputs', d], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out['steps'] == 3 and out['warmup'] == 1 and out['full'] is False
    assert out['unit'] == 'images/s' and out['higher_is_better'] is True and out['dtype'] == 'fp32'
    assert out['ms_per_step'] > 0
    assert abs(out['value'] - 256 * 1000.0 / out['ms_per_step']) <= 0.01 * out['value']
    for k in ('trials_per_hour_measured', 'probe_trials_per_hour', 'ensemble_qps', 'baseline_configs'):
        assert k not in out
    files = sorted(os.listdir(d))
    assert files == sorted(n + '.npy' for n in out['dumped_outputs']['arrays'])
    assert {'params.npy', 'grads.npy', 'bn_running.npy', 'loss_sum.npy', 'seen.npy'} <= set(files)
    arrs = {f: np.load(os.path.join(d, f)) for f in files}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 * 10 ** 6
    assert arrs['seen.npy'].tolist() == [3 * 256]               # the counters cover the timed steps only
    assert np.count_nonzero(arrs['grads.npy']) > 0 and np.count_nonzero(arrs['params.npy']) > 0
