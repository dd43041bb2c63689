"""bench.py's contract beside its headline: a plain run times exactly the K steps it is given and nothing else (every other leg is
behind --full), and --dump-outputs writes what the last timed step handed its caller as small float32 / float64 .npy files."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_KEYS = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step', 'steps', 'warmup', 'final_loss')
FULL_ONLY_KEYS = ('ms_per_step_median', 'roofline', 'roofline_by_class', 'op_time_ms', 'fit_e2e', 'configs', 'cpu_baseline')


def _dump(tmp, name, monkeypatch, logits):
    import bench
    from salt_amd import architectures as A
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: None)      # the CPU model: nothing in flight
    torch.manual_seed(0)
    net = A.UNetResNet(34, 2, use_hypercolumn=True, dropout_2d=0.0, pretrained=False)
    path = os.path.join(str(tmp), name)
    names = bench.dump_outputs(path, types.SimpleNamespace(model=net), types.SimpleNamespace(logits=logits), 0.25)
    return path, names


def test_dump_outputs_writes_small_seeded_float_arrays(tmp_path, monkeypatch):
    logits = torch.randn(4, 2, 128, 128, generator=torch.Generator().manual_seed(3))
    p1, names = _dump(tmp_path, 'a', monkeypatch, logits)
    p2, _ = _dump(tmp_path, 'b', monkeypatch, logits)
    assert sorted(os.listdir(p1)) == sorted(n + '.npy' for n in names) == ['logits.npy', 'loss.npy', 'param_norms.npy', 'params_sample.npy']
    total = 0
    for f in os.listdir(p1):
        a, b = np.load(os.path.join(p1, f)), np.load(os.path.join(p2, f))
        assert a.dtype in (np.float32, np.float64), f
        assert np.array_equal(a, b), f                                     # same model, same seed: the same sample
        total += os.path.getsize(os.path.join(p1, f))
    assert total <= 64 << 20
    assert np.array_equal(np.load(os.path.join(p1, 'logits.npy')), logits.numpy())
    assert np.load(os.path.join(p1, 'loss.npy')).tolist() == [0.25]
    import bench
    assert np.load(os.path.join(p1, 'params_sample.npy')).shape == (bench.DUMP_PARAM_SAMPLE,)


def test_dump_outputs_samples_logits_above_the_cap(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, 'DUMP_LOGITS_MAX', 1000)
    logits = torch.arange(4 * 2 * 64 * 64, dtype=torch.float32).reshape(4, 2, 64, 64)
    p, _ = _dump(tmp_path, 'c', monkeypatch, logits)
    lg = np.load(os.path.join(p, 'logits.npy'))
    assert lg.shape == (1000,) and lg.dtype == np.float32
    assert np.all(np.diff(lg) > 0) and np.array_equal(lg, np.floor(lg))     # distinct elements of the array, in storage order


def test_bench_has_full_and_dump_outputs_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--help'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert '--full' in r.stdout and '--dump-outputs' in r.stdout


@pytest.mark.gpu
def test_plain_bench_times_the_requested_steps_and_dumps_them(tmp_path):
    out_dir = str(tmp_path / 'dump')
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--dump-outputs', out_dir],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert all(k in out for k in HEADLINE_KEYS), sorted(out)
    assert not any(k in out for k in FULL_ONLY_KEYS), sorted(out)
    assert out['steps'] == 3 and out['warmup'] == 1 and out['unit'] == 'images/s' and out['higher_is_better'] is True
    assert out['ms_per_step'] > 0 and abs(out['value'] - 32 * 1e3 / out['ms_per_step']) <= 1e-2 * out['value']
    files = sorted(os.listdir(out_dir))
    assert files == ['logits.npy', 'loss.npy', 'param_norms.npy', 'params_sample.npy']
    for f in files:
        a = np.load(os.path.join(out_dir, f))
        assert a.dtype in (np.float32, np.float64) and np.all(np.isfinite(a)), f
    assert np.load(os.path.join(out_dir, 'logits.npy')).shape == (32, 2, 128, 128)
    assert abs(float(np.load(os.path.join(out_dir, 'loss.npy'))[0]) - out['final_loss']) <= 1e-5
