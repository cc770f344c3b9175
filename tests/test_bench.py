"""bench.py: the plain run (headline only) and what --dump-outputs writes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT


def _bench(monkeypatch):
    monkeypatch.setenv('HSA_ENABLE_IPC_MODE_LEGACY', '0')      # (bench sets it at import; restored after the test)
    import bench
    return bench


@pytest.mark.parametrize('sample', [None, 17])
def test_dump_outputs_indexes_parameters_in_model_order(tmp_path, monkeypatch, sample):
    """params / grads are read in model.parameters() order whatever the flat-buffer layout; a model above DUMP_SAMPLE
    elements contributes one seeded position per stratum, the same on every call"""
    bench = _bench(monkeypatch)
    from imagecaptioning.pytorch_amd.flat import FlatParams
    if sample:
        monkeypatch.setattr(bench, 'DUMP_SAMPLE', sample)
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(5, 3), torch.nn.Linear(3, 2))
    flat = FlatParams(net)
    for n, p in zip(flat.names, flat.params):
        flat.grad_views[n].copy_(torch.randn(p.shape))
    want_p = torch.cat([p.detach().flatten() for p in net.parameters()]).numpy()
    want_g = torch.cat([flat.grad_views[n].flatten() for n in flat.names]).numpy()
    got = []
    for d in (tmp_path / 'a', tmp_path / 'b'):
        bench.dump_outputs(str(d), torch.tensor(1.5), {'loss': torch.tensor(1.5), 'reward': torch.tensor(0.25)}, flat)
        got.append({f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))})
    a, b = got
    assert set(a) == {'loss', 'out_reward', 'params', 'grads'}
    assert all(v.dtype == np.float32 for v in a.values())
    assert a['loss'].tolist() == [1.5] and a['out_reward'].tolist() == [0.25]
    assert all(np.array_equal(a[k], b[k]) for k in a)
    if sample is None:
        assert np.array_equal(a['params'], want_p) and np.array_equal(a['grads'], want_g)
    else:
        assert a['params'].shape == (sample,)
        pos = [int(np.flatnonzero(want_p == v)[0]) for v in a['params']]
        assert pos == sorted(set(pos)), 'one distinct position per stratum, in order'
        assert np.array_equal(a['grads'], want_g[pos])


@pytest.mark.gpu
def test_plain_bench_run_dumps_the_last_timed_step(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`: K timed steps, the headline line without the --full objects,
    and the last timed step's outputs as float32 .npy files (<= 64 MB) that agree with the line"""
    out = tmp_path / 'dump'
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--dump-outputs', str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line['steps'] == 3 and line['warmup'] == 1 and line['ms_per_step'] > 0 and line['value'] > 0
    assert line['unit'] == 'captions/s' and line['higher_is_better'] is True and line['dtype'] == 'f32'
    assert not {'roofline', 'cpu_baseline', 'other_configs', 'early_exit_eos_biased'} & set(line)
    files = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert set(files) == {'loss', 'out_reward', 'params', 'grads'}
    assert sum(os.path.getsize(out / (k + '.npy')) for k in files) <= 64 << 20
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in files.values())
    assert files['loss'][0] == np.float32(line['loss'])
    assert files['params'].size == files['grads'].size == 1 << 22
    assert np.abs(files['grads']).max() > 0
