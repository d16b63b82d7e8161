"""bench.py --dump-outputs (dump_outputs): file names, dtypes, the 64 MB budget and its fixed sample; and that --steps below 1
is refused before anything runs.  CPU only: the helper is fed host tensors."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location('bench_under_test', os.path.join(ROOT, 'bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_writes_whole_arrays_as_float32_or_float64(tmp_path):
    bench = _bench()
    g = torch.Generator().manual_seed(0)
    y = torch.rand(2, 3, 8, 8, generator=g)
    arrays = {'output': y, 'half': y.to(torch.bfloat16), 'frame': (y * 255).to(torch.uint8), 'loss_l_g_pix': 0.125,
              'wide': y.double()}
    bench.dump_outputs(str(tmp_path / 'out'), arrays)
    assert sorted(os.listdir(tmp_path / 'out')) == sorted(f'{k}.npy' for k in arrays)
    got = {k: np.load(tmp_path / 'out' / f'{k}.npy') for k in arrays}
    assert got['output'].dtype == np.float32 and got['output'].shape == (2, 3, 8, 8) and np.array_equal(got['output'], y.numpy())
    assert got['half'].dtype == np.float32 and np.array_equal(got['half'], y.to(torch.bfloat16).float().numpy())
    assert got['frame'].dtype == np.float32 and np.array_equal(got['frame'], (y * 255).to(torch.uint8).numpy().astype(np.float32))
    assert got['loss_l_g_pix'].dtype == np.float64 and got['loss_l_g_pix'].shape == () and float(got['loss_l_g_pix']) == 0.125
    assert got['wide'].dtype == np.float64 and np.array_equal(got['wide'], y.double().numpy())


def test_dump_over_budget_keeps_a_fixed_sample_within_it(tmp_path):
    bench = _bench()
    budget = 4096
    big = torch.arange(5000, dtype=torch.float32).reshape(5, 1000)
    small = torch.full((10,), 7.0)
    for run in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / run), {'big': big, 'small': small}, budget)
    files = [tmp_path / r / f for r in ('a', 'b') for f in ('big.npy', 'small.npy')]
    a, b = np.load(files[0]), np.load(files[2])
    assert np.array_equal(a, b)                                  # the same sample in every run
    assert a.dtype == np.float32 and a.ndim == 1 and 0 < a.size <= budget // 2 // 4
    assert np.all(np.diff(a) > 0) and np.all(np.isin(a, big.numpy()))  # sorted, distinct elements of the array
    assert np.array_equal(np.load(files[1]), small.numpy())     # under its share: written whole
    assert sum(np.load(f).nbytes for f in files[:2]) <= budget


def test_bench_refuses_fewer_than_one_step():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '0', '--no-secondary'], capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 2 and '--steps must be at least 1' in r.stderr, r.stderr[-2000:]
