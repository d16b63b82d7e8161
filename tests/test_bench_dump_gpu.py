"""bench.py --dump-outputs on the headline path: the dumped batch is what the 23-block network computes for the benchmark's seeded
input, and ``--steps`` is the number of timed forwards the line reports."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import image_restoration_amd as ira
from image_restoration_amd.utils import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_headline_dump_is_the_network_output(cuda, tmp_path):
    out = tmp_path / 'dump'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '3', '--warmup', '1', '--no-secondary',
                        '--no-cpu-baseline', '--dump-outputs', str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.strip()][-1])
    assert line['steps'] == 3 and line['warmup'] == 1
    assert os.listdir(out) == ['output.npy']
    y = np.load(out / 'output.npy')
    assert y.dtype == np.float32 and y.shape == (16, 3, 512, 512) and y.nbytes <= 64 << 20

    import bench
    net = ira.build_network(dict(type='RRDBNet', **bench.CFG)).to(cuda).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.rrdbnet_state_dict(0, **bench.CFG).items()}, strict=True)
    x = torch.from_numpy(synth.uniform_input(1234, (bench.BATCH, 3, bench.TILE, bench.TILE))).to(cuda)
    with torch.no_grad():
        ref = net(x).cpu().numpy()
    assert float(np.abs(y - ref).max()) <= 1e-5
