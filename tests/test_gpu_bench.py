"""bench.py's plain run: exactly --steps timed steps, none of the --full records, and --dump-outputs writes what the timed
forward returned -- bit for bit what the same forward returns in this process on the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_steps_and_dumps_the_timed_outputs(tmp_path):
    B, J = 32, 17
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '7', '--warmup', '2', '--batch', str(B),
                        '--dump-outputs', str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line['steps'] == 7 and line['timing']['blocks'] == 1 and line['ms_per_step'] > 0
    assert not {'roofline', 'variants', 'config3', 'parity', 'cpu_baseline', 'clocks'} & set(line)
    verts, pose3d = np.load(tmp_path / 'verts.npy'), np.load(tmp_path / 'pose3d.npy')
    assert verts.shape == (B, 6890, 3) and pose3d.shape == (B, J, 3) and verts.dtype == np.float32

    import bench
    from gator_amd import synthetic
    model, _, _ = bench.build_model(J, 'fused', torch.device('cuda', 0))
    model.precision = 'f32'
    x = torch.from_numpy(synthetic.synthetic_pose2d(B, J, seed=1000)).cuda()      # bench.py's rank-0 input
    v, p = model(x)
    torch.cuda.synchronize()
    assert np.array_equal(v.cpu().numpy(), verts) and np.array_equal(p.cpu().numpy(), pose3d)
