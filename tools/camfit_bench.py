#!/usr/bin/env python3
"""Time the demo's camera fit (1500 Adam steps, demo/run.py:123-164) on the GPU: the fused device fit (gator_fit_camera_f32) at several
batch sizes against the demo's own torch loop over models.project_net at B = 1 and the same loop with a batched [B,3] parameter.
HIP events around each call after warm-up; the median of --reps calls.  Not part of bench.py; no speed gate.

    python tools/camfit_bench.py [--reps 5] [--out profiles/r07_camfit.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gator_amd import camera, models  # noqa: E402

STEPS = 1500


def batch(B, seed=0, nj=17):
    rs = np.random.RandomState(seed)
    tg = 250 + (rs.rand(B, nj, 2) - 0.5) * 300
    s = rs.uniform(0.7, 1.2, (B, 1, 1))
    p = (tg - 250) / (s * 250) + rs.randn(B, nj, 2) * 0.03
    j3 = np.concatenate([p, rs.randn(B, nj, 1) * 0.1], 2)
    return (torch.from_numpy(j3.astype(np.float32)).cuda(), torch.from_numpy(tg.astype(np.float32)).cuda(),
            torch.from_numpy(rs.rand(B, 3).astype(np.float32)).cuda())


def timed(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def torch_loop(layer, p, t):
    """demo/run.py:135-157 as it is (nn.L1Loss over the whole batch, torch.optim.Adam, the demo's schedule)."""
    crit = torch.nn.L1Loss()
    opt = torch.optim.Adam(layer.parameters(), lr=0.1)
    for j in range(STEPS):
        loss = crit(layer(p), t)
        opt.zero_grad()
        loss.backward()
        opt.step()
        if j == 500:
            for g in opt.param_groups:
                g['lr'] = 0.05
        if j == 1000:
            for g in opt.param_groups:
                g['lr'] = 0.001


class BatchedCamLayer(models.project_net.OptimzeCamLayer):
    """OptimzeCamLayer with a [B,3] parameter: one camera per sample, one loss over the batch."""
    def __init__(self, crop_size, B):
        super().__init__(crop_size)
        self.cam_param = torch.nn.Parameter(torch.rand((B, 3)))

    def forward(self, pose3d):
        output = pose3d[:, :, :2] + self.cam_param[:, None, 1:]
        return output * self.cam_param[:, None, :1] * self.img_res + self.img_res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'r07_camfit.txt'))
    a = ap.parse_args()
    dev = torch.cuda.get_device_name(0)
    rows = []
    for B in (1, 256, 4096, 65536):
        p, t, i = batch(B)
        ms = timed(lambda: camera.fit_camera(p, t, init=i), a.reps)
        rows.append(('fused device fit (gator_fit_camera_f32)', B, ms))
        print(rows[-1], flush=True)
    p, t, _ = batch(1)
    layer = models.project_net.get_model(crop_size=500).cuda()
    ms = timed(lambda: torch_loop(layer, p, t[:, :17]), max(1, a.reps // 2))
    rows.append(('demo torch loop, [1,3] parameter', 1, ms))
    print(rows[-1], flush=True)
    p, t, _ = batch(256)
    layer = BatchedCamLayer(500, 256).cuda()
    ms = timed(lambda: torch_loop(layer, p, t), max(1, a.reps // 2))
    rows.append(('torch loop, batched [B,3] parameter', 256, ms))
    print(rows[-1], flush=True)
    lines = ['camera fit, %d Adam steps per sample (demo/run.py:123-164), %s, torch %s' % (STEPS, dev, torch.__version__),
             'HIP events around each call after one warm-up call; median of %d calls (torch loops: %d)' % (a.reps, max(1, a.reps // 2)),
             '', '%-42s %7s %12s %14s' % ('form', 'B', 'ms / call', 'us / sample')]
    for name, B, ms in rows:
        lines.append('%-42s %7d %12.3f %14.3f' % (name, B, ms, ms * 1e3 / B))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
