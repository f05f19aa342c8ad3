#!/usr/bin/env python3
"""Time the detector noise: gator_amd.noise.noisy_input on the device at B = 64 and 1024 (both models), and -- when the reference tree is
given -- the reference's own host function lib/noise_utils.synthesize_pose on this machine's CPU, one thread, per sample.

  python tools/noise_bench.py [--reference <tree>] [--out profiles/detector_noise.txt] [--iters 50]

Each part that cannot run here (no HIP device, no reference tree) is written as "not measured", never filled in.  The speed-up line is
written only when both parts ran in this one process, on this one machine."""
import argparse
import os
import platform
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tests import noise_refs as nr  # noqa: E402


def poses(B, seed=0):
    rs = np.random.RandomState(seed)
    return np.stack([nr.coco_pose(rs, scale=rs.uniform(1.0, 5.0), centre=rs.uniform(200, 800, 2), pelvis_neck=True) for _ in range(B)])


def device_part(iters):
    try:
        import torch
        if not torch.cuda.is_available():
            return None, ['device: not measured (no HIP device in this process)']
        from gator_amd import noise
    except Exception as e:  # noqa: BLE001
        return None, ['device: not measured (%s)' % e]
    rs = np.random.RandomState(1)
    lines, per_call = ['device: %s, median of %d calls timed with events after 10 warm-up calls' % (torch.cuda.get_device_name(0), iters)], {}
    table = np.abs(rs.randn(17, 5)) + 0.5
    table[:, 4] = rs.uniform(0.5, 1.0, 17)
    models = {'coco': (noise.CocoDetectorNoise(), 19, nr.COCO_FLIP_PAIRS), 'stats': (noise.ErrorStatsNoise(table[:, :2], table[:, 2:4], table[:, 4]), 17, nr.H36M_FLIP_PAIRS)}
    for name, (model, J, pairs) in models.items():
        for B in (64, 1024):
            x = torch.from_numpy(poses(B)[:, :J]).cuda()
            rot = torch.from_numpy((rs.rand(B) * 60 - 30).astype(np.float32)).cuda()
            flip = torch.from_numpy((rs.rand(B) < 0.5).astype(np.int32)).cuda()
            step = torch.zeros(1, dtype=torch.int64, device='cuda')
            ms = []
            for i in range(iters + 10):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                step.add_(1)
                a.record()
                noise.noisy_input(x, model, seed=3, step=step, rot_deg=rot, flip=flip)
                b.record()
                b.synchronize()
                if i >= 10:
                    ms.append(a.elapsed_time(b))
            med = statistics.median(ms)
            per_call[(name, B)] = med
            lines.append('  %-5s B = %4d   %8.3f ms per call (min %.3f, max %.3f)   %9.0f samples/s' % (name, B, med, min(ms), max(ms), B / med * 1e3))
    return per_call, lines


def host_part(ref_root, n=40):
    if not ref_root:
        return None, ["reference's host function: not measured (no reference tree given)"]
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    import gen_golden_noise
    synthesize_pose, _ = gen_golden_noise.reference_functions(ref_root)
    p = poses(n, seed=2)[:, :17]
    joints = np.concatenate([p, np.ones((n, 17, 1), np.float32)], 2)
    areas = [float(np.prod(q.max(0) - q.min(0))) for q in p]
    synthesize_pose(joints[0].copy(), areas[0])
    t = time.perf_counter()
    for q, a in zip(joints, areas):
        synthesize_pose(q.copy(), a)
    ms = (time.perf_counter() - t) / n * 1e3
    return ms, ["reference's host function: lib/noise_utils.synthesize_pose, numpy %s on %s, one process: %.2f ms per sample (mean of %d), "
                '%.0f ms for a batch of 64, %.0f ms for 1024' % (np.__version__, platform.processor() or platform.machine(), ms, n, ms * 64, ms * 1024)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=None)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'detector_noise.txt'))
    ap.add_argument('--iters', type=int, default=50)
    args = ap.parse_args()
    dev, dev_lines = device_part(args.iters)
    host, host_lines = host_part(args.reference)
    lines = ['detector noise (tools/noise_bench.py)', ''] + dev_lines + [''] + host_lines + ['']
    if dev and host:
        for B in (64, 1024):
            lines.append('speed-up of the coco model over the host function on this machine, B = %4d: %.0fx' % (B, host * B / dev[('coco', B)]))
    else:
        lines.append('speed-up on one machine: not measured (the two parts did not run in one process)')
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(text)
    print(text)


if __name__ == '__main__':
    main()
