#!/usr/bin/env python3
"""Time the temporal evaluation (gator_amd.temporal: one-euro smoothing, acceleration error, MPJPE and PA-MPJPE of the smoothed sequence)
on two workloads:

  1. a test set of 24 videos x 1500 frames x 14 joints: the filter's launch, and the two launches of gator_sequence_errors as a pair;
  2. the filter alone on one 300-frame [T,6890,3] mesh sequence (a flicker-free overlay).

and the same work by the reference's host loop, restated here in numpy (lib/smooth_utils.py:14-72 frame by frame,
lib/coord_utils.py:194-222, data/PW3D/dataset.py:391-403 with the oracle's rigid_align): restated, not imported, because this tool also
runs where the reference tree is absent.

Device times are HIP events around a window of launches after one window of warm-up, the median of --reps windows; host times a host
clock, the median of --reps runs (1 run of the 36 000-frame loop).  From the filter's time follow the cycles per sequential step at
the clock the device reports: the kernel is one dependent chain of T steps whatever C and V.  Without a GPU the host figures are
written and every device figure is marked "not measured".  Not part of bench.py; no speed gate.

    python tools/temporal_bench.py [--reps 5] [--out profiles/temporal.txt]

The block it writes replaces the one under its marker line in --out and leaves the rest of that file alone."""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gator_amd import temporal  # noqa: E402
from oracle import gator_oracle as go  # noqa: E402

MARKER = '== timings: tools/temporal_bench.py =='
NOT_MEASURED = 'not measured'


class OneEuro:
    """lib/smooth_utils.py:14-46, as it stands there."""

    def __init__(self, t0, x0, min_cutoff, beta, d_cutoff=1.0):
        self.min_cutoff, self.beta, self.d_cutoff = float(min_cutoff), float(beta), float(d_cutoff)
        self.x_prev, self.dx_prev, self.t_prev = x0, 0.0, t0

    @staticmethod
    def factor(t_e, cutoff):
        r = 2 * math.pi * cutoff * t_e
        return r / (r + 1)

    def __call__(self, t, x):
        t_e = t - self.t_prev
        a_d = self.factor(t_e, self.d_cutoff)
        dx = (x - self.x_prev) / t_e
        dx_hat = a_d * dx + (1 - a_d) * self.dx_prev
        a = self.factor(t_e, self.min_cutoff + self.beta * np.abs(dx_hat))
        x_hat = a * x + (1 - a) * self.x_prev
        self.x_prev, self.dx_prev, self.t_prev = x_hat, dx_hat, t
        return x_hat


def host_smooth(pred, min_cutoff, beta):
    """lib/smooth_utils.py:49-72: one Python step per frame."""
    f = OneEuro(np.zeros_like(pred[0]), pred[0], min_cutoff, beta)
    out = np.zeros_like(pred)
    out[0] = pred[0]
    for idx, pose in enumerate(pred[1:]):
        idx += 1
        out[idx] = f(np.ones_like(pose) * idx, pose)
    return out


def host_block(pred, gt, lengths):
    """data/PW3D/dataset.py:391-413 -> (accel, MPJPE, PA-MPJPE)."""
    acc, mp, pa = [], [], []
    s = 0
    for T in lengths:
        p, g = host_smooth(pred[s:s + T], 0.004, 0.005), gt[s:s + T]
        s += T
        ag = g[:-2] - 2 * g[1:-1] + g[2:]
        ap = p[:-2] - 2 * p[1:-1] + p[2:]
        acc.append(np.mean(np.mean(np.linalg.norm(ap - ag, axis=2), axis=1)))
        mp.append(np.mean(np.sqrt(np.sum((p - g) ** 2, 2))))
        for i in range(len(p)):
            pa.append(np.sqrt(np.sum((go.rigid_align(p[i], g[i]) - g[i]) ** 2, 1)))
    return float(np.mean(acc)), float(np.mean(mp)), float(np.mean(pa))


def joints_set(V=24, T=1500, ne=14, seed=0):
    rs = np.random.RandomState(seed)
    g = np.concatenate([rs.randn(1, ne, 3) * 300.0 + np.cumsum(rs.randn(T, ne, 3) * 8.0, 0) for _ in range(V)])
    p = g * 1.03 + rs.randn(V * T, ne, 3) * 12.0
    return p.astype(np.float32), g.astype(np.float32), (T,) * V


def mesh_sequence(T=300, seed=1):
    rs = np.random.RandomState(seed)
    return (rs.randn(1, 6890, 3) * 400.0 + np.cumsum(rs.randn(T, 6890, 3) * 5.0, 0) + rs.randn(T, 6890, 3) * 3.0).astype(np.float32)


def reported_clock_mhz():
    """hipDeviceAttributeClockRate (the peak clock, kHz) of the current device, through the runtime the library is bound to."""
    import ctypes
    from gator_amd import _lib
    khz = ctypes.c_int(0)
    rc = _lib.load().hipDeviceGetAttribute(ctypes.byref(khz), 5, torch.cuda.current_device())      # 5: hipDeviceAttributeClockRate
    if rc != 0 or khz.value <= 0:
        raise RuntimeError('hipDeviceGetAttribute(ClockRate) failed (%d)' % rc)
    return khz.value / 1e3


def event_time(fn, iters, reps):
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def host_time(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), min(ts), max(ts)


def fmt(name, t):
    return '%-72s %s' % (name, NOT_MEASURED if t is None else '%12.4f ms   (%.4f .. %.4f)' % t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'temporal.txt'))
    a = ap.parse_args()
    gpu = torch.cuda.is_available()
    p, g, L = joints_set()
    mesh = mesh_sequence()
    F, V, T = len(p), len(L), L[0]
    p64, g64 = p.astype(np.float64), g.astype(np.float64)

    t_host_set = host_time(lambda: host_block(p64, g64, L), 1)
    t_host_smooth = host_time(lambda: [host_smooth(p64[v * T:(v + 1) * T], 0.004, 0.005) for v in range(V)], 1)
    m64 = mesh.astype(np.float64)
    t_host_mesh = host_time(lambda: host_smooth(m64, 0.004, 0.7), a.reps)
    want = host_block(p64, g64, L)

    t_euro = t_rows = t_reduce = t_mesh = None
    head, clock_mhz, worst = 'no GPU: device figures %s' % NOT_MEASURED, None, None
    if gpu:
        props = torch.cuda.get_device_properties(0)
        clock_mhz = reported_clock_mhz()
        head = '%s (%s), torch %s, reported clock %.0f MHz' % (torch.cuda.get_device_name(0), getattr(props, 'gcnArchName', '?'), torch.__version__, clock_mhz)
        pd, gd = torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda()
        seg = torch.from_numpy(np.arange(V + 1, dtype=np.int64) * T).cuda()
        _, _, summ = temporal.sequence_errors(pd, gd, lengths=L)
        got = (summ['accel'], summ['MPJPE'], summ['PA-MPJPE'])
        worst = max(abs(x - y) / abs(y) for x, y in zip(got, want))
        x = pd.reshape(F, -1).contiguous()
        sm = torch.empty(x.shape, device='cuda', dtype=torch.float64)
        rows = torch.empty((F, 3), device='cuda', dtype=torch.float64)
        sums = torch.empty((V, 6), device='cuda', dtype=torch.float64)
        t_euro = event_time(lambda: temporal._launch_one_euro(x, seg, V, 0.004, 0.005, 1.0, 1.0, sm), 10, a.reps)
        smj = sm.reshape(F, -1, 3)
        t_rows = event_time(lambda: temporal._launch_sequence_errors(smj, gd, None, seg, V, rows, sums), 10, a.reps)
        # gator_sequence_errors queues its two kernels in one call, so events see them as a pair; the same call on 3 frames per video
        # shows what of the pair's time is launch floor
        tiny_seg = torch.from_numpy(np.arange(V + 1, dtype=np.int64) * 3).cuda()
        t_reduce = event_time(lambda: temporal._launch_sequence_errors(smj[:3 * V], gd[:3 * V], None, tiny_seg, V, rows, sums), 10, a.reps)
        md = torch.from_numpy(mesh).cuda().reshape(len(mesh), -1)
        mseg = torch.tensor([0, len(mesh)], dtype=torch.int64, device='cuda')
        mo = torch.empty(md.shape, device='cuda', dtype=torch.float64)
        t_mesh = event_time(lambda: temporal._launch_one_euro(md, mseg, 1, 0.004, 0.7, 1.0, 1.0, mo), 10, a.reps)
        mref = host_smooth(m64[:, :64], 0.004, 0.7)
        assert np.array_equal(mo.cpu().numpy().reshape(m64.shape)[:, :64], mref), 'the mesh filter differs from the host loop'

    def cycles(t, steps):
        return NOT_MEASURED if t is None else '%.0f cycles per step (%d sequential steps, %.3f us each)' % (t[0] * 1e-3 * clock_mhz * 1e6 / steps, steps, t[0] * 1e3 / steps)

    lines = [MARKER, head,
             'Device: HIP events around a window of 10 launches after one window of warm-up, median (min .. max) of %d windows.' % a.reps,
             'Host: the reference-style numpy loop restated in the tool, host clock, fp64 arrays already on the host.',
             '',
             'workload 1: %d videos x %d frames x 14 joints (min_cutoff 0.004, beta 0.005)' % (V, T),
             fmt('  k_one_euro<double>, [%d, 42] float32 -> float64' % F, t_euro),
             '      ' + cycles(t_euro, T - 1),
             fmt('  k_seq_errors<double> + k_seq_reduce (gator_sequence_errors, two launches)', t_rows),
             fmt('  the same call on %d videos x 3 frames (launch floor of the pair)' % V, t_reduce),
             fmt('  host: smooth_pose loop alone', t_host_smooth),
             fmt('  host: the whole block (smooth, accel, MPJPE, PA-MPJPE per frame)', t_host_set),
             '  worst relative difference of the three averages, device vs host loop: %s' % (NOT_MEASURED if worst is None else '%.2e' % worst),
             '',
             'workload 2: the filter alone on one %d-frame [T,6890,3] mesh sequence (min_cutoff 0.004, beta 0.7)' % len(mesh),
             fmt('  k_one_euro<double>, [%d, 20670] float32 -> float64' % len(mesh), t_mesh),
             '      ' + cycles(t_mesh, len(mesh) - 1),
             fmt('  host: smooth_pose loop', t_host_mesh)]
    if gpu:
        lines.append('  the first 64 channels of the device result equal the host loop bit for bit')
    for ln in lines:
        print(ln, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    head_text = open(a.out).read().split(MARKER)[0] if os.path.exists(a.out) else ''
    with open(a.out, 'w') as fh:
        fh.write(head_text + '\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
