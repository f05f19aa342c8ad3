#!/usr/bin/env python3
"""Figures of the SMPL fit (SMPLLayer.fit, csrc/smpl_fit.hip) for profiles/smpl_fit.txt.

  python tools/smpl_fit_bench.py --host     no GPU needed: the float32 floor of the reference (tests/smpl_fit_refs.float32_floor, host
                                            test 4: the margins the device bounds are set from) and the time of the numpy float64
                                            reference fit at NV = 6890, one sample, 20 iterations, on this CPU
  python tools/smpl_fit_bench.py            on the GPU, NV = 6890 (synthetic model of SMPL's dimensions), B = 1 / 64 / 256, iters = 20:
                                            the whole fit call, the stage entry (k_smpl_pose + k_smpl_fit_normal + k_smpl_fit_reduce:
                                            one evaluation of M) and the layer's forward on the same batch

Method (GPU): device events around a window of back-to-back calls after warm-up of the same shape, the number of calls chosen so that a
window lasts about half a second; three windows, the median and the spread.  Rates are whole-call figures: the stage's
2 * N * N * 3 * NV FLOP per sample (N = 96; the kernel computes the 6 upper tiles of 9, so it executes 2/3 of that) over the stage
entry's time, against the 157.3 TFLOP/s fp32-matrix peak.  A kernel-only time wants a kernel trace in a run of its own."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import smpl_fit_refs as fr  # noqa: E402
from tests import smpl_refs as sr  # noqa: E402

PEAK_F32_MATRIX = 157.3e12
NV, ITERS = 6890, 20


def big_case(B):
    m = sr.synthetic_model(NV, 24, 10, 16)
    rs = np.random.RandomState(77)
    ax = rs.randn(B, 24, 3)
    ax /= np.linalg.norm(ax, axis=-1, keepdims=True)
    pose = (ax * rs.uniform(0, 0.8, (B, 24, 1))).reshape(B, 72).astype(np.float32)
    return m, (pose, rs.randn(B, 10).astype(np.float32), rs.randn(B, 3).astype(np.float32))


def host():
    print('reference side (numpy, no device) -- host test 4 of tests/test_host_smpl_fit_refs.py')
    print('  e32 = rms of (float32 forward - float64 forward) at the true parameters; rms = the float32-emulated fit of %d iterations,' % fr.ITERS)
    print('  evaluated by the float64 lbs_forward against the target (metres)')
    rows, ratio, excess = fr.float32_floor()
    for label, e32, rms in rows:
        print('  %-14s e32 %.3e   rms %.9e   rms / e32 %.3f' % (label, e32, rms, rms / e32))
    print('  largest rms / e32 over the case table: %.4f   ->  K_FLOOR = 2 x = %.4f (tests/smpl_fit_refs.py holds %.4f)' % (ratio, 2 * ratio, fr.K_FLOOR))
    print('  noisy target (5 mm): rms32 / rms64 - 1 = %.3e   ->  EPS_NOISY = 10 x |.| = %.3e (tests/smpl_fit_refs.py holds %.3e)'
          % (excess, 10 * abs(excess), fr.EPS_NOISY))
    m, truth = big_case(1)
    tgt, _ = sr.lbs_forward(m, *truth)
    t0 = time.perf_counter()
    st, rms = fr.fit(m, tgt[0], None, ITERS)
    dt = time.perf_counter() - t0
    print('  numpy float64 reference fit, NV %d, 1 sample, %d iterations, this CPU (%d threads available): %.2f s, final rms %.3e m'
          % (NV, ITERS, os.cpu_count() or 1, dt, rms))


def time_calls(fn, torch, min_window=0.5, windows=3):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    n = max(3, int(min_window / max((time.perf_counter() - t0) / 3, 1e-6)))
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3 / n)
    return statistics.median(out), min(out), max(out), n


def gpu(batches):
    import torch
    from gator_amd import smpl
    if not torch.cuda.is_available():
        raise SystemExit('smpl_fit_bench: no HIP device (a timing needs the GPU; --host gives the reference-side figures)')
    m, truth = big_case(max(batches))
    layer = smpl.SMPLLayer.from_arrays(m['v_template'], m['shapedirs'], m['posedirs'], m['weights'], m['J_regressor'], m['parents'])
    P, N = layer.fit_width()
    dev = [torch.from_numpy(a).cuda() for a in truth]
    target, _ = layer(*dev)
    print('device: %s   model: NV %d NJ 24 NB 10 (synthetic)   P %d N %d   iters %d' % (torch.cuda.get_device_name(0), NV, P, N, ITERS))
    print('%5s %14s %12s %16s %16s %14s %14s' % ('B', 'fit ms/call', 'fits/s', 'stage us/call', 'stage of fp32 mx', 'forward us', 'max rms (m)'))
    for B in batches:
        x = target[:B].contiguous()
        a = [t[:B].contiguous() for t in dev]
        rms = layer.fit(x, iters=ITERS)[3]
        t, lo, hi, n = time_calls(lambda: layer.fit(x, iters=ITERS), torch)
        ts, slo, shi, ns = time_calls(lambda: layer.fit_normal(a[0], a[1], a[2], x), torch)
        tf, flo, fhi, nf = time_calls(lambda: layer(*a), torch)
        flop = B * 2.0 * N * N * 3 * NV
        print('%5d %14.3f %12.0f %16.1f %15.1f%% %14.1f %14.3e   (windows of %d / %d / %d calls; fit %.3f..%.3f ms, stage %.1f..%.1f us, forward %.1f..%.1f us)'
              % (B, t * 1e3, B / t, ts * 1e6, 100 * flop / ts / PEAK_F32_MATRIX, tf * 1e6, float(rms.max()), n, ns, nf, lo * 1e3, hi * 1e3,
                 slo * 1e6, shi * 1e6, flo * 1e6, fhi * 1e6), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--host', action='store_true', help='the reference-side figures only (no GPU)')
    ap.add_argument('--batches', default='1,64,256')
    a = ap.parse_args()
    if a.host:
        host()
    else:
        gpu([int(b) for b in a.batches.split(',')])


if __name__ == '__main__':
    main()
