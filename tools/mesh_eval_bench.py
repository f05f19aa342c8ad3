#!/usr/bin/env python3
"""Time the whole-mesh evaluation of a batch (MPJPE, PA-MPJPE, SMPL-joint MPJPE, MPVPE, PA-MPVPE per sample) three ways, at B = 64 and
256, N = 6890, on the GPU:

  a. gator_mesh_errors_f32, one launch (regressors, index list and output allocated beforehand);
  b. the same numbers from what the device had before it: JointRegressor, joint_errors, eval.mpvpe (a batch mean), the SMPL-joint
     error in torch ops, and a batched float64 torch.linalg.svd for the mesh fit;
  c. the reference's host loop restated in numpy (lib/core/base.py:233 copies both meshes to the host, data/PW3D/dataset.py:337-375
     walks the samples; the Procrustes step on the mesh that :360-361 comment out is included, since a. and b. compute it).

a. and b. are timed with HIP events around a window of launches after warm-up, the median of --reps windows; c. with a host clock
around the copies and the loop, the median of --reps runs.  The three sets of numbers are compared before anything is timed.
Not part of bench.py; no speed gate.  A run without a GPU fails: there is nothing to measure.

    python tools/mesh_eval_bench.py [--reps 5] [--out profiles/mesh_eval.txt]

The block it writes replaces the one under its marker line in --out and leaves the rest of that file alone."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gator_amd import eval as geval  # noqa: E402
from oracle import gator_oracle as go  # noqa: E402

MARKER = '== timings: tools/mesh_eval_bench.py =='
N = geval.N_VERTS


def sparse_rows(rs, n_joint, per_row):
    d = np.zeros((n_joint, N), np.float32)
    for j in range(n_joint):
        w = rs.rand(per_row) + 0.1
        d[j, rs.choice(N, per_row, replace=False)] = (w / w.sum()).astype(np.float32)
    return d


def batch(B, seed=0):
    """Meshes in metres, errors of a few cm; the shipped regressors' shapes (24 x 6890 with 5, 17 x 6890 with 6 weights per row)."""
    rs = np.random.RandomState(seed)
    t = rs.randn(B, N, 3) * 0.4 + rs.uniform(-1.0, 1.0, (B, 1, 3))
    p = 1.02 * t + rs.randn(B, 1, 3) * 0.03 + rs.randn(B, N, 3) * 0.04
    return (torch.from_numpy(p.astype(np.float32)).cuda(), torch.from_numpy(t.astype(np.float32)).cuda(),
            sparse_rows(rs, 24, 5), sparse_rows(rs, 17, 6))


def event_time(fn, iters, reps):
    """ms per call: HIP events around `iters` calls, the median of `reps` windows, after one window of warm-up."""
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


def torch_pa_mpvpe(pm, tm):
    """lib/coord_utils.py:127-149 on every sample at once, float64 on the device: [B] mean |aligned - target|."""
    a, b = pm.double(), tm.double()
    ca, cb = a.mean(1, keepdim=True), b.mean(1, keepdim=True)
    a0, b0 = a - ca, b - cb
    H = torch.einsum('bnr,bnc->brc', a0, b0) / N
    U, S, Vh = torch.linalg.svd(H)
    R = Vh.transpose(1, 2) @ U.transpose(1, 2)
    neg = torch.linalg.det(R) < 0
    S = torch.where(neg[:, None], S * torch.tensor([1.0, 1.0, -1.0], device=S.device, dtype=S.dtype), S)
    Vh = torch.where(neg[:, None, None], Vh * torch.tensor([[1.0], [1.0], [-1.0]], device=S.device, dtype=S.dtype), Vh)
    R = Vh.transpose(1, 2) @ U.transpose(1, 2)
    c = S.sum(1) / (a0 ** 2).sum((1, 2)) * N
    al = c[:, None, None] * (a0 @ R.transpose(1, 2)) + cb
    pa = torch.sqrt(((al - b) ** 2).sum(2)).mean(1)
    return pa


def torch_ops(P, T, Jr, Je):
    """b.: [B,5], column 3 filled with eval.mpvpe's batch mean."""
    pm, tm = P * 1000.0, T * 1000.0
    jp, jt = Jr(pm), Jr(tm)
    e = geval.joint_errors(Je(pm), Je(tm))
    smpl = torch.sqrt((((jp - jp[:, :1]) - (jt - jt[:, :1])) ** 2).sum(2)).mean(1)
    mp = geval.mpvpe(pm, tm, jp, jt)
    pa = torch_pa_mpvpe(pm, tm)
    return torch.stack([e[:, 0], e[:, 1], smpl, mp.expand_as(smpl), pa.float()], 1)


def host_loop(P, T, jr, je, ev):
    """c.: both meshes to the host (lib/core/base.py:219,233), then data/PW3D/dataset.py:337-375 per sample, in numpy as it is there."""
    pm, tm = (P * 1000).cpu().numpy(), (T * 1000).cpu().numpy()
    out = np.empty((len(pm), 5))
    for n in range(len(pm)):
        mo, mg = pm[n], tm[n]
        jo, jg = np.dot(jr, mo), np.dot(jr, mg)
        co = np.concatenate((mo, jo))
        co = co - co[N]
        cg = np.concatenate((mg, jg))
        cg = cg - cg[N]
        out[n, 2] = np.sqrt(np.sum((co[N:] - cg[N:]) ** 2, 1)).mean()
        mo, mg = co[:N], cg[:N]
        out[n, 3] = np.sqrt(np.sum((mo - mg) ** 2, 1)).mean()
        out[n, 4] = np.sqrt(np.sum((go.rigid_align(mo, mg) - mg) ** 2, 1)).mean()
        ho, hg = np.dot(je, mo), np.dot(je, mg)
        ho, hg = (ho - ho[0])[ev], (hg - hg[0])[ev]
        out[n, 0] = np.sqrt(np.sum((ho - hg) ** 2, 1)).mean()
        out[n, 1] = np.sqrt(np.sum((go.rigid_align(ho, hg) - hg) ** 2, 1)).mean()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_eval.txt'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('mesh_eval_bench: no GPU, nothing to measure')
    ev = list(geval.H36M_EVAL_JOINTS)
    lines = [MARKER, '%s (%s), torch %s; B x %d vertices, metres x 1000, regressors 24 x %d (5 per row) and 17 x %d (6 per row)'
             % (torch.cuda.get_device_name(0), getattr(torch.cuda.get_device_properties(0), 'gcnArchName', '?'), torch.__version__, N, N, N),
             'Windows: 50 calls for a, 5 for b.',
             'a, b: HIP events around a window of calls after one window of warm-up, median (min .. max) of %d windows; c: host clock around' % a.reps,
             'the two device-to-host copies and the loop, median of %d runs.  The columns of a, b and c were compared first (worst difference below).' % a.reps,
             '', '%-64s %5s %12s %22s %12s' % ('form', 'B', 'ms / call', '(min .. max)', 'us / sample')]
    for B in (64, 256):
        P, T, jr, je = batch(B)
        Jr, Je = geval.JointRegressor(jr, 'cuda'), geval.JointRegressor(je, 'cuda')
        idx = torch.as_tensor(ev, dtype=torch.int32, device='cuda')
        out = torch.empty((B, 5), device='cuda')
        launch = lambda: geval._launch_mesh_errors(P, T, Jr, 0, Je, idx, 0, 1000.0, 1000.0, out)      # noqa: E731
        ours = launch().cpu().numpy().astype(np.float64)
        theirs = torch_ops(P, T, Jr, Je).cpu().numpy().astype(np.float64)
        host = host_loop(P, T, jr, je, ev)
        cols = [0, 1, 2, 4]
        d_b = max(np.abs(ours[:, cols] - theirs[:, cols]).max(), abs(ours[:, 3].mean() - theirs[0, 3]))
        d_c = np.abs(ours - host).max()
        rows = [('a. gator_mesh_errors_f32, one launch', event_time(launch, 50, a.reps)),
                ('b. torch ops on the device (fp64 batched svd for the mesh fit)', event_time(lambda: torch_ops(P, T, Jr, Je), 5, a.reps))]
        ts = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_loop(P, T, jr, je, ev)
            ts.append((time.perf_counter() - t0) * 1e3)
        rows.append(('c. reference host loop in numpy (with the two copies)', (float(np.median(ts)), min(ts), max(ts))))
        for name, (ms, lo, hi) in rows:
            lines.append('%-64s %5d %12.4f %22s %12.3f' % (name, B, ms, '(%.4f .. %.4f)' % (lo, hi), ms * 1e3 / B))
            print(lines[-1], flush=True)
        lines.append('%-64s %5d   worst |a - b| %.2e mm, worst |a - c| %.2e mm (errors of %.0f .. %.0f mm)' % ('', B, d_b, d_c, ours.min(), ours.max()))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    head = open(a.out).read().split(MARKER)[0] if os.path.exists(a.out) else ''
    with open(a.out, 'w') as fh:
        fh.write(head + '\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
