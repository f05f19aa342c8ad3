#!/usr/bin/env python3
"""Throughput of the device SMPL layer (gator_amd.smpl.SMPLLayer) at NV = 6890 on a synthetic model of SMPL's dimensions.

  python tools/smpl_bench.py                      on the GPU: B = 1, 64, 1024, 8192 against the batched torch-op formulation of the same
                                                  math on the same device in the same process (what a user would otherwise write)
  python tools/smpl_bench.py --cpu-reference DIR  on a machine that has the reference tree at DIR: the real smplpytorch SMPL_Layer on
                                                  the CPU at B = 1 and 64, on 1 and 16 threads (no GPU needed)

Method: device events around a window of back-to-back calls, after warm-up of the same shape; the number of calls is chosen so that a
window lasts about half a second; three windows, the median is reported and the spread printed.  Rates over peak are whole-call
figures (both kernels and their launches), against the 157.3 TFLOP/s fp32-matrix and 8.0 TB/s HBM peaks of the MI355X: the blend
GEMM's 2 * 217 * 3 * 6890 FLOP and the 6890 * 12 output bytes per sample are counted, nothing else."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import smpl_refs as sr  # noqa: E402

PEAK_F32_MATRIX = 157.3e12
PEAK_HBM = 8.0e12


def inputs(B, nj, nb, seed):
    rs = np.random.RandomState(seed)
    return ((rs.randn(B, nj * 3) * 0.4).astype(np.float32), rs.uniform(-2.5, 2.5, (B, nb)).astype(np.float32),
            (rs.randn(B, 3) * 1.2).astype(np.float32))


class TorchLBS:
    """The layer's formulas as batched torch ops on the device: Rodrigues, blend shapes as two matmuls, the chain as 24 batched
    4x4 products, the per-vertex transforms [B,NV,12] as a matmul with the dense weights, the skinning as an elementwise sum."""

    def __init__(self, m, device):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)  # noqa: E731
        nv = m['v_template'].shape[0]
        self.nv, self.nj = nv, m['weights'].shape[1]
        self.vt = t(m['v_template'])
        self.sd = t(m['shapedirs'].reshape(nv * 3, -1).T)            # [NB, NV*3]
        self.pd = t(m['posedirs'].reshape(nv * 3, -1).T)             # [207, NV*3]
        self.w = t(m['weights'])
        self.jr = t(m['J_regressor'])
        self.parents = [int(p) for p in m['parents']]
        self.eye = torch.eye(3, device=device)

    def __call__(self, pose, betas, trans):
        B, nj = pose.shape[0], self.nj
        a = pose.view(B, nj, 3)
        angle = (a + 1e-8).norm(dim=2, keepdim=True)
        half = angle * 0.5
        q = torch.cat([torch.cos(half), torch.sin(half) * (a / angle)], 2)
        q = q / q.norm(dim=2, keepdim=True)
        w, x, y, z = q.unbind(2)
        R = torch.stack([w * w + x * x - y * y - z * z, 2 * x * y - 2 * w * z, 2 * w * y + 2 * x * z,
                         2 * w * z + 2 * x * y, w * w - x * x + y * y - z * z, 2 * y * z - 2 * w * x,
                         2 * x * z - 2 * w * y, 2 * w * x + 2 * y * z, w * w - x * x - y * y + z * z], 2).view(B, nj, 3, 3)
        pose_map = (R[:, 1:] - self.eye).reshape(B, (nj - 1) * 9)
        v_shaped = self.vt + (betas @ self.sd).view(B, self.nv, 3)
        J = torch.matmul(self.jr, v_shaped)
        v_posed = v_shaped + (pose_map @ self.pd).view(B, self.nv, 3)
        bottom = torch.tensor([0.0, 0.0, 0.0, 1.0], device=pose.device).expand(B, 1, 4)
        G = [torch.cat([torch.cat([R[:, 0], J[:, 0, :, None]], 2), bottom], 1)]
        for j in range(1, nj):
            p = self.parents[j]
            L = torch.cat([torch.cat([R[:, j], (J[:, j] - J[:, p])[:, :, None]], 2), bottom], 1)
            G.append(G[p] @ L)
        G = torch.stack(G, 1)                                       # [B,NJ,4,4]
        A = G[:, :, :3, :].clone()
        A[:, :, :, 3] -= (G[:, :, :3, :3] @ J[:, :, :, None])[..., 0]
        T = (self.w @ A.reshape(B, nj, 12)).view(B, self.nv, 3, 4)   # the layer's th_T, 3 rows of it
        verts = (T[..., :3] * v_posed[:, :, None, :]).sum(3) + T[..., 3]
        return verts + trans[:, None, :], G[:, :, :3, 3] + trans[:, None, :]


def time_calls(fn, min_window=0.5, windows=3):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    n = max(5, int(min_window / max((time.perf_counter() - t0) / 3, 1e-6)))
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


def gpu_bench(batches):
    from gator_amd import smpl
    if not torch.cuda.is_available():
        raise SystemExit('smpl_bench: no HIP device (a timing needs the GPU; use --cpu-reference for the CPU baseline)')
    m = sr.synthetic_model(6890, 24, 10, 16)
    layer = smpl.SMPLLayer.from_arrays(m['v_template'], m['shapedirs'], m['posedirs'], m['weights'], m['J_regressor'], m['parents'])
    base = TorchLBS(m, 'cuda')
    nv, K = 6890, 10 + 207
    print('device: %s   model: NV %d NJ 24 NB 10 (synthetic)   K = %d' % (torch.cuda.get_device_name(0), nv, K))
    print('%6s %14s %14s %8s %12s %12s %16s %14s' % ('B', 'layer us/call', 'meshes/s', 'x torch', 'torch us/call', 'torch mesh/s', 'of fp32 matrix', 'of HBM write'))
    for B in batches:
        pose, betas, trans = (torch.from_numpy(a).cuda() for a in inputs(B, 24, 10, 5))
        v, j = layer(pose, betas, trans)
        bv, bj = base(pose, betas, trans)
        dv, dj = float((v - bv).abs().max()), float((j - bj).abs().max())
        del bv, bj, v, j
        t, lo, hi, n = time_calls(lambda: layer(pose, betas, trans))
        tb, blo, bhi, nb = time_calls(lambda: base(pose, betas, trans))
        print('%6d %14.1f %14.0f %8.1f %12.1f %12.0f %15.1f%% %13.1f%%   (windows of %d / %d calls; layer %.1f..%.1f us, torch %.1f..%.1f us; '
              'max |layer - torch| verts %.1e joints %.1e)'
              % (B, t * 1e6, B / t, tb / t, tb * 1e6, B / tb, 100 * B * 2.0 * K * 3 * nv / t / PEAK_F32_MATRIX, 100 * B * nv * 12.0 / t / PEAK_HBM,
                 n, nb, lo * 1e6, hi * 1e6, blo * 1e6, bhi * 1e6, dv, dj), flush=True)


def cpu_reference(ref_root):
    from tools.gen_golden_smpl import reference_layer
    m = sr.synthetic_model(6890, 24, 10, 16)
    layer = reference_layer(ref_root, m)
    print('reference SMPL_Layer.forward on the CPU, fp32, synthetic model NV 6890')
    print('%8s %4s %14s %12s' % ('threads', 'B', 'ms/call', 'meshes/s'))
    for threads in (1, 16):
        torch.set_num_threads(threads)
        for B in (1, 64):
            args = [torch.from_numpy(a) for a in inputs(B, 24, 10, 5)]
            with torch.no_grad():
                for _ in range(2):
                    layer(*args)
                n = 20 if B == 1 else 5
                ts = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    for _ in range(n):
                        layer(*args)
                    ts.append((time.perf_counter() - t0) / n)
            t = statistics.median(ts)
            print('%8d %4d %14.2f %12.0f' % (threads, B, t * 1e3, B / t), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cpu-reference', metavar='DIR', help='time the real reference layer on the CPU; DIR is the reference tree')
    ap.add_argument('--batches', default='1,64,1024,8192')
    a = ap.parse_args()
    if a.cpu_reference:
        cpu_reference(a.cpu_reference)
    else:
        gpu_bench([int(b) for b in a.batches.split(',')])


if __name__ == '__main__':
    main()
