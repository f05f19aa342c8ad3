#!/usr/bin/env python3
"""Forward + backward through the device SMPL layer (gator_amd.smpl.SMPLLayer under autograd) at NV = 6890 on a synthetic model of
SMPL's dimensions, against the autograd of the batched torch-op formulation of the same math (tools/smpl_bench.py: TorchLBS) on the
same device in the same process: what a user would otherwise write.

  python tools/smpl_backward_bench.py [--batches 1,64,256,1024]

Two workloads per batch: `full`, a loss on the vertices and the joints (both upstream gradients), and `joints`, a loss on the joints
alone (the layer is asked for the joints only and does no per-vertex work; TorchLBS computes its whole forward as written and
differentiates the joints).  Gradients are taken for pose, betas and trans with torch.autograd.grad.

Method (tools/smpl_bench.py: time_calls): device events around a window of back-to-back calls after warm-up of the same shape, the
number of calls chosen so that a window lasts about half a second; three windows, the median is reported with the extremes."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import smpl_refs as sr  # noqa: E402
from tools.smpl_bench import TorchLBS, inputs, time_calls  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1,64,256,1024')
    a = ap.parse_args()
    from gator_amd import smpl
    if not torch.cuda.is_available():
        raise SystemExit('smpl_backward_bench: no HIP device (a timing needs the GPU)')
    m = sr.synthetic_model(6890, 24, 10, 16)
    layer = smpl.SMPLLayer.from_arrays(m['v_template'], m['shapedirs'], m['posedirs'], m['weights'], m['J_regressor'], m['parents'])
    base = TorchLBS(m, 'cuda')
    print('device: %s   model: NV 6890 NJ 24 NB 10 (synthetic)   forward + backward, us per call, median of 3 windows (min .. max)' % torch.cuda.get_device_name(0))
    print('%6s %-7s %30s %30s %8s %22s' % ('B', 'loss on', 'layer', 'torch ops (TorchLBS)', 'x torch', 'max |g - g_torch| / max|g|'))
    rs = np.random.RandomState(9)
    for B in [int(b) for b in a.batches.split(',')]:
        leaves = [torch.from_numpy(x).cuda().requires_grad_(True) for x in inputs(B, 24, 10, 5)]
        gV = torch.from_numpy(rs.randn(B, 6890, 3).astype(np.float32)).cuda()
        gJ = torch.from_numpy(rs.randn(B, 24, 3).astype(np.float32)).cuda()

        def layer_full():
            v, j = layer(*leaves)
            return torch.autograd.grad([v, j], leaves, [gV, gJ])

        def torch_full():
            v, j = base(*leaves)
            return torch.autograd.grad([v, j], leaves, [gV, gJ])

        def layer_joints():
            _, j = layer(*leaves, want_verts=False)
            return torch.autograd.grad([j], leaves, [gJ])

        def torch_joints():
            _, j = base(*leaves)
            return torch.autograd.grad([j], leaves, [gJ])

        for what, ours, theirs in (('full', layer_full, torch_full), ('joints', layer_joints, torch_joints)):
            diff = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(ours(), theirs()))
            t, lo, hi, n = time_calls(ours)
            tb, blo, bhi, nb = time_calls(theirs)
            print('%6d %-7s %10.1f (%8.1f .. %8.1f) %10.1f (%8.1f .. %8.1f) %8.1f %22.1e   (windows of %d / %d calls)'
                  % (B, what, t * 1e6, lo * 1e6, hi * 1e6, tb * 1e6, blo * 1e6, bhi * 1e6, tb / t, diff, n, nb), flush=True)


if __name__ == '__main__':
    main()
