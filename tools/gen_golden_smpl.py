#!/usr/bin/env python3
"""Generate tests/golden/smpl_layer.npz by running the REAL smplpytorch SMPL_Layer.forward (the reference's vendored copy) on the CPU
in fp32 on the synthetic models of tests/smpl_refs.py.  Dev-container only, like tools/gen_golden.py: the reference tree is needed.

The layer's __init__ reads a licence-gated pkl through chumpy; its forward reads six buffers and a parent list.  So the layer object
is made with SMPL_Layer.__new__ and the buffers are registered from the synthetic arrays: no pkl, no chumpy, the real forward.

Per case (tests/smpl_refs.py: CASES) the file holds the generator's arguments, the sha256 of the generated model, the inputs, the
reference's fp32 outputs for the first few samples, and max |ref32 - fp64 restatement| over all samples, for verts and for joints:
the reference's own fp32 error, which the device tests take as their yardstick.

Usage:  python tools/gen_golden_smpl.py [path of the reference tree]"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests import smpl_refs as sr  # noqa: E402


def reference_layer(ref_root, m, center_idx=None):
    sys.path.insert(0, os.path.join(ref_root, 'smplpytorch'))
    from smplpytorch.pytorch.smpl_layer import SMPL_Layer
    layer = SMPL_Layer.__new__(SMPL_Layer)
    torch.nn.Module.__init__(layer)
    layer.center_idx = center_idx
    layer.gender = 'neutral'
    nb = m['shapedirs'].shape[2]
    layer.register_buffer('th_betas', torch.zeros(1, nb))
    layer.register_buffer('th_shapedirs', torch.Tensor(m['shapedirs']))
    layer.register_buffer('th_posedirs', torch.Tensor(m['posedirs']))
    layer.register_buffer('th_v_template', torch.Tensor(m['v_template']).unsqueeze(0))
    layer.register_buffer('th_J_regressor', torch.Tensor(m['J_regressor']))
    layer.register_buffer('th_weights', torch.Tensor(m['weights']))
    layer.register_buffer('th_faces', torch.from_numpy(m['faces']).long())
    parents = [int(p) for p in m['parents']]
    parents[0] = 4294967295                       # what the model files hold there
    layer.kintree_parents = parents
    layer.num_joints = len(parents)
    return layer


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else '/root/reference'
    torch.set_num_threads(1)
    out = {}
    meta = {}
    for name, (margs, opt, keep) in sr.CASES.items():
        m = sr.synthetic_model(*margs)
        pose, betas, trans = sr.case_inputs(name)
        use_b = opt.get('betas', True) and margs[2] > 0
        use_t = opt.get('trans', True)
        cidx = opt.get('center_idx')
        scale = opt.get('out_scale', 1.0)
        layer = reference_layer(ref_root, m, cidx)
        with torch.no_grad():
            args = [torch.from_numpy(pose)]
            args.append(torch.from_numpy(betas) if use_b else torch.zeros(1))
            if use_t:
                args.append(torch.from_numpy(trans))
            v32, j32 = layer(*args)
            v32, j32 = v32.numpy().astype(np.float32), j32.numpy().astype(np.float32)
        if scale != 1.0:                          # the datasets' `*= 1000` on the float32 arrays
            v32 = v32 * np.float32(scale)
            j32 = j32 * np.float32(scale)
        v64, j64 = sr.lbs_forward(m, pose, betas if use_b else None, trans if use_t else None, cidx, scale)
        assert np.isfinite(v32).all() and np.isfinite(j32).all(), name
        sv, sj = float(np.abs(v32 - v64).max()), float(np.abs(j32 - j64).max())
        out[name + '.pose'], out[name + '.betas'], out[name + '.trans'] = pose, betas, trans
        out[name + '.verts32'], out[name + '.joints32'] = v32[:keep], j32[:keep]
        out[name + '.spread'] = np.array([sv, sj], np.float64)
        meta[name] = {'model': list(margs), 'options': opt, 'sha256': sr.model_sha256(m), 'stored': keep}
        print('%-18s NV %5d  |ref32 - fp64| max: verts %.3e  joints %.3e  (x %g)' % (name, margs[0], sv, sj, scale))
    out['meta'] = np.array(json.dumps(meta, sort_keys=True))
    path = os.path.join(REPO, 'tests', 'golden', 'smpl_layer.npz')
    np.savez_compressed(path, **out)
    print('%s: %d bytes' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
