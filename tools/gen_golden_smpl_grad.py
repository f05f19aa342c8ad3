#!/usr/bin/env python3
"""Generate tests/golden/smpl_layer_grad.npz: the fp32 autograd of the REAL smplpytorch SMPL_Layer (built as
tools/gen_golden_smpl.py builds it, on the CPU) on every case of tests/smpl_refs.py: CASES, with the seeded upstream gradients of
tests/smpl_grad_refs.py.  Dev-container only: the reference tree is needed.

Per case the file holds, for the full upstream (grad_verts and grad_joints), the fp32 g_pose / g_betas / g_trans of the first few
samples, and for each upstream (full, verts only, joints only) spread = max |reference fp32 - float64 VJP| over all 65 samples, one
figure per output (0 for an input the case does not use): the reference's own fp32 error, the device tests' yardstick.

Usage:  python tools/gen_golden_smpl_grad.py <path of the reference tree>"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests import smpl_grad_refs as gr  # noqa: E402
from tests import smpl_refs as sr  # noqa: E402
from tools.gen_golden_smpl import reference_layer  # noqa: E402

STORED = 4          # samples whose fp32 gradients are kept (a case that stores fewer forward samples keeps that many)


def reference_grads(layer, args, scale, gV, gJ):
    """fp32 autograd of the reference layer: -> {'pose', 'betas', 'trans'} float32 numpy, None for an absent input."""
    leaves = [None if a is None else torch.from_numpy(a).clone().requires_grad_(True) for a in args]
    call = [leaves[0], leaves[1] if leaves[1] is not None else torch.zeros(1)]
    if leaves[2] is not None:
        call.append(leaves[2])
    verts, joints = layer(*call)
    if scale != 1.0:                              # the datasets' `*= 1000`
        verts, joints = verts * scale, joints * scale
    outs, grads = [], []
    if gV is not None:
        outs.append(verts)
        grads.append(torch.from_numpy(gV))
    if gJ is not None:
        outs.append(joints)
        grads.append(torch.from_numpy(gJ))
    have = [x for x in leaves if x is not None]
    got = iter(torch.autograd.grad(outs, have, grads, allow_unused=True))
    res = {}
    for name, leaf in zip(gr.OUTPUTS, leaves):
        if leaf is None:
            res[name] = None
        else:
            g = next(got)
            res[name] = np.zeros(leaf.shape, np.float32) if g is None else g.numpy().astype(np.float32)
    return res


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__.split('Usage:')[1].strip())
    ref_root = sys.argv[1]
    torch.set_num_threads(1)
    out, meta = {}, {}
    for name, (margs, opt, keep) in sr.CASES.items():
        m = sr.synthetic_model(*margs)
        o = gr.case_options(name)
        args = gr.case_arguments(name)
        gV, gJ = gr.upstream(name)
        layer = reference_layer(ref_root, m, o['center_idx'])
        stored = min(STORED, keep)
        for which in gr.UPSTREAMS:
            v, j = gr.select_upstream(which, gV, gJ)
            g32 = reference_grads(layer, args, o['out_scale'], v, j)
            g64 = gr.vjp64(m, args, o, v, j)
            spread = []
            for k in gr.OUTPUTS:
                if g32[k] is None:
                    spread.append(0.0)
                    continue
                assert np.isfinite(g32[k]).all(), (name, which, k)
                spread.append(float(np.abs(g32[k] - g64[k]).max()))
                if which == 'full':
                    out['%s.g_%s32' % (name, k)] = g32[k][:stored]
            out['%s.spread.%s' % (name, which)] = np.array(spread, np.float64)
            rel = ['%.1e' % (s / max(np.abs(g64[k]).max(), 1e-300)) if g64[k] is not None else '-' for s, k in zip(spread, gr.OUTPUTS)]
            print('%-18s %-6s |ref32 - vjp64| max: pose %.3e betas %.3e trans %.3e   over max|g|: %s' % ((name, which) + tuple(spread) + (' '.join(rel),)),
                  flush=True)
        meta[name] = {'model': list(margs), 'options': opt, 'stored': stored}
    out['meta'] = np.array(json.dumps(meta, sort_keys=True))
    path = os.path.join(REPO, 'tests', 'golden', 'smpl_layer_grad.npz')
    np.savez_compressed(path, **out)
    print('%s: %d bytes' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
