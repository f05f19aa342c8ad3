#!/usr/bin/env python3
"""Generate tests/golden/mesh_eval.npz by running the REAL reference's lib/coord_utils.rigid_align on a few 431-point float32 sets (the
coarse mesh's size): the whole-mesh Procrustes step that data/PW3D/dataset.py:360-361 keeps commented out.  Dev-container only, like
tools/gen_golden.py: the reference tree is needed, only the small fixture written here travels.

Per set the file holds the float32 inputs, the per-vertex distance |aligned - B| of the reference run on the inputs widened to
float64, and the mean of that distance from the float64 run and from the run on the float32 arrays as they are (numpy then stays in
float32: the reference's own arithmetic error on a mesh).

Usage:  python tools/gen_golden_mesh_eval.py <path of the reference tree>"""
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 431


def reference_coord_utils(ref_root):
    core, config = types.ModuleType('core'), types.ModuleType('core.config')      # coord_utils imports cfg and never reads it here
    config.cfg = None
    core.config = config
    sys.modules.setdefault('core', core)
    sys.modules.setdefault('core.config', config)
    sys.path.insert(0, os.path.join(ref_root, 'lib'))
    import coord_utils
    return coord_utils


def make_sets():
    rs = np.random.RandomState(431)
    A, B, names = [], [], []
    for name in ('noisy similarity image', 'mirrored', 'far centroid, scale 0.3'):
        a = rs.randn(N, 3) * 250.0
        q, r = np.linalg.qr(rs.randn(3, 3))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 2] = -q[:, 2]
        src = a * np.array([1.0, 1.0, -1.0]) if name == 'mirrored' else a
        scale = 0.3 if name.startswith('far') else 1.1
        b = scale * src @ q.T + rs.randn(3) * 60.0 + rs.randn(N, 3) * 15.0
        if name.startswith('far'):
            a = a + np.array([1e5, -1e5, 5e4])              # 100 m in mm
        A.append(a.astype(np.float32))
        B.append(b.astype(np.float32))
        names.append(name)
    return np.stack(A), np.stack(B), names


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    cu = reference_coord_utils(sys.argv[1])
    A, B, names = make_sets()
    dist64 = np.stack([np.sqrt(((cu.rigid_align(a.astype(np.float64), b.astype(np.float64)) - b) ** 2).sum(1)) for a, b in zip(A, B)])
    mean32 = np.array([np.sqrt(((cu.rigid_align(a, b).astype(np.float64) - b) ** 2).sum(1)).mean() for a, b in zip(A, B)])
    out = os.path.join(REPO, 'tests', 'golden', 'mesh_eval.npz')
    np.savez(out, A=A, B=B, names=np.array(names), pa_dist64=dist64, pa_mpvpe64=dist64.mean(1), pa_mpvpe32=mean32)
    for n, m64, m32 in zip(names, dist64.mean(1), mean32):
        print('%-28s PA-MPVPE %.6f mm (float64)   %.6f mm (float32 arrays)' % (n, m64, m32))
    print('%s: %d bytes' % (out, os.path.getsize(out)))


if __name__ == '__main__':
    main()
