#!/usr/bin/env python3
"""Write tests/golden/train_batch.npz: the reference's own cam2pixel, world2cam (lib/coord_utils.py:104-114), j3d_processing and
flip_3d_joint (lib/aug_utils.py:42-48,67-83) on seeded inputs, for tests/test_host_batch_refs.py to pin tests/batch_refs.py to.

Usage:  python tools/gen_golden_batch.py [path of the reference checkout, default /root/reference]

Runs where the reference is checked out; only the data written here is committed.  Shims as in tools/gen_golden.py: a stub cv2
(aug_utils imports it; nothing recorded here reaches it) and a stub core.config (the real one creates directories at import)."""
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests import batch_refs as br  # noqa: E402  (the flip pairs only)

OUT = os.path.join(REPO, 'tests', 'golden', 'train_batch.npz')
ROTS, FLIPS = (0.0, 30.0, -90.0, 17.25), (0, 1)


def install_shims(ref):
    sys.modules['cv2'] = types.ModuleType('cv2')
    core, cc = types.ModuleType('core'), types.ModuleType('core.config')
    cc.cfg = types.SimpleNamespace()
    core.config = cc
    sys.modules.update({'core': core, 'core.config': cc})
    sys.path.insert(0, os.path.join(ref, 'lib'))


def main():
    install_shims(sys.argv[1] if len(sys.argv) > 1 else '/root/reference')
    import aug_utils
    import coord_utils
    rs = np.random.RandomState(20240)
    z = {}
    cam = rs.randn(19, 3) * np.array([400.0, 700.0, 300.0]) + np.array([0.0, 0.0, 4500.0])
    cam[3, 2], cam[4, 2] = 0.0, -cam[4, 2]                       # Z = 0 and Z < 0: the IEEE results
    f, c = np.array([1145.04940459, 1143.78109572]), np.array([512.54150496, 515.45148698])
    z['cam'], z['focal'], z['princpt'] = cam, f, c
    with np.errstate(divide='ignore', invalid='ignore'):
        z['cam2pixel'] = coord_utils.cam2pixel(cam, f, c)
        z['cam2pixel_f32'] = coord_utils.cam2pixel(cam.astype(np.float32), f.astype(np.float32), c.astype(np.float32))
    R = np.linalg.qr(rs.randn(3, 3))[0]
    t = rs.randn(3) * 1000
    z['R'], z['t'] = R, t
    z['world2cam'] = coord_utils.world2cam(cam, R, t)
    for name, pairs, nj in (('h36m', br.H36M_FLIP_PAIRS, 17), ('coco', br.COCO_FLIP_PAIRS, 19)):
        S = rs.randn(nj, 3) * 300
        z['S_' + name] = S
        z['flip3d_' + name] = aug_utils.flip_3d_joint(S.copy(), pairs)
        for r in ROTS:
            for fl in FLIPS:
                out = aug_utils.j3d_processing(S.copy(), r, fl, pairs)
                assert out.dtype == np.float32
                z['j3d_%s_%g_%d' % (name, r, fl)] = out
    z['rots'], z['flips'] = np.array(ROTS), np.array(FLIPS)
    np.savez(OUT, **z)
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
