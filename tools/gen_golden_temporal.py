#!/usr/bin/env python3
"""Generate tests/golden/temporal.npz by running the REAL reference's lib/smooth_utils (smooth_pose, OneEuroFilter) and
lib/coord_utils.compute_error_accel on a few short videos of 14 joints: the per-video block that data/PW3D/dataset.py:383-415 keeps
commented out.  Dev-container only, like tools/gen_golden_mesh_eval.py: the reference tree is needed, only the fixture travels.

The file holds data only:
  lengths            the videos' lengths (1, 2, 3, 5, 64, 65, 130), frames stored one video after another
  pred, gt           float32 [F,14,3]: random-walk joints in millimetres, the prediction with added jitter; fed to the reference as float64
  params             [3,2]: the (min_cutoff, beta) sets;  smooth_0 .. smooth_2: smooth_pose of every video under each, float64 [F,14,3]
  dt_video, dt, dt_params, smooth_dt
                     one run with dt = 1/30 on one video: OneEuroFilter called directly with t = idx * dt
  valid              uint8 [F]: invalid frames at a video's first frame, its last frame and interior frames
  accel, accel_valid compute_error_accel(gt, smooth_0) per video without / with vis = valid, concatenated over the videos
                     (a video shorter than 3 frames contributes nothing; with vis only the kept triples are there)

Usage:  python tools/gen_golden_temporal.py <path of the reference tree>"""
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tests import temporal_refs as tr  # noqa: E402

DT, DT_VIDEO, DT_PARAMS = 1.0 / 30.0, 5, (1.0, 0.007)


def reference_modules(ref_root):
    core, config = types.ModuleType('core'), types.ModuleType('core.config')      # coord_utils imports cfg and never reads it here
    config.cfg = None
    core.config = config
    sys.modules.setdefault('core', core)
    sys.modules.setdefault('core.config', config)
    sys.path.insert(0, os.path.join(ref_root, 'lib'))
    import coord_utils
    import smooth_utils
    return smooth_utils, coord_utils


def make_inputs():
    rs = np.random.RandomState(383)
    gt = tr.walk(rs, tr.LENGTHS, jitter=0.0)
    pred = (gt.astype(np.float64) + rs.randn(*gt.shape) * 12.0 + rs.randn(1, 14, 3) * 20.0).astype(np.float32)
    s = tr.seg_starts(tr.LENGTHS)
    valid = np.ones(len(gt), np.uint8)
    valid[s[3] + 2] = 0                  # the 5-frame video: its middle frame, so no triple is left
    valid[s[4]] = 0                      # a first frame
    valid[s[6] - 1] = 0                  # a last frame
    valid[s[6] + 40] = valid[s[6] + 41] = valid[s[6] + 77] = 0      # interior frames
    return pred, gt, valid, s


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    su, cu = reference_modules(sys.argv[1])
    pred, gt, valid, s = make_inputs()
    p64, g64 = pred.astype(np.float64), gt.astype(np.float64)
    vids = list(zip(s[:-1], s[1:]))
    out = dict(lengths=np.array(tr.LENGTHS, np.int64), pred=pred, gt=gt, valid=valid, params=np.array(tr.PARAMS, np.float64))
    for k, (mc, beta) in enumerate(tr.PARAMS):
        out['smooth_%d' % k] = np.concatenate([su.smooth_pose(p64[a:b], min_cutoff=mc, beta=beta) for a, b in vids])
        assert out['smooth_%d' % k].dtype == np.float64
    a, b = vids[DT_VIDEO]
    x = p64[a:b]
    f = su.OneEuroFilter(np.zeros_like(x[0]), x[0], min_cutoff=DT_PARAMS[0], beta=DT_PARAMS[1])
    out.update(dt_video=np.int64(DT_VIDEO), dt=np.float64(DT), dt_params=np.array(DT_PARAMS, np.float64),
               smooth_dt=np.stack([x[0]] + [f(np.ones_like(x[i]) * (i * DT), x[i]) for i in range(1, len(x))]))
    sm = out['smooth_0']
    out['accel'] = np.concatenate([cu.compute_error_accel(g64[a:b], sm[a:b]) for a, b in vids])
    out['accel_valid'] = np.concatenate([cu.compute_error_accel(g64[a:b], sm[a:b], vis=valid[a:b].astype(bool)) for a, b in vids])
    path = os.path.join(REPO, 'tests', 'golden', 'temporal.npz')
    np.savez_compressed(path, **out)
    print('%d frames, %d triples, %d under the mask' % (len(pred), len(out['accel']), len(out['accel_valid'])))
    print('%s: %d bytes' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
