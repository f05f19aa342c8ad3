#!/usr/bin/env python3
"""Generate tests/golden/detector_noise.npz by running the REAL reference's lib/noise_utils.synthesize_pose and
data/Human36M/dataset.py's generate_syn_error / get_stat.  Dev-container only, like tools/gen_golden_temporal.py: the reference tree is
needed, only the fixture travels.  easydict (imported by noise_utils) and the dataset module's other imports are stood in for locally;
the two functions themselves and the error table (data/Human36M/noise_stats.py) are the reference's.

The file holds data only:
  poses [4,17,3] float32     crop-space COCO poses (x, y, validity): all 17 valid; 10 valid; 5 valid (the three probability tiers); a
                             narrow, small-area pose whose partners lie within ks50 of each other (the exclusion masks reject many
                             candidates).  Partners are distinct everywhere.
  areas [4]                  the `area` each was run with (the extent of its box)
  n_draws                    synthesize_pose calls per pose
  hist_self [4,17,5] int64   per (pose, joint): the output's distance from the clean joint in [0, ks85), [ks85, ks50), [ks50, ks10),
                             >= ks10, and the number of zeroed outputs (tests/noise_refs.py::histogram)
  hist_partner [4,17,5]      the same against the clean partner joint (zeros for joint 0, which has none)
  stats_table [17,5] float64 get_stat's table in the Human3.6M joint order: mean x, y, std x, y, weight
  stats_n, stats_mean [17,2], stats_std [17,2], stats_rate [17]
                             generate_syn_error over stats_n calls: mean and std of the applied noise, share of calls that applied it

Usage:  python tools/gen_golden_noise.py <path of the reference tree> [draws per pose, default 5000]"""
import os
import random
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tests import noise_refs as nr  # noqa: E402


class _Anything(types.ModuleType):
    """A module whose every attribute exists: what the dataset module imports and these two functions never touch."""
    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        return type(name, (), {})


def reference_functions(ref_root):
    easydict = types.ModuleType('easydict')

    class EasyDict(dict):
        __getattr__ = dict.__getitem__
        __setattr__ = dict.__setitem__
    easydict.EasyDict = EasyDict
    sys.modules.setdefault('easydict', easydict)
    for name in ('core', 'core.config', 'graph_utils', 'smpl', 'coord_utils', 'aug_utils', 'funcs_utils', 'vis', 'pycocotools',
                 'pycocotools.coco', 'transforms3d', 'cv2'):
        sys.modules.setdefault(name, _Anything(name))
    sys.path.insert(0, os.path.join(ref_root, 'lib'))
    sys.path.insert(0, os.path.join(ref_root, 'data'))
    import noise_utils
    from Human36M.dataset import Human36M
    return noise_utils.synthesize_pose, Human36M


def make_poses():
    rs = np.random.RandomState(421)
    poses = np.ones((4, 17, 3), np.float32)
    for k in range(3):
        poses[k, :, :2] = nr.coco_pose(rs, scale=2.0, centre=(144.0, 192.0))
    narrow = nr.coco_pose(rs, scale=2.0, centre=(0.0, 0.0)).astype(np.float64)
    poses[3, :, :2] = (narrow * np.array([0.3, 1.0]) + np.array([144.0, 192.0])).astype(np.float32)
    poses[1, [0, 3, 4, 6, 9, 13, 16], 2] = 0            # 10 valid: both ears, one of a pair here and there
    poses[2, :, 2] = 0
    poses[2, [1, 2, 5, 11, 14], 2] = 1                  # 5 valid: both eyes, single members of three pairs
    for p in poses:
        for q, w in nr.SYMMETRY:
            assert np.abs(p[q, :2] - p[w, :2]).max() > 1.0
    areas = np.array([np.prod(p[:, :2].max(0).astype(np.float64) - p[:, :2].min(0).astype(np.float64)) for p in poses])
    return poses, areas


def main():
    if len(sys.argv) not in (2, 3):
        sys.exit(__doc__)
    n = int(sys.argv[2]) if len(sys.argv) == 3 else 5000
    synthesize_pose, Human36M = reference_functions(sys.argv[1])
    poses, areas = make_poses()
    np.random.seed(1431)
    random.seed(1431)
    hs, hp = np.zeros((4, 17, 5), np.int64), np.zeros((4, 17, 5), np.int64)
    for k, (pose, area) in enumerate(zip(poses, areas)):
        out = np.stack([synthesize_pose(pose.copy(), area, num_overlap=0)[:, :2] for _ in range(n)])
        for j in range(17):
            hs[k, j] = nr.histogram(out[:, j], pose[j, :2], area, j)
            q = nr.partner_of(j)
            if q >= 0:
                hp[k, j] = nr.histogram(out[:, j], pose[q, :2], area, j)
        print('pose %d: area %.1f, zeroed %d' % (k, area, hs[k, :, 4].sum()), flush=True)
    fake = types.SimpleNamespace(human36_joint_num=17, human36_joints_name=(
        'Pelvis', 'R_Hip', 'R_Knee', 'R_Ankle', 'L_Hip', 'L_Knee', 'L_Ankle', 'Torso', 'Neck', 'Nose', 'Head', 'L_Shoulder', 'L_Elbow', 'L_Wrist',
        'R_Shoulder', 'R_Elbow', 'R_Wrist'))
    stat = Human36M.get_stat(fake)
    fake.human36_error_distribution = stat
    table = np.array([[s['mean'][0], s['mean'][1], s['std'][0], s['std'][1], s['weight']] for s in stat], np.float64)
    stats_n = 20000
    draws = np.stack([Human36M.generate_syn_error(fake) for _ in range(stats_n)]).astype(np.float64)
    applied = (draws != 0).any(2)
    path = os.path.join(REPO, 'tests', 'golden', 'detector_noise.npz')
    np.savez_compressed(path, poses=poses, areas=areas, n_draws=np.int64(n), hist_self=hs, hist_partner=hp, stats_table=table,
                        stats_n=np.int64(stats_n), stats_rate=applied.mean(0),
                        stats_mean=np.stack([draws[applied[:, j], j].mean(0) for j in range(17)]),
                        stats_std=np.stack([draws[applied[:, j], j].std(0) for j in range(17)]))
    print('%s: %d bytes' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
