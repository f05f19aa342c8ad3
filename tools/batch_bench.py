#!/usr/bin/env python3
"""Time of gator_amd.batch.camera_frame_batch at NV = 6890 on a synthetic model of SMPL's dimensions, B = 64 and 1024:

  1. the new call: the Human3.6M recipe (cam_R, compensated translation, dataset joints, fitting gate, rot / flip, coco lift set) and
     the configuration the parent's targets_from_smpl can express (trans only: no R, no augmentation) -- the latter still projects and
     crops, which targets_from_smpl does not;
  2. the parent's smpl.targets_from_smpl on that common configuration;
  3. the float64 numpy restatement of the Human3.6M recipe on the host (tests/batch_refs.py + tests/smpl_refs.py), at B = 64 only: its
     [B,6890,3,4] float64 intermediates do not fit a sensible budget at 1024, so that row is per-sample arithmetic, marked as such;
  and the two new kernels alone.

Method (tools/smpl_bench.py's): device events around a window of back-to-back calls after warm-up of the same shape, the number of
calls chosen so that a window lasts about 0.3 s; three windows, the median reported, the spread printed.  Every figure is a whole
call: its launches, its allocations through torch's caching allocator and its host code."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import batch_refs as br  # noqa: E402
from tests import smpl_refs as sr  # noqa: E402


def time_calls(fn, min_window=0.3, windows=3):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='64,1024')
    ap.add_argument('--host-batch', type=int, default=64)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('batch_bench: no HIP device')
    from gator_amd import batch, smpl
    from gator_amd import eval as gator_eval
    m = sr.synthetic_model(6890, 24, 10, 16)
    layer = smpl.SMPLLayer.from_arrays(m['v_template'], m['shapedirs'], m['posedirs'], m['weights'], m['J_regressor'], m['parents'])
    rs = np.random.RandomState(9)
    h, k = br.sparse_regressor(17, 6890, rs), br.sparse_regressor(17, 6890, rs)
    jr = [gator_eval.JointRegressor(x[3].astype(np.float32), 'cuda') for x in (h, k)]
    d = lambda x, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(x)).to('cuda', dt)  # noqa: E731
    print('device: %s   model: NV 6890 NJ 24 NB 10 (synthetic), 17-joint stand-in regressors of %d / %d entries' % (torch.cuda.get_device_name(0), jr[0].nnz, jr[1].nnz))
    rows = []
    for B in [int(b) for b in a.batches.split(',')]:
        c = br.camera_case(3, B, 5, 'coco', False, special=False)            # its poses' companions only: R, translations, intrinsics, rot, flip
        pose = (rs.randn(B, 72) * 0.4).astype(np.float32)
        betas = rs.uniform(-2.5, 2.5, (B, 10)).astype(np.float32)
        jc = (rs.randn(B, 17, 3) * 300 + np.array([0, 0, 4500.0])).astype(np.float32)
        ji = (rs.rand(B, 17, 2) * 1000).astype(np.float32)
        P, S, T, R, CT, F, C = d(pose), d(betas), d(c['trans']), d(c['R']), d(c['cam_t']), d(c['focal']), d(c['princpt'])
        JC, JI, ROT, FL = d(jc), d(ji), d(c['rot_deg']), d(c['flip'], torch.int32)
        h36m = lambda: batch.camera_frame_batch(layer, P, S, trans=T, cam_R=R, cam_t=CT, compensate_root=True, focal=F, princpt=C,  # noqa: E731
                                                regressor_h36m=jr[0], regressor_coco=jr[1], input_joint_name='coco', joint_cam=JC, joint_img=JI,
                                                fitting_thr=25.0, rot_deg=ROT, flip=FL, flip_pairs=br.COCO_FLIP_PAIRS)
        common = lambda: batch.camera_frame_batch(layer, P, S, trans=T, focal=F, princpt=C, regressor_h36m=jr[0], regressor_coco=jr[1],  # noqa: E731
                                                  input_joint_name='coco')
        parent = lambda: smpl.targets_from_smpl(layer, P, S, T, jr[0], jr[1], input_joint_name='coco')  # noqa: E731
        lay = lambda: layer(P, S, None)  # noqa: E731
        po, bo = torch.empty_like(P), torch.empty_like(S)
        prep = lambda: batch._launch_prepare(P, R, S, 0, po, bo)  # noqa: E731
        verts, joints = layer(P, S, None)
        o = [torch.empty(B, 17, 3, device='cuda'), torch.empty(B, 19, 3, device='cuda'), torch.empty(B, 19, 2, device='cuda'),
             torch.empty(B, device='cuda'), torch.empty(B, 3, device='cuda')]
        pairs = d(np.asarray(br.COCO_FLIP_PAIRS, np.int32), torch.int32)
        mesh = torch.empty_like(verts)
        cam = lambda: batch._launch_camera_targets(verts, joints, T, CT, R, True, F, C, jr[0], jr[1], 1, JC, JI, ROT, FL, pairs, 25.0, 0, mesh, *o)  # noqa: E731
        res = {}
        for name, fn in (('camera_frame_batch, Human3.6M recipe', h36m), ('camera_frame_batch, common configuration', common),
                         ('targets_from_smpl (parent), common configuration', parent), ('SMPLLayer alone', lay),
                         ('gator_batch_prepare_f32 alone', prep), ('gator_camera_targets_f32 alone', cam)):
            t, lo, hi, n = time_calls(fn)
            res[name] = t
            print('B %5d  %-52s %9.1f us/call  %11.0f samples/s   (%.1f..%.1f us over 3 windows of %d calls)' % (B, name, t * 1e6, B / t, lo * 1e6, hi * 1e6, n), flush=True)
        bytes_cam = B * 6890 * 12 * 2.0
        print('B %5d  new / parent on the common configuration: %.2f x the parent\'s time;  k_camera_targets moves %.1f MB: %.2f TB/s'
              % (B, res['camera_frame_batch, common configuration'] / res['targets_from_smpl (parent), common configuration'],
                 bytes_cam / 1e6, bytes_cam / res['gator_camera_targets_f32 alone'] / 1e12), flush=True)
        rows.append((B, res))
    # 3. the host restatement
    B = a.host_batch
    c = br.camera_case(3, B, 5, 'coco', False, special=False)
    pose = (rs.randn(B, 72) * 0.4).astype(np.float32)
    betas = rs.uniform(-2.5, 2.5, (B, 10)).astype(np.float32)
    jc = (rs.randn(B, 17, 3) * 300 + np.array([0, 0, 4500.0])).astype(np.float32)
    ji = (rs.rand(B, 17, 2) * 1000).astype(np.float32)

    def host():
        p64 = br.root_to_camera(pose, c['R'])[0]
        v, j = sr.lbs_forward(m, p64, br.mean_shape_rule(betas.astype(np.float64)), None)
        return br.camera_targets(v, j, c['focal'], c['princpt'], h[3], k[3], 'coco', c['trans'], c['cam_t'], c['R'], True, jc, ji, c['rot_deg'],
                                 c['flip'], br.COCO_FLIP_PAIRS, 25.0)
    host()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        host()
        ts.append(time.perf_counter() - t0)
    th = statistics.median(ts)
    print('host  B %5d  float64 numpy restatement, Human3.6M recipe %12.1f ms/call  %11.1f samples/s   (%.1f..%.1f ms over 3 calls, %d threads)'
          % (B, th * 1e3, B / th, min(ts) * 1e3, max(ts) * 1e3, torch.get_num_threads()))
    for Bd, res in rows:
        t = res['camera_frame_batch, Human3.6M recipe']
        print('B %5d  device call against the host restatement, per sample: %.0f x%s' % (Bd, (th / B) / (t / Bd), '' if Bd == B else '   (host rate measured at B = %d, not at %d)' % (B, Bd)))


if __name__ == '__main__':
    main()
