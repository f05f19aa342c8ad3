#!/usr/bin/env python3
"""Time the device's 2D pose overlay (gator_amd/vis.py, csrc/draw2d.hip): the whole gator_draw2d_u8 call (k_draw_build + k_draw_tiles)
on the COCO skeleton of demo/run.py (19 limbs, 57 primitives a person), every person about a third of the frame high, at
(frames, H x W, people per frame) = (1, 224^2, 1), (1, 1080p, 1), (64, 224^2, 1), (16, 1080p, 1), (16, 1080p, 8): out of place at alpha = 1
and 0.5, in place, and a plain device copy of the frames (the floor of an out-of-place call: the same bytes read and written once).
Also both forms of the tile kernel (gator_draw2d_set_tile_rows: 64 x 4 tiles with one pixel a thread, 64 x 16 with four) at those
shapes and at (256, 224^2, 1), (2, 1080p, 1), (4, 1080p, 1), (8, 1080p, 1): the rows the built-in choice between them (kTallTileFrom) rests on.

The C ABI is called directly on preallocated tensors, so a window holds launches and nothing else.  HIP events around a window of calls
after one window of warm-up, the median (min .. max) of --reps windows.  At one small frame the launches are shorter than their
enqueue: those rows measure the host.  A run without a GPU fails.

    python tools/draw_bench.py [--reps 5] [--out profiles/draw2d.txt]

The block it writes replaces the one under its marker line in --out and leaves the rest of that file alone."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gator_amd import _lib, vis  # noqa: E402

MARKER = '== timings: tools/draw_bench.py =='
SKELETON = ((1, 2), (0, 1), (0, 2), (2, 4), (1, 3), (6, 8), (8, 10), (5, 7), (7, 9), (12, 14), (14, 16), (11, 13), (13, 15), (17, 11), (17, 12),
            (17, 18), (18, 5), (18, 6), (18, 0))
# a standing person in a unit box (x right, y down), COCO order + pelvis + neck
POSE = np.array([(0.50, 0.08), (0.53, 0.06), (0.47, 0.06), (0.57, 0.08), (0.43, 0.08), (0.65, 0.22), (0.35, 0.22), (0.72, 0.40), (0.28, 0.40),
                 (0.75, 0.56), (0.25, 0.56), (0.60, 0.55), (0.40, 0.55), (0.62, 0.77), (0.38, 0.77), (0.63, 0.98), (0.37, 0.98), (0.50, 0.55),
                 (0.50, 0.22)], np.float64)


def event_time(fn, iters, reps):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'draw2d.txt'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('draw_bench: no GPU, nothing to measure')
    import bench
    lib = _lib.load()
    d = vis.SkeletonDrawer(SKELETON, 19, 'cuda:0')
    col = torch.as_tensor(vis.rainbow_colors(19), dtype=torch.float32).cuda()
    lines = [MARKER, '%s (%s), torch %s; COCO skeleton, 19 limbs = 57 primitives a person, a person a third of the frame high'
             % (torch.cuda.get_device_name(0), getattr(torch.cuda.get_device_properties(0), 'gcnArchName', '?'), torch.__version__),
             'HIP events around a window of calls after one window of warm-up, median (min .. max) of %d windows; ms per call.' % a.reps,
             'GB/s counts 3 B read + 3 B written per pixel (in place: the touched tiles only, not counted).', '']
    for N, H, W, per in ((1, 224, 224, 1), (1, 1080, 1920, 1), (64, 224, 224, 1), (16, 1080, 1920, 1), (16, 1080, 1920, 8),
                         (256, 224, 224, 1), (2, 1080, 1920, 1), (4, 1080, 1920, 1), (8, 1080, 1920, 1)):
        iters = 200 if N * H * W < 4e6 else 20
        rng = np.random.default_rng(0)
        P = N * per
        size = H / 3.0
        origin = np.stack([rng.uniform(0, W - size * 0.6, P), rng.uniform(0, H - size, P)], 1)
        joints = torch.from_numpy((origin[:, None] + POSE[None] * [size * 0.6, size]).astype(np.float32)).cuda()
        idx = np.repeat(np.arange(N, dtype=np.int32), per)
        img = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, device='cuda')
        out, out2 = torch.empty_like(img), torch.empty_like(img)
        same = img.clone()

        def call(alpha, src, dst):
            args = _lib.Draw2dArgs(struct_size=ctypes.sizeof(_lib.Draw2dArgs), n_people=P, n_images=N, H=H, W=W, joint_dim=2, style=_lib.DRAW_KEYPOINTS,
                                   kp_thre=0.4, alpha=alpha, joints=joints.data_ptr(), colors=col.data_ptr(), bbox=None, images=src.data_ptr(),
                                   out=dst.data_ptr(), image_index=idx.ctypes.data if per > 1 else None)
            ref = ctypes.byref(args)
            return lambda: _lib.check(lib.gator_draw2d_u8(d._h, ref, None), 'draw_bench')

        f1, fh, fi = call(1.0, img, out), call(0.5, img, out), call(1.0, same, same)
        f1()
        torch.cuda.synchronize()
        assert torch.equal(out, d.draw(img, joints, image_index=idx if per > 1 else None))
        touched = float((out != img).any(3).float().mean())
        lines.append('%d frame(s) of %d x %d (W x H), %d person(s) each: %.4f of the pixels drawn on, %d workgroups in the one-row form, window of %d calls'
                     % (N, W, H, per, touched, N * -(-W // 64) * -(-H // 4), iters))
        px = N * H * W
        rows = []
        for form in (1, 4, 1, 4):                      # alternating: the spread between the two rows of a form is the noise
            d.set_tile_rows(form)
            rows.append(('alpha = 1, forced %d row(s) a thread' % form, event_time(f1, iters, a.reps), 6 * px))
        d.set_tile_rows(0)
        rows += [('gator_draw2d_u8, alpha = 1', event_time(f1, iters, a.reps), 6 * px),
                ('gator_draw2d_u8, alpha = 0.5', event_time(fh, iters, a.reps), 6 * px),
                ('gator_draw2d_u8, in place', event_time(fi, iters, a.reps), None),
                ('copy of the frames (floor)', event_time(lambda: out2.copy_(img), iters, a.reps), 6 * px)]
        for name, (ms, lo, hi), nbytes in rows:
            lines.append('  %-36s %10.4f %22s %s' % (name, ms, '(%.4f .. %.4f)' % (lo, hi), '' if nbytes is None else '%8.1f GB/s' % (nbytes / ms / 1e6)))
            print(lines[-1], flush=True)
    lines += ['', 'clocks after the run: %s' % (bench.gpu_clocks(0),)]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    head = open(a.out).read().split(MARKER)[0] if os.path.exists(a.out) else ''
    with open(a.out, 'w') as fh:
        fh.write(head + '\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
