#!/usr/bin/env python3
"""Time the device renderer (gator_amd/render.py): its three launches and the whole call, on a synthetic closed mesh of SMPL's size
(a UV sphere of 82 rings x 84 segments: 6890 vertices, 13776 faces) scaled to cover about a tenth of the frame, at
(B, H x W) = (1, 224^2), (1, 1080p), (64, 224^2), (16, 1080p), with and without a background image.  Also: the resolve launch's achieved
bytes/s next to a plain device copy of the same image (its floor), and the raster launch at several small/large-box thresholds.

The C ABI is called directly on preallocated tensors, so a window holds launches and nothing else.  HIP events around a window of calls
after one window of warm-up, the median (min .. max) of --reps windows.  At B = 1, 224^2 the launches are shorter than their enqueue:
those rows measure the host.  There is no earlier renderer on the device to compare with; no ratio is formed.  A run without a GPU fails.

    python tools/render_bench.py [--reps 5] [--out profiles/render.txt]

The block it writes replaces the one under its marker line in --out and leaves the rest of that file alone."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gator_amd import _lib, render  # noqa: E402

MARKER = '== timings: tools/render_bench.py =='
RINGS, SEGS = 82, 84
BOXES = (16, 64, 256, 1024, 4096)      # small/large-box thresholds tried (pixels of a triangle's clamped bounding box)


def uv_sphere():
    """Closed, outward-wound unit sphere: RINGS * SEGS + 2 vertices, 2 * RINGS * SEGS faces."""
    th = np.pi * (np.arange(RINGS) + 1) / (RINGS + 1)
    ph = 2 * np.pi * np.arange(SEGS) / SEGS
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.cos(th), np.ones(SEGS)), np.outer(np.sin(th), np.sin(ph))], -1).reshape(-1, 3)
    v = np.concatenate([[[0.0, 1.0, 0.0]], ring, [[0.0, -1.0, 0.0]]])
    f = []
    at = lambda r, s: 1 + r * SEGS + s % SEGS      # noqa: E731
    last = len(v) - 1
    for s in range(SEGS):
        f.append((0, at(0, s + 1), at(0, s)))
        f.append((last, at(RINGS - 1, s), at(RINGS - 1, s + 1)))
        for r in range(RINGS - 1):
            a, b, c, d = at(r, s), at(r, s + 1), at(r + 1, s + 1), at(r + 1, s)
            f += [(a, b, c), (a, c, d)]
    f = np.array(f, np.int64)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert ((n * v[f].mean(1)).sum(1) > 0).all() and len(v) == 6890 and len(f) == 13776
    return v.astype(np.float32), f


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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'render.txt'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('render_bench: no GPU, nothing to measure')
    import bench
    lib = _lib.load()
    base, faces = uv_sphere()
    r = render.MeshRenderer(faces, 'cuda:0')
    V, F = r.n_verts, r.n_faces
    lights = np.ascontiguousarray(render.DEMO_LIGHTS, np.float32)
    lp, st = lights.ctypes.data_as(ctypes.c_void_p), None
    lines = [MARKER, '%s (%s), torch %s; UV sphere of %d vertices / %d faces, radius set to cover a tenth of the frame, back faces culled'
             % (torch.cuda.get_device_name(0), getattr(torch.cuda.get_device_properties(0), 'gcnArchName', '?'), torch.__version__, V, F),
             'HIP events around a window of calls after one window of warm-up, median (min .. max) of %d windows; ms per call.' % a.reps,
             'raster = clear of the key buffer + k_render_raster.  copy = torch copy_ of the [B,H,W,3] uint8 image, the resolve launch\'s floor;',
             'resolve GB/s counts 8 B key + 3 B out (+ 3 B background) per pixel, not the per-covered-pixel gathers.', '']
    for B, H, W in ((1, 224, 224), (1, 1080, 1920), (64, 224, 224), (16, 1080, 1920)):
        iters = 200 if B * H * W < 4e6 else 20
        rad_px = np.sqrt(0.1 * W * H / np.pi)
        s = 0.8
        rng = np.random.default_rng(0)
        verts = torch.from_numpy((base[None] * s + rng.uniform(-0.05, 0.05, (B, 1, 3)) * [1, 1, 0]).astype(np.float32)).cuda()
        cam = torch.tensor([[2 * rad_px / (s * W), 2 * rad_px / (s * H), 0.0, 0.0]] * B, dtype=torch.float32, device='cuda')
        xy = torch.empty((B, V, 2), dtype=torch.int32, device='cuda')
        z = torch.empty((B, V), device='cuda')
        nrm = torch.empty((B, V, 3), device='cuda')
        keys = torch.empty((B, H, W), dtype=torch.int64, device='cuda')
        rgb = torch.empty((B, H, W, 3), dtype=torch.uint8, device='cuda')
        rgb2 = torch.empty_like(rgb)
        bg = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device='cuda')
        chk = lambda rc: _lib.check(rc, 'render_bench')      # noqa: E731
        f_vert = lambda: chk(lib.gator_render_vertices_f32(r._h, verts.data_ptr(), cam.data_ptr(), B, H, W, None, xy.data_ptr(), z.data_ptr(), nrm.data_ptr(), st))      # noqa: E731
        f_rast = lambda: chk(lib.gator_render_raster(r._h, xy.data_ptr(), z.data_ptr(), None, B, B, H, W, 1, keys.data_ptr(), st))      # noqa: E731
        f_reso = lambda b: chk(lib.gator_render_resolve(r._h, keys.data_ptr(), xy.data_ptr(), nrm.data_ptr(), None, None, B, b, B, H, W, lp, 2, 0.3,      # noqa: E731
                                                        rgb.data_ptr(), None, None, st))
        f_all = lambda b: chk(lib.gator_render_f32(r._h, verts.data_ptr(), cam.data_ptr(), None, None, B, b, B, H, W, None, lp, 2, 0.3, 1,      # noqa: E731
                                                   rgb.data_ptr(), None, None, st))
        f_vert(), f_rast(), f_reso(None), f_all(None)
        f_rast()      # the keys of the last launch feed the resolve rows
        torch.cuda.synchronize()
        covered = float((keys != -1).float().mean())
        assert torch.equal(rgb, r.render(verts, cam, size=(W, H)))
        lines.append('B = %d, %d x %d (W x H): %.3f of the pixels covered, window of %d calls' % (B, W, H, covered, iters))
        px = B * H * W
        rows = [('k_render_vertices', event_time(f_vert, iters, a.reps), None)]
        rows.append(('clear of the key buffer alone', event_time(lambda: keys.fill_(-1), iters, a.reps), 8 * px))
        for box in BOXES:
            r.set_small_box(box)
            rows.append(('raster, small box <= %d px' % box, event_time(f_rast, iters, a.reps), None))
        r.set_small_box(0)
        rows.append(('k_render_resolve, no background', event_time(lambda: f_reso(None), iters, a.reps), 11 * px))
        rows.append(('k_render_resolve, background', event_time(lambda: f_reso(bg.data_ptr()), iters, a.reps), 14 * px))
        rows.append(('copy of the image (floor)', event_time(lambda: rgb2.copy_(bg), iters, a.reps), 6 * px))
        rows.append(('gator_render_f32, no background', event_time(lambda: f_all(None), iters, a.reps), None))
        rows.append(('gator_render_f32, background', event_time(lambda: f_all(bg.data_ptr()), iters, a.reps), None))
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
