"""The 2D pose overlay restated in numpy (gator_amd/csrc/draw2d.hip's header comment, include/gator_hip.h: gator_draw2d_u8): coverage per
primitive, the ordered integer blend, the final mix.  The device is to agree with this byte for byte, so every float64 step here is
one correctly rounded numpy operation in the order the kernel takes it, and every integer is an exact int64."""
import numpy as np

GUARD = 2 ** 20
KEYPOINTS, COCO = 0, 1
BOX_COLOR = (255, 255, 0)


def to_pixel(v):
    """float32 coordinates -> (int64 pixel, finite): astype(np.int32)'s truncation, clamped to +-2^20; 0 where not finite."""
    v = np.asarray(v, np.float32).astype(np.float64)
    ok = np.isfinite(v)
    return np.clip(np.trunc(np.where(ok, v, 0.0)), -GUARD, GUARD).astype(np.int64), ok


def to_c8(color):
    """A colour on the 0..255 scale -> three ints: float32, rounded half to even, clamped; NaN -> 0."""
    c = np.asarray(color, np.float32)
    c = np.where(np.isnan(c), np.float32(0), c)
    return tuple(int(x) for x in np.clip(np.rint(c), 0, 255))


def capsule(a, b, t, c8):
    return {'kind': 'capsule', 'a': (int(a[0]), int(a[1])), 'b': (int(b[0]), int(b[1])), 't': int(t), 'c8': tuple(c8)}


def disc(c, r, c8):
    return {'kind': 'disc', 'a': (int(c[0]), int(c[1])), 'r': int(r), 'c8': tuple(c8)}


def ring(c, r, t, c8):
    return {'kind': 'ring', 'a': (int(c[0]), int(c[1])), 'r': int(r), 't': int(t), 'c8': tuple(c8)}


def _dist(dx, dy):
    return np.sqrt((dx * dx + dy * dy).astype(np.float64))


def coverage(prim, H, W):
    """cov [H,W] float64 of one primitive, before quantisation."""
    py, px = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing='ij')
    ax, ay = prim['a']
    apx, apy = px - ax, py - ay
    if prim['kind'] == 'capsule':
        bx, by = prim['b']
        abx, aby = bx - ax, by - ay
        dot, len2 = abx * apx + aby * apy, abx * abx + aby * aby
        d_a, d_b = _dist(apx, apy), _dist(px - bx, py - by)
        cross = np.abs(abx * apy - aby * apx).astype(np.float64)
        with np.errstate(divide='ignore', invalid='ignore'):
            d_line = cross / np.sqrt(np.float64(len2))
        d = np.where(dot <= 0, d_a, np.where(dot >= len2, d_b, d_line))
        cov = (prim['t'] * 0.5 + 0.5) - d
    elif prim['kind'] == 'disc':
        cov = (prim['r'] + 0.5) - _dist(apx, apy)
    else:
        cov = (prim['t'] * 0.5 + 0.5) - np.abs(_dist(apx, apy) - np.float64(prim['r']))
    return np.clip(cov, 0.0, 1.0)


def quantise(cov):
    return np.floor(255.0 * cov + 0.5).astype(np.int64)


def coverage_q(prim, H, W):
    return quantise(coverage(prim, H, W))


def blend(canvas, q, c8):
    """canvas [H,W,3] integer, q [H,W]: dst = (dst (255 - q) + c8 q + 127) // 255 per channel, in place on an int64 canvas."""
    for k in range(3):
        canvas[:, :, k] = (canvas[:, :, k] * (255 - q) + c8[k] * q + 127) // 255
    return canvas


def mix(img, canvas, alpha):
    """cv2.addWeighted(img, 1 - alpha, canvas, alpha, 0) as float32: two products, one sum, rounded half to even, clamped."""
    a = np.float32(alpha)
    w = np.float32(1) - a
    s = img.astype(np.float32) * w + canvas.astype(np.float32) * a
    return np.clip(np.rint(s), 0, 255).astype(np.uint8)


def person_prims(joints, skeleton, colors, bbox=None, kp_thre=0.4, style=KEYPOINTS):
    """joints [J,2|3] float32, colors [L,3], bbox [4,2] or None -> the person's primitives in drawing order (skipped ones left out)."""
    joints = np.asarray(joints, np.float32)
    prims = []
    if bbox is not None:
        xy, ok = to_pixel(np.asarray(bbox, np.float32).reshape(4, 2))
        ok = ok.all(1)
        for k in range(4):
            n = (k + 1) % 4
            if ok[k] and ok[n]:
                prims.append(capsule(xy[k], xy[n], 1, BOX_COLOR))
    xy, fin = to_pixel(joints[:, :2])
    good = fin.all(1)
    if joints.shape[1] == 3:
        good &= joints[:, 2] > np.float32(kp_thre)
    for l, (i1, i2) in enumerate(skeleton):
        c8 = to_c8(colors[l])
        if good[i1] and good[i2]:
            prims.append(capsule(xy[i1], xy[i2], 2, c8))
        for i in (i1, i2):
            if good[i]:
                prims.append(ring(xy[i], 2, 3, c8) if style == COCO else disc(xy[i], 3, c8))
    return prims


def draw_prims(img, prims, alpha=1.0):
    """One frame [H,W,3] uint8 and its primitives in order -> the frame drawn."""
    H, W = img.shape[:2]
    canvas = img.astype(np.int64)
    for p in prims:
        blend(canvas, coverage_q(p, H, W), p['c8'])
    return mix(img, canvas, alpha)


def draw(images, joints, skeleton, colors, bbox=None, image_index=None, kp_thre=0.4, alpha=1.0, style=KEYPOINTS):
    """images [N,H,W,3] uint8, joints [P,J,2|3], bbox [P,4,2] or None, image_index [P] or None (person p in image p) -> [N,H,W,3]."""
    images = np.asarray(images, np.uint8)
    out = np.empty_like(images)
    idx = np.arange(len(joints)) if image_index is None else np.asarray(image_index)
    for n in range(len(images)):
        prims = []
        for p in np.nonzero(idx == n)[0]:
            prims += person_prims(joints[p], skeleton, colors, None if bbox is None else bbox[p], kp_thre, style)
        out[n] = draw_prims(images[n], prims, alpha)
    return out
