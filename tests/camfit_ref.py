"""Numpy restatement of the demo's camera fit (demo/run.py:123-164 with lib/models/project_net.py:6-17), batched over samples.

One Adam step of torch 2.10's single-tensor CPU path per iteration, on the three weak-perspective parameters of every sample:
    o = (p_xy + t) * s * r + r                      r = crop_size / 2
    loss = mean |o - target|                        nn.L1Loss over n_fit x 2 elements
    g = sign(o - target) / (2 n_fit)                sums over the joints in joint order
    m = m + (g - m) * (1 - b1);  v = v * b2 + (1 - b2) * g * g
    p = p + (-step_size * m) / (sqrt(v) / sqrt(1 - b2^t) + eps)       step_size = lr / (1 - b1^t), both factors in double

`dtype=np.float64` is the reference the device fit is judged against; `dtype=np.float32` states the kernel's own roundings."""
import numpy as np

BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
DEMO_SCHEDULE = ((0, 0.1), (500, 0.05), (1000, 0.001))


def lr_at(j, schedule=DEMO_SCHEDULE):
    """Learning rate of 0-based step j: the first pair's lr, then every later (m, lr) from step m + 1 on (the demo changes the
    rate after optimizer.step() at j == m)."""
    lr = float(schedule[0][1])
    for m, v in schedule[1:]:
        if j >= int(m) + 1:
            lr = float(v)
    return lr


def adam_factors(steps, schedule=DEMO_SCHEDULE):
    """[steps, 2] float64: (step_size, sqrt(bias_correction2)) of each step, as torch forms them in Python doubles."""
    out = np.zeros((steps, 2), np.float64)
    for j in range(steps):
        t = float(j + 1)
        out[j, 0] = lr_at(j, schedule) / (1 - BETA1 ** t)
        out[j, 1] = (1 - BETA2 ** t) ** 0.5
    return out


def project(joints3d, cam, crop_size, dtype=np.float64):
    """OptimzeCamLayer.forward for a batch: joints3d [B,J,3|2], cam [B,3] -> [B,J,2]."""
    f = np.dtype(dtype).type
    r = f(crop_size / 2)
    p = np.asarray(joints3d)[:, :, :2].astype(dtype)
    c = np.asarray(cam).astype(dtype)
    return (p + c[:, None, 1:]) * c[:, None, :1] * r + r


def l1(joints3d, target, cam, crop_size, n_fit=17, dtype=np.float64):
    o = project(np.asarray(joints3d)[:, :n_fit], cam, crop_size, dtype)
    d = np.abs(o - np.asarray(target)[:, :n_fit, :2].astype(dtype))
    acc = np.zeros(d.shape[0], dtype)
    for j in range(n_fit):
        acc = acc + d[:, j, 0]
        acc = acc + d[:, j, 1]
    return acc / dtype(2 * n_fit)


def fit(joints3d, target, init, steps=1500, schedule=DEMO_SCHEDULE, crop_size=500, n_fit=17, dtype=np.float64):
    """-> (cam [B,3], loss [B]) after `steps` Adam steps from `init`."""
    f = np.dtype(dtype).type
    p = np.asarray(joints3d)[:, :n_fit, :2].astype(dtype)
    tg = np.asarray(target)[:, :n_fit, :2].astype(dtype)
    cam = np.array(init, dtype=dtype).reshape(-1, 3)
    m = np.zeros_like(cam)
    v = np.zeros_like(cam)
    r = f(crop_size / 2)
    inv_n = f(1.0) / f(2 * n_fit)
    b1c, b2, b2c, eps = f(1 - BETA1), f(BETA2), f(1 - BETA2), f(EPS)
    tab = adam_factors(steps, schedule)
    with np.errstate(invalid='ignore', over='ignore'):
        for j in range(steps):
            s, t = cam[:, 0:1], cam[:, None, 1:]
            o1 = p + t
            o = o1 * s[:, :, None] * r + r
            sg = np.sign(o - tg)
            gr = sg * inv_n * r                        # dL/d(o1 * s)
            gs = np.zeros(cam.shape[0], dtype)
            gx = np.zeros(cam.shape[0], dtype)
            gy = np.zeros(cam.shape[0], dtype)
            for k in range(n_fit):
                gs = gs + gr[:, k, 0] * o1[:, k, 0]
                gs = gs + gr[:, k, 1] * o1[:, k, 1]
                gx = gx + gr[:, k, 0] * s[:, 0]
                gy = gy + gr[:, k, 1] * s[:, 0]
            g = np.stack([gs, gx, gy], 1)
            m = m + (g - m) * b1c
            v = v * b2 + b2c * (g * g)
            denom = np.sqrt(v) / f(tab[j, 1]) + eps
            cam = cam + (f(-tab[j, 0]) * m) / denom
    return cam, l1(joints3d, target, cam, crop_size, n_fit, dtype)


def crop_cam_to_image(cam, bbox, img_w, img_h, dtype=np.float32):
    """convert_crop_cam_to_orig_img (demo/run.py:21-39) with an explicit image width and height -> [B,4] (sx, sy, tx, ty)."""
    f = np.dtype(dtype).type
    cam = np.asarray(cam).astype(dtype)
    bbox = np.asarray(bbox).astype(dtype)
    x, y, w, h = bbox[:, 0], bbox[:, 1], bbox[:, 2], bbox[:, 3]
    cx, cy = x + w / f(2), y + h / f(2)
    hw, hh = f(img_w / 2.), f(img_h / 2.)
    with np.errstate(divide='ignore', invalid='ignore'):           # a rejected box (h = 0) gives inf / nan, as in the demo
        sx = cam[:, 0] * (f(1.) / (f(img_w) / h))
        sy = cam[:, 0] * (f(1.) / (f(img_h) / h))
        tx = ((cx - hw) / hw / sx) + cam[:, 1]
        ty = ((cy - hh) / hh / sy) + cam[:, 2]
    return np.stack([sx, sy, tx, ty], 1)
