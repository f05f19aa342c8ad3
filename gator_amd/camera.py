"""The demo's camera step on the device (demo/run.py:21-39,123-164): from raw 2D joints and the model's 3D joints to the weak-perspective
camera that lays the mesh over the image.

  raw joints [B,J,2|3] --crop_joints-->  target in crop pixels [B,J(+2),2], bbox1 [B,4], valid [B]        demo/run.py:124-127
  forward_joints' joints [B,n,3] + target --fit_camera-->  cam [B,3] (s, tx, ty), loss [B][, orig_cam [B,4]]   demo/run.py:138-157,21-39

fit_camera runs the reference's 1500 Adam steps of models.project_net.OptimzeCamLayer for every sample of the batch in one launch;
fit_mesh_to_image is the demo's whole flow, batched; render_fit draws its result over the frames (gator_amd.render, demo/renderer.py) and
draw_fit the detections it started from (gator_amd.vis, lib/vis.py)."""
import ctypes

import numpy as np
import torch

from . import _lib

DEMO_SCHEDULE = ((0, 0.1), (500, 0.05), (1000, 0.001))     # demo/run.py:135,154-157: lr 0.1, 0.05 after step 500, 0.001 after step 1000
DEMO_CROP = 500                                             # demo/run.py:177 virtual_crop_size



def crop_joints(joints, crop_size=DEMO_CROP, box_scale=1.25, box_aspect=1.0, add_pelvis_neck=False):
    """joints [B,J,2|3] f32 on a HIP device (pixels) -> (xy [B,J(+2),2] in crop pixels, bbox [B,4] = bbox1 (x, y, w, h),
    valid [B] int32: 0 where process_bbox rejects the box; xy and bbox are 0 there).  crop_size is an int or (width, height)."""
    _lib.need_device('crop_joints', joints, what='joints')
    if joints.dim() != 3 or joints.shape[2] < 2:
        raise ValueError('crop_joints: expected [B,J,2|3], got %s' % (tuple(joints.shape),))
    cw, ch = (crop_size, crop_size) if np.isscalar(crop_size) else crop_size
    x = joints.contiguous().float()
    B, J, C = x.shape
    dev = x.device
    xy = torch.empty((B, J + (2 if add_pelvis_neck else 0), 2), device=dev, dtype=torch.float32)
    bbox = torch.empty((B, 4), device=dev, dtype=torch.float32)
    valid = torch.empty((B,), device=dev, dtype=torch.int32)
    _lib.check(_lib.load().gator_crop_joints_f32(x.data_ptr(), B, J, C, int(bool(add_pelvis_neck)), float(box_aspect), float(box_scale),
                                                 int(cw), int(ch), xy.data_ptr(), bbox.data_ptr(), valid.data_ptr(), _lib.stream_ptr(dev)),
               'gator_crop_joints_f32')
    return xy, bbox, valid


def fit_camera(joints3d, target, init=None, steps=1500, schedule=DEMO_SCHEDULE, crop_size=DEMO_CROP, n_fit=17, bbox=None, image_size=None):
    """Fit the weak-perspective camera of every sample: joints3d [B,n,3] (metres), target [B,m,2] (crop pixels), both on one HIP
    device; the first n_fit joints of each are used.  init [B,3] (default: torch.rand on the device, as OptimzeCamLayer draws it).
    schedule: up to 8 (milestone, lr) pairs -- the first lr from step 0, every later lr from step milestone + 1.
    -> (cam [B,3], loss [B]) or, with bbox [B,4] and image_size = (width, height), (cam, loss, orig_cam [B,4] = (sx, sy, tx, ty))."""
    _lib.need_device('fit_camera', joints3d, target)
    if joints3d.dim() != 3 or joints3d.shape[2] != 3 or target.dim() != 3 or target.shape[2] != 2 or target.shape[0] != joints3d.shape[0]:
        raise ValueError('fit_camera: expected joints3d [B,n,3] and target [B,m,2], got %s and %s' % (tuple(joints3d.shape), tuple(target.shape)))
    if (bbox is None) != (image_size is None):
        raise ValueError('fit_camera: bbox and image_size go together')
    dev = joints3d.device
    p = joints3d.contiguous().float()
    t = target.to(dev).contiguous().float()
    B = p.shape[0]
    c0 = torch.rand((B, 3), device=dev) if init is None else torch.as_tensor(init, dtype=torch.float32, device=dev).reshape(B, 3).contiguous()
    sched = list(schedule)
    ms = (ctypes.c_int32 * max(len(sched), 1))(*[int(m) for m, _ in sched])
    lrs = (ctypes.c_double * max(len(sched), 1))(*[float(v) for _, v in sched])
    cam = torch.empty((B, 3), device=dev, dtype=torch.float32)
    loss = torch.empty((B,), device=dev, dtype=torch.float32)
    bb = oc = None
    w = h = 0.0
    if bbox is not None:
        bb = torch.as_tensor(bbox, dtype=torch.float32, device=dev).reshape(B, 4).contiguous()
        oc = torch.empty((B, 4), device=dev, dtype=torch.float32)
        w, h = float(image_size[0]), float(image_size[1])
    _lib.check(_lib.load().gator_fit_camera_f32(p.data_ptr(), B, p.shape[1], t.data_ptr(), t.shape[1], int(n_fit), c0.data_ptr(), int(crop_size),
                                                int(steps), ms, lrs, len(sched), _lib.ptr(bb), w, h, cam.data_ptr(),
                                                loss.data_ptr(), _lib.ptr(oc), _lib.stream_ptr(dev)),
               'gator_fit_camera_f32')
    return (cam, loss) if oc is None else (cam, loss, oc)


def fit_mesh_to_image(model, raw_joints, joint_set, image_size, init=None, steps=1500, schedule=DEMO_SCHEDULE, crop_size=DEMO_CROP):
    """The demo's flow (demo/run.py:193-211 with optimize_cam_param, :123-164) for a batch of detections.
    model: a gator_amd GATOR with its joint regressor registered (set_joint_regressor: the COCO one for 'coco', the H36M one for 'human36');
    raw_joints [B,17,2|3] pixels on the model's device; image_size = (width, height) of the images.
    -> dict of mesh [B,6890,3], pose3d, joints (regressed, metres), cam [B,3], orig_cam [B,4], bbox [B,4], loss [B], valid [B]."""
    from . import preprocess
    if joint_set not in ('coco', 'human36'):
        raise ValueError("fit_mesh_to_image: joint_set is 'coco' or 'human36', got %r" % (joint_set,))
    coco = joint_set == 'coco'
    x = raw_joints.contiguous().float()
    pose2d = preprocess.normalise_pose2d(x, add_pelvis_neck=coco)
    joints, pose3d, mesh = model.forward_joints(pose2d, with_verts=True)
    target, bbox, valid = crop_joints(x, crop_size, add_pelvis_neck=coco)
    cam, loss, orig_cam = fit_camera(joints, target, init=init, steps=steps, schedule=schedule, crop_size=crop_size,
                                     n_fit=joints.shape[1], bbox=bbox, image_size=image_size)
    return {'mesh': mesh, 'pose3d': pose3d, 'joints': joints, 'cam': cam, 'orig_cam': orig_cam, 'bbox': bbox, 'loss': loss, 'valid': valid}


def render_fit(fit, faces_or_renderer, images=None, image_size=None, colors=None):
    """fit_mesh_to_image's dict -> the overlay images [B,H,W,3] uint8 on the device (gator_amd.render: the demo's renderer, batched).
    faces_or_renderer: the mesh's faces [F,3] or a render.MeshRenderer to reuse (its workspace then serves every call);
    images: [B,H,W,3] uint8 on the device to draw over, or None (black) with image_size = (width, height); colors: (3,) or [B,3]."""
    from . import render
    mesh, cam = fit['mesh'], fit['orig_cam']
    if images is None and image_size is None:
        raise ValueError('render_fit: give images or image_size = (width, height)')
    if images is not None:
        size = (int(images.shape[2]), int(images.shape[1]))
        if image_size is not None and (int(image_size[0]), int(image_size[1])) != size:
            raise ValueError('render_fit: image_size %s does not match images of %d x %d (width x height)' % (tuple(image_size), size[0], size[1]))
    else:
        size = (int(image_size[0]), int(image_size[1]))
    r = faces_or_renderer if isinstance(faces_or_renderer, render.MeshRenderer) else render.MeshRenderer(faces_or_renderer, mesh.device, n_verts=mesh.shape[1])
    return r.render(mesh, cam, background=images, color=render.DEMO_COLOR if colors is None else colors, size=size)


def draw_fit(fit, raw_joints, skeleton, images, add_pelvis_neck=False, box=False, kp_thre=0.4, alpha=1.0, colors=None, out=None):
    """The detections over the frames, next to render_fit (demo/run.py:214-219, batched): raw_joints [B,17,2|3] is what fit_mesh_to_image
    was given, images [B,H,W,3] uint8 on its device.  skeleton: the joint set's limb pairs, or a vis.SkeletonDrawer to reuse.
    add_pelvis_neck appends the two extra COCO joints by crop_joints' rule (the mean of the hips and of the shoulders; demo/run.py:103-121
    gives them the product of the two confidences).  A third column is the detector's confidence, tested against kp_thre; the demo draws
    every joint (two columns).  box=True also draws fit['bbox'], the box the camera was fitted in.  -> [B,H,W,3] uint8 on the device."""
    from . import vis
    _lib.need_device('draw_fit', raw_joints, images)
    x = raw_joints.contiguous().float()
    if x.dim() != 3 or x.shape[2] not in (2, 3):
        raise ValueError('draw_fit: expected raw_joints [B,J,2|3], got %s' % (tuple(x.shape),))
    if add_pelvis_neck:
        if x.shape[1] < 17:
            raise ValueError('draw_fit: add_pelvis_neck needs the 17 COCO joints, got %d' % x.shape[1])
        extra = torch.stack([(x[:, 11] + x[:, 12]) * 0.5, (x[:, 5] + x[:, 6]) * 0.5], 1)
        if x.shape[2] == 3:
            extra[:, 0, 2] = x[:, 11, 2] * x[:, 12, 2]
            extra[:, 1, 2] = x[:, 5, 2] * x[:, 6, 2]
        x = torch.cat([x, extra], 1)
    corners = None
    if box:
        b = fit['bbox'].to(x.device).float()
        x0, y0, x1, y1 = b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]
        corners = torch.stack([torch.stack([x0, y0], 1), torch.stack([x1, y0], 1), torch.stack([x1, y1], 1), torch.stack([x0, y1], 1)], 1)
    d = skeleton if isinstance(skeleton, vis.SkeletonDrawer) else vis.SkeletonDrawer(skeleton, x.shape[1], x.device)
    return d.draw(images, x, colors=colors, bbox=corners, kp_thre=kp_thre, alpha=alpha, out=out)
