"""Camera-frame training batches on the device: the deterministic part of the datasets' __getitem__ (data/Human36M/dataset.py:254-309,
339-407, data/AMASS/dataset.py:182-304, PW3D / COCO / MuCo alike) for a whole batch, around gator_amd.smpl.SMPLLayer:

  root_to_camera(pose, R)            the root orientation composed with the camera rotation        -> gator_batch_prepare_f32
  camera_frame_batch(layer, ...)     (inputs, targets, meta), the triple the datasets return       -> gator_batch_prepare_f32,
                                     the layer, gator_camera_targets_f32, preprocess.preprocess_chain
                                     or, with noise=, gator_amd.noise.noisy_input

The kernels are csrc/train_batch.hip.  Every output is a pure function of the inputs -- with noise=, of the inputs, noise_seed and
noise_step: the detector noise (lib/noise_utils.py, generate_syn_error) is gator_amd.noise's.  There is no CPU path."""
import ctypes

import numpy as np
import torch

from . import _lib
from . import eval as gator_eval
from . import preprocess

SMPL_ROOT = 0                    # smpl_root_joint_idx of every dataset (lib/smpl.py)
COCO_MIN_JOINTS = 13             # add_pelvis_and_neck reads joints 5, 6, 11, 12
MAX_LIFT_JOINTS = 64             # csrc/train_batch.hip: kCamMaxJoints
LIFT_SETS = {'human36': _lib.LIFT_HUMAN36, 'coco': _lib.LIFT_COCO}


def _tensor(x, who, name):
    if x is None:
        return None
    if not isinstance(x, torch.Tensor):
        raise ValueError('%s: %s must be a tensor, got %s' % (who, name, type(x).__name__))
    return x


def _rows(x, shape, who, name, device, dtype=torch.float32, broadcast=False):
    """x as a contiguous tensor of `shape` = (B, ...); broadcast: x may come without the leading B."""
    x = _tensor(x, who, name)
    if x is None:
        return None
    if broadcast and tuple(x.shape) == tuple(shape[1:]):
        x = x.unsqueeze(0).expand(shape)
    if tuple(x.shape) != tuple(shape):
        raise ValueError('%s: %s must be %s, got %s' % (who, name, list(shape), list(x.shape)))
    if dtype == torch.float32 and not x.is_floating_point():
        raise ValueError('%s: %s must be a floating-point tensor, got %s' % (who, name, x.dtype))
    if x.device != device:
        raise ValueError('%s: %s lives on %s, the pose on %s' % (who, name, x.device, device))
    return x.to(dtype).contiguous()


def _checked_pose(pose, n_joints, who):
    pose = _tensor(pose, who, 'pose')
    if pose is None or pose.dim() != 2 or pose.shape[0] < 1 or pose.shape[1] != n_joints * 3 or not pose.is_floating_point():
        raise ValueError('%s: pose must be a floating-point tensor [B,%d] with B >= 1, got %s' %
                         (who, n_joints * 3, None if pose is None else (list(pose.shape), pose.dtype)))
    return pose


def _launch_prepare(pose, R, betas, root_idx, pose_out, betas_out):
    """pose [B,NJ*3], R [B,3,3] | None, betas [B,NB] | None: contiguous float32 on one HIP device.  One launch."""
    _lib.check(_lib.load().gator_batch_prepare_f32(pose.data_ptr(), _lib.ptr(R), _lib.ptr(betas), pose.shape[0], pose.shape[1],
                                                   0 if betas is None else betas.shape[1], int(root_idx), pose_out.data_ptr(),
                                                   _lib.ptr(betas_out), _lib.stream_ptr(pose.device)), 'gator_batch_prepare_f32')
    return pose_out, betas_out


def root_to_camera(pose, R, root_idx=SMPL_ROOT):
    """The datasets' "rotate global pose" (data/Human36M/dataset.py:267-274, data/AMASS/dataset.py:188-196) for a batch: pose [B,NJ*3]
    with joint root_idx replaced by the rotation vector of R @ exp(root); R [B,3,3] or [3,3].  fp64 on the device, angle in [0, pi].
    A zero root vector is the identity rotation (the reference yields NaN there); every other joint is copied bit for bit."""
    who = 'root_to_camera'
    pose = _tensor(pose, who, 'pose')
    if pose is None or pose.dim() != 2 or pose.shape[0] < 1 or pose.shape[1] < 3 or pose.shape[1] % 3 or not pose.is_floating_point():
        raise ValueError('%s: pose must be a floating-point tensor [B,NJ*3] with B >= 1' % who)
    if not 0 <= int(root_idx) < pose.shape[1] // 3:
        raise ValueError('%s: root joint %d outside [0, %d)' % (who, int(root_idx), pose.shape[1] // 3))
    if R is None:
        raise ValueError('%s: R is required' % who)
    R = _rows(R, (pose.shape[0], 3, 3), who, 'R', pose.device, broadcast=True)
    _lib.need_device(who, pose)
    p = pose.float().contiguous()
    with torch.cuda.device(p.device):
        return _launch_prepare(p, R, None, root_idx, torch.empty_like(p), None)[0]


def _camera_targets_args(verts, joints, trans, cam_t, R, compensate_root, focal, princpt, reg_h, reg_c, lift_set, joint_cam, joint_img,
                         rot, flip, pairs, fitting_thr, root_idx, mesh, reg_pose3d, lift_pose3d, joint_img_out, fit_error, valid):
    """gator_camera_targets_args of contiguous float32 (flip, pairs: int32) tensors on one HIP device, checked by the caller; reg_h /
    reg_c: what eval._as_coo returns (reg_c may be None).  The struct holds addresses only: the tensors must outlive the launch."""
    a = _lib.CameraTargetsArgs()
    a.struct_size = ctypes.sizeof(_lib.CameraTargetsArgs)
    a.batch, a.n_verts, a.n_smpl_joints, a.root_idx = verts.shape[0], verts.shape[1], joints.shape[1], int(root_idx)
    a.compensate_root, a.lift_set, a.n_pairs = int(bool(compensate_root)), int(lift_set), 0 if pairs is None else int(pairs.shape[0])
    a.fitting_thr = float(fitting_thr)
    a.verts, a.joints, a.trans, a.cam_t, a.R = verts.data_ptr(), joints.data_ptr(), _lib.ptr(trans), _lib.ptr(cam_t), _lib.ptr(R)
    a.focal, a.princpt = focal.data_ptr(), princpt.data_ptr()
    a.reg_h36m, a.reg_h36m_n_verts = gator_eval._coo_struct(reg_h), _n_verts(reg_h)
    if reg_c is not None:
        a.reg_coco, a.reg_coco_n_verts = gator_eval._coo_struct(reg_c), _n_verts(reg_c)
    a.joint_cam, a.joint_img, a.rot_deg, a.flip = _lib.ptr(joint_cam), _lib.ptr(joint_img), _lib.ptr(rot), _lib.ptr(flip)
    a.flip_pairs = _lib.ptr(pairs) if a.n_pairs else None
    a.mesh, a.reg_pose3d, a.lift_pose3d = mesh.data_ptr(), reg_pose3d.data_ptr(), lift_pose3d.data_ptr()
    a.joint_img_out, a.fit_error, a.valid = joint_img_out.data_ptr(), fit_error.data_ptr(), valid.data_ptr()
    return a


def _launch_camera_targets(verts, *rest):
    """_camera_targets_args' arguments.  One launch; nothing is allocated and the host does not wait."""
    a = _camera_targets_args(verts, *rest)
    _lib.check(_lib.load().gator_camera_targets_f32(ctypes.byref(a), _lib.stream_ptr(verts.device)), 'gator_camera_targets_f32')


def _n_verts(reg):
    return gator_eval.N_VERTS if isinstance(reg, gator_eval.JointRegressor) else reg.n_verts


def _checked_pairs(flip_pairs, n_lift, who):
    try:
        pairs = [(int(u), int(v)) for u, v in flip_pairs]
    except (TypeError, ValueError):
        raise ValueError('%s: flip_pairs must be pairs of joint indices' % who)
    for u, v in pairs:
        if not (0 <= u < n_lift and 0 <= v < n_lift):
            raise ValueError('%s: flip pair (%d, %d) outside the %d joints of the lift set' % (who, u, v, n_lift))
    return pairs


def camera_frame_batch(layer, pose, shape, *, trans=None, cam_R=None, cam_t=None, compensate_root=False, focal, princpt, regressor_h36m,
                       regressor_coco=None, input_joint_name='human36', joint_cam=None, joint_img=None, fitting_thr=float('inf'),
                       rot_deg=None, flip=None, flip_pairs=(), res=(288, 384), noise=None, noise_seed=0, noise_step=0):
    """The deterministic part of a training dataset's __getitem__ for a batch on the device -> (inputs, targets, meta), the triple the
    datasets return (data/Human36M/dataset.py:403-407):

      inputs   {'pose2d' [B,Jl,2]}                                    the cropped, standardised 2D input (preprocess.preprocess_chain)
      targets  {'mesh' [B,NV,3] m, 'lift_pose3d' [B,Jl,3] mm, 'reg_pose3d' [B,Jh,3] mm}, root-relative
      meta     {'mesh_valid' [B,NV,1], 'lift_pose3d_valid' [B,Jl,1], 'reg_pose3d_valid' [B,Jh,1]}  broadcast views of one [B,3] tensor,
               {'fit_error' [B] mm (NaN without joint_cam), 'input_valid' [B] int32 (0 where process_bbox rejects the box and the
               reference drops the sample), 'joint_img' [B,Jl,2] pixels}

    `targets | meta` is what Trainer.step takes.  layer: gator_amd.smpl.SMPLLayer; pose [B,NJ*3], shape [B,NB] | None in the fit's own
    frame; cam_R [B,3,3] | [3,3]: the root orientation becomes R exp(root) (Human36M:267-274, AMASS:188-196; a zero root vector is the
    identity here, NaN in the reference) and a shape with any |beta| > 3 the mean shape (Human36M:265).  The translation, metres:
    compensate_root=False: trans + cam_t, a missing one counting as 0 (AMASS: cam_t; PW3D / COCO / MuCo: trans); compensate_root=True:
    R trans + cam_t - root + R root with the layer's root joint (Human36M:288-292, cam_t = t / 1000).  focal, princpt [B,2] | [2]:
    cam2pixel (lib/coord_utils.py:104-109).  regressor_h36m / regressor_coco: eval.JointRegressor, a dense [n_joint, NV] array or
    eval._Coo; input_joint_name 'human36' | 'coco' picks the lift set (coco: + pelvis and neck, relative to the pelvis).
    joint_cam [B,Jh,3] mm and joint_img [B,Jh,2|3]: the dataset's own joints (Human3.6M): they give the root, reg_pose3d, the human36
    input and the fitting error; fit_error > fitting_thr clears mesh_valid, and lift_pose3d_valid too for coco (Human36M:396-401).
    rot_deg [B], flip [B], flip_pairs: the augmentation, applied to lift_pose3d (j3d_processing, lib/aug_utils.py:67-83) and to the 2D
    input -- never to the mesh, as in the reference.

    noise: a gator_amd.noise.CocoDetectorNoise or ErrorStatsNoise (use_gt_input: False, the reference's replace_joint_img): the
    reference adds the detector noise AFTER the crop affine, in crop pixels, before the flip -- not in image pixels -- so
    inputs['pose2d'] is then noise.noisy_input(meta['joint_img'], noise, seed=noise_seed, step=noise_step, rot_deg=.., flip=..,
    flip_pairs=.., res=res), bit for bit; meta['joint_img'] stays the clean pixel-space input and meta['joint_crop_noisy'] [B,Jl,2]
    holds the perturbed crop-space joints.  noise_step: an int or a one-element int64 tensor on the device (see noisy_input; row b is
    sample b of the stream -- a sharded caller calls noisy_input itself with its sample_offset).  With noise=None (the default)
    nothing changes.

    Launches: gator_batch_prepare_f32, the layer's two (metres, no translation, no centring), gator_camera_targets_f32 writing the mesh
    into the layer's vertex buffer in place, and preprocess_chain (or noisy_input's two or three).  Nothing waits for the device."""
    who = 'camera_frame_batch'
    for name in ('num_verts', 'num_joints', 'num_betas', 'forward'):
        if not hasattr(layer, name):
            raise ValueError('%s: layer must be a gator_amd.smpl.SMPLLayer (no %s)' % (who, name))
    NV, NJ, NB = layer.num_verts, layer.num_joints, layer.num_betas
    pose = _checked_pose(pose, NJ, who)
    B, dev = pose.shape[0], pose.device
    if input_joint_name not in LIFT_SETS:
        raise ValueError("%s: input_joint_name is 'coco' or 'human36', got %r" % (who, input_joint_name))
    coco = input_joint_name == 'coco'
    if coco and regressor_coco is None:
        raise ValueError("%s: input_joint_name 'coco' needs regressor_coco" % who)
    if compensate_root and cam_R is None:
        raise ValueError('%s: compensate_root needs cam_R' % who)
    if regressor_h36m is None:
        raise ValueError('%s: regressor_h36m is required' % who)
    betas = _rows(shape, (B, NB), who, 'shape', dev) if NB else None
    trans = _rows(trans, (B, 3), who, 'trans', dev)
    cam_t = _rows(cam_t, (B, 3), who, 'cam_t', dev)
    R = _rows(cam_R, (B, 3, 3), who, 'cam_R', dev, broadcast=True)
    if focal is None or princpt is None:
        raise ValueError('%s: focal and princpt are required' % who)
    focal = _rows(focal, (B, 2), who, 'focal', dev, broadcast=True)
    princpt = _rows(princpt, (B, 2), who, 'princpt', dev, broadcast=True)
    reg_h = gator_eval._as_coo(regressor_h36m, NV, dev, who)
    reg_c = None if regressor_coco is None else gator_eval._as_coo(regressor_coco, NV, dev, who)
    Jh = reg_h.n_joint
    if reg_c is not None and not COCO_MIN_JOINTS <= reg_c.n_joint <= MAX_LIFT_JOINTS - 2:
        raise ValueError('%s: a coco regressor of %d joints (%d..%d: pelvis and neck come from joints 5, 6, 11, 12)'
                         % (who, reg_c.n_joint, COCO_MIN_JOINTS, MAX_LIFT_JOINTS - 2))
    Jl = reg_c.n_joint + 2 if coco else Jh
    joint_cam = _rows(joint_cam, (B, Jh, 3), who, 'joint_cam', dev)
    joint_img = _tensor(joint_img, who, 'joint_img')
    if joint_img is not None:
        if joint_img.dim() != 3 or joint_img.shape[2] not in (2, 3):
            raise ValueError('%s: joint_img must be [%d,%d,2|3], got %s' % (who, B, Jh, list(joint_img.shape)))
        joint_img = _rows(joint_img[:, :, :2], (B, Jh, 2), who, 'joint_img', dev)
    if joint_cam is not None and joint_img is None and not coco:
        raise ValueError("%s: the dataset's joint_cam needs its joint_img for input_joint_name 'human36'" % who)
    thr = float(fitting_thr)
    if np.isnan(thr):
        raise ValueError('%s: fitting_thr is NaN' % who)
    if rot_deg is not None and not isinstance(rot_deg, torch.Tensor):
        rot_deg = torch.as_tensor(np.asarray(rot_deg, np.float32), device=dev)
    if flip is not None and not isinstance(flip, torch.Tensor):
        flip = torch.as_tensor(np.asarray(flip).astype(np.int32), device=dev)
    if flip is not None and (flip.is_floating_point() or flip.is_complex()):
        raise ValueError('%s: flip must be boolean or integer, got %s' % (who, flip.dtype))
    rot = _rows(rot_deg, (B,), who, 'rot_deg', dev)
    fl = _rows(flip, (B,), who, 'flip', dev, dtype=torch.int32)
    pair_list = _checked_pairs(flip_pairs, Jl, who)
    try:
        res = (int(res[0]), int(res[1]))
    except (TypeError, ValueError, IndexError):
        raise ValueError('%s: res must be (width, height)' % who)
    if res[0] < 1 or res[1] < 1:
        raise ValueError('%s: res %s must be positive' % (who, (res,)))
    if noise is not None:
        from . import noise as gator_noise
        if not isinstance(noise, (gator_noise.CocoDetectorNoise, gator_noise.ErrorStatsNoise)):
            raise ValueError('%s: noise must be a gator_amd.noise.CocoDetectorNoise or ErrorStatsNoise, got %s' % (who, type(noise).__name__))
        if isinstance(noise, gator_noise.CocoDetectorNoise) and Jl < gator_noise.COCO_JOINTS:
            raise ValueError('%s: CocoDetectorNoise needs the %d COCO joints first, the lift set has %d' % (who, gator_noise.COCO_JOINTS, Jl))
        if isinstance(noise, gator_noise.ErrorStatsNoise) and noise.n_joints != Jl:
            raise ValueError('%s: the error table has %d joints, the lift set %d' % (who, noise.n_joints, Jl))
    _lib.need_device(who, pose)

    with torch.cuda.device(dev):
        p = pose.float().contiguous()
        pose_c, betas_c = p, betas
        if R is not None or betas is not None:
            pose_c = torch.empty_like(p) if R is not None else p
            betas_c = None if betas is None else torch.empty_like(betas)
            _launch_prepare(p, R, betas, SMPL_ROOT, pose_c, betas_c)
        saved = layer.out_scale, layer.center_idx
        layer.out_scale, layer.center_idx = 1.0, None
        try:
            verts, joints = layer.forward(pose_c, betas_c, None)
        finally:
            layer.out_scale, layer.center_idx = saved
        pairs = torch.as_tensor(pair_list, dtype=torch.int32, device=dev).reshape(-1, 2).contiguous() if pair_list else None
        reg3d = torch.empty((B, Jh, 3), device=dev, dtype=torch.float32)
        lift3d = torch.empty((B, Jl, 3), device=dev, dtype=torch.float32)
        img = torch.empty((B, Jl, 2), device=dev, dtype=torch.float32)
        fit = torch.empty((B,), device=dev, dtype=torch.float32)
        valid = torch.empty((B, 3), device=dev, dtype=torch.float32)
        _launch_camera_targets(verts, joints, trans, cam_t, R, compensate_root, focal, princpt, reg_h, reg_c, LIFT_SETS[input_joint_name],
                               joint_cam, joint_img, rot, fl, pairs, thr, SMPL_ROOT, verts, reg3d, lift3d, img, fit, valid)
        if noise is None:
            pose2d, input_valid = preprocess.preprocess_chain(img, rot, fl, pair_list, res=res)
        else:
            pose2d, input_valid, crop_noisy = gator_noise.noisy_input(img, noise, seed=noise_seed, step=noise_step, rot_deg=rot, flip=fl,
                                                                      flip_pairs=pair_list, res=res)
    inputs = {'pose2d': pose2d}
    targets = {'mesh': verts, 'lift_pose3d': lift3d, 'reg_pose3d': reg3d}
    meta = {'mesh_valid': valid[:, 0].reshape(B, 1, 1).expand(B, NV, 1), 'lift_pose3d_valid': valid[:, 1].reshape(B, 1, 1).expand(B, Jl, 1),
            'reg_pose3d_valid': valid[:, 2].reshape(B, 1, 1).expand(B, Jh, 1), 'fit_error': fit, 'input_valid': input_valid, 'joint_img': img}
    if noise is not None:
        meta['joint_crop_noisy'] = crop_noisy
    return inputs, targets, meta
