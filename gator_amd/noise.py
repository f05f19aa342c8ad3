"""The detector noise of the training input on the device (use_gt_input: False, every *_train_*.yml of the reference): the datasets'
replace_joint_img step (data/Human36M/dataset.py:369-389, 421-453) inside the input chain of preprocess.preprocess_chain --

  box -> process_bbox -> crop affine (rotation) -> float32 crop joints -> NOISE, in crop pixels -> flip -> /[W,H] -> standardise

  CocoDetectorNoise()                  lib/noise_utils.synthesize_pose: the PoseFix-style jitter / miss / inversion / good synthesis
  ErrorStatsNoise(mean, std, weight)   generate_syn_error from a per-joint error table (the caller's: the Human3.6M table is the
                                       reference's data and is not shipped)
  noisy_input(joint_img, model, ...)   -> (pose2d, input_valid, noisy_crop); model=None with detections=: the test split's branch

The algorithm is the reference's with numpy's generators replaced by a Philox4x32 stream keyed by (seed, step, sample index): a
sample's row is the same bits whatever the batch or its sharding (include/gator_hip.h: gator_preprocess_noise_f32 has the stream's
layout, csrc/detector_noise.hip the kernels).  There is no CPU path."""
import ctypes
import math

import numpy as np
import torch

from . import _lib

COCO_JOINTS = _lib.NOISE_COCO_JOINTS
MAX_JOINTS = 32                                   # csrc/internal.h: kMaxJ
CASES = ('jitter', 'miss', 'inversion', 'swap', 'good')          # decisions[..., 5]; -1: the joint was zeroed


class CocoDetectorNoise:
    """The rule table of lib/noise_utils.synthesize_pose, as data.  sigmas: the COCO keypoint sigmas (kps_sigmas before the / 10);
    symmetry: kps_symmetry; the probabilities are per joint group and tier of the number of valid joints among the 17
    (jitter: <= 10 | more; miss: <= 5 | <= 10 | more); candidates per set.  swap never happens (near_joints is empty at every call
    site) and its probability goes to the good case, as in the reference."""
    sigmas = (.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89)
    symmetry = ((1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16))
    ks = (0.10, 0.50, 0.85)
    tier_valid = (5, 10)
    n_jitter, n_miss, n_inv, n_good = 500, 2000, 500, 125

    @staticmethod
    def jitter_prob(j, tier):
        """tier 0: at most 10 valid joints; 1: more"""
        group = 0 if j == 0 or 13 <= j <= 16 else 1 if 1 <= j <= 10 else 2          # nose, knee, ankle | ear, eye, upper body | hip
        return ((0.15, 0.20, 0.25), (0.10, 0.15, 0.20))[tier][group]

    @staticmethod
    def miss_prob(j, tier):
        """tier 0: at most 5 valid joints; 1: at most 10; 2: more"""
        group = 0 if j <= 4 else 1 if j in (5, 6, 15, 16) else 2                      # face | shoulder, ankle | other parts
        return ((0.15, 0.20, 0.25), (0.10, 0.13, 0.15), (0.02, 0.05, 0.10))[tier][group]

    @staticmethod
    def inv_prob(j):
        return 0.01 if j <= 4 else 0.03 if j <= 10 else 0.06                          # face | upper body | lower body

    def partner(self):
        p = [-1] * COCO_JOINTS
        for q, w in self.symmetry:
            p[q], p[w] = w, q
        return p

    def struct(self):
        """-> _lib.CocoNoiseModel.  The doubles are computed here, once, with numpy as the reference computes them."""
        m = _lib.CocoNoiseModel()
        var = (np.array(self.sigmas) / 10.0 * 2) ** 2
        for j in range(COCO_JOINTS):
            m.var[j] = float(var[j])
            m.inv_prob[j] = self.inv_prob(j)
            for t in range(2):
                m.jitter_prob[t][j] = self.jitter_prob(j, t)
            for t in range(3):
                m.miss_prob[t][j] = self.miss_prob(j, t)
            m.partner[j] = self.partner()[j]
        for k in range(3):
            m.log_ks[k] = float(np.log(self.ks[k]))
        m.n_jitter, m.n_miss, m.n_inv, m.n_good = self.n_jitter, self.n_miss, self.n_inv, self.n_good
        m.tier_valid[0], m.tier_valid[1] = self.tier_valid
        return m


class ErrorStatsNoise:
    """generate_syn_error's table: mean [J,2], std [J,2] in pixels of a 256-pixel crop, weight [J] = the probability that a joint
    is perturbed.  (The reference reads them from data/Human36M/noise_stats.py, in the order of its joints.)"""

    def __init__(self, mean, std, weight):
        mean, std, weight = (np.asarray(v, np.float64) for v in (mean, std, weight))
        if mean.ndim != 2 or mean.shape[1] != 2 or std.shape != mean.shape or weight.shape != mean.shape[:1]:
            raise ValueError('ErrorStatsNoise: mean [J,2], std [J,2], weight [J], got %s, %s, %s' % (mean.shape, std.shape, weight.shape))
        if not 1 <= len(mean) <= MAX_JOINTS:
            raise ValueError('ErrorStatsNoise: %d joints (1..%d)' % (len(mean), MAX_JOINTS))
        if not (np.isfinite(mean).all() and np.isfinite(std).all() and np.isfinite(weight).all()) or (std < 0).any():
            raise ValueError('ErrorStatsNoise: the table must be finite, std >= 0')
        self.table = np.concatenate([mean, std, weight[:, None]], 1)                 # [J,5]
        self._dev = {}

    @property
    def n_joints(self):
        return len(self.table)

    def device_table(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = torch.as_tensor(self.table, dtype=torch.float64, device=device).contiguous()
        return self._dev[key]


def _checked_step(step, who):
    if isinstance(step, torch.Tensor):
        if step.dtype != torch.int64 or step.numel() != 1:
            raise ValueError('%s: a device step is one int64, got %s %s' % (who, step.dtype, list(step.shape)))
        return None, step
    step = int(step)
    if not 0 <= step < 2 ** 32:
        raise ValueError('%s: step %d outside [0, 2^32)' % (who, step))
    return step, None


def noisy_input(joint_img, model, *, seed, step=0, sample_offset=0, joint_valid=None, rot_deg=None, flip=None, flip_pairs=(), res=(288, 384),
                detections=None, return_decisions=False):
    """joint_img [B,J,2|3] float32 on a HIP device, image pixels -> (pose2d [B,J,2], input_valid [B] int32, noisy_crop [B,J,2]).

    model: CocoDetectorNoise (J >= 17: joints 0..16 are perturbed, later rows keep their clean values), ErrorStatsNoise of J joints, or
    None with detections [B,J,2|3]: the test split, a detector's joints through the crop of joint_img's box, nothing drawn.
    seed: the stream's 64-bit key; step: an int in [0, 2^32) or a one-element int64 tensor on the device (its low 32 bits; read by the
    kernels, so a captured graph draws fresh noise per replay when the caller advances it); sample_offset: the global index of row 0 --
    row b of any batch is the single-sample call with sample_offset + b.  joint_valid [B,J] (default: all valid) only decides
    whether a partner counts as a centre and which probability tier applies; invalid joints are perturbed too.  rot_deg, flip,
    flip_pairs, res: as preprocess.preprocess_chain.  input_valid is 0 where process_bbox rejects the box (zeros in both outputs).
    return_decisions: a fourth result [B,17,8] int32 (CocoDetectorNoise; -1 rows where the box is rejected): the accepted counts of
    jitter, miss around the joint, miss around the partner, inversion, good; the case (CASES, -1 zeroed); the picked index; the index
    into the partner's miss points or -1.
    Two launches (three with CocoDetectorNoise); nothing waits for the device."""
    who = 'noisy_input'
    if not isinstance(joint_img, torch.Tensor) or joint_img.dim() != 3 or joint_img.shape[2] not in (2, 3) or not joint_img.is_floating_point():
        raise ValueError('%s: joint_img must be a floating-point tensor [B,J,2|3]' % who)
    B, J, C = joint_img.shape
    if not 1 <= J <= MAX_JOINTS:
        raise ValueError('%s: %d joints (1..%d)' % (who, J, MAX_JOINTS))
    if model is None:
        if detections is None:
            raise ValueError('%s: a noise model or detections is required' % who)
        mode = _lib.NOISE_DETECTIONS
        if not isinstance(detections, torch.Tensor) or tuple(detections.shape) != (B, J, C) or not detections.is_floating_point():
            raise ValueError('%s: detections must be a floating-point tensor %s like joint_img' % (who, [B, J, C]))
    elif detections is not None:
        raise ValueError('%s: detections replace the joints; they take no noise model' % who)
    elif isinstance(model, CocoDetectorNoise):
        mode = _lib.NOISE_COCO
        if J < COCO_JOINTS:
            raise ValueError('%s: CocoDetectorNoise needs the %d COCO joints first, got %d' % (who, COCO_JOINTS, J))
    elif isinstance(model, ErrorStatsNoise):
        mode = _lib.NOISE_STATS
        if model.n_joints != J:
            raise ValueError('%s: the error table has %d joints, the input %d' % (who, model.n_joints, J))
    else:
        raise ValueError('%s: model must be CocoDetectorNoise, ErrorStatsNoise or None, got %s' % (who, type(model).__name__))
    if return_decisions and mode != _lib.NOISE_COCO:
        raise ValueError('%s: only CocoDetectorNoise takes decisions' % who)
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError('%s: seed %d outside [0, 2^64)' % (who, seed))
    step, step_dev = _checked_step(step, who)
    sample_offset = int(sample_offset)
    if sample_offset < 0 or sample_offset + B > 2 ** 32:
        raise ValueError('%s: samples %d .. %d outside [0, 2^32]' % (who, sample_offset, sample_offset + B))
    try:
        pair_list = [(int(u), int(v)) for u, v in flip_pairs]
    except (TypeError, ValueError):
        raise ValueError('%s: flip_pairs must be pairs of joint indices' % who)
    if any(u < 0 or v < 0 for u, v in pair_list):
        raise ValueError('%s: negative joint index in flip_pairs' % who)
    try:
        res = (int(res[0]), int(res[1]))
    except (TypeError, ValueError, IndexError):
        raise ValueError('%s: res must be (width, height)' % who)
    if res[0] < 1 or res[1] < 1:
        raise ValueError('%s: res %s must be positive' % (who, (res,)))
    if joint_valid is not None and (not isinstance(joint_valid, torch.Tensor) or tuple(joint_valid.shape) not in ((B, J), (B, J, 1))):
        raise ValueError('%s: joint_valid must be a tensor [B,J]' % who)
    if rot_deg is not None and not isinstance(rot_deg, torch.Tensor):
        rot_deg = np.asarray(rot_deg, np.float32)
    if flip is not None and not isinstance(flip, torch.Tensor):
        flip = np.asarray(flip).astype(np.int32)
    if flip is not None and isinstance(flip, torch.Tensor) and (flip.is_floating_point() or flip.is_complex()):
        raise ValueError('%s: flip must be boolean or integer, got %s' % (who, flip.dtype))
    for name, v in (('rot_deg', rot_deg), ('flip', flip)):
        if v is not None and tuple(v.shape) != (B,):
            raise ValueError('%s: %s must be [%d], got %s' % (who, name, B, list(v.shape)))
    _lib.need_device(who, joint_img, joint_valid, detections, step_dev)
    dev = joint_img.device
    with torch.cuda.device(dev):
        x = joint_img.contiguous().float()
        a = _lib.PreprocessNoiseArgs()
        a.struct_size = ctypes.sizeof(_lib.PreprocessNoiseArgs)
        a.batch, a.n_joints, a.comps, a.mode, a.n_pairs, a.res_w, a.res_h = B, J, C, mode, len(pair_list), res[0], res[1]
        a.seed, a.step, a.sample_offset = seed, step or 0, sample_offset
        keep = [x]                                   # the struct holds addresses only: the tensors must outlive the call

        def put(t, dtype):
            if t is None:
                return None
            t = torch.as_tensor(t, device=dev).to(dtype).contiguous()
            keep.append(t)
            return t.data_ptr()

        a.joints = x.data_ptr()
        a.step_dev = put(step_dev, torch.int64)
        a.joint_valid = put(None if joint_valid is None else joint_valid.reshape(B, J), torch.float32)
        a.detections = put(detections, torch.float32)
        a.rot_deg, a.flip = put(rot_deg, torch.float32), put(flip, torch.int32)
        a.flip_pairs = put(np.asarray(pair_list, np.int32).reshape(-1, 2), torch.int32) if pair_list else None
        pose2d = torch.empty((B, J, 2), device=dev, dtype=torch.float32)
        crop = torch.empty((B, J, 2), device=dev, dtype=torch.float32)
        valid = torch.empty((B,), device=dev, dtype=torch.int32)
        a.pose2d, a.valid, a.noisy_crop = pose2d.data_ptr(), valid.data_ptr(), crop.data_ptr()
        decisions = None
        if mode == _lib.NOISE_COCO:
            coco = model.struct()
            a.coco = ctypes.pointer(coco)
            area = torch.empty((B,), device=dev, dtype=torch.float64)
            a.area = area.data_ptr()
            if return_decisions:
                decisions = torch.full((B, COCO_JOINTS, 8), -1, device=dev, dtype=torch.int32)
                a.decisions = decisions.data_ptr()
        elif mode == _lib.NOISE_STATS:
            a.stats = model.device_table(dev).data_ptr()
        if B:
            _lib.check(_lib.load().gator_preprocess_noise_f32(ctypes.byref(a), _lib.stream_ptr(dev)), 'gator_preprocess_noise_f32')
    if return_decisions:
        return pose2d, valid, crop, decisions
    return pose2d, valid, crop
