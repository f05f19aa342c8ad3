"""The per-video, temporal part of the evaluation, kept on the GPU (data/PW3D/dataset.py:383-415, which the reference keeps commented
out but complete):

  smooth_pose       lib/smooth_utils.smooth_pose, a one-euro filter over each video          -> gator_one_euro_f32
  accel_error       lib/coord_utils.compute_error_accel                                     -> gator_sequence_errors, column 0
  sequence_errors   the whole block: smooth, acceleration error, MPJPE and PA-MPJPE of the smoothed sequence, their three averages

The reference walks every frame in a Python loop on the host; here a test set is three launches (csrc/temporal.hip) and one copy of
[V,6] sums.  The filter's float64 output equals the reference's bit for bit for finite inputs: the recursion is the same IEEE
operations in the same order, with no contracted multiply-add.

Frames are grouped into videos either by `lengths` (consecutive videos, in order) or by `video_indices` (the reference's
self.video_indices: one index array per video, the frames of a video in temporal order); with neither, the input is one video."""
import numpy as np
import torch

from . import _lib

PREFETCH = 8                # csrc/temporal.hip: kPrefetch, the depth of k_one_euro's load ring
MAX_EVAL_JOINTS = 32        # csrc/procrustes.h: kMaxPts
SEQUENCE_ERROR_COLUMNS = ('accel', 'MPJPE', 'PA-MPJPE')        # the columns of the per-frame rows and of the per-video means


def _segments(F, lengths, video_indices, who):
    """-> (seg_start: int64 numpy [V+1], order: int64 numpy [F] or None).  order[k] = the input frame that stands at place k once the
    videos lie one after another; None when the input already does.  Everything is checked here, on the host."""
    if lengths is not None and video_indices is not None:
        raise ValueError('%s: give lengths or video_indices, not both' % who)
    if video_indices is not None:
        vids = [np.asarray(v).ravel() for v in video_indices]
        if not vids:
            raise ValueError('%s: video_indices is empty' % who)
        for v in vids:
            if v.size and not np.issubdtype(v.dtype, np.integer):
                raise ValueError('%s: video_indices must hold integers, got %s' % (who, v.dtype))
        lens = np.array([v.size for v in vids], np.int64)
        order = np.concatenate(vids).astype(np.int64)
        if order.size and (order.min() < 0 or order.max() >= F):
            bad = order[(order < 0) | (order >= F)][0]
            raise ValueError('%s: frame index %d outside [0, %d)' % (who, bad, F))
        if order.size != F or (np.bincount(order, minlength=F) != 1).any():
            raise ValueError('%s: video_indices must use each of the %d frames exactly once (%d indices given)' % (who, F, order.size))
    else:
        lens = np.array([F], np.int64) if lengths is None else np.asarray(lengths).ravel()
        if lens.size and not np.issubdtype(lens.dtype, np.integer):
            raise ValueError('%s: lengths must hold integers, got %s' % (who, lens.dtype))
        lens = lens.astype(np.int64)
        order = None
    if lens.size == 0 or (lens < 1).any():
        raise ValueError('%s: every video needs at least one frame' % who)
    if int(lens.sum()) != F:
        raise ValueError('%s: the videos hold %d frames, the input %d' % (who, int(lens.sum()), F))
    seg = np.zeros(lens.size + 1, np.int64)
    np.cumsum(lens, out=seg[1:])
    return seg, order


def _checked_frames(x, who, name='pred'):
    if not isinstance(x, torch.Tensor) or x.dim() < 1 or x.shape[0] < 1 or x.numel() == 0:
        raise ValueError('%s: %s must be a tensor [F, ...] with F >= 1 and at least one channel' % (who, name))
    if not x.is_floating_point():
        raise ValueError('%s: %s must be a floating-point tensor, got %s' % (who, name, x.dtype))


def _checked_joints(pred, gt, who):
    _checked_frames(pred, who)
    _checked_frames(gt, who, 'gt')
    if pred.dim() != 3 or pred.shape[2] != 3 or pred.shape != gt.shape:
        raise ValueError('%s: expected two [F,ne,3] tensors, got %s and %s' % (who, tuple(pred.shape), tuple(gt.shape)))
    if not 3 <= pred.shape[1] <= MAX_EVAL_JOINTS:
        raise ValueError('%s: %d evaluation joints (3..%d)' % (who, pred.shape[1], MAX_EVAL_JOINTS))
    if pred.device != gt.device:
        raise ValueError('%s: pred lives on %s, gt on %s' % (who, pred.device, gt.device))


def _checked_valid(valid, F, device, who):
    if valid is None:
        return None
    if not isinstance(valid, torch.Tensor):
        valid = torch.as_tensor(np.asarray(valid))
    if valid.dim() != 1 or valid.shape[0] != F:
        raise ValueError('%s: valid must be [F] = [%d], got %s' % (who, F, tuple(valid.shape)))
    if valid.is_floating_point() or valid.is_complex():
        raise ValueError('%s: valid must be boolean or integer, got %s' % (who, valid.dtype))
    if isinstance(valid, torch.Tensor) and valid.is_cuda and valid.device != device:
        raise ValueError('%s: valid lives on %s, the joints on %s' % (who, valid.device, device))
    return valid


def _launch_one_euro(x, seg, V, min_cutoff, beta, d_cutoff, dt, out):
    """x: contiguous float32 [F,C] on a HIP device, seg: int64 [V+1] there, out: float64 or float32 [F,C] there.  One launch."""
    _lib.check(_lib.load().gator_one_euro_f32(x.data_ptr(), seg.data_ptr(), x.shape[0], V, x.shape[1], float(min_cutoff), float(beta),
                                              float(d_cutoff), float(dt), 1 if out.dtype == torch.float64 else 0, out.data_ptr(),
                                              _lib.stream_ptr(x.device)), 'gator_one_euro_f32')
    return out


def _launch_sequence_errors(p, g, valid, seg, V, rows, sums):
    """p: contiguous float64 or float32 [F,ne,3], g: contiguous float32, valid: uint8 [F] or None, rows [F,3] / sums [V,6] float64.  Two launches."""
    _lib.check(_lib.load().gator_sequence_errors(p.data_ptr(), 1 if p.dtype == torch.float64 else 0, g.data_ptr(),
                                                 _lib.ptr(valid), seg.data_ptr(), p.shape[0], V, p.shape[1],
                                                 rows.data_ptr(), sums.data_ptr(), _lib.stream_ptr(p.device)), 'gator_sequence_errors')


def _filter_params(min_cutoff, beta, d_cutoff, dt, who):
    vals = [float(min_cutoff), float(beta), float(d_cutoff), float(dt)]
    if not all(np.isfinite(vals)) or vals[3] <= 0.0:
        raise ValueError('%s: min_cutoff, beta, d_cutoff must be finite and dt positive, got %s' % (who, vals))
    return vals


def smooth_pose(pred, lengths=None, video_indices=None, min_cutoff=0.004, beta=0.7, d_cutoff=1.0, dt=1.0, out_dtype=torch.float64):
    """lib/smooth_utils.smooth_pose over every video of `pred` [F, ...] (any trailing shape: joints [F,14,3], whole meshes [F,6890,3])
    in one launch; the defaults are the reference's.  Returns a tensor of pred's shape and of out_dtype: float64 is the reference's
    arithmetic bit for bit on the float32 input, float32 is its rounding.  The first frame of a video is copied.  A non-finite value
    makes its own channel NaN for the rest of its own video, as numpy does.

    With video_indices the frames are gathered into video order before the kernel and scattered back after it: the result stands in
    the order of the input."""
    who = 'smooth_pose'
    _checked_frames(pred, who)
    if out_dtype not in (torch.float64, torch.float32):
        raise ValueError('%s: out_dtype must be torch.float64 or torch.float32' % who)
    F = pred.shape[0]
    seg, order = _segments(F, lengths, video_indices, who)
    par = _filter_params(min_cutoff, beta, d_cutoff, dt, who)
    _lib.need_device(who, pred)
    dev = pred.device
    x = pred.reshape(F, -1).float()
    seg_d = torch.from_numpy(seg).to(dev)
    order_d = None if order is None else torch.from_numpy(order).to(dev)
    x = (x if order_d is None else x.index_select(0, order_d)).contiguous()
    out = torch.empty(x.shape, device=dev, dtype=out_dtype)
    _launch_one_euro(x, seg_d, len(seg) - 1, *par, out)
    if order_d is not None:
        out = torch.empty_like(out).index_copy_(0, order_d, out)
    return out.reshape(pred.shape)


def _errors(pred, gt, lengths, video_indices, valid, smooth, par, who):
    """-> (rows [F,3] float64 on the device, in the order of the input; sums [V,6] float64 on the device).  No host synchronisation."""
    _checked_joints(pred, gt, who)
    F, ne = pred.shape[0], pred.shape[1]
    seg, order = _segments(F, lengths, video_indices, who)
    valid = _checked_valid(valid, F, pred.device, who)
    _lib.need_device(who, pred)
    dev, V = pred.device, len(seg) - 1
    seg_d = torch.from_numpy(seg).to(dev)
    order_d = None if order is None else torch.from_numpy(order).to(dev)
    g = gt.float()
    p = pred if pred.dtype == torch.float64 and not smooth else pred.float()
    v = None if valid is None else (valid.to(dev) != 0).to(torch.uint8)
    if order_d is not None:
        p, g = p.index_select(0, order_d), g.index_select(0, order_d)
        v = None if v is None else v.index_select(0, order_d)
    p, g = p.contiguous(), g.contiguous()
    if smooth:
        sm = torch.empty((F, ne * 3), device=dev, dtype=torch.float64)
        p = _launch_one_euro(p.reshape(F, ne * 3), seg_d, V, *par, sm).reshape(F, ne, 3)
    rows = torch.empty((F, 3), device=dev, dtype=torch.float64)
    sums = torch.empty((V, 6), device=dev, dtype=torch.float64)
    _launch_sequence_errors(p, g, None if v is None else v.contiguous(), seg_d, V, rows, sums)
    if order_d is not None:
        rows = torch.empty_like(rows).index_copy_(0, order_d, rows)
    return rows, sums


def accel_error(gt, pred, lengths=None, valid=None):
    """lib/coord_utils.compute_error_accel(gt, pred, vis) for every video at once: [F] float64 on the device, entry i the acceleration
    error of the frames (i, i+1, i+2) -- the mean over joints of |(p_i - 2 p_i+1 + p_i+2) - (g_i - 2 g_i+1 + g_i+2)|.  The entry is
    NaN for the last two frames of each video and for a triple that holds a frame with valid == 0; the reference's result for one
    video is this video's entries without the NaNs.  gt, pred: [F,ne,3] on the device, 3 <= ne <= 32; pred may be float64 (a smoothed
    sequence) or float32, gt is read as float32."""
    rows, _ = _errors(pred, gt, lengths, None, valid, False, None, 'accel_error')
    return rows[:, 0]


def sequence_errors(pred, gt, lengths=None, video_indices=None, smooth=True, min_cutoff=0.004, beta=0.005, valid=None):
    """The commented block of the datasets' `evaluate` (data/PW3D/dataset.py:383-415) in one call: per video, smooth the prediction
    (smooth=True; min_cutoff and beta default to that block's 0.004 and 0.005), then the acceleration error, the MPJPE and the
    PA-MPJPE of the result -- three launches and no host synchronisation before the one copy of the per-video sums.

    pred, gt: the root-aligned evaluation joints [F,ne,3] on the device, 3 <= ne <= 32 (what the reference collects in pred_j3d /
    gt_j3d); no root is subtracted here.  valid [F] (optional) marks frames whose triples are left out of the acceleration error.

    Returns (rows, per_video, summary):
      rows       [F,3] float64 on the device, columns SEQUENCE_ERROR_COLUMNS, in the order of the input's frames; column 0 as accel_error;
      per_video  [V,3] float64 numpy: each video's mean of the three columns (column 0 over its non-NaN rows);
      summary    {'accel': mean over videos of each video's mean, 'MPJPE': mean over videos of each video's mean,
                  'PA-MPJPE': mean over all frames} -- the reference's three averages.

    A video shorter than 3 frames has no triple: its acceleration mean is NaN, as np.mean of an empty array is, and then so is
    summary['accel'], exactly as the reference's would be.  This is reported, not hidden: drop such videos before the call if a
    number is wanted.  The same holds for a video all of whose triples are invalid.  A non-finite prediction makes its rows NaN; a NaN
    acceleration row is not counted, but the same frame's MPJPE is NaN and shows in per_video and summary."""
    who = 'sequence_errors'
    par = _filter_params(min_cutoff, beta, 1.0, 1.0, who)
    rows, sums = _errors(pred, gt, lengths, video_indices, valid, bool(smooth), par, who)
    s = sums.cpu().numpy()                              # the one device-to-host copy
    with np.errstate(invalid='ignore', divide='ignore'):
        per_video = np.stack([s[:, 0] / s[:, 3], s[:, 1] / s[:, 4], s[:, 2] / s[:, 4]], 1)
        summary = {'accel': float(per_video[:, 0].mean()), 'MPJPE': float(per_video[:, 1].mean()),
                   'PA-MPJPE': float(s[:, 2].sum() / s[:, 4].sum())}
    return rows, per_video, summary
