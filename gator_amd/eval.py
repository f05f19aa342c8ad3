"""Caller-side steps that FOLLOW the hot path in the reference's eval loop (SURVEY 8f "next" rows), kept on the GPU:

  joints  = J_regressor @ (verts * 1000)          lib/core/base.py:219-221, demo/run.py:142   -> gator_regress_joints_f32
  MPJPE   = mean || root-aligned pred - target ||  data/PW3D/dataset.py:273-286, data/Human36M/dataset.py:466-478
  PA-MPJPE via the rigid (Procrustes) alignment    lib/coord_utils.py:127-149                  -> gator_rigid_align_f32

so that evaluation needs [B,17,3] + a few scalars on the host instead of a D2H copy of every 82 kB mesh
(lib/core/base.py:223,232-237 copy each mesh to the host twice)."""
import ctypes

import numpy as np
import torch

from . import _lib

H36M_EVAL_JOINTS = (1, 2, 3, 4, 5, 6, 8, 10, 11, 12, 13, 14, 15, 16)     # data/PW3D/dataset.py:46
N_VERTS = 6890                                                            # SMPL vertices (csrc/internal.h: kNV)


def _checked_eval_joints(eval_joints, n_joint, who):
    """The evaluation indices as a list of ints, each in [0, n_joint): the kernels use them as raw offsets, so a negative or too
    large one is refused here, from the Python list, before anything is sent to the device."""
    idx = [int(i) for i in eval_joints]
    bad = [i for i in idx if i < 0 or i >= n_joint]
    if bad:
        raise ValueError('%s: evaluation joint index %d outside [0, %d)' % (who, bad[0], n_joint))
    return idx


class JointRegressor:
    """Sparse [n_joint, 6890] regressor held on the device as COO (107 / 105 non-zeros for the shipped regressors)."""

    def __init__(self, dense, device):
        d = np.asarray(dense, np.float32)
        if d.ndim != 2 or d.shape[0] < 1 or d.shape[1] != N_VERTS:      # a column is used as a vertex offset on the device, unchecked
            raise ValueError('JointRegressor: expected a dense [n_joint, %d] matrix, got %s' % (N_VERTS, tuple(d.shape)))
        r, c = np.nonzero(d)
        self.n_joint = int(d.shape[0])
        self.nnz = int(r.size)
        self.row = torch.from_numpy(r.astype(np.int32)).to(device)
        self.col = torch.from_numpy(c.astype(np.int32)).to(device)
        self.val = torch.from_numpy(d[r, c].astype(np.float32)).to(device)

    def __call__(self, verts):
        """verts [B,6890,3] f32 on the device -> joints [B,n_joint,3] (same unit as verts)."""
        if not verts.is_cuda:
            raise RuntimeError('JointRegressor: verts must live on a HIP device')
        verts = verts.contiguous().float()
        B = verts.shape[0]
        out = torch.empty((B, self.n_joint, 3), device=verts.device, dtype=torch.float32)
        st = ctypes.c_void_p(torch.cuda.current_stream(verts.device).cuda_stream)
        _lib.check(_lib.load().gator_regress_joints_f32(verts.data_ptr(), B, self.row.data_ptr(), self.col.data_ptr(),
                                                       self.val.data_ptr(), self.nnz, self.n_joint, out.data_ptr(), st),
                   'gator_regress_joints_f32')
        return out


def mpjpe(pred_joint, target_joint, eval_joints=H36M_EVAL_JOINTS, root=0):
    """Root-align, select the evaluation joints, mean Euclidean distance (data/PW3D/dataset.py:273-286).  Device tensors."""
    p = pred_joint - pred_joint[:, root:root + 1]
    t = target_joint - target_joint[:, root:root + 1]
    if eval_joints is not None:
        idx = torch.as_tensor(eval_joints, device=p.device)
        p, t = p[:, idx], t[:, idx]
    return torch.sqrt(((p - t) ** 2).sum(2)).mean()


def mpvpe(pred_mesh, target_mesh, pred_joint, target_joint, root=0):
    """Mesh error after aligning both meshes to their own root joint (data/PW3D/dataset.py:275,283)."""
    p = pred_mesh - pred_joint[:, root:root + 1]
    t = target_mesh - target_joint[:, root:root + 1]
    return torch.sqrt(((p - t) ** 2).sum(2)).mean()


def rigid_align(a, b):
    """Batched similarity (Procrustes) alignment of a onto b, [B,N,3] device tensors (lib/coord_utils.py:127-149:
    rotation by SVD of the covariance with the reflection fix, scale = trace(S)/var(a), translation of the centroids):
    gator_rigid_align_f32, one 3x3 one-sided-Jacobi SVD per sample in fp64."""
    if not (a.is_cuda and b.is_cuda):
        raise RuntimeError('rigid_align: inputs must live on a HIP device')
    if a.shape != b.shape or a.dim() != 3 or a.shape[2] != 3:
        raise ValueError('rigid_align: expected two [B,N,3] tensors, got %s and %s' % (tuple(a.shape), tuple(b.shape)))
    a32, b32 = a.contiguous().float(), b.contiguous().float()
    out = torch.empty_like(a32)
    st = ctypes.c_void_p(torch.cuda.current_stream(a.device).cuda_stream)
    _lib.check(_lib.load().gator_rigid_align_f32(a32.data_ptr(), b32.data_ptr(), a32.shape[0], a32.shape[1], out.data_ptr(), st),
               'gator_rigid_align_f32')
    return out.to(a.dtype)


def pa_mpjpe(pred_joint, target_joint, eval_joints=H36M_EVAL_JOINTS):
    idx = torch.as_tensor(_checked_eval_joints(eval_joints, pred_joint.shape[1], 'pa_mpjpe'), device=pred_joint.device)
    p, t = pred_joint[:, idx], target_joint[:, idx]
    return torch.sqrt(((rigid_align(p, t) - t) ** 2).sum(2)).mean()


def joint_errors(pred_joint, target_joint, eval_joints=H36M_EVAL_JOINTS, root=0, pred_scale=1.0):
    """Per-sample (MPJPE, PA-MPJPE) in one launch (gator_joint_errors_f32): pred_joint [B,nj,3] (multiplied by pred_scale on the fly:
    1000 for metres -> mm), target_joint [B,nj,3] -> [B,2].  mpjpe()/pa_mpjpe() above are its two columns averaged over the batch."""
    if not (pred_joint.is_cuda and target_joint.is_cuda):
        raise RuntimeError('joint_errors: inputs must live on a HIP device')
    p, t = pred_joint.contiguous().float(), target_joint.contiguous().float()
    if p.dim() != 3 or p.shape[2] != 3 or p.shape != t.shape:
        raise ValueError('joint_errors: expected two [B,nj,3] tensors, got %s and %s' % (tuple(p.shape), tuple(t.shape)))
    B, nj = p.shape[0], p.shape[1]
    idx = None if eval_joints is None else torch.as_tensor(_checked_eval_joints(eval_joints, nj, 'joint_errors'), dtype=torch.int32, device=p.device)
    out = torch.empty((B, 2), device=p.device, dtype=torch.float32)
    st = ctypes.c_void_p(torch.cuda.current_stream(p.device).cuda_stream)
    _lib.check(_lib.load().gator_joint_errors_f32(p.data_ptr(), t.data_ptr(), B, nj, idx.data_ptr() if idx is not None else None,
                                                  int(idx.numel()) if idx is not None else 0, int(root), float(pred_scale), out.data_ptr(), st),
               'gator_joint_errors_f32')
    return out
