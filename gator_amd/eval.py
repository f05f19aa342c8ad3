"""Caller-side steps that FOLLOW the hot path in the reference's eval loop (SURVEY 8f "next" rows), kept on the GPU:

  joints  = J_regressor @ (verts * 1000)          lib/core/base.py:219-221, demo/run.py:142   -> gator_regress_joints_f32
  MPJPE   = mean || root-aligned pred - target ||  data/PW3D/dataset.py:273-286, data/Human36M/dataset.py:466-478
  PA-MPJPE via the rigid (Procrustes) alignment    lib/coord_utils.py:127-149                  -> gator_rigid_align_f32

  MPVPE, PA-MPVPE, SMPL-joint MPJPE per sample      data/PW3D/dataset.py:337-375                -> gator_mesh_errors_f32

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
        _lib.need_device('JointRegressor', verts, what='verts')
        verts = verts.contiguous().float()
        B = verts.shape[0]
        out = torch.empty((B, self.n_joint, 3), device=verts.device, dtype=torch.float32)
        _lib.check(_lib.load().gator_regress_joints_f32(verts.data_ptr(), B, self.row.data_ptr(), self.col.data_ptr(),
                                                       self.val.data_ptr(), self.nnz, self.n_joint, out.data_ptr(), _lib.stream_ptr(verts.device)),
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
    _lib.need_device('rigid_align', a, b)
    if a.shape != b.shape or a.dim() != 3 or a.shape[2] != 3:
        raise ValueError('rigid_align: expected two [B,N,3] tensors, got %s and %s' % (tuple(a.shape), tuple(b.shape)))
    a32, b32 = a.contiguous().float(), b.contiguous().float()
    out = torch.empty_like(a32)
    _lib.check(_lib.load().gator_rigid_align_f32(a32.data_ptr(), b32.data_ptr(), a32.shape[0], a32.shape[1], out.data_ptr(), _lib.stream_ptr(a.device)),
               'gator_rigid_align_f32')
    return out.to(a.dtype)


def pa_mpjpe(pred_joint, target_joint, eval_joints=H36M_EVAL_JOINTS):
    idx = torch.as_tensor(_checked_eval_joints(eval_joints, pred_joint.shape[1], 'pa_mpjpe'), device=pred_joint.device)
    p, t = pred_joint[:, idx], target_joint[:, idx]
    return torch.sqrt(((rigid_align(p, t) - t) ** 2).sum(2)).mean()


def joint_errors(pred_joint, target_joint, eval_joints=H36M_EVAL_JOINTS, root=0, pred_scale=1.0):
    """Per-sample (MPJPE, PA-MPJPE) in one launch (gator_joint_errors_f32): pred_joint [B,nj,3] (multiplied by pred_scale on the fly:
    1000 for metres -> mm), target_joint [B,nj,3] -> [B,2].  mpjpe()/pa_mpjpe() above are its two columns averaged over the batch."""
    _lib.need_device('joint_errors', pred_joint, target_joint)
    p, t = pred_joint.contiguous().float(), target_joint.contiguous().float()
    if p.dim() != 3 or p.shape[2] != 3 or p.shape != t.shape:
        raise ValueError('joint_errors: expected two [B,nj,3] tensors, got %s and %s' % (tuple(p.shape), tuple(t.shape)))
    B, nj = p.shape[0], p.shape[1]
    idx = None if eval_joints is None else torch.as_tensor(_checked_eval_joints(eval_joints, nj, 'joint_errors'), dtype=torch.int32, device=p.device)
    out = torch.empty((B, 2), device=p.device, dtype=torch.float32)
    _lib.check(_lib.load().gator_joint_errors_f32(p.data_ptr(), t.data_ptr(), B, nj, _lib.ptr(idx),
                                                  int(idx.numel()) if idx is not None else 0, int(root), float(pred_scale), out.data_ptr(),
                                                  _lib.stream_ptr(p.device)), 'gator_joint_errors_f32')
    return out


# ---- whole-mesh evaluation: gator_mesh_errors_f32 (data/PW3D/dataset.py:322-375, data/Human36M/dataset.py:515-600) ----------------

MESH_ERROR_COLUMNS = ('MPJPE', 'PA-MPJPE', 'MPJPE_SMPL', 'MPVPE', 'PA-MPVPE')      # the columns of mesh_errors(), in order
MAX_REGRESSOR_JOINTS = 64                                                          # csrc/mesh_eval.hip: kMaxRegJoints


class _Coo:
    """A sparse [n_joint, n_verts] regressor on a device as COO, for any n_verts (JointRegressor stays the 6890-column one).  Entries
    may come in any order and duplicates add.  Rows and columns are checked here, on the host: the kernel uses a column as a raw
    vertex offset."""

    def __init__(self, row, col, val, n_joint, n_verts, device, who='mesh_errors'):
        row, col, val = np.asarray(row, np.int64).ravel(), np.asarray(col, np.int64).ravel(), np.asarray(val, np.float32).ravel()
        if not (row.size == col.size == val.size):
            raise ValueError('%s: COO arrays of %d / %d / %d entries' % (who, row.size, col.size, val.size))
        if not 1 <= int(n_joint) <= MAX_REGRESSOR_JOINTS:
            raise ValueError('%s: a regressor of %d joints (1..%d)' % (who, int(n_joint), MAX_REGRESSOR_JOINTS))
        if row.size and (row.min() < 0 or row.max() >= n_joint):
            raise ValueError('%s: regressor row outside [0, %d)' % (who, n_joint))
        if col.size and (col.min() < 0 or col.max() >= n_verts):
            raise ValueError('%s: regressor column outside [0, %d)' % (who, n_verts))
        self.n_joint, self.n_verts, self.nnz = int(n_joint), int(n_verts), int(row.size)
        # one spare element: an empty regressor still has three arrays to point at
        self.row = torch.from_numpy(np.append(row, 0).astype(np.int32)).to(device)
        self.col = torch.from_numpy(np.append(col, 0).astype(np.int32)).to(device)
        self.val = torch.from_numpy(np.append(val, np.float32(0))).to(device)

    @classmethod
    def from_dense(cls, dense, device, who='mesh_errors'):
        d = np.asarray(dense, np.float32)
        if d.ndim != 2:
            raise ValueError('%s: expected a dense [n_joint, n_verts] regressor, got %s' % (who, tuple(d.shape)))
        r, c = np.nonzero(d)
        return cls(r, c, d[r, c], d.shape[0], d.shape[1], device, who)

    def struct(self):
        return _lib.GatorCoo(self.row.data_ptr(), self.col.data_ptr(), self.val.data_ptr(), self.nnz, self.n_joint)


def _as_coo(reg, n_verts, device, who):
    """A dense matrix, a JointRegressor or a _Coo -> something with row / col / val / nnz / n_joint on `device` for n_verts vertices."""
    if isinstance(reg, JointRegressor):
        have = N_VERTS
    elif isinstance(reg, _Coo):
        have = reg.n_verts
    else:
        reg = _Coo.from_dense(reg, device, who)
        have = reg.n_verts
    if have != n_verts:
        raise ValueError('%s: a regressor over %d vertices for meshes of %d' % (who, have, n_verts))
    if not 1 <= reg.n_joint <= MAX_REGRESSOR_JOINTS:
        raise ValueError('%s: a regressor of %d joints (1..%d)' % (who, reg.n_joint, MAX_REGRESSOR_JOINTS))
    if reg.row.device != torch.device(device):
        raise ValueError('%s: the regressor lives on %s, the meshes on %s' % (who, reg.row.device, device))
    return reg


def _coo_struct(reg):
    return reg.struct() if isinstance(reg, _Coo) else _lib.GatorCoo(reg.row.data_ptr(), reg.col.data_ptr(), reg.val.data_ptr(), reg.nnz, reg.n_joint)


def _checked_root(root, n_joint, who):
    root = int(root)
    if not 0 <= root < n_joint:
        raise ValueError('%s: root joint %d outside [0, %d)' % (who, root, n_joint))
    return root


def _checked_eval_set(eval_joints, n_joint, who):
    """None (all joints) or the checked index list; 3..32 evaluation joints either way."""
    idx = None if eval_joints is None else _checked_eval_joints(eval_joints, n_joint, who)
    n = n_joint if idx is None else len(idx)
    if not 3 <= n <= 32:
        raise ValueError('%s: %d evaluation joints (3..32)' % (who, n))
    return idx


def _checked_meshes(pred_mesh, target_mesh, who):
    if pred_mesh.dim() != 3 or pred_mesh.shape[2] != 3 or pred_mesh.shape != target_mesh.shape or pred_mesh.shape[0] < 1 or pred_mesh.shape[1] < 3:
        raise ValueError('%s: expected two [B,N,3] meshes with B >= 1 and N >= 3, got %s and %s' % (who, tuple(pred_mesh.shape), tuple(target_mesh.shape)))
    if pred_mesh.device != target_mesh.device:
        raise ValueError('%s: the meshes live on %s and %s' % (who, pred_mesh.device, target_mesh.device))


def _launch_mesh_errors(p, t, root_reg, root, eval_reg, idx, eval_root, pred_scale, target_scale, out):
    """p, t: contiguous float32 [B,N,3] on one HIP device; idx: int32 device tensor or None; out: float32 [B,5] there, written in place.
    Everything is checked by the callers; nothing here allocates device memory or waits for the device."""
    ev = _coo_struct(eval_reg) if eval_reg is not None else None
    _lib.check(_lib.load().gator_mesh_errors_f32(p.data_ptr(), t.data_ptr(), p.shape[0], p.shape[1], float(pred_scale), float(target_scale),
                                                 ctypes.byref(_coo_struct(root_reg)), root, ctypes.byref(ev) if ev is not None else None, eval_root,
                                                 _lib.ptr(idx), int(idx.numel()) if idx is not None else 0,
                                                 out.data_ptr(), _lib.stream_ptr(p.device)), 'gator_mesh_errors_f32')
    return out


def mesh_errors(pred_mesh, target_mesh, root_regressor, root=0, eval_regressor=None, eval_joints=H36M_EVAL_JOINTS, eval_root=0,
                pred_scale=1.0, target_scale=1.0):
    """Per-sample (MPJPE, PA-MPJPE, MPJPE_SMPL, MPVPE, PA-MPVPE) of two [B,N,3] device meshes in one launch (gator_mesh_errors_f32),
    [B,5] on the device: what the datasets' `evaluate` computes per sample on the host (data/PW3D/dataset.py:337-375).

    root_regressor [n_joint <= 64, N]: both meshes are aligned on its joint `root` (columns 2-4; the 24-joint SMPL regressor for
    `evaluate`, the H36M regressor for compute_both_err).  eval_regressor [n_joint <= 64, N] with eval_root and eval_joints (3..32
    indices, None = all joints) gives columns 0 and 1; without it they are NaN.  A regressor is a dense array or a JointRegressor.
    Each mesh is multiplied by its scale in float32 on the fly (1000 for metres -> mm, lib/core/base.py:219)."""
    who = 'mesh_errors'
    _checked_meshes(pred_mesh, target_mesh, who)
    N, device = pred_mesh.shape[1], pred_mesh.device
    root_reg = _as_coo(root_regressor, N, device, who)
    root = _checked_root(root, root_reg.n_joint, who)
    eval_reg, idx = None, None
    if eval_regressor is not None:
        eval_reg = _as_coo(eval_regressor, N, device, who)
        eval_root = _checked_root(eval_root, eval_reg.n_joint, who)
        idx = _checked_eval_set(eval_joints, eval_reg.n_joint, who)
    _lib.need_device(who, pred_mesh)
    p, t = pred_mesh.contiguous().float(), target_mesh.contiguous().float()
    idx_t = None if idx is None else torch.as_tensor(idx, dtype=torch.int32, device=device)
    out = torch.empty((p.shape[0], 5), device=device, dtype=torch.float32)
    return _launch_mesh_errors(p, t, root_reg, root, eval_reg, idx_t, int(eval_root), pred_scale, target_scale, out)


class MeshEvaluator:
    """The rows of mesh_errors() over a whole test set, kept on the device: update() per batch (one launch into a buffer that grows by
    doubling; no host synchronisation, no device-to-host copy), summary() once at the end (one copy).  Replaces compute_both_err per
    batch plus the datasets' `evaluate` over the collected meshes (lib/core/base.py:219-237,255)."""

    def __init__(self, root_regressor, eval_regressor=None, n_verts=N_VERTS, device='cuda', root=0, eval_joints=H36M_EVAL_JOINTS, eval_root=0,
                 pred_scale=1.0, target_scale=1.0, capacity=1024):
        who = 'MeshEvaluator'
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('MeshEvaluator: needs a HIP device')
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.n_verts = int(n_verts)
        self.root_reg = _as_coo(root_regressor, self.n_verts, self.device, who)
        self.root = _checked_root(root, self.root_reg.n_joint, who)
        self.eval_reg, self.idx, self.eval_root = None, None, int(eval_root)
        if eval_regressor is not None:
            self.eval_reg = _as_coo(eval_regressor, self.n_verts, self.device, who)
            self.eval_root = _checked_root(eval_root, self.eval_reg.n_joint, who)
            idx = _checked_eval_set(eval_joints, self.eval_reg.n_joint, who)
            self.idx = None if idx is None else torch.as_tensor(idx, dtype=torch.int32, device=self.device)
        self.pred_scale, self.target_scale = float(pred_scale), float(target_scale)
        self._rows = torch.empty((max(1, int(capacity)), 5), device=self.device, dtype=torch.float32)
        self.reset()

    def reset(self):
        self._count, self._batches = 0, []

    def __len__(self):
        return self._count

    def update(self, pred_mesh, target_mesh):
        """Append the rows of one batch; returns them ([B,5], a view of the buffer as it is now)."""
        who = 'MeshEvaluator.update'
        _checked_meshes(pred_mesh, target_mesh, who)
        if not pred_mesh.is_cuda or pred_mesh.device != self.device:
            raise RuntimeError('%s: the meshes must live on %s' % (who, self.device))
        if pred_mesh.shape[1] != self.n_verts:
            raise ValueError('%s: meshes of %d vertices, regressors over %d' % (who, pred_mesh.shape[1], self.n_verts))
        B = pred_mesh.shape[0]
        if self._count + B > self._rows.shape[0]:
            grown = torch.empty((max(2 * self._rows.shape[0], self._count + B), 5), device=self.device, dtype=torch.float32)
            grown[:self._count].copy_(self._rows[:self._count])          # stream-ordered: no synchronisation
            self._rows = grown
        out = self._rows[self._count:self._count + B]
        _launch_mesh_errors(pred_mesh.contiguous().float(), target_mesh.contiguous().float(), self.root_reg, self.root, self.eval_reg, self.idx,
                            self.eval_root, self.pred_scale, self.target_scale, out)
        self._batches.append((self._count, B))
        self._count += B
        return out

    def rows(self):
        """[n,5] float32 on the host: the one device-to-host copy."""
        return self._rows[:self._count].cpu().numpy()

    def summary(self):
        """The per-sample means of the datasets' `evaluate` under MESH_ERROR_COLUMNS' names, and 'MPVPE_batch_mean' / 'MPJPE_batch_mean':
        the mean over update() calls of each call's mean, which Tester.test prints (lib/core/base.py:239-241) -- the two differ when the
        last batch is short."""
        if not self._count:
            raise RuntimeError('MeshEvaluator.summary: no sample yet')
        r = self.rows().astype(np.float64)
        out = {name: float(r[:, k].mean()) for k, name in enumerate(MESH_ERROR_COLUMNS)}
        for name, k in (('MPVPE_batch_mean', 3), ('MPJPE_batch_mean', 0)):
            out[name] = float(np.mean([r[s:s + n, k].mean() for s, n in self._batches]))
        return out
