"""The SMPL body-model layer on the device (gator_smpl_*, csrc/smpl_lbs.hip): what every training dataset of the reference calls at
batch 1 on the CPU to build its ground-truth mesh (smplpytorch/pytorch/smpl_layer.py:65-158; data/AMASS/dataset.py:182-213,
data/COCO/dataset.py:147-166), batched.

  SMPLLayer(pose [B,72], betas [B,10] | None, trans [B,3] | None)  ->  (verts [B,6890,3], joints [B,24,3])      the layer's own call
  get_smpl_coord(layer, pose, shape, trans)                        ->  (mesh, joints + five face key points), mm   the datasets' wrapper
  targets_from_smpl(layer, pose, shape, trans, regressors ...)     ->  {'mesh', 'reg_pose3d', 'lift_pose3d'}        Trainer.step's targets
  SMPLLayer.fit(verts [B,6890,3], iters, init) / fit_to_mesh(layer, verts) -> (pose, betas, trans, rms)             the inverse: mesh -> parameters

The model's arrays come from the caller: the official files are licence-gated and are no part of this package.  The layer is
differentiable in pose, betas and trans (gator_smpl_backward_f32, csrc/smpl_backward.hip), once; not in the model's arrays."""
import ctypes
import pickle

import numpy as np
import torch

from . import _lib

FACE_KPS_VERTEX = (331, 2802, 6262, 3489, 3990)      # lib/smpl.py:22: nose, L/R eye, L/R ear as mesh vertices


def _plain(x):
    """A value of a model file as numpy: chumpy arrays carry .r, the joint regressor is a scipy sparse matrix."""
    if hasattr(x, 'r') and not isinstance(x, np.ndarray):
        x = x.r
    if hasattr(x, 'toarray'):
        x = x.toarray()
    return np.asarray(x)


def _f32(a):
    return np.ascontiguousarray(_plain(a), dtype=np.float32)


def model_arrays(d):
    """A mapping with the model files' keys (v_template, shapedirs, posedirs, weights, J_regressor, kintree_table, f) -> the layer's
    arguments as plain numpy arrays: {v_template, shapedirs, posedirs, weights, J_regressor, parents, faces}."""
    kt = _plain(d['kintree_table']) if 'kintree_table' in d else _plain(d['parents'])
    faces = d['f'] if 'f' in d else (d['faces'] if 'faces' in d else None)
    return {'v_template': _f32(d['v_template']), 'shapedirs': _f32(d['shapedirs']) if 'shapedirs' in d else None,
            'posedirs': _f32(d['posedirs']), 'weights': _f32(d['weights']), 'J_regressor': _f32(d['J_regressor']),
            'parents': (kt[0] if kt.ndim == 2 else kt).astype(np.int64), 'faces': None if faces is None else _plain(faces).astype(np.int64)}


def read_npz(path):
    with np.load(path) as z:
        return model_arrays({k: z[k] for k in z.files})


def read_pkl(path):
    """The model pickle as the reference reads it (pickle, latin1).  The official files hold chumpy objects, so unpickling them needs
    chumpy installed; a file re-saved with plain numpy arrays (and a scipy sparse or dense regressor) needs nothing."""
    with open(path, 'rb') as fh:
        return model_arrays(pickle.load(fh, encoding='latin1'))


class _LayerFunction(torch.autograd.Function):
    """The layer under autograd: the same forward entry, and gator_smpl_backward_f32 on the saved float32 inputs with the center_idx /
    out_scale of that call (the attributes may have changed by the time backward runs).  First derivatives only."""

    @staticmethod
    def forward(ctx, layer, center, out_scale, want_verts, want_joints, pose, betas, trans):
        verts, joints = layer._run(pose, betas, trans, center, out_scale, want_verts, want_joints)
        ctx.layer, ctx.center, ctx.out_scale = layer, center, out_scale
        ctx.save_for_backward(pose, betas, trans)
        ctx.set_materialize_grads(False)                  # an output the loss does not reach arrives as None, not as zeros
        outs = tuple(o for o in (verts, joints) if o is not None)
        ctx.which = (want_verts, want_joints)
        return outs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        layer = ctx.layer
        pose, betas, trans = ctx.saved_tensors
        grads = list(grads)
        gv = grads.pop(0) if ctx.which[0] else None
        gj = grads.pop(0) if ctx.which[1] else None
        need = ctx.needs_input_grad[5:8]
        B = pose.shape[0]
        new = lambda ok, ref: torch.empty_like(ref) if (ok and ref is not None) else None      # noqa: E731
        g_pose, g_betas, g_trans = new(need[0], pose), new(need[1], betas), new(need[2], trans)
        if gv is None and gj is None:                     # neither output reached the loss
            for g in (g_pose, g_betas, g_trans):
                if g is not None:
                    g.zero_()
        elif B and (g_pose is not None or g_betas is not None or g_trans is not None):
            gv = None if gv is None else gv.contiguous().float()
            gj = None if gj is None else gj.contiguous().float()
            ptr = _lib.ptr
            layer._call('gator_smpl_backward_f32', ptr(pose), ptr(betas), ptr(trans), B, ctx.center, ctx.out_scale, ptr(gv), ptr(gj), ptr(g_pose),
                        ptr(g_betas), ptr(g_trans), _lib.stream_ptr(layer.device))
        return None, None, None, None, None, g_pose, g_betas, g_trans


class SMPLLayer(_lib.DeviceHandle):
    """smplpytorch's SMPL_Layer on one HIP device.  Same call order (pose, betas, trans), the same center_idx attribute, th_faces /
    th_J_regressor / th_weights / kintree_parents as the reference layer exposes them.  out_scale multiplies the (translated or
    centred) outputs: 1000 for the datasets' millimetres.

    Differentiable, like the reference layer: when grad mode is on and pose, betas or trans requires grad, the outputs carry a
    grad_fn and loss.backward() fills the inputs' .grad with the exact vector-Jacobian product, computed on the device from the
    inputs (nothing per vertex is kept from the forward; an output that was not asked for or not used costs nothing, and a loss on
    the joints alone does no per-vertex work).  First derivatives only, and none with respect to the model's arrays.  Otherwise the
    call is the plain forward: the same launches, the same bits, no grad_fn."""
    PREFIX = 'gator_smpl'
    NO_CPU = 'the layer runs on a HIP device (there is no CPU path)'
    _ctx = property(lambda self: self._h)      # the C ABI's name for this handle

    def __init__(self, v_template, shapedirs, posedirs, weights, J_regressor, parents, faces=None, center_idx=None, device='cuda',
                 out_scale=1.0, gender='neutral'):
        vt, w, jr = _f32(v_template), _f32(weights), _f32(J_regressor)
        if vt.ndim != 2 or w.ndim != 2 or jr.ndim != 2 or vt.shape[1] != 3:
            raise ValueError('SMPLLayer: v_template [NV,3], weights [NV,NJ] and J_regressor [NJ,NV] are 2-D arrays')
        nv, nj = vt.shape[0], w.shape[1]
        sd = np.zeros((nv, 3, 0), np.float32) if shapedirs is None else _f32(shapedirs)
        pd = _f32(posedirs)
        par = np.asarray(_plain(parents)).astype(np.int64).reshape(-1)
        if w.shape[0] != nv or jr.shape != (nj, nv) or sd.ndim != 3 or sd.shape[:2] != (nv, 3) or pd.shape != (nv, 3, (nj - 1) * 9) or par.shape != (nj,):
            raise ValueError('SMPLLayer: inconsistent model shapes: v_template %s shapedirs %s posedirs %s weights %s J_regressor %s parents %s'
                             % (vt.shape, sd.shape, pd.shape, w.shape, jr.shape, par.shape))
        par32 = np.ascontiguousarray(np.where((par < 0) | (par >= 2 ** 31), -1, par).astype(np.int32))
        self.num_verts, self.num_joints, self.num_betas = nv, nj, sd.shape[2]
        self.center_idx, self.out_scale, self.gender = center_idx, float(out_scale), gender
        self.kintree_parents = [int(p) for p in par]
        self.th_faces = None if faces is None else torch.from_numpy(np.asarray(_plain(faces)).astype(np.int64))
        self.th_J_regressor = torch.from_numpy(jr)
        self.th_weights = torch.from_numpy(w)
        self.th_v_template = torch.from_numpy(vt).unsqueeze(0)
        model = _lib.SmplModel(ctypes.sizeof(_lib.SmplModel), nv, nj, sd.shape[2], vt.ctypes.data, sd.ctypes.data if sd.size else None,
                               pd.ctypes.data, w.ctypes.data, jr.ctypes.data, par32.ctypes.data)
        self._create(device, ctypes.byref(model))

    @classmethod
    def from_arrays(cls, v_template, shapedirs, posedirs, weights, J_regressor, parents, faces=None, **kw):
        return cls(v_template, shapedirs, posedirs, weights, J_regressor, parents, faces=faces, **kw)

    @classmethod
    def from_npz(cls, path, **kw):
        return cls(**read_npz(path), **kw)

    @classmethod
    def from_pkl(cls, path, **kw):
        return cls(**read_pkl(path), **kw)

    def _call(self, name, *args):
        """The C entry `name` on this layer's ctx, with the layer's device current; a failure raises with the library's message."""
        with torch.cuda.device(self.device):
            _lib.check(getattr(_lib.load(), name)(self._ctx, *args), name)

    def workspace(self):
        """(device address, batch capacity) of the ctx's workspace: a test hook."""
        base, cap = ctypes.c_void_p(), ctypes.c_int64()
        self._call('gator_smpl_workspace', ctypes.byref(base), ctypes.byref(cap))
        return base.value or 0, cap.value

    def workspace_bytes(self):
        """(bytes held by the ctx's grown blocks, growths since create): a test hook; a repeated call at a known batch moves neither."""
        b, n = ctypes.c_int64(), ctypes.c_int64()
        self._call('gator_smpl_workspace_bytes', ctypes.byref(b), ctypes.byref(n))
        return b.value, n.value

    def _arg(self, x, width, name, B):
        if x is None:
            return None
        if not x.is_cuda or x.device != self.device:
            raise RuntimeError('SMPLLayer: %s must live on %s' % (name, self.device))
        x = x.contiguous().float()
        if x.dim() != 2 or x.shape != (B, width):
            raise ValueError('SMPLLayer: %s must be [%d,%d], got %s' % (name, B, width, tuple(x.shape)))
        return x

    def forward(self, th_pose_axisang, th_betas=None, th_trans=None, want_verts=True, want_joints=True):
        if th_pose_axisang.dim() != 2:
            raise ValueError('SMPLLayer: pose must be [B,%d], got %s' % (self.num_joints * 3, tuple(th_pose_axisang.shape)))
        B = th_pose_axisang.shape[0]
        pose = self._arg(th_pose_axisang, self.num_joints * 3, 'pose', B)
        betas = self._arg(th_betas, self.num_betas, 'betas', B) if self.num_betas else None
        trans = self._arg(th_trans, 3, 'trans', B)
        center = -1 if (self.center_idx is None or trans is not None) else int(self.center_idx)
        if torch.is_grad_enabled() and any(x is not None and x.requires_grad for x in (pose, betas, trans)):
            outs = list(_LayerFunction.apply(self, center, self.out_scale, want_verts, want_joints, pose, betas, trans))
            return (outs.pop(0) if want_verts else None), (outs.pop(0) if want_joints else None)
        return self._run(pose, betas, trans, center, self.out_scale, want_verts, want_joints)

    def _run(self, pose, betas, trans, center, out_scale, want_verts, want_joints):
        B = pose.shape[0]
        verts = torch.empty((B, self.num_verts, 3), device=self.device, dtype=torch.float32) if want_verts else None
        joints = torch.empty((B, self.num_joints, 3), device=self.device, dtype=torch.float32) if want_joints else None
        ptr = _lib.ptr
        self._call('gator_smpl_forward_f32', ptr(pose), ptr(betas), ptr(trans), B, center, out_scale, ptr(verts), ptr(joints),
                   _lib.stream_ptr(self.device))
        return verts, joints

    __call__ = forward

    def fit_width(self):
        """(P, N): the fit's unknowns, 3 NJ + NB + 3, and the padded width of its normal matrix."""
        P, N = ctypes.c_int32(), ctypes.c_int32()
        self._call('gator_smpl_fit_width', ctypes.byref(P), ctypes.byref(N))
        return P.value, N.value

    def _verts_arg(self, verts):
        if verts.dim() != 3 or verts.shape[1:] != (self.num_verts, 3):
            raise ValueError('SMPLLayer: verts must be [B,%d,3], got %s' % (self.num_verts, tuple(verts.shape)))
        if not verts.is_cuda or verts.device != self.device:
            raise RuntimeError('SMPLLayer: verts must live on %s' % (self.device,))
        return verts.contiguous().float()

    def fit(self, verts, iters=20, init=None):
        """The inverse of forward: (pose [B,NJ*3], betas [B,NB], trans [B,3], rms [B]) whose forward (out_scale 1, no centring) is the
        least-squares fit to verts [B,NV,3] (the layer's unit), by `iters` Levenberg-Marquardt steps on the device
        (gator_smpl_fit_f32, csrc/smpl_fit.hip).  init: a (pose, betas, trans) tuple, e.g. the previous frame's result; None starts
        from zero pose, zero betas and the centroid offset.  rms: the root mean square vertex distance of the returned state.
        No host synchronisation; capturable into a graph; a sample with a non-finite input comes back as NaN, alone.

        Deliberately out of scope: pose and shape priors, joint-limit constraints, per-vertex weights, fitting to 2D evidence, and
        models with more than 4 influences per vertex (refused).  The result is the unconstrained least-squares fit in vertex
        space: on a mesh that no parameters reproduce, nothing keeps the pose plausible.  For any of these, take the fit as the start
        and refine through the layer itself with a torch optimiser: forward is differentiable in pose, betas and trans."""
        verts = self._verts_arg(verts)
        B = verts.shape[0]
        if init is not None:
            if len(init) != 3:
                raise ValueError('SMPLLayer.fit: init is a (pose, betas, trans) tuple')
            ip, ib, it = (self._arg(init[0], self.num_joints * 3, 'init pose', B), self._arg(init[1], self.num_betas, 'init betas', B),
                          self._arg(init[2], 3, 'init trans', B))
        else:
            ip = ib = it = None
        pose, betas, trans, rms = (torch.empty(shape, device=self.device, dtype=torch.float32)
                                   for shape in ((B, self.num_joints * 3), (B, self.num_betas), (B, 3), (B,)))
        ptr = _lib.ptr
        self._call('gator_smpl_fit_f32', ptr(verts), ptr(ip), ptr(ib), ptr(it), B, int(iters), ptr(pose), ptr(betas), ptr(trans), ptr(rms),
                   _lib.stream_ptr(self.device))
        return pose, betas, trans, rms

    def fit_normal(self, pose, betas, trans, verts):
        """The fit's stage entry (gator_smpl_fit_normal_f32): M = [J | r]^T [J | r] at the given state, [B,N,N] float32 with
        H = M[:, :P, :P], g = M[:, :P, P] and the squared error M[:, P, P].  Only the upper triangle is specified."""
        verts = self._verts_arg(verts)
        B = verts.shape[0]
        pose = self._arg(pose, self.num_joints * 3, 'pose', B)
        betas = self._arg(betas, self.num_betas, 'betas', B)
        trans = self._arg(trans, 3, 'trans', B)
        N = self.fit_width()[1]
        M = torch.zeros((B, N, N), device=self.device, dtype=torch.float32)
        ptr = _lib.ptr
        self._call('gator_smpl_fit_normal_f32', ptr(pose), ptr(betas), ptr(trans), ptr(verts), B, ptr(M), _lib.stream_ptr(self.device))
        return M


def fit_to_mesh(layer, verts, **kw):
    """SMPLLayer.fit as a function: verts [B,NV,3] -> (pose, betas, trans, rms); iters= and init= as there."""
    return layer.fit(verts, **kw)


def get_smpl_coord(layer, pose, shape, trans=None):
    """The datasets' get_smpl_coord, batched (data/COCO/dataset.py:147-166, data/AMASS/dataset.py:199-213): a shape with any |beta| > 3
    becomes the mean shape, the layer runs with millimetre output ((x + trans) * 1000, trans in metres), and the five face key-point
    vertices are appended to the joints (lib/smpl.py:22-36).  -> (mesh [B,NV,3], joints [B,NJ+5,3]) in mm."""
    if shape is not None:
        shape = shape.float()
        shape = torch.where((shape.abs() > 3).any(dim=1, keepdim=True), torch.zeros_like(shape), shape)
    saved = layer.out_scale
    layer.out_scale = 1000.0
    try:
        mesh, joints = layer(pose, shape, trans)
    finally:
        layer.out_scale = saved
    idx = torch.as_tensor(FACE_KPS_VERTEX, device=mesh.device)
    return mesh, torch.cat([joints, mesh[:, idx]], 1)


def targets_from_smpl(layer, pose, shape, trans, regressor_h36m, regressor_coco=None, input_joint_name='human36'):
    """The un-augmented tail of the datasets' __getitem__ (data/AMASS/dataset.py:252-265,301) on the device: mesh and joints from the
    layer in mm, the H36M (and COCO + pelvis + neck) joints regressed from the mesh, everything root-relative.
    regressor_*: gator_amd.eval.JointRegressor.  -> the dict Trainer.step takes: 'mesh' [B,6890,3] in metres, 'reg_pose3d' [B,17,3]
    and 'lift_pose3d' [B,17|19,3] in mm.  The camera-frame root rotation, augmentation and noise stay with the caller
    (gator_amd.batch.camera_frame_batch builds the first two on the device)."""
    mesh, _ = get_smpl_coord(layer, pose, shape, trans)
    h36m = regressor_h36m(mesh)
    root = h36m[:, :1]
    if input_joint_name == 'coco':
        if regressor_coco is None:
            raise ValueError("targets_from_smpl: input_joint_name 'coco' needs regressor_coco")
        coco = regressor_coco(mesh)
        pelvis = (coco[:, 11:12] + coco[:, 12:13]) * 0.5          # add_pelvis_and_neck, data/AMASS/dataset.py:215-227
        neck = (coco[:, 5:6] + coco[:, 6:7]) * 0.5
        coco = torch.cat([coco, pelvis, neck], 1)
        lift = coco - coco[:, -2:-1]
    elif input_joint_name == 'human36':
        lift = h36m - root
    else:
        raise ValueError("targets_from_smpl: input_joint_name is 'coco' or 'human36', got %r" % (input_joint_name,))
    return {'mesh': (mesh - root) / 1000, 'reg_pose3d': h36m - root, 'lift_pose3d': lift}
