"""References of the camera-frame batch tests (gator_amd.batch, csrc/train_batch.hip): numpy float64 restatements of the reference's
lines, and a float32-literal restatement that keeps the reference's dtype at each step.

  root rotation        data/Human36M/dataset.py:267-274, data/AMASS/dataset.py:188-196   root_to_camera (through scipy's Rotation: the
                                                                                        reference's transforms3d is not installed, and
                                                                                        an independent route is the point)
  mean-shape rule      data/Human36M/dataset.py:265                                      mean_shape_rule
  translation          data/Human36M/dataset.py:287-298, data/AMASS/dataset.py:205-211   camera_targets, step 1
  cam2pixel, world2cam lib/coord_utils.py:104-114
  j3d_processing       lib/aug_utils.py:42-48,67-83
  fitting error        data/Human36M/dataset.py:302-309, gate :392-401
  pelvis and neck      data/Human36M/dataset.py:322-334

tests/golden/train_batch.npz (tools/gen_golden_batch.py) holds the reference's own cam2pixel, j3d_processing, flip_3d_joint and world2cam
on seeded inputs; tests/test_host_batch_refs.py pins the restatement to it.  Nothing here shares code with the kernels."""
import numpy as np
from scipy.spatial.transform import Rotation

H36M_FLIP_PAIRS = ((1, 4), (2, 5), (3, 6), (14, 11), (15, 12), (16, 13))            # data/Human36M/dataset.py:59
COCO_FLIP_PAIRS = ((1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16))
EPS32 = 2.0 ** -24               # half an ulp of float32, relative: one rounding to nearest


def exp_rotvec(r):
    """[..., 3] rotation vectors -> [..., 3, 3]; the zero vector is the identity."""
    r = np.asarray(r, np.float64)
    return Rotation.from_rotvec(r.reshape(-1, 3)).as_matrix().reshape(r.shape[:-1] + (3, 3))


def log_rotmat(M):
    M = np.asarray(M, np.float64)
    return Rotation.from_matrix(M.reshape(-1, 3, 3)).as_rotvec().reshape(M.shape[:-2] + (3,))


def root_to_camera(pose, R, root_idx=0):
    """-> (pose with the root replaced by log(R exp(root)), the products R exp(root) [B,3,3]), float64."""
    out = np.array(pose, np.float64)
    sl = slice(root_idx * 3, root_idx * 3 + 3)
    M = np.asarray(R, np.float64) @ exp_rotvec(out[:, sl])
    out[:, sl] = log_rotmat(M)
    return out, M


def mean_shape_rule(betas):
    b = np.array(betas)
    b[(np.abs(b) > 3).any(1)] = 0
    return b


def cam2pixel(cam_coord, f, c):
    with np.errstate(divide='ignore', invalid='ignore'):
        x = cam_coord[:, 0] / cam_coord[:, 2] * f[0] + c[0]
        y = cam_coord[:, 1] / cam_coord[:, 2] * f[1] + c[1]
    return np.stack([x, y, cam_coord[:, 2]], 1)


def world2cam(world_coord, R, t):
    return (R @ world_coord.T).T + t.reshape(1, 3)


def flip_3d_joint(kp, flip_pairs):
    kp = kp.copy()
    for a, b in flip_pairs:
        kp[[a, b]] = kp[[b, a]]
    kp[:, 0] = -kp[:, 0]
    return kp


def j3d_processing(S, r, f, flip_pairs):
    """float64 in, float64 out (the reference ends with astype('float32'))."""
    rot_mat = np.eye(3)
    if not r == 0:
        rot_rad = -r * np.pi / 180
        sn, cs = np.sin(rot_rad), np.cos(rot_rad)
        rot_mat[0, :2] = [cs, -sn]
        rot_mat[1, :2] = [sn, cs]
    S = np.einsum('ij,kj->ki', rot_mat, S)
    return flip_3d_joint(S, flip_pairs) if f else S


def add_pelvis_and_neck(j):
    return np.concatenate([j, (j[11:12] + j[12:13]) * 0.5, (j[5:6] + j[6:7]) * 0.5])


def get_fitting_error(h36m_joint, smpl_mesh, regressor):
    h36m_joint = h36m_joint - h36m_joint[0, None, :]
    from_smpl = regressor @ smpl_mesh
    from_smpl = from_smpl - from_smpl.mean(0)[None, :] + h36m_joint.mean(0)[None, :]
    return np.sqrt(((h36m_joint - from_smpl) ** 2).sum(1)).mean()


def _opt(x, b, dt=np.float64):
    return None if x is None else np.asarray(x[b], dt)


def camera_targets(verts, joints, focal, princpt, reg_h36m, reg_coco=None, lift_set='human36', trans=None, cam_t=None, R=None,
                   compensate_root=False, joint_cam=None, joint_img=None, rot_deg=None, flip=None, flip_pairs=(), fitting_thr=np.inf,
                   root_idx=0):
    """The whole step in float64, sample by sample, as the datasets' __getitem__ does it.  reg_*: dense [J, NV].  -> a dict of the
    six outputs, 'mesh_cam' (mm) and 'scale' [B]: the largest sum of |w| |coordinate| that feeds a sample's outputs, for the bounds."""
    B = len(verts)
    Jd = np.asarray(reg_h36m, np.float64)
    Jc = None if reg_coco is None else np.asarray(reg_coco, np.float64)
    out = {k: [] for k in ('mesh', 'reg_pose3d', 'lift_pose3d', 'joint_img', 'fit_error', 'valid', 'mesh_cam', 'scale', 'joint_cam_abs')}
    for b in range(B):
        v = np.asarray(verts[b], np.float64)
        tr, ct, Rb = _opt(trans, b), _opt(cam_t, b), _opt(R, b)
        tr = np.zeros(3) if tr is None else tr
        ct = np.zeros(3) if ct is None else ct
        if compensate_root:
            smpl_trans = (Rb @ tr[:, None]).reshape(1, 3) + ct.reshape(1, 3)
            root = np.asarray(joints[b][root_idx], np.float64).reshape(1, 3)
            smpl_trans = smpl_trans - root + (Rb @ root.T).T
        else:
            smpl_trans = (tr + ct).reshape(1, 3)
        mesh_cam = (v + smpl_trans) * 1000
        h36m = Jd @ mesh_cam
        f, c = np.asarray(focal[b], np.float64), np.asarray(princpt[b], np.float64)
        ds = _opt(joint_cam, b)
        root_h = h36m[:1] if ds is None else ds[:1]
        reg = h36m - h36m[:1] if ds is None else ds - ds[:1]
        if lift_set == 'coco':
            coco = add_pelvis_and_neck(Jc @ mesh_cam)
            lift, img, cam_abs = coco - coco[-2:-1], cam2pixel(coco, f, c)[:, :2], coco
        else:
            lift, cam_abs = reg, h36m
            img = cam2pixel(h36m, f, c)[:, :2] if joint_img is None else np.asarray(joint_img[b], np.float64)[:, :2]
        r = 0.0 if rot_deg is None else float(rot_deg[b])
        fl = 0 if flip is None else int(flip[b])
        lift = j3d_processing(lift, r, fl, flip_pairs)
        mesh = mesh_cam - root_h
        valid = np.ones(3)
        err = np.nan
        if ds is not None:
            err = get_fitting_error(reg, mesh, Jd)
            if err > fitting_thr:
                valid[0] = 0
                if lift_set == 'coco':
                    valid[1] = 0
        scale = max(np.abs(mesh_cam).max(), (np.abs(Jd) @ np.abs(mesh_cam)).max(), 0.0 if Jc is None else (np.abs(Jc) @ np.abs(mesh_cam)).max(),
                    0.0 if ds is None else np.abs(ds).max())
        for k, x in (('mesh', mesh / 1000), ('reg_pose3d', reg), ('lift_pose3d', lift), ('joint_img', img), ('fit_error', err),
                     ('valid', valid), ('mesh_cam', mesh_cam), ('scale', scale), ('joint_cam_abs', cam_abs)):
            out[k].append(x)
    return {k: np.array(x) for k, x in out.items()}


ACC = 1e-10          # fp64 accumulation, relative to the magnitudes summed: ~1e6 fp64 roundings, far above any list length here


def tolerances(ref, focal, projected):
    """Element-wise bounds for the six outputs against `ref` (camera_targets' dict): one float32 rounding, 2^-23 |ref|, plus the fp64
    accumulation ACC * scale in the output's unit.  A pixel carries the accumulation error of X, Y and Z through X / Z * f:
    f (1 + |X / Z|) / |Z| times it (first order)."""
    s = ref['scale']
    tol = {'mesh': 2 * EPS32 * np.abs(ref['mesh']) + ACC * s[:, None, None] / 1000,
           'reg_pose3d': 2 * EPS32 * np.abs(ref['reg_pose3d']) + ACC * s[:, None, None],
           'lift_pose3d': 2 * EPS32 * np.abs(ref['lift_pose3d']) + 2 * ACC * s[:, None, None],
           'fit_error': 2 * EPS32 * np.abs(ref['fit_error']) + ACC * s}
    if projected:
        P = ref['joint_cam_abs']
        with np.errstate(divide='ignore', invalid='ignore'):
            gain = np.asarray(focal, np.float64)[:, None, :] * (1 + np.abs(P[:, :, :2] / P[:, :, 2:])) / np.abs(P[:, :, 2:])
        tol['joint_img'] = 2 * EPS32 * np.abs(ref['joint_img']) + ACC * s[:, None, None] * gain
    else:
        tol['joint_img'] = np.zeros_like(ref['joint_img'])          # passed through
    return tol


def camera_targets_f32(verts, joints, focal, princpt, reg_h36m, reg_coco=None, lift_set='human36', trans=None, cam_t=None, R=None,
                       compensate_root=False, joint_cam=None, joint_img=None, rot_deg=None, flip=None, flip_pairs=(), fitting_thr=np.inf,
                       root_idx=0):
    """The same step with the reference's dtype at each line: the layer's float32 mesh and joints, float32 R / t / trans and a float32
    translation added and scaled in place (Human36M:262,288-298), float32 regressors and np.dot, cam2pixel in float32 with the focal
    lengths as Python floats, j3d_processing through a float64 rotation matrix and astype('float32'), the fitting error in float32."""
    f32 = np.float32
    B = len(verts)
    Jd = np.asarray(reg_h36m, f32)
    Jc = None if reg_coco is None else np.asarray(reg_coco, f32)
    out = {k: [] for k in ('mesh', 'reg_pose3d', 'lift_pose3d', 'joint_img', 'fit_error', 'valid')}
    for b in range(B):
        mesh_cam = np.array(verts[b], f32)
        tr, ct, Rb = _opt(trans, b, f32), _opt(cam_t, b, f32), _opt(R, b, f32)
        tr = np.zeros(3, f32) if tr is None else tr
        ct = np.zeros(3, f32) if ct is None else ct
        if compensate_root:
            smpl_trans = np.dot(Rb, tr[:, None]).reshape(1, 3) + ct.reshape(1, 3)
            root = np.asarray(joints[b][root_idx], f32).reshape(1, 3)
            smpl_trans = smpl_trans - root + np.dot(Rb, root.transpose(1, 0)).transpose(1, 0)
        else:
            smpl_trans = (tr + ct).reshape(1, 3)
        mesh_cam += smpl_trans
        mesh_cam *= 1000
        h36m = np.dot(Jd, mesh_cam)
        f, c = [float(x) for x in focal[b]], [float(x) for x in princpt[b]]
        ds = _opt(joint_cam, b, f32)
        root_h = h36m[:1] if ds is None else ds[:1]
        reg = h36m - h36m[:1] if ds is None else ds - ds[:1]
        if lift_set == 'coco':
            coco = add_pelvis_and_neck(np.dot(Jc, mesh_cam))
            lift, img = coco - coco[-2:-1], cam2pixel(coco, f, c)[:, :2]
        else:
            lift = reg
            img = cam2pixel(h36m, f, c)[:, :2] if joint_img is None else np.asarray(joint_img[b], f32)[:, :2]
        r = 0.0 if rot_deg is None else float(rot_deg[b])
        fl = 0 if flip is None else int(flip[b])
        lift = j3d_processing(lift, r, fl, flip_pairs).astype(f32)
        mesh = mesh_cam - root_h
        valid = np.ones(3, f32)
        err = f32(np.nan)
        if ds is not None:
            err = get_fitting_error(reg, mesh, Jd)
            if err > fitting_thr:
                valid[0] = 0
                if lift_set == 'coco':
                    valid[1] = 0
        for k, x in (('mesh', mesh / 1000), ('reg_pose3d', reg), ('lift_pose3d', lift), ('joint_img', img.astype(f32)), ('fit_error', err),
                     ('valid', valid)):
            assert np.asarray(x).dtype == f32, k
            out[k].append(x)
    return {k: np.array(x) for k, x in out.items()}


# --- seeded inputs ------------------------------------------------------------------------------------------------------------------

def sparse_regressor(n_joint, nv, rs, special=()):
    """Sparse convex rows (8 draws of a vertex, Dirichlet weights) as COO lists -> (row, col, val float32, dense float64 [n_joint, nv]).
    special = (empty, duplicated, negative): a row without entries, a row whose entries all name one vertex twice, a row with one
    negative weight (the rows still sum to 1 except the empty one)."""
    row, col, val = [], [], []
    for j in range(n_joint):
        idx = rs.randint(0, nv, 8)
        w = rs.dirichlet(np.ones(8)).astype(np.float32)
        if special and j == special[0]:
            continue
        if special and j == special[1]:
            idx[4:] = idx[:4]
        if special and j == special[2]:
            w[0], w[1] = np.float32(-0.25), np.float32(w[1] + w[0] + 0.25)
        row += [j] * 8
        col += list(idx)
        val += list(w)
    perm = rs.permutation(len(row))                                     # entries in no particular order
    row, col, val = np.array(row, np.int64)[perm], np.array(col, np.int64)[perm], np.array(val, np.float32)[perm]
    dense = np.zeros((n_joint, nv))
    np.add.at(dense, (row, col), val.astype(np.float64))
    return row, col, val, dense


def camera_case(nv, B, seed, lift_set='human36', dataset_joints=False, special=True, n_h36m=17, n_coco=17):
    """Seeded float32 inputs for gator_camera_targets_f32 on given vertices: a body-sized point cloud ~4 m in front of a camera, SMPL-like
    joints, rotations, both translations, intrinsics, regressors (with the three special rows), optional dataset joints 20-40 mm off the
    regressed ones, rot / flip from {0, 30, -90} x {0, 1} cycling over the batch."""
    rs = np.random.RandomState(seed)
    f32 = np.float32
    c = {'verts': ((rs.rand(B, nv, 3) - 0.5) * np.array([0.9, 1.7, 0.4])).astype(f32), 'joints': (rs.randn(B, 24, 3) * 0.3).astype(f32),
         'trans': (rs.randn(B, 3) * 0.5).astype(f32), 'cam_t': (rs.randn(B, 3) * 0.3 + np.array([0, 0, 4.5])).astype(f32),
         'R': Rotation.from_rotvec(rs.randn(B, 3) * 0.4).as_matrix().astype(f32),
         'focal': (1145.0 + rs.randn(B, 2) * 5).astype(f32), 'princpt': (np.array([512.0, 515.0]) + rs.randn(B, 2) * 3).astype(f32)}
    c['reg_h36m_coo'] = sparse_regressor(n_h36m, nv, rs, (9, 10, 13) if special else ())
    c['reg_coco_coo'] = sparse_regressor(n_coco, nv, rs, (3, 4, 14) if special else ())
    c['reg_h36m'], c['reg_coco'] = c['reg_h36m_coo'][3], c['reg_coco_coo'][3]
    c['rot_deg'] = np.array([(0.0, 30.0, -90.0)[i % 3] for i in range(B)], f32)
    c['flip'] = np.array([(i // 3) % 2 for i in range(B)], np.int32)
    c['lift_set'] = lift_set
    c['flip_pairs'] = COCO_FLIP_PAIRS if lift_set == 'coco' else H36M_FLIP_PAIRS
    c['joint_cam'] = c['joint_img'] = None
    if dataset_joints:
        mesh_cam = (c['verts'].astype(np.float64) + (c['trans'].astype(np.float64) + c['cam_t'])[:, None, :]) * 1000
        h = np.einsum('jv,bvc->bjc', c['reg_h36m'], mesh_cam)
        c['joint_cam'] = (h + rs.randn(B, n_h36m, 3) * np.linspace(5, 60, B)[:, None, None]).astype(f32)
        c['joint_img'] = np.stack([cam2pixel(c['joint_cam'][b].astype(np.float64), c['focal'][b], c['princpt'][b])[:, :2] for b in range(B)]).astype(f32)
    return c


def reference_of(c, **kw):
    """camera_targets on a camera_case with the un-compensated translation trans + cam_t, overridden by kw."""
    a = dict(trans=c['trans'], cam_t=c['cam_t'], R=None, compensate_root=False, joint_cam=c['joint_cam'], joint_img=c['joint_img'],
             rot_deg=c['rot_deg'], flip=c['flip'], flip_pairs=c['flip_pairs'], lift_set=c['lift_set'])
    a.update(kw)
    fn = a.pop('fn', camera_targets)
    return fn(c['verts'], c['joints'], c['focal'], c['princpt'], c['reg_h36m'], c['reg_coco'] if a['lift_set'] == 'coco' else None, **a)
