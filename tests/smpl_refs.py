"""References of the SMPL layer tests: the synthetic body models (no licensed file anywhere: arrays of SMPL's shapes drawn from a
seeded np.random.RandomState) and the float64 numpy restatement of smplpytorch's SMPL_Layer.forward (smpl_layer.py:65-158,
rodrigues_layer.py:13-52).  The restatement shares no code with the kernels; tests/golden/smpl_layer.npz (written by
tools/gen_golden_smpl.py from the real layer) pins it to the reference."""
import hashlib

import numpy as np

SMPL_PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21)
ARRAYS = ('v_template', 'shapedirs', 'posedirs', 'weights', 'J_regressor', 'parents', 'faces')


def synthetic_model(nv, nj=24, nb=10, seed=0, dense_weights=False):
    """A body model of the given size, float32 as the layer holds it: the template in a body-sized box (metres), shapedirs ~1e-2,
    posedirs ~2e-3, 4 Dirichlet skinning weights per vertex (dense_weights: all nj), an 8-vertex convex regressor row per joint."""
    rs = np.random.RandomState(seed)
    m = {}
    m['v_template'] = ((rs.rand(nv, 3) - 0.5) * np.array([0.9, 1.7, 0.4])).astype(np.float32)
    m['shapedirs'] = (rs.randn(nv, 3, nb) * 1e-2).astype(np.float32)
    m['posedirs'] = (rs.randn(nv, 3, (nj - 1) * 9) * 2e-3).astype(np.float32)
    w = np.zeros((nv, nj), np.float32)
    ni = nj if dense_weights else min(4, nj)
    for v in range(nv):
        w[v, rs.permutation(nj)[:ni]] = rs.dirichlet(np.ones(ni)).astype(np.float32)
    m['weights'] = w
    r = np.zeros((nj, nv), np.float32)
    for j in range(nj):
        idx = rs.randint(0, nv, 8)
        np.add.at(r[j], idx, rs.dirichlet(np.ones(8)).astype(np.float32))
    m['J_regressor'] = r
    m['parents'] = np.array([SMPL_PARENTS[j] if j < 24 else j - 1 for j in range(nj)], np.int64)
    m['faces'] = rs.randint(0, nv, (max(2 * nv - 4, 1), 3)).astype(np.int64)
    return m


def model_sha256(m):
    h = hashlib.sha256()
    for k in ARRAYS:
        a = np.ascontiguousarray(m[k])
        h.update(('%s %s %s;' % (k, a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def rodrigues(a):
    """batch_rodrigues + quat2mat on [..., 3] axis-angles -> [..., 3, 3], with the layer's `+ 1e-8` inside the norm."""
    a = np.asarray(a, np.float64)
    angle = np.sqrt(((a + 1e-8) ** 2).sum(-1, keepdims=True))
    axis = a / angle
    q = np.concatenate([np.cos(angle * 0.5), np.sin(angle * 0.5) * axis], -1)
    q = q / np.sqrt((q ** 2).sum(-1, keepdims=True))
    w, x, y, z = (q[..., i] for i in range(4))
    R = np.stack([w * w + x * x - y * y - z * z, 2 * x * y - 2 * w * z, 2 * w * y + 2 * x * z,
                  2 * w * z + 2 * x * y, w * w - x * x + y * y - z * z, 2 * y * z - 2 * w * x,
                  2 * x * z - 2 * w * y, 2 * w * x + 2 * y * z, w * w - x * x - y * y + z * z], -1)
    return R.reshape(a.shape[:-1] + (3, 3))


def lbs_forward(m, pose, betas=None, trans=None, center_idx=None, out_scale=1.0):
    """float64: (pose [B,NJ*3], betas [B,NB] | None, trans [B,3] | None) -> (verts [B,NV,3], joints [B,NJ,3]),
    (layer output + trans - centre joint) * out_scale; center_idx only without trans, as the layer applies it."""
    f = {k: np.asarray(m[k], np.float64) for k in ('v_template', 'shapedirs', 'posedirs', 'weights', 'J_regressor')}
    nj = f['weights'].shape[1]
    pose = np.asarray(pose, np.float64)
    B = pose.shape[0]
    R = rodrigues(pose.reshape(B, nj, 3))
    pose_map = (R[:, 1:] - np.eye(3)).reshape(B, (nj - 1) * 9)
    v_shaped = np.broadcast_to(f['v_template'], (B,) + f['v_template'].shape)
    if betas is not None and f['shapedirs'].shape[2]:
        v_shaped = v_shaped + np.einsum('vck,bk->bvc', f['shapedirs'], np.asarray(betas, np.float64))
    J = np.einsum('jv,bvc->bjc', f['J_regressor'], v_shaped)
    v_posed = v_shaped + np.einsum('vck,bk->bvc', f['posedirs'], pose_map)
    G = np.zeros((B, nj, 4, 4))
    G[:, :, 3, 3] = 1.0
    for j in range(nj):
        L = np.zeros((B, 4, 4))
        L[:, 3, 3] = 1.0
        L[:, :3, :3] = R[:, j]
        if j == 0:
            L[:, :3, 3] = J[:, 0]
            G[:, 0] = L
        else:
            p = int(m['parents'][j])
            L[:, :3, 3] = J[:, j] - J[:, p]
            G[:, j] = G[:, p] @ L
    A = G[:, :, :3, :].copy()
    A[:, :, :, 3] -= np.einsum('bjrc,bjc->bjr', G[:, :, :3, :3], J)
    T = np.einsum('vj,bjrc->bvrc', f['weights'], A)
    verts = np.einsum('bvrc,bvc->bvr', T[..., :3], v_posed) + T[..., 3]
    joints = G[:, :, :3, 3].copy()
    if trans is not None:
        if center_idx is not None:
            raise ValueError('center_idx goes with trans = None')
        off = np.asarray(trans, np.float64)[:, None, :]
    elif center_idx is not None:
        off = -joints[:, center_idx:center_idx + 1].copy()
    else:
        off = 0.0
    return (verts + off) * out_scale, (joints + off) * out_scale


# --- the golden cases: tools/gen_golden_smpl.py runs the real layer on them, the tests rebuild models and read inputs from the file ---
N_SAMPLES = 65
# name -> (model arguments (nv, nj, nb, seed, dense), forward options, samples whose fp32 reference outputs are stored)
CASES = {
    'nv1': ((1, 24, 10, 11, False), {}, 65),
    'nv63': ((63, 24, 10, 12, False), {}, 8),
    'nv64': ((64, 24, 10, 13, False), {}, 8),
    'nv65': ((65, 24, 10, 14, False), {}, 8),
    'nv127': ((127, 24, 10, 21, False), {}, 4),
    'nv128': ((128, 24, 10, 22, False), {}, 4),
    'nv129': ((129, 24, 10, 23, False), {}, 4),
    'nv257': ((257, 24, 10, 15, False), {}, 8),
    'nv6890': ((6890, 24, 10, 16, False), {}, 3),
    'families': ((257, 24, 10, 17, False), {'families': True}, 16),
    'no_betas_no_trans': ((65, 24, 10, 18, False), {'betas': False, 'trans': False}, 8),
    'center0': ((65, 24, 10, 18, False), {'trans': False, 'center_idx': 0}, 8),
    'center23': ((65, 24, 10, 18, False), {'trans': False, 'center_idx': 23}, 8),
    'scale1000': ((65, 24, 10, 18, False), {'out_scale': 1000.0}, 8),
    'dense': ((65, 24, 10, 19, True), {}, 8),
    'nb0': ((65, 24, 0, 20, False), {'betas': False}, 8),
}
FAMILIES = ('zero', 'root_only', 'tiny', 'pi', 'five_rad', 'betas_pm3')


def case_inputs(name):
    """The case's inputs, float32: pose [65,72], betas [65,nb], trans [65,3] (|trans| ~ 2 m).  Poses are random axis-angles of up to
    ~1.2 rad per joint; the 'families' case starts with one sample per pose family."""
    (nv, nj, nb, seed, dense), opt, _ = CASES[name]
    rs = np.random.RandomState(1000 + seed)
    B = N_SAMPLES
    pose = (rs.randn(B, nj * 3) * 0.4).astype(np.float32)
    betas = rs.uniform(-2.5, 2.5, (B, nb)).astype(np.float32)
    trans = (rs.randn(B, 3) * 1.2).astype(np.float32)
    if opt.get('families'):
        pose[0] = 0.0                                                   # finite only with the `+ 1e-8`
        pose[1, 3:] = 0.0                                               # root-only rotation
        pose[2] = (rs.randn(nj * 3) * 1e-7).astype(np.float32)          # entries ~1e-7
        pose[3, 3:6] = (np.float32(np.pi), 0.0, 0.0)                    # a rotation by exactly pi (fp32's pi)
        pose[3, 48:51] = (0.0, 0.0, np.float32(np.pi))
        v = rs.randn(3)
        pose[4, 0:3] = (v / np.linalg.norm(v) * 5.0).astype(np.float32)  # an angle of 5 rad
        pose[4, 27:30] = (0.0, 5.0, 0.0)
        betas[5] = np.where(rs.rand(nb) < 0.5, -3.0, 3.0).astype(np.float32)
    return pose, betas, trans
