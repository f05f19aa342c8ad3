"""The fp64 reference of gator_mesh_errors_f32 per sample, built from the oracle's regress_joints, mpjpe and rigid_align only, and the
regressors and meshes the mesh-evaluation tests share (tests/test_host_mesh_eval_refs.py, tests/test_gpu_mesh_eval.py).  Numpy and
the oracle on the host; nothing here touches a device."""
import numpy as np
import torch

from oracle import gator_oracle as go

H36M_EVAL = (1, 2, 3, 4, 5, 6, 8, 10, 11, 12, 13, 14, 15, 16)      # data/PW3D/dataset.py:46


def dense_of(row, col, val, n_joint, n_verts):
    """The dense fp64 matrix of a COO list of float32 values: duplicates add, an untouched row stays zero."""
    d = np.zeros((n_joint, n_verts))
    np.add.at(d, (np.asarray(row, np.int64), np.asarray(col, np.int64)), np.asarray(val, np.float32).astype(np.float64))
    return d


def sparse_rows(rs, n_joint, n_verts, per_row=6):
    """A dense float32 [n_joint, n_verts] regressor whose rows each hold min(per_row, n_verts) positive weights that sum to 1 (to
    float32 rounding), like the shipped SMPL / H36M regressors."""
    d = np.zeros((n_joint, n_verts), np.float32)
    k = min(per_row, n_verts)
    for j in range(n_joint):
        c = rs.choice(n_verts, k, replace=False)
        w = rs.rand(k) + 0.1
        d[j, c] = (w / w.sum()).astype(np.float32)
    return d


def scaled(x32, scale):
    """What both sides start from: float32(x) * float32(scale), widened (lib/core/base.py:219 multiplies the float32 mesh)."""
    return (np.asarray(x32, np.float32) * np.float32(scale)).astype(np.float64)


def _regress(dense64, mesh64):
    return go.regress_joints(np.asarray(dense64, np.float64), torch.from_numpy(mesh64[None])).numpy()


def _pa(p, t):
    """mean |rigid_align(p, t) - t|; NaN where numpy's SVD refuses a non-finite covariance."""
    try:
        return float(np.sqrt(((go.rigid_align(p, t) - t) ** 2).sum(1)).mean())
    except np.linalg.LinAlgError:
        return float('nan')


def oracle_mesh_errors(pred32, tgt32, root_dense, root=0, eval_dense=None, eval_joints=H36M_EVAL, eval_root=0, pred_scale=1.0,
                       target_scale=1.0):
    """[B,5] fp64: the five columns of gator_mesh_errors_f32 as data/PW3D/dataset.py:337-375 forms them, sample by sample.
    root_dense / eval_dense: dense [n_joint, N] regressors (fp64 images of the float32 values the device holds)."""
    P, T = scaled(pred32, pred_scale), scaled(tgt32, target_scale)
    N = P.shape[1]
    out = np.full((len(P), 5), np.nan)
    with np.errstate(all='ignore'):
        for b, (p, t) in enumerate(zip(P, T)):
            jp, jt = _regress(root_dense, p), _regress(root_dense, t)                       # [1,nj,3]
            # dataset.py:345-348: mesh and joints in one array, aligned on row N + root
            cp, ct = np.concatenate([p[None], jp], 1), np.concatenate([t[None], jt], 1)
            out[b, 2] = go.mpjpe(jp, jt, None, root)
            out[b, 3] = go.mpjpe(cp, ct, list(range(N)), N + root)
            out[b, 4] = _pa(p - jp[0, root], t - jt[0, root])
            if eval_dense is not None:
                ep, et = _regress(eval_dense, p), _regress(eval_dense, t)
                ev = None if eval_joints is None else list(eval_joints)
                out[b, 0] = go.mpjpe(ep, et, ev, eval_root)
                ep, et = (ep - ep[:, eval_root:eval_root + 1])[0], (et - et[:, eval_root:eval_root + 1])[0]
                out[b, 1] = _pa(ep, et) if ev is None else _pa(ep[ev], et[ev])
    return out


def mesh_bound(want, pred32, tgt32, pred_scale=1.0, target_scale=1.0):
    """Per sample and column: the suite's criterion for an error column, 2e-5 max(1, want), plus the input-rounding term of the
    aligned-points criterion, 3e-7 max|scaled coordinate of the sample|."""
    big = np.maximum(np.abs(scaled(pred32, pred_scale)).max((1, 2)), np.abs(scaled(tgt32, target_scale)).max((1, 2)))
    return 2e-5 * np.maximum(1.0, want) + 3e-7 * big[:, None]


def body_like(rs, B, N, err_mm=40.0):
    """(pred, target) float32 [B,N,3] in METRES, |coordinate| <= 4: a point cloud of ~0.5 m spread somewhere within 2 m of the origin,
    and a prediction that is a slightly turned, scaled and noisy image of it (errors of a few cm)."""
    t = rs.randn(B, N, 3) * 0.5 + rs.uniform(-2.0, 2.0, (B, 1, 3))
    ang = rs.randn(B) * 0.05
    R = np.stack([np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]) for a in ang])
    p = 1.03 * np.einsum('bnk,brk->bnr', t, R) + rs.randn(B, 1, 3) * 0.05 + rs.randn(B, N, 3) * (err_mm / 1000.0)
    return np.clip(p, -4.0, 4.0).astype(np.float32), np.clip(t, -4.0, 4.0).astype(np.float32)
