"""The fp64 Procrustes oracle (oracle.gator_oracle.rigid_align / pa_mpjpe) on closed-form cases, on the CPU: the reference the device
tests of tests/test_gpu_eval_edges.py lean on is itself checked where no GPU is needed."""
import numpy as np
import pytest

from oracle import gator_oracle as go
from tests.eval_edge_refs import random_rotation


def _similarity(rs, n):
    a = rs.randn(n, 3) * 300.0
    c, R, t = 0.5 + rs.rand(), random_rotation(rs), rs.randn(3) * 100.0
    return a, c, R, t


@pytest.mark.parametrize('n', [3, 4, 14, 32])
def test_exact_similarity_image_is_recovered(n):
    """b = c R a + t: the alignment reproduces b, and PA-MPJPE is zero (N = 3 is always coplanar: rank-2 covariance)."""
    rs = np.random.RandomState(100 + n)
    for _ in range(20):
        a, c, R, t = _similarity(rs, n)
        b = c * a @ R.T + t
        got = go.rigid_align(a, b)
        assert np.abs(got - b).max() <= 1e-12 * np.abs(b).max()
        assert go.pa_mpjpe(a[None], b[None]) <= 1e-12 * np.abs(b).max()


@pytest.mark.parametrize('n', [4, 14, 32])
def test_mirrored_target_leaves_the_analytic_residual(n):
    """b = c R M a + t with the mirror M = diag(1, 1, -1): no rotation reaches it.  H = cov(a) (c M R^T) has the singular values
    c lambda_i (lambda: eigenvalues of cov(a), descending), so the best ROTATION leaves
        sum |aligned - b|^2 = n c^2 (tr cov(a) - (lambda_0 + lambda_1 - lambda_2)^2 / tr cov(a)).
    The residual is a difference of two terms of the size of the target's total variance n c^2 tr cov(a), so that is what fp64 rounding
    is relative to: 1e-12 of it."""
    rs = np.random.RandomState(200 + n)
    for _ in range(20):
        a, c, R, t = _similarity(rs, n)
        b = c * (a * np.array([1.0, 1.0, -1.0])) @ R.T + t
        lam = np.sort(np.linalg.eigvalsh(np.cov(a.T, bias=True)))[::-1]
        want = n * c * c * (lam.sum() - (lam[0] + lam[1] - lam[2]) ** 2 / lam.sum())
        got = ((go.rigid_align(a, b) - b) ** 2).sum()
        assert abs(got - want) <= 1e-12 * n * c * c * lam.sum()
        cc, RR, tt = go.rigid_transform_3d(a, b)
        assert abs(np.linalg.det(RR) - 1.0) <= 1e-12


@pytest.mark.parametrize('n', [3, 14])
def test_collinear_source_gives_the_one_dimensional_least_squares_fit(n):
    """a_i = o + alpha_i d exactly (integers): H has rank 1, R is fixed only on d, and that is all the result needs.  With
    alpha' = alpha - mean(alpha): aligned_i = mean(b) + alpha'_i w / sum(alpha'^2), w = sum_j alpha'_j (b_j - mean(b)) -- the per-coordinate
    least-squares regression of b on alpha, a set of points on one line."""
    rs = np.random.RandomState(300 + n)
    for _ in range(50):
        d = rs.randint(-3, 4, 3).astype(np.float64)
        if not d.any():
            d[0] = 1.0
        alpha = rs.permutation(np.arange(-n, n))[:n].astype(np.float64)
        a = rs.randint(-50, 51, 3) + alpha[:, None] * d
        b = rs.randn(n, 3) * 300.0 + rs.randn(3) * 100.0
        al = alpha - alpha.mean()
        w = (al[:, None] * (b - b.mean(0))).sum(0)
        want = b.mean(0) + al[:, None] * w / (al ** 2).sum()
        got = go.rigid_align(a, b)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(b).max()
        off = got - got.mean(0)
        assert np.abs(np.cross(off, w / np.linalg.norm(w))).max() <= 1e-12 * np.abs(b).max()       # on the fitted line


def _align_with_basis(A, B, turn):
    """rigid_align as the oracle computes it, with the last two columns of numpy's U (the null space of a rank-1 covariance) turned by
    the angle `turn` in their plane."""
    n = A.shape[0]
    ca, cb = A.mean(0), B.mean(0)
    H = (A - ca).T @ (B - cb) / n
    U, s, V = np.linalg.svd(H)
    cs, sn = np.cos(turn), np.sin(turn)
    U = U.copy()
    U[:, 1:] = U[:, 1:] @ np.array([[cs, -sn], [sn, cs]])
    R = V.T @ U.T
    if np.linalg.det(R) < 0:
        s[-1] = -s[-1]
        V[2] = -V[2]
        R = V.T @ U.T
    c = 1 / np.var(A, axis=0).sum() * s.sum()
    return ((c * R) @ A.T).T + (-(c * R) @ ca + cb)


@pytest.mark.parametrize('n', [3, 14])
def test_collinear_target_residual_does_not_depend_on_the_null_space_basis(n):
    """Target exactly on a line, source generic: rank-1 covariance from the target side.  The rotation is not unique (the source may be
    turned about the line), but every optimal choice leaves each point at the same distance from its target -- the condition under which
    the device is compared with the oracle on |aligned - b| there."""
    rs = np.random.RandomState(400 + n)
    for _ in range(50):
        a = rs.randn(n, 3) * 300.0
        e = rs.randint(-3, 4, 3).astype(np.float64)
        if not e.any():
            e[2] = 1.0
        b = rs.randint(-50, 51, 3) + rs.permutation(np.arange(-n, n))[:n, None].astype(np.float64) * e
        d0 = np.linalg.norm(_align_with_basis(a, b, 0.0) - b, axis=1)
        assert np.abs(d0 - np.linalg.norm(go.rigid_align(a, b) - b, axis=1)).max() <= 1e-12 * np.abs(b).max()      # turn 0 IS the oracle
        d1 = np.linalg.norm(_align_with_basis(a, b, rs.uniform(0.3, 2 * np.pi - 0.3)) - b, axis=1)
        assert np.abs(d0 - d1).max() <= 1e-12
        assert abs(go.pa_mpjpe(a[None], b[None]) - d1.mean()) <= 1e-12 * np.abs(b).max()
