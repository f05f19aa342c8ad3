"""Input families, fp64 references and bounds for the evaluation / preprocessing edge tests (tests/test_gpu_eval_edges.py,
tests/test_oracle_procrustes.py).  Everything here is numpy on the host; the references are oracle.gator_oracle and plain fp64 numpy."""
import numpy as np

from oracle import gator_oracle as go

F32_EPS = 2.0 ** -24          # half an ulp of float32 relative to the value: the rounding of one float32 store


def random_rotation(rs):
    q, r = np.linalg.qr(rs.randn(3, 3))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


def rotations(rs, B):
    return np.stack([random_rotation(rs) for _ in range(B)])


def image_of(rs, a, noise=20.0, scale=1.1, shift=50.0):
    """A noisy similarity image of every sample of a [B,N,3]."""
    B, N = a.shape[:2]
    R = rotations(rs, B)
    return scale * np.einsum('bnk,brk->bnr', a, R) + rs.randn(B, 1, 3) * shift + rs.randn(B, N, 3) * noise


def _int_dirs(rs, B, lo=-3, hi=3):
    d = rs.randint(lo, hi + 1, (B, 3)).astype(np.float64)
    d[~d.any(1), 0] = 1.0
    return d


def lattice_line(rs, B, N):
    """Exactly collinear in float32 and in fp64: integer offset + integer multiples of a small integer direction."""
    alpha = np.stack([rs.permutation(np.arange(-N, N))[:N] for _ in range(B)]).astype(np.float64)
    return rs.randint(-50, 51, (B, 1, 3)) + alpha[:, :, None] * _int_dirs(rs, B)[:, None, :]


def axis_line(rs, B, N):
    """Points on one coordinate axis (any float32 abscissae): the other two coordinates are exactly zero."""
    p = np.zeros((B, N, 3))
    ax = rs.randint(0, 3, B)
    p[np.arange(B), :, ax] = (rs.randn(B, N) * 300.0).astype(np.float32)
    return p


def lattice_plane(rs, B, N, near=None):
    """Exactly coplanar in a plane that is no coordinate plane: integer offset + integer combinations of two small integer vectors.
    near [B,N,3]: take the lattice point closest to each given point instead of a random one."""
    e1 = _int_dirs(rs, B)
    e2 = _int_dirs(rs, B)
    par = ~np.cross(e1, e2).any(1)                       # parallel pair: swap in a vector that is not
    e2[par] = np.roll(e1[par], 1, axis=1) + np.array([0.0, 0.0, 1.0])
    par = ~np.cross(e1, e2).any(1)
    e2[par] = e1[par] + np.array([1.0, 0.0, 0.0])
    assert np.cross(e1, e2).any(1).all()
    E = np.stack([e1, e2], 2) * 8.0                      # [B,3,2]
    o = rs.randint(-50, 51, (B, 1, 3)).astype(np.float64)
    if near is None:
        k = rs.randint(-20, 21, (B, N, 2)).astype(np.float64)
        k[:, 0], k[:, 1], k[:, 2] = (0, 0), (7, 0), (0, 9)          # never all on one line
    else:
        k = np.stack([np.round(np.linalg.lstsq(E[i], (near[i] - o[i]).T, rcond=None)[0].T) for i in range(B)])
    return o + np.einsum('brk,bnk->bnr', E, k)


def polyhedron(rs, B, which):
    """Octahedron (6) or cube (8) vertices under a random rotation: an isotropic covariance, three equal singular values."""
    if which == 'octahedron':
        v = np.concatenate([np.eye(3), -np.eye(3)])
    else:
        v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
    return 300.0 * np.einsum('nk,brk->bnr', v, rotations(rs, B)) + rs.randn(B, 1, 3) * 100.0


# name -> what is compared: 'points' (the aligned points are unique), 'dist' (only |aligned - b| is), 'centroid', 'nonfinite'
FAMILIES = {}


def family(name, mode='points', ns=(14,)):
    def deco(fn):
        FAMILIES[name] = (fn, mode, ns)
        return fn
    return deco


def _generic(rs, B, N):
    return rs.randn(B, N, 3) * 300.0


@family('generic', ns=(3, 14))          # N = 3 is always coplanar
def _f(rs, B, N):
    a = _generic(rs, B, N)
    return a, image_of(rs, a)


@family('mirrored')
def _f(rs, B, N):
    a = _generic(rs, B, N)
    return a, image_of(rs, a * np.array([1.0, 1.0, -1.0]))


@family('mirrored and coplanar')
def _f(rs, B, N):
    a = lattice_plane(rs, B, N)
    Q = rotations(rs, B)
    m = a - 2.0 * np.einsum('bnk,bk->bn', a, Q[:, :, 0])[:, :, None] * Q[:, None, :, 0]      # mirrored in a random plane
    return a, image_of(rs, m, noise=5.0)


@family('coplanar a (rotated plane)')
def _f(rs, B, N):
    a = lattice_plane(rs, B, N)
    return a, image_of(rs, a, noise=5.0)


@family('coplanar b (rotated plane)')
def _f(rs, B, N):
    a = _generic(rs, B, N)
    return a, lattice_plane(rs, B, N, near=image_of(rs, a))


@family('coplanar a and b (rotated planes)')
def _f(rs, B, N):
    a = lattice_plane(rs, B, N)
    return a, lattice_plane(rs, B, N, near=image_of(rs, a, noise=5.0))


def _thin(rs, B, N, ratio):
    p = _generic(rs, B, N)
    p[:, :, 2] *= ratio                  # tiny float32 values are exact: the thickness survives the rounding of the inputs
    return p


for _r in (1e-12, 1e-9, 1e-6, 1e-3):
    @family('plane thickness %g on a' % _r)
    def _f(rs, B, N, r=_r):
        a = _thin(rs, B, N, r)
        return a, image_of(rs, a)

    @family('plane thickness %g on b' % _r)
    def _f(rs, B, N, r=_r):
        b = _thin(rs, B, N, r)
        return image_of(rs, b), b

for _w in ('octahedron', 'cube'):
    @family('repeated singular values (%s)' % _w, ns=({'octahedron': 6, 'cube': 8}[_w],))
    def _f(rs, B, N, w=_w):
        a = polyhedron(rs, B, w)
        b = image_of(rs, a, noise=0.0)
        b[B // 2:] += rs.randn(B - B // 2, N, 3) * 20.0         # first half: exact image, three equal singular values; second: nearly
        return a, b


@family('b == a')
def _f(rs, B, N):
    a = (_generic(rs, B, N) + rs.randn(B, 1, 3) * 100.0).astype(np.float32).astype(np.float64)
    return a, a.copy()


@family('b = exact similarity image of a')
def _f(rs, B, N):
    a = _generic(rs, B, N)
    return a, image_of(rs, a, noise=0.0)


for _c in (1e4, -1e4, 1e6, -1e6):
    @family('centroids at %+g, spread 1e2' % _c)
    def _f(rs, B, N, c=_c):
        a = rs.randn(B, N, 3) * 100.0
        b = image_of(rs, a, noise=10.0, shift=0.0) - c * np.array([1.0, -1.0, 0.5])
        return a + c, b

for _s in (1e-6, 1e-3, 1e3, 1e6):
    @family('overall scale %g' % _s)
    def _f(rs, B, N, s=_s):
        a = rs.randn(B, N, 3)
        return a * s, image_of(rs, a, noise=0.1, shift=1.0) * s


@family('a exactly collinear (lattice direction)', ns=(3, 14))
def _f(rs, B, N):
    return lattice_line(rs, B, N), _generic(rs, B, N) + rs.randn(B, 1, 3) * 100.0


@family('a exactly collinear (coordinate axis)', ns=(3, 14))
def _f(rs, B, N):
    return axis_line(rs, B, N), _generic(rs, B, N) + rs.randn(B, 1, 3) * 100.0


@family('b exactly collinear, a generic', mode='dist', ns=(3, 14))
def _f(rs, B, N):
    b = lattice_line(rs, B, N)
    b[B // 2:] = axis_line(rs, B - B // 2, N)
    return _generic(rs, B, N), b


@family('a and b exactly collinear', mode='dist', ns=(3, 14))
def _f(rs, B, N):
    a, b = lattice_line(rs, B, N), lattice_line(rs, B, N)
    b[B // 2:] = axis_line(rs, B - B // 2, N)
    return a, b


for _r in (1e-12, 1e-9, 1e-6):
    @family('a near-collinear, line thickness %g' % _r)
    def _f(rs, B, N, r=_r):
        a = _generic(rs, B, N)
        ax = rs.randint(0, 3, B)
        keep = np.zeros((B, 1, 3))
        keep[np.arange(B), 0, ax] = 1.0
        return a * (keep + (1.0 - keep) * r), _generic(rs, B, N) + rs.randn(B, 1, 3) * 100.0


@family('all target points identical', mode='centroid')
def _f(rs, B, N):
    return _generic(rs, B, N), np.repeat(rs.randn(B, 1, 3) * 300.0, N, axis=1)


def make_family(name, N, B=65, seed=0):
    """-> (a32, b32, a64, b64, mode): the float32 inputs both sides are fed, and the fp64 draws they were rounded from."""
    fn, mode, _ = FAMILIES[name]
    rs = np.random.RandomState((seed * 1000003 + sum(ord(ch) for ch in name) * 131 + N) % (2 ** 31))
    a, b = fn(rs, B, N)
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    assert np.isfinite(a32).all() and np.isfinite(b32).all()
    return a32, b32, a, b, mode


def family_cases():
    return [(name, n) for name, (_, _, ns) in FAMILIES.items() for n in ns]


def oracle_align(a, b):
    """go.rigid_align on every sample, fp64.  Non-finite results (var(a) = 0, NaN inputs) come back as numpy gives them."""
    with np.errstate(all='ignore'):
        out = []
        for x, y in zip(np.asarray(a, np.float64), np.asarray(b, np.float64)):
            try:
                out.append(go.rigid_align(x, y))
            except np.linalg.LinAlgError:               # numpy's SVD refuses to converge on NaN / Inf
                out.append(np.full(x.shape, np.nan))
        return np.stack(out)


def points_bound(b, ref):
    """The suite's criterion for aligned points (tests/test_gpu_caller_side.py), per sample: 3e-7 max|b| + 1e-6 max|ref|."""
    return 3e-7 * np.abs(b).max((1, 2)) + 1e-6 * np.abs(ref).max((1, 2))


def rss(x, b):
    return ((np.asarray(x, np.float64) - np.asarray(b, np.float64)) ** 2).sum((1, 2))


def rss_floor(ref, rss_ref):
    """What rounding the aligned points to float32 can add to a residual sum of squares: the device stores x + d with |d_k| <= 2^-24 |x_k|,
    so |d| <= dn = sqrt(3N) 2^-24 max|x| and sum|r + d|^2 <= sum|r|^2 + 2 |r| dn + dn^2."""
    N = ref.shape[1]
    dn = np.sqrt(3.0 * N) * F32_EPS * np.abs(ref).max((1, 2))
    return 2.0 * np.sqrt(rss_ref) * dn + dn * dn


def perturbed_fits(rs, a, b, count=8):
    """The oracle's (c, R, t) of every sample, each perturbed `count` times by a relative 1e-4 .. 1e-2 (scale, a rotation about a random
    axis, a shift of that fraction of the target's spread) -> residual sums of squares [count, B], fp64."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.empty((count, len(a)))
    for i, (x, y) in enumerate(zip(a, b)):
        c, R, t = go.rigid_transform_3d(x, y)
        spread = np.sqrt(((y - y.mean(0)) ** 2).sum(1).mean())
        for k in range(count):
            eps = 10.0 ** rs.uniform(-4, -2, 3)
            ax = rs.randn(3)
            ax /= np.linalg.norm(ax)
            K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
            dR = np.eye(3) + np.sin(eps[1]) * K + (1 - np.cos(eps[1])) * K @ K
            # the rotation turns about the centroid of a, so that it is a small change of the FIT whatever the distance to the origin
            ca = x.mean(0)
            pert = (c * (1 + eps[0] * rs.choice([-1, 1]))) * ((x - ca) @ (dR @ R).T + ca @ R.T) + t + eps[2] * spread * rs.randn(3)
            out[k, i] = ((pert - y) ** 2).sum()
    return out


def oracle_joint_errors(pred32, tgt32, eval_joints, root, pred_scale):
    """Both columns of gator_joint_errors_f32 from the oracle, per sample.  The oracle is fed float32(pred) * float32(pred_scale), as
    the reference multiplies the float32 mesh by 1000 before it regresses the joints."""
    p = (pred32.astype(np.float32) * np.float32(pred_scale)).astype(np.float64)
    t = tgt32.astype(np.float64)
    ev = None if eval_joints is None else list(eval_joints)
    e0 = np.array([go.mpjpe(p[i:i + 1], t[i:i + 1], ev, root) for i in range(len(p))])
    pr, tr = p - p[:, root:root + 1], t - t[:, root:root + 1]
    with np.errstate(all='ignore'):
        e1 = np.array([go.pa_mpjpe(pr[i:i + 1], tr[i:i + 1], ev) for i in range(len(p))])
    return e0, e1


def errors_bound(want):
    """The suite's criterion for the error columns (tests/test_gpu_eval_path.py): 2e-5 max(1, want)."""
    return 2e-5 * np.maximum(1.0, want)
