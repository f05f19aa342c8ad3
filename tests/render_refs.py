"""numpy references of the renderer (int64 coverage, float64 everything else) and the meshes its tests draw.  They restate
demo/renderer.py's geometry and the documented lighting on their own; nothing here is shared with gator_amd/csrc/render.hip.
tests/test_host_render_refs.py checks them on the CPU; tests/test_gpu_render.py holds the kernels against them.

Tolerances, derived here (u = 2^-24, the fp32 unit roundoff):

D_NORMAL = 1.  k_render_vertices sums the face cross products and normalises in fp64 and rounds each component once to fp32.  The fp64
  chain (6 subtractions, 6 products, 3 differences and one addition per face and component, a 3x3 rotation, the norm, one division:
  fewer than 20 (F_v + 2) roundings of 2^-53) moves a component by at most 20 (F_v + 2) 2^-53 sum|n_f| / |sum n_f|, below 2^-40 of the
  bound for any vertex of fewer than 1000 faces; the final rounding of a component of magnitude <= 1 is at most u / 2.  Since
  sum|n_f| >= |sum n_f|, every component is within 1 * u * sum|n_f| / |sum n_f| of the fp64 normal.

D_Z = 24.  k_render_raster's depth of one face at a pixel is z = za + wb (zb - za) + wc (zc - za) in fp32 with wb = fl(E_ca) / fl(area).
  With Z = max|z_i|:  zb - za is off by <= u |zb - za| <= 2 u Z;  wb carries 3 roundings (two conversions, one division);  the product
  wb (zb - za) therefore <= (1 + 3 + 1) u wb 2 Z = 10 u wb Z, both products together <= 10 u Z because wb + wc <= 1;  each of the two
  additions rounds a convex combination of the z_i, <= u Z each.  One face: <= 12 u Z.  The device picks the face whose COMPUTED depth is
  smallest, so its true depth exceeds the true minimum by at most the errors of two faces: 24 u Z.  (A face of constant depth is exact.)

Clip planes.  Coverage is compared bit for bit, and a fragment is clipped on its depth: fp32 on the device, fp64 here.  The two agree
  on every face of constant depth (both forms are exact there, so z = +-1 and one ulp beyond are decided alike); the sloped faces of the
  test scenes stay inside |z| <= 0.9 (the sentinel test: seeded draws from (-1, 1)), farther than 12 u from the planes."""
import numpy as np

SENTINEL = -2 ** 31
GUARD_PX = float(2 ** 20)
D_NORMAL = 1.0
D_Z = 24.0
U32 = 2.0 ** -24

AMBIENT = 0.3
LIGHTS = np.array([[0.0, -np.sqrt(0.5), -np.sqrt(0.5), 1.2], [np.sqrt(0.5), 0.0, -np.sqrt(0.5), 1.2]])
COLOR = np.array([1.0, 1.0, 0.9])


# ---- geometry -----------------------------------------------------------------------------------------------------------------------
def apply_rotation(verts, R=None):
    """What demo/renderer.py draws, back in the model's coordinates: flip with Rx(180), rotate, flip back."""
    v = np.asarray(verts, np.float64)
    if R is None:
        return v
    F = np.diag([1.0, -1.0, -1.0])
    return v @ (F @ np.asarray(R, np.float64) @ F).T


def project(verts, cam, W, H, R=None):
    """verts [V,3], cam (sx, sy, tx, ty) -> px [V], py [V] (float64 pixels), z [V]."""
    u = apply_rotation(verts, R)
    sx, sy, tx, ty = (float(c) for c in cam)
    with np.errstate(all='ignore'):
        px = (1.0 + sx * (u[:, 0] + tx)) / 2.0 * W
        py = (1.0 + sy * (u[:, 1] + ty)) / 2.0 * H
    return px, py, u[:, 2]


def snap(px, py, verts):
    """24.8 fixed point, round to nearest even; SENTINEL for a vertex that is not finite or beyond the guard band.  -> [V,2] int64."""
    with np.errstate(all='ignore'):
        ok = np.isfinite(np.asarray(verts, np.float64)).all(1) & (np.abs(px) <= GUARD_PX) & (np.abs(py) <= GUARD_PX)
    out = np.full((len(px), 2), SENTINEL, np.int64)
    out[ok, 0] = np.rint(px[ok] * 256.0).astype(np.int64)
    out[ok, 1] = np.rint(py[ok] * 256.0).astype(np.int64)
    return out


def snap_margin(p):
    """Distance of p * 256 from the nearest rounding boundary (k + 1/2)."""
    t = np.asarray(p, np.float64) * 256.0
    return np.abs(t - np.floor(t) - 0.5)


def face_normals(verts, faces):
    v = np.asarray(verts, np.float64)
    return np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])


def vertex_normals(verts, faces, R=None):
    """Area-weighted vertex normals of the drawn mesh -> (normals [V,3] unit, ratio [V] = sum|n_f| / |sum n_f|)."""
    fn = face_normals(apply_rotation(verts, R), faces)
    V = len(verts)
    acc, mag = np.zeros((V, 3)), np.zeros(V)
    for c in range(3):
        np.add.at(acc, faces[:, c], fn)
        np.add.at(mag, faces[:, c], np.linalg.norm(fn, axis=1))
    ln = np.linalg.norm(acc, axis=1)
    with np.errstate(all='ignore'):
        return acc / np.maximum(ln, np.finfo(np.float64).tiny)[:, None], mag / ln


# ---- coverage and visibility --------------------------------------------------------------------------------------------------------
def _owns(dx, dy):
    return (dy < 0) | ((dy == 0) & (dx > 0))


def face_at(xy, z, face, ii, jj, cull=True):
    """One face at pixel centres (rows ii, columns jj; int arrays of one shape): -> (covered [bool], depth [float64], weights [.,3]).
    xy [V,2] int64 fixed point, z [V] float64.  Exact integer coverage with the top-left rule; depth and weights from the exact edge
    values in float64; a fragment whose depth lies outside [-1, 1] is not covered."""
    ii, jj = np.asarray(ii, np.int64), np.asarray(jj, np.int64)
    none = np.zeros(ii.shape, bool), np.full(ii.shape, np.inf), np.zeros(ii.shape + (3,))
    p = xy[np.asarray(face)]
    if (p == SENTINEL).any():
        return none
    a, b, c = (int(p[0, 0]), int(p[0, 1])), (int(p[1, 0]), int(p[1, 1])), (int(p[2, 0]), int(p[2, 1]))
    area = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
    if area == 0 or (cull and area > 0):         # x right, y down: front faces have a negative cross product
        return none
    X, Y = jj * 256 + 128, ii * 256 + 128
    s = 1 if area > 0 else -1
    inside = np.ones(ii.shape, bool)
    E = []
    for (p0, p1) in ((a, b), (b, c), (c, a)):
        dx, dy = s * (p1[0] - p0[0]), s * (p1[1] - p0[1])         # the edge as the oriented triangle (E > 0 inside) runs it
        e = dx * (Y - p0[1]) - dy * (X - p0[0])
        inside &= (e > 0) | ((e == 0) & bool(_owns(np.int64(dx), np.int64(dy))))
        E.append(e.astype(np.float64))
    A = float(s * area)
    w = np.stack([E[1] / A, E[2] / A, E[0] / A], -1)                 # weight of a is the edge opposite a: b->c
    zz = np.asarray(z, np.float64)[np.asarray(face)]
    depth = zz[0] + w[..., 1] * (zz[1] - zz[0]) + w[..., 2] * (zz[2] - zz[0])     # exact on a face of constant depth (the clip planes)
    inside &= (depth >= -1.0) & (depth <= 1.0)
    return inside, depth, w


def rasterise(meshes, faces, H, W, cull=True):
    """meshes: list of (xy [V,2] int64, z [V]) sharing one image, in slot order.  -> dict of [H,W] arrays:
    count (faces covering the pixel), zmin (fp64 minimum depth, inf where empty), winner (smallest id = slot * F + face among the faces
    AT that minimum, -1 where empty), zabs (max |z_i| over the vertices of the covering faces)."""
    F = len(faces)
    count = np.zeros((H, W), np.int64)
    zmin = np.full((H, W), np.inf)
    winner = np.full((H, W), -1, np.int64)
    zabs = np.zeros((H, W))
    for slot, (xy, z) in enumerate(meshes):
        for f, face in enumerate(faces):
            p = xy[face]
            if (p == SENTINEL).any():
                continue
            j0, j1 = max(0, int(np.ceil((p[:, 0].min() - 128) / 256.0))), min(W - 1, int(np.floor((p[:, 0].max() - 128) / 256.0)))
            i0, i1 = max(0, int(np.ceil((p[:, 1].min() - 128) / 256.0))), min(H - 1, int(np.floor((p[:, 1].max() - 128) / 256.0)))
            if j0 > j1 or i0 > i1:
                continue
            ii, jj = np.meshgrid(np.arange(i0, i1 + 1), np.arange(j0, j1 + 1), indexing='ij')
            cov, depth, _ = face_at(xy, z, face, ii, jj, cull)
            if not cov.any():
                continue
            ci, cj, cd = ii[cov], jj[cov], depth[cov]
            count[ci, cj] += 1
            zabs[ci, cj] = np.maximum(zabs[ci, cj], np.abs(np.asarray(z, np.float64)[face]).max())
            better = cd < zmin[ci, cj]               # ids ascend, so an equal depth keeps the earlier, smaller id
            zmin[ci[better], cj[better]] = cd[better]
            winner[ci[better], cj[better]] = slot * F + f
    return {'count': count, 'zmin': zmin, 'winner': winner, 'zabs': zabs}


def depth_of_ids(meshes, faces, ids, cull=True):
    """fp64 depth of face `ids[i,j]` (slot * F + face, -1 = none) at every pixel and whether it covers that pixel."""
    H, W = ids.shape
    F = len(faces)
    depth, cov = np.full((H, W), np.inf), np.zeros((H, W), bool)
    for fid in np.unique(ids[ids >= 0]):
        ii, jj = np.nonzero(ids == fid)
        xy, z = meshes[int(fid) // F]
        c, d, _ = face_at(xy, z, faces[int(fid) % F], ii, jj, cull)
        depth[ii, jj], cov[ii, jj] = d, c
    return depth, cov


def decode_keys(keys):
    """[.,H,W] int64 storage of the uint64 keys -> (id [int64, -1 where empty], depth [float32, inf where empty])."""
    k = np.asarray(keys).view(np.uint64)
    empty = k == np.uint64(0xFFFFFFFFFFFFFFFF)
    o = (k >> np.uint64(32)).astype(np.uint32)
    bits = np.where(o & np.uint32(0x80000000), o & np.uint32(0x7FFFFFFF), ~o).astype(np.uint32)
    ids = (k & np.uint64(0xFFFFFFFF)).astype(np.int64)
    ids[empty] = -1
    depth = bits.view(np.float32).copy()
    depth[empty] = np.inf
    return ids, depth


# ---- shading ------------------------------------------------------------------------------------------------------------------------
def shade(normals, base=COLOR, lights=LIGHTS, ambient=AMBIENT):
    """unit normals [.,3] -> linear-to-display colour in [0, 1], [.,3] float64 (before the 255 scale)."""
    n = np.asarray(normals, np.float64)
    L = np.asarray(lights, np.float64).reshape(-1, 4)
    acc = np.zeros(n.shape[:-1])
    for k in range(len(L)):
        acc += L[k, 3] * np.maximum(0.0, n @ L[k, :3])
    lin = np.asarray(base, np.float64) * (ambient + acc / np.pi)[..., None]
    return np.clip(np.maximum(lin, 0.0) ** (1.0 / 2.2), 0.0, 1.0)


def resolve(meshes, normals, faces, ids, colors=None, lights=LIGHTS, ambient=AMBIENT, background=None):
    """ids [H,W] (slot * F + face, -1 empty); normals: list of [V,3] per slot -> float64 image [H,W,3] in 0..255 (unrounded where
    covered, the background's bytes where empty)."""
    H, W = ids.shape
    F = len(faces)
    out = np.zeros((H, W, 3)) if background is None else np.asarray(background, np.float64).copy()
    for fid in np.unique(ids[ids >= 0]):
        ii, jj = np.nonzero(ids == fid)
        slot, f = int(fid) // F, int(fid) % F
        _, _, w = face_at(meshes[slot][0], meshes[slot][1] * 0.0, faces[f], ii, jj, cull=False)
        n = w @ np.asarray(normals[slot], np.float64)[faces[f]]
        n = n / np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), np.finfo(np.float64).tiny)
        base = COLOR if colors is None else np.asarray(colors, np.float64).reshape(-1, 3)[slot if np.ndim(colors) == 2 else 0]
        out[ii, jj] = 255.0 * shade(n, base, lights, ambient)
    return out


# ---- meshes -------------------------------------------------------------------------------------------------------------------------
def icosphere(subdiv):
    """Unit icosphere, outward (counter-clockwise seen from outside) faces: 12, 42, 162, 642, ... vertices."""
    t = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdiv):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v), np.array(f, np.int64)


def grid_mesh(n, rng, flip_windings=True):
    """(n+1) x (n+1) vertices on the integer lattice, each cell split along a random diagonal, each triangle's winding random (or all
    front facing).  -> (lattice points [V,2] as (column, row) cell corners, faces [2 n^2, 3])."""
    pts = np.array([(x, y) for y in range(n + 1) for x in range(n + 1)], np.float64)
    idx = lambda x, y: y * (n + 1) + x
    faces = []
    for y in range(n):
        for x in range(n):
            a, b, c, d = idx(x, y), idx(x + 1, y), idx(x + 1, y + 1), idx(x, y + 1)
            tris = [(a, c, b), (a, d, c)] if rng.integers(2) else [(a, d, b), (b, d, c)]      # front facing: negative cross, y down
            for t in tris:
                faces.append(t[::-1] if (flip_windings and rng.integers(2)) else t)
    return pts, np.array(faces, np.int64)


def verts_at_pixels(px, py, W, H, z=0.0, cam=(1.0, 1.0, 0.0, 0.0)):
    """Model-space vertices that the camera maps onto the given pixel positions (float64; exact for dyadic positions and sizes)."""
    sx, sy, tx, ty = cam
    x = (2.0 * np.asarray(px, np.float64) / W - 1.0) / sx - tx
    y = (2.0 * np.asarray(py, np.float64) / H - 1.0) / sy - ty
    return np.stack([x, y, np.broadcast_to(np.asarray(z, np.float64), x.shape)], -1)
