"""The device renderer (gator_amd/render.py, csrc/render.hip) against tests/render_refs.py: each of the three launches alone, the whole
call, the reference's Renderer class, camera.render_fit, and the C ABI's argument checks.  Measured figures are printed (pytest -s)
and recorded in profiles/render.txt."""
import ctypes

import numpy as np
import pytest
import torch

from tests import render_refs as rr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def T(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def renderer(faces, n_verts=None):
    from gator_amd import render
    return render.MeshRenderer(faces, DEV, n_verts=n_verts)


def strip_faces(V):
    return np.array([(k, k + 1, k + 2) if k % 2 == 0 else (k + 1, k, k + 2) for k in range(V - 2)], np.int64)


_ICO = {}


def ico(sub):
    if sub not in _ICO:
        _ICO[sub] = rr.icosphere(sub)
    return _ICO[sub]


# ---- stage 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M', [1, 2, 65])
@pytest.mark.parametrize('V', [3, 63, 64, 65, 642])
def test_stage1_projection_depth_and_normals(V, M):
    from gator_amd import render
    rng = np.random.default_rng(V * 100 + M)
    if V == 642:
        base, faces = ico(3)
        verts = (base[None] * rng.uniform(0.3, 0.9, (M, 1, 1)) + rng.uniform(-0.1, 0.1, (M, 1, 3))).astype(np.float32)
    else:
        faces = strip_faces(V)
        verts = rng.uniform(-1, 1, (M, V, 3)).astype(np.float32)
    cam = np.concatenate([rng.uniform(0.5, 1.5, (M, 2)), rng.uniform(-0.3, 0.3, (M, 2))], 1).astype(np.float32)
    W, H = 97, 65
    R = render.demo_rotation(angle=25.0, axis=[1, 2, 3], rotate=True) if M == 2 else None
    r = renderer(faces, V)
    xy, z, n = (t.cpu().numpy() for t in r.project(T(verts, torch.float32), T(cam, torch.float32), size=(W, H), rot=R))
    Rf = None if R is None else R.astype(np.float32).astype(np.float64)          # the C ABI takes the matrix as float32
    worst_n = 0.0
    for m in range(M):
        px, py, zz = rr.project(verts[m], cam[m], W, H, Rf)
        want = rr.snap(px, py, verts[m])
        assert (want != rr.SENTINEL).all()
        assert np.abs(xy[m] - want).max() <= 1
        p = np.stack([px, py], 1)
        safe = rr.snap_margin(p) > 4 * rr.U32 * np.abs(p * 256)
        assert safe.mean() > 0.5
        np.testing.assert_array_equal(xy[m][safe], want[safe])
        if R is None:
            np.testing.assert_array_equal(z[m].view(np.int32), verts[m, :, 2].view(np.int32))
        else:
            assert np.abs(z[m] - zz).max() <= rr.U32 * np.abs(zz).max()
        nref, ratio = rr.vertex_normals(verts[m], faces, Rf)
        err = np.abs(n[m] - nref).max(1)
        bound = rr.D_NORMAL * rr.U32 * ratio
        assert (err <= bound).all(), (err / bound).max()
        worst_n = max(worst_n, (err / (rr.U32 * ratio)).max())
    print('stage1 V=%d M=%d: normal error / (u sum|n_f| / |sum n_f|) = %.3f (D = %g)' % (V, M, worst_n, rr.D_NORMAL))


def test_stage1_sentinels():
    V, W, H = 65, 64, 64
    rng = np.random.default_rng(1)
    verts = rng.uniform(-1, 1, (2, V, 3)).astype(np.float32)
    cam = np.array([[1, 1, 0, 0], [1, 1, 0, 0]], np.float32)
    verts[0, 3, 1] = np.nan
    verts[0, 10, 0] = np.inf
    verts[1, 0, 2] = -np.inf
    verts[1, 64, 0] = 2.0 ** 21 / (W / 2)          # px = W / 2 + 2^21
    verts[1, 20, 1] = -2.0 ** 21 / (H / 2)
    verts[1, 30, 0] = (2.0 ** 20 - W / 2) / (W / 2)   # px = 2^20 exactly: the last position inside the guard band
    r = renderer(strip_faces(V), V)
    xy, z, n = (t.cpu().numpy() for t in r.project(T(verts, torch.float32), T(cam, torch.float32), size=(W, H)))
    bad = np.zeros((2, V), bool)
    bad[0, 3] = bad[0, 10] = bad[1, 0] = bad[1, 64] = bad[1, 20] = True
    assert (xy[bad] == rr.SENTINEL).all() and (xy[~bad] != rr.SENTINEL).all()
    assert xy[1, 30, 0] == 2 ** 28
    fin = np.isfinite(verts).all(2)
    np.testing.assert_array_equal(z[fin].view(np.int32), verts[..., 2][fin].view(np.int32))
    # a face that touches a sentinel vertex draws nothing, the others still do
    keys = r.rasterise(T(xy, torch.int32), T(z, torch.float32), size=(W, H), cull_backfaces=False).cpu().numpy()
    ids, _ = rr.decode_keys(keys)
    faces = strip_faces(V)
    for m in range(2):
        touched = np.nonzero(bad[m][faces].any(1))[0]
        assert not np.isin(ids[m], touched).any()
        ref = rr.rasterise([(xy[m].astype(np.int64), z[m].astype(np.float64))], faces, H, W, cull=False)
        np.testing.assert_array_equal(ids[m] >= 0, ref['count'] > 0)


# ---- stage 2 ------------------------------------------------------------------------------------------------------------------------
def fixed(px, py):
    return np.stack([np.rint(np.asarray(px, np.float64) * 256), np.rint(np.asarray(py, np.float64) * 256)], -1).astype(np.int64)


def check_raster(xy, z, faces, H, W, cull, exact_winner=False, slots=1, label=None):
    """xy [S,V,2] int, z [S,V] float32: S meshes in ONE image.  Coverage bit-exact; the winner within D_Z of the fp64 minimum."""
    xy, z = np.asarray(xy).reshape(slots, -1, 2), np.asarray(z, np.float32).reshape(slots, -1)
    r = renderer(faces, xy.shape[1])
    keys = r.rasterise(T(xy, torch.int32), T(z, torch.float32), image_index=np.zeros(slots, np.int64), n_images=1, size=(W, H),
                       cull_backfaces=cull).cpu().numpy()
    ids, depth = rr.decode_keys(keys)
    meshes = [(xy[s].astype(np.int64), z[s].astype(np.float64)) for s in range(slots)]
    ref = rr.rasterise(meshes, faces, H, W, cull)
    np.testing.assert_array_equal(ids[0] >= 0, ref['count'] > 0)
    cov = ref['count'] > 0
    ratio = derr = 0.0
    if cov.any():
        d, c = rr.depth_of_ids(meshes, faces, ids[0], cull)
        assert c[cov].all()                                       # the device's face does cover the pixel
        excess = d[cov] - ref['zmin'][cov]
        assert (excess <= rr.D_Z * rr.U32 * ref['zabs'][cov]).all()
        tie = excess == 0                                         # exact ties: the smaller id
        np.testing.assert_array_equal(ids[0][cov][tie], ref['winner'][cov][tie])
        derr = np.abs(depth[0][cov] - d[cov]).max() / (rr.U32 * max(ref['zabs'].max(), 1e-30))      # one face's fp32 depth: half of D_Z
        assert derr <= rr.D_Z / 2
        with np.errstate(all='ignore'):
            q = excess / (rr.U32 * ref['zabs'][cov])
        ratio = float(np.nanmax(np.where(ref['zabs'][cov] > 0, q, 0.0)))
    if exact_winner:
        np.testing.assert_array_equal(ids[0], ref['winner'])
    if label:
        print('%s: %d covered, winner excess / (u max|z|) = %.3f (D_z = %g), depth error / (u max|z|) = %.3f (D_z / 2)'
              % (label, cov.sum(), ratio, rr.D_Z, derr))
    return ids[0], ref


def soup(rng, F, H, W, big=2):
    """F random triangles over (and around) an H x W image, both windings, a few of them large, depths in (-0.9, 0.9)."""
    c = np.stack([rng.uniform(-4, W + 4, F), rng.uniform(-4, H + 4, F)], 1)
    size = np.full(F, 3.0)
    size[rng.choice(F, min(big, F), replace=False)] = max(H, W) * 0.6
    p = c[:, None, :] + rng.uniform(-1, 1, (F, 3, 2)) * size[:, None, None]
    z = rng.uniform(-0.9, 0.9, (F, 3)).astype(np.float32)
    return fixed(p[..., 0].ravel(), p[..., 1].ravel()), z.ravel(), np.arange(3 * F).reshape(F, 3)


@pytest.mark.parametrize('cull', [True, False])
def test_stage2_single_triangle_and_quad_through_pixel_centres(cull):
    for faces in ([[0, 1, 2]], [[0, 2, 1]]):
        check_raster(fixed([0.7, 6.2, 2.9], [0.3, 1.1, 4.8]), np.array([0.1, -0.3, 0.4]), np.array(faces), 5, 7, cull, label='triangle 7x5')
    xy = fixed([0.5, 40.5, 40.5, 0.5], [0.5, 0.5, 40.5, 40.5])
    for faces in ([[0, 2, 1], [0, 3, 2]], [[0, 1, 2], [0, 2, 3]], [[0, 2, 1], [0, 2, 3]]):
        ids, ref = check_raster(xy, np.zeros(4), np.array(faces), 64, 64, cull, exact_winner=True)
        assert ref['count'].max() <= 1


@pytest.mark.parametrize('cull', [True, False])
def test_stage2_grid_with_every_vertex_on_a_pixel_centre(cull):
    rng = np.random.default_rng(9)
    pts, faces = rr.grid_mesh(8, rng, flip_windings=True)
    ids, ref = check_raster(fixed(pts[:, 0] + 3.5, pts[:, 1] + 2.5), np.zeros(len(pts)), faces, 63, 65, cull, exact_winner=True)
    if not cull:
        want = np.zeros((63, 65), bool)
        want[2:10, 3:11] = True
        np.testing.assert_array_equal(ids >= 0, want)
        assert ref['count'].max() == 1


@pytest.mark.parametrize('cull', [True, False])
def test_stage2_slivers_zero_area_and_off_screen(cull):
    rng = np.random.default_rng(2)
    # slivers thinner than a pixel, every direction
    F = 40
    a = rng.uniform(5, 59, (F, 2))
    ang = rng.uniform(0, 2 * np.pi, F)
    b = a + 30 * np.stack([np.cos(ang), np.sin(ang)], 1)
    c = a + 15 * np.stack([np.cos(ang), np.sin(ang)], 1) + rng.uniform(-0.3, 0.3, (F, 1)) * np.stack([-np.sin(ang), np.cos(ang)], 1)
    p = np.stack([a, b, c], 1).reshape(-1, 2)
    z = rng.uniform(-0.5, 0.5, 3 * F)
    check_raster(fixed(p[:, 0], p[:, 1]), z, np.arange(3 * F).reshape(F, 3), 64, 64, cull, label='slivers 64x64')
    # zero area: collinear, repeated vertices, a point -- among two real triangles
    xy = fixed([1, 5, 9, 1, 9, 3.5, 3.5], [1, 5, 9, 9, 1, 3.5, 3.5])
    faces = np.array([[0, 1, 2], [0, 0, 3], [5, 5, 5], [5, 6, 5], [0, 3, 2], [0, 2, 4], [1, 1, 1]])
    ids, _ = check_raster(xy, np.linspace(-0.5, 0.5, 7), faces, 10, 10, cull)
    assert not np.isin(ids, (0, 1, 2, 3, 6)).any()
    # fully and partly off every side, small and large, and the degenerate image sizes
    for (H, W) in ((63, 65), (1, 1), (1, 129), (5, 7)):
        xyf, zf, faces = soup(rng, 48, H, W, big=6)
        far = fixed(np.array([-50, -40, -45, W + 40, W + 50, W + 45]), np.array([-50, H + 60, 2, -30, H + 3, H + 90]))
        check_raster(np.concatenate([xyf, far]), np.concatenate([zf, np.zeros(6, np.float32)]),
                     np.concatenate([faces, [[144, 145, 146], [147, 148, 149]]]), H, W, cull, label='soup %dx%d' % (W, H))


@pytest.mark.parametrize('F', [63, 64, 65, 255, 256, 257])
def test_stage2_face_counts_either_side_of_the_wave_and_block_sizes(F):
    rng = np.random.default_rng(F)
    xy, z, faces = soup(rng, F, 64, 64)
    for cull in (True, False):
        check_raster(xy, z, faces, 64, 64, cull, label='soup F=%d cull=%d' % (F, cull))


@pytest.mark.parametrize('cull', [True, False])
def test_stage2_full_cover_triangle_and_the_long_strip(cull):
    xy = fixed([-700, 1500, -700], [-700, -700, 1500])
    for faces in ([[0, 2, 1]], [[0, 1, 2]]):
        ids, ref = check_raster(xy, np.array([0.2, -0.4, 0.6]), np.array(faces), 300, 300, cull)
        front = faces == [[0, 2, 1]]
        assert (ids >= 0).all() if (front or not cull) else (ids < 0).all()
    xy = fixed([-3, 2060, 1000], [-2, -1, 4])
    check_raster(xy, np.array([0.5, -0.5, 0.0]), np.array([[0, 1, 2], [0, 2, 1]]), 1, 2049, cull, label='strip 2049x1')


def test_stage2_depth_ties_ulps_and_clip_planes():
    quad = lambda x0: ([x0, x0 + 6, x0 + 6, x0], [1, 1, 7, 7])
    f = lambda k: [[4 * k, 4 * k + 2, 4 * k + 1], [4 * k, 4 * k + 3, 4 * k + 2]]
    # coplanar duplicates: the smaller id; one fp32 ulp apart: the nearer one, whatever its id
    px, py = quad(1)
    half, below = np.float32(0.5), np.nextafter(np.float32(0.5), np.float32(0))
    for zs, win in (([half, half, half], (0, 1)), ([half, below, half], (2, 3)), ([below, half, half], (0, 1)), ([half, half, below], (4, 5))):
        xy = fixed(px * 3, py * 3)
        z = np.repeat(np.array(zs, np.float32), 4)
        ids, ref = check_raster(xy, z, np.array(f(0) + f(1) + f(2)), 8, 8, True, exact_winner=True)
        assert np.isin(ids[ids >= 0], win).all() and (ids >= 0).sum() == 36
    # the clip planes: +-1 is drawn, one ulp beyond is not
    one = np.float32(1)
    zs = [one, -one, np.nextafter(one, np.float32(2)), np.nextafter(-one, np.float32(-2))]
    px = np.concatenate([quad(1 + 8 * k)[0] for k in range(4)])
    py = np.concatenate([quad(0)[1]] * 4)
    ids, ref = check_raster(fixed(px, py), np.repeat(np.array(zs, np.float32), 4), np.array(f(0) + f(1) + f(2) + f(3)), 8, 32, True, exact_winner=True)
    assert (ids[1:7, 1:7] >= 0).all() and (ids[1:7, 9:15] >= 0).all() and (ids[:, 16:] < 0).all()


def two_spheres(W, H, M=2, seed=0):
    base, faces = ico(3)
    rng = np.random.default_rng(seed)
    verts = np.stack([base * 0.55 + [-0.2, 0.05, 0.0], base * 0.5 + [0.25, -0.1, 0.1]] +
                     [base * rng.uniform(0.3, 0.7) + rng.uniform(-0.3, 0.3, 3) * [1, 1, 0.3] for _ in range(M - 2)]).astype(np.float32)
    cam = np.tile(np.array([[0.9, 0.9 * W / H, 0.05, -0.02]], np.float32), (M, 1))
    return verts[:M], cam[:M], faces


def test_stage2_interpenetrating_icospheres_share_one_depth_buffer():
    W, H = 64, 48
    verts, cam, faces = two_spheres(W, H)
    r = renderer(faces)
    xy, z, _ = r.project(T(verts, torch.float32), T(cam, torch.float32), size=(W, H))
    for cull in (True, False):
        check_raster(xy.cpu().numpy(), z.cpu().numpy(), faces, H, W, cull, slots=2, label='two icospheres cull=%d' % cull)


# ---- stage 3 and the whole call -----------------------------------------------------------------------------------------------------
def reference_image(verts, cam, faces, W, H, background=None, colors=None, R=None):
    """All meshes into ONE image -> (winner ids [H,W], float64 image [H,W,3])."""
    meshes, normals = [], []
    for m in range(len(verts)):
        px, py, z = rr.project(verts[m], cam[m], W, H, R)
        meshes.append((rr.snap(px, py, verts[m]), z))
        normals.append(rr.vertex_normals(verts[m], faces, R)[0])
    ref = rr.rasterise(meshes, faces, H, W)
    return ref, rr.resolve(meshes, normals, faces, ref['winner'], colors=colors, background=background)


def test_stage3_colours_background_and_optional_outputs():
    from gator_amd import render
    W, H = 64, 48
    verts, cam, faces = two_spheres(W, H)
    rng = np.random.default_rng(3)
    bg = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    colors = np.array([[1.0, 1.0, 0.9], [0.2, 0.6, 1.0]], np.float32)
    R = render.demo_rotation(rotate=True)
    r = renderer(faces)
    for rot in (None, R):
        xy, z, n = r.project(T(verts, torch.float32), T(cam, torch.float32), size=(W, H), rot=rot)
        keys = r.rasterise(xy, z, image_index=[0, 0], n_images=1, size=(W, H))
        rgb, fid, dep = (t.cpu().numpy()[0] for t in r.resolve(keys, xy, n, background=T(bg, torch.uint8), color=T(colors, torch.float32),
                                                               image_index=[0, 0], return_face_id=True, return_depth=True))
        ids, kd = rr.decode_keys(keys.cpu().numpy())
        np.testing.assert_array_equal(fid, ids[0])
        np.testing.assert_array_equal(dep, kd[0])
        assert (np.isinf(dep) == (fid < 0)).all() and (np.abs(dep[fid >= 0]) <= 1).all()
        Rf = None if rot is None else rot.astype(np.float32).astype(np.float64)
        ref, img = reference_image(verts, cam, faces, W, H, background=bg[0], colors=colors, R=Rf)
        np.testing.assert_array_equal(fid >= 0, ref['winner'] >= 0)
        np.testing.assert_array_equal(rgb[fid < 0], bg[0][fid < 0])
        same = (fid == ref['winner']) & (fid >= 0)
        assert same.sum() >= 0.98 * (fid >= 0).sum()
        diff = np.abs(rgb[same].astype(np.int64) - np.rint(img[same]).astype(np.int64))
        assert diff.max() <= 1
        print('stage3 rot=%s: %d covered, %d with the reference face, %.4f of their bytes equal, none off by more than 1'
              % (rot is not None, (fid >= 0).sum(), same.sum(), (diff == 0).mean()))


def test_render_equals_its_three_stages_and_repeats_bit_for_bit():
    W, H = 65, 63
    verts, cam, faces = two_spheres(W, H, M=4, seed=4)
    idx = [0, 0, 1, 2]
    bg = T(np.random.default_rng(0).integers(0, 256, (3, H, W, 3), dtype=np.uint8), torch.uint8)
    r = renderer(faces)
    v, c = T(verts, torch.float32), T(cam, torch.float32)
    for cull in (True, False):
        a = r.render(v, c, background=bg, image_index=idx, size=(W, H), return_face_id=True, return_depth=True, cull_backfaces=cull)
        b = r.render(v, c, background=bg, image_index=idx, size=(W, H), return_face_id=True, return_depth=True, cull_backfaces=cull)
        xy, z, n = r.project(v, c, size=(W, H))
        keys = r.rasterise(xy, z, image_index=idx, n_images=3, size=(W, H), cull_backfaces=cull)
        s = r.resolve(keys, xy, n, background=bg, image_index=idx, return_face_id=True, return_depth=True)
        for x, y, w in zip(a, b, s):
            assert torch.equal(x, y) and torch.equal(x, w)
        assert (a[1] >= 0).any() and (a[1] < 0).any()


def test_an_image_does_not_depend_on_its_batch():
    W, H = 64, 64
    verts, cam, faces = two_spheres(W, H, M=65, seed=6)
    r = renderer(faces)
    v, c = T(verts, torch.float32), T(cam, torch.float32)
    full = r.render(v, c, size=(W, H), return_face_id=True, return_depth=True)
    three = r.render(v[:3], c[:3], size=(W, H), return_face_id=True, return_depth=True)
    for m in (0, 2, 64):
        alone = r.render(v[m:m + 1], c[m:m + 1], size=(W, H), return_face_id=True, return_depth=True)
        for k in range(3):
            assert torch.equal(alone[k][0], full[k][m])
            if m < 3:
                assert torch.equal(alone[k][0], three[k][m])
    assert len({bytes(full[0][m].cpu().numpy().tobytes()) for m in range(65)}) > 60


def test_two_people_in_one_frame_share_the_depth_buffer():
    W, H = 64, 48
    verts, cam, faces = two_spheres(W, H)
    r = renderer(faces)
    rgb, fid = r.render(T(verts, torch.float32), T(cam, torch.float32), image_index=[0, 0], n_images=1, size=(W, H), return_face_id=True)
    rgb, fid = rgb.cpu().numpy()[0], fid.cpu().numpy()[0]
    ref, img = reference_image(verts, cam, faces, W, H)
    np.testing.assert_array_equal(fid >= 0, ref['winner'] >= 0)
    F = len(faces)
    assert (fid[fid >= 0] < F).any() and (fid[fid >= 0] >= F).any()          # both meshes are visible
    same = fid == ref['winner']
    assert same.mean() >= 0.98
    assert np.abs(rgb[same].astype(np.int64) - np.rint(img[same]).astype(np.int64)).max() <= 1
    # the other order of the same two meshes: the same picture (the ids swap slots)
    rgb2 = r.render(T(verts[::-1].copy(), torch.float32), T(cam[::-1].copy(), torch.float32), image_index=[0, 0], n_images=1, size=(W, H)).cpu().numpy()[0]
    assert (rgb2 == rgb).mean() > 0.999


def test_renderer_mirror_composites_as_the_reference_does(tmp_path):
    from gator_amd import render
    W, H = 48, 40
    verts, cam, faces = two_spheres(W, H)
    img = np.random.default_rng(8).uniform(0, 255.99, (H, W, 3))                   # float64 background: the reference truncates it
    R = render.Renderer(faces, resolution=(W, H), orig_img=True)
    for kw in ({}, {'rotate': True}, {'angle': 30, 'axis': [0, 1, 0], 'color': (0.3, 0.8, 0.5)}):
        out = R.render(img, verts[0], cam[0], **kw)
        assert out.dtype == np.uint8 and out.shape == (H, W, 3)
        rgb, fid = R.renderer.render(T(verts[:1], torch.float32), T(cam[:1], torch.float32), color=kw.get('color', (1.0, 1.0, 0.9)), size=(W, H),
                                     return_face_id=True, rot=render.demo_rotation(kw.get('angle'), kw.get('axis'), kw.get('rotate', False)))
        mask = (fid[0].cpu().numpy() >= 0)[:, :, None]
        np.testing.assert_array_equal(out, (rgb[0].cpu().numpy() * mask + (1 - mask) * img).astype(np.uint8))
        assert mask.any() and not mask.all()
        assert (out[~mask[..., 0]] == np.floor(img[~mask[..., 0]])).all()
    with pytest.raises(NotImplementedError):
        render.Renderer(faces, wireframe=True)
    path = tmp_path / 'mesh.obj'
    R.render(img, verts[0], cam[0], mesh_filename=str(path))
    lines = path.read_text().splitlines()
    assert sum(ln.startswith('v ') for ln in lines) == len(verts[0]) and sum(ln.startswith('f ') for ln in lines) == len(faces)
    x, y, z = (float(t) for t in lines[0].split()[1:])
    assert abs(x - verts[0, 0, 0]) < 1e-6 and abs(y + verts[0, 0, 1]) < 1e-6 and abs(z + verts[0, 0, 2]) < 1e-6


def test_render_fit_takes_the_fit_dict_to_images():
    from gator_amd import camera, render
    W, H = 80, 60
    verts, cam, faces = two_spheres(W, H, M=3, seed=2)
    fit = {'mesh': T(verts, torch.float32), 'orig_cam': T(cam, torch.float32)}
    out = camera.render_fit(fit, faces, image_size=(W, H))
    assert out.shape == (3, H, W, 3) and out.dtype == torch.uint8 and out.is_cuda
    r = renderer(faces)
    assert torch.equal(out, r.render(fit['mesh'], fit['orig_cam'], size=(W, H)))
    bg = T(np.random.default_rng(1).integers(0, 256, (3, H, W, 3), dtype=np.uint8), torch.uint8)
    col = T(np.array([[1, 0.5, 0.5], [0.5, 1, 0.5], [0.5, 0.5, 1]]), torch.float32)
    out = camera.render_fit(fit, r, images=bg, colors=col)
    assert torch.equal(out, r.render(fit['mesh'], fit['orig_cam'], background=bg, color=col, size=(W, H)))
    with pytest.raises(ValueError):
        camera.render_fit(fit, r)


def test_workspace_stops_growing_after_the_largest_call():
    verts, cam, faces = two_spheres(64, 64, M=8, seed=5)
    r = renderer(faces)
    v, c = T(verts, torch.float32), T(cam, torch.float32)
    assert r.workspace() == (0, 0)
    r.render(v[:2], c[:2], size=(32, 32))
    small = r.workspace()
    r.render(v, c, size=(129, 65), image_index=[0, 0, 1, 1, 2, 3, 4, 5], n_images=8)
    top = r.workspace()
    assert top[0] > small[0] and top[1] > small[1]
    for M, size, idx in ((1, (16, 16), None), (8, (64, 64), None), (3, (129, 65), [2, 2, 0]), (8, (129, 65), [7, 6, 5, 4, 3, 2, 1, 0]), (5, (1, 1), None)):
        r.render(v[:M], c[:M], size=size, image_index=idx, n_images=None if idx is None else 8)
        assert r.workspace() == top


# ---- argument checks ----------------------------------------------------------------------------------------------------------------
def test_argument_checks_return_einval_with_a_reason_and_launch_nothing():
    from gator_amd import _lib
    lib = _lib.load()
    EINVAL = -1
    h = ctypes.c_void_p()

    def create(faces, nf, nv):
        f = np.ascontiguousarray(faces, np.int32)
        rc = lib.gator_renderer_create(f.ctypes.data_as(ctypes.c_void_p), nf, nv, ctypes.byref(h))
        return rc, lib.gator_last_error().decode()

    for faces, nf, nv, why in (([[0, 1, 3]], 1, 3, 'vertex index 3'), ([[0, -1, 2]], 1, 3, 'vertex index -1'), ([[0, 1, 2]], 0, 3, 'n_faces'),
                               ([[0, 1, 1]], 1, 2, 'n_verts')):
        rc, msg = create(faces, nf, nv)
        assert rc != 0 and why in msg and not h.value, (rc, msg)
    from gator_amd import render
    r = render.MeshRenderer(np.array([[0, 1, 2]]), DEV)
    verts = T(np.array([[[-1, -1, 0], [1, -1, 0], [0, 1, 0]]] * 2, np.float32), torch.float32)
    cam = T(np.array([[1, 1, 0, 0]] * 2, np.float32), torch.float32)
    lights = np.ascontiguousarray(render.DEMO_LIGHTS, np.float32)
    rgb = torch.full((2, 8, 8, 3), 7, dtype=torch.uint8, device=DEV)
    fid = torch.full((2, 8, 8), 7, dtype=torch.int32, device=DEV)

    def call(handle=None, v=verts, M=2, N=2, H=8, W=8, idx=None, lt=lights, nl=2, amb=0.3, out=rgb, rot=None, face_ids=None):
        ix = None if idx is None else np.ascontiguousarray(idx, np.int32)
        ro = None if rot is None else np.ascontiguousarray(rot, np.float32)
        rc = lib.gator_render_f32(r._h if handle is None else handle, v.data_ptr() if v is not None else None, cam.data_ptr(), None,
                                  ix.ctypes.data_as(ctypes.c_void_p) if ix is not None else None, M, None, N, H, W,
                                  ro.ctypes.data_as(ctypes.c_void_p) if ro is not None else None, lt.ctypes.data_as(ctypes.c_void_p), nl, amb, 1,
                                  out.data_ptr() if out is not None else None, face_ids.data_ptr() if face_ids is not None else None, None, None)
        return rc, lib.gator_last_error().decode()

    bad = (({'H': 0}, 'H and W'), ({'W': 8193}, 'H and W'), ({'H': 8193}, 'H and W'), ({'M': 0}, 'n_meshes'), ({'N': 0}, 'n_images'),
           ({'idx': [0, 2]}, 'image_index[1] = 2'), ({'idx': [-1, 0]}, 'image_index[0] = -1'), ({'N': 1}, 'n_meshes 2 > n_images 1'),
           ({'nl': 5}, 'lights'), ({'amb': float('nan')}, 'ambient'), ({'out': None}, 'no output'), ({'v': None}, 'null'),
           ({'rot': [1, 0, 0, 0, float('inf'), 0, 0, 0, 1]}, 'rot3x3'), ({'handle': ctypes.c_void_p()}, 'null handle'))
    for kw, why in bad:
        rc, msg = call(**kw)
        assert rc == EINVAL and why in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert (rgb == 7).all() and (fid == 7).all()              # nothing was launched
    # the id range: (most meshes in one image) * n_faces must stay below 2^32, below 2^31 when face ids go out
    F = 1 << 17
    big = render.MeshRenderer(np.tile(np.array([[0, 1, 2]]), (F, 1)), DEV)
    for M, ids_out, why in ((32768, None, 'below 2^32'), (16384, fid, 'below 2^31')):
        rc, msg = call(handle=big._h, M=M, N=1, idx=np.zeros(M, np.int32), face_ids=ids_out)
        assert rc == EINVAL and 'max_meshes_per_image * n_faces' in msg and why in msg, (rc, msg)
    torch.cuda.synchronize()
    assert (rgb == 7).all() and (fid == 7).all()
    rc, msg = call()
    torch.cuda.synchronize()
    assert rc == 0 and not (rgb == 7).all()
    # the stage entry points check the same things
    with pytest.raises(RuntimeError, match='H and W'):
        r.project(verts, cam, size=(0, 8))
    xy, z, n = r.project(verts, cam, size=(8, 8))
    with pytest.raises(RuntimeError, match=r'image_index\[1\] = 5'):
        r.rasterise(xy, z, image_index=[0, 5], n_images=2, size=(8, 8))
    with pytest.raises(RuntimeError, match='H and W'):
        r.rasterise(xy, z, size=(8, 9000))
    keys = r.rasterise(xy, z, size=(8, 8))
    # the stage methods take only what the kernels index by: this device, these dtypes, the renderer's vertex count
    for bad_xy, bad_z in ((xy.long(), z), (xy[:, :2], z[:, :2]), (xy.cpu(), z), (xy, z.double()), (xy, z[:1])):
        with pytest.raises(ValueError):
            r.rasterise(bad_xy, bad_z, size=(8, 8))
    for bad_keys, bad_xy, bad_n in ((keys.int(), xy, n), (keys, xy, n[:, :2]), (keys, xy.long(), n), (keys.cpu(), xy, n), (keys, xy, n.double())):
        with pytest.raises(ValueError):
            r.resolve(bad_keys, bad_xy, bad_n)
    assert torch.equal(r.resolve(keys.transpose(1, 2).contiguous().transpose(1, 2), xy, n), r.resolve(keys, xy, n))      # a strided view is copied
    with pytest.raises(RuntimeError, match='lights'):
        r.resolve(keys, xy, n, lights=np.ones((5, 4)))
    with pytest.raises(RuntimeError):
        render.MeshRenderer(np.array([[0, 1, 2]]), 'cpu')
