"""The renderer's numpy references (tests/render_refs.py) checked on the CPU against closed forms, and the C ABI's declarations."""
import os
import re

import numpy as np

from tests import render_refs as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fixed(px, py):
    return np.stack([np.rint(np.asarray(px, np.float64) * 256), np.rint(np.asarray(py, np.float64) * 256)], -1).astype(np.int64)


def test_shared_edges_through_pixel_centres_are_covered_exactly_once():
    """The 9x9 grid: every vertex on a pixel centre, random diagonals and windings, culling off -- each pixel centre inside the grid
    lies on a vertex, an edge or a diagonal of two to eight faces, and exactly one of them owns it."""
    rng = np.random.default_rng(5)
    for trial in range(4):
        pts, faces = rr.grid_mesh(8, rng)
        xy = _fixed(pts[:, 0] + 1.5, pts[:, 1] + 2.5)          # lattice point k sits on the centre of pixel (k + 1, k + 2)
        r = rr.rasterise([(xy, np.zeros(len(xy)))], faces, 13, 12, cull=False)
        want = np.zeros((13, 12), np.int64)
        want[2:10, 1:9] = 1                                    # centres 1.5 .. 8.5 of the half-open square [1.5, 9.5) x [2.5, 10.5)
        np.testing.assert_array_equal(r['count'], want)


def test_vertex_fan_centred_on_a_pixel_centre_is_covered_exactly_once():
    n = 7
    ang = np.arange(n) * 2 * np.pi / n + 0.3
    px = np.concatenate([[4.5], 4.5 + 3.2 * np.cos(ang)])
    py = np.concatenate([[4.5], 4.5 + 3.2 * np.sin(ang)])
    faces = np.array([(0, 1 + (k + 1) % n, 1 + k) for k in range(n)], np.int64)      # y down: this order has a negative cross product
    r = rr.rasterise([(_fixed(px, py), np.zeros(n + 1))], faces, 9, 9, cull=True)
    assert r['count'][4, 4] == 1
    assert r['count'].max() == 1 and r['count'].sum() >= 20


def test_axis_aligned_right_triangle_has_its_closed_form_pixel_count():
    """a = (0.5, 0.5), b = (0.5, 0.5 + n), c = (0.5 + n, 0.5 + n): every edge runs through pixel centres.  Oriented with E > 0 inside
    the triangle runs a -> c -> b: the hypotenuse goes down (d.y > 0, not owned), the bottom edge goes left (d.y == 0, d.x < 0, not
    owned), the left edge goes up (d.y < 0, owned).  Pixel (i, j) is therefore covered iff 0 <= j < i < n: n (n - 1) / 2 pixels."""
    for n in (1, 2, 5, 16):
        px, py = np.array([0.5, 0.5, 0.5 + n]), np.array([0.5, 0.5 + n, 0.5 + n])
        for faces in ([[0, 1, 2]], [[0, 2, 1]]):
            r = rr.rasterise([(_fixed(px, py), np.zeros(3))], np.array(faces), n + 2, n + 2, cull=False)
            assert r['count'].sum() == n * (n - 1) // 2
            ii, jj = np.nonzero(r['count'])
            assert (jj < ii).all() and (ii < n).all()


def test_zero_area_and_culled_faces_draw_nothing():
    px, py = np.array([1.0, 5.0, 9.0, 1.0]), np.array([1.0, 5.0, 9.0, 9.0])
    xy = _fixed(px, py)
    assert rr.rasterise([(xy, np.zeros(4))], np.array([[0, 1, 2]]), 10, 10, cull=False)['count'].sum() == 0      # collinear
    assert rr.rasterise([(xy, np.zeros(4))], np.array([[0, 0, 3]]), 10, 10, cull=False)['count'].sum() == 0      # repeated vertex
    front, back = np.array([[0, 3, 2]]), np.array([[0, 2, 3]])
    assert rr.rasterise([(xy, np.zeros(4))], front, 10, 10, cull=True)['count'].sum() > 0
    assert rr.rasterise([(xy, np.zeros(4))], back, 10, 10, cull=True)['count'].sum() == 0
    np.testing.assert_array_equal(rr.rasterise([(xy, np.zeros(4))], back, 10, 10, cull=False)['count'],
                                  rr.rasterise([(xy, np.zeros(4))], front, 10, 10, cull=True)['count'])


def test_depth_order_of_two_parallel_quads():
    px, py = np.array([1.0, 7.0, 7.0, 1.0] * 2), np.array([1.0, 1.0, 7.0, 7.0] * 2)
    z = np.array([0.5] * 4 + [-0.25] * 4)
    faces = np.array([[0, 2, 1], [0, 3, 2], [4, 6, 5], [4, 7, 6]])
    r = rr.rasterise([(_fixed(px, py), z)], faces, 8, 8)
    cov = r['count'] > 0
    assert cov.sum() == 36 and (r['count'][cov] == 2).all()
    assert (r['zmin'][cov] == -0.25).all() and np.isin(r['winner'][cov], (2, 3)).all()
    # coplanar duplicates: the smaller id wins; beyond the clip planes: nothing
    r = rr.rasterise([(_fixed(px, py), np.full(8, 0.5))], faces, 8, 8)
    assert np.isin(r['winner'][cov], (0, 1)).all()
    assert rr.rasterise([(_fixed(px, py), np.full(8, 1.0))], faces, 8, 8)['count'].sum() == 72
    assert rr.rasterise([(_fixed(px, py), np.full(8, np.nextafter(1.0, 2.0)))], faces, 8, 8)['count'].sum() == 0


def test_icosphere_normals_are_radial():
    for sub, nv in ((0, 12), (1, 42), (3, 642)):
        v, f = rr.icosphere(sub)
        assert len(v) == nv and len(f) == 20 * 4 ** sub
        fn = rr.face_normals(v, f)
        assert ((fn * v[f].mean(1)).sum(1) > 0).all()           # outward winding
        n, ratio = rr.vertex_normals(v, f)
        k = nv if sub <= 1 else 42          # vertices on a symmetry axis of the icosahedron (5-fold: the first 12, 2-fold: the next 30)
        assert np.abs(n[:k] - v[:k]).max() <= 1e-12
        assert np.abs(n - v).max() <= 0.02
        assert (ratio >= 1.0 - 1e-12).all()
    # the radial direction exactly, after subdivision, on the symmetric vertices (the 12 original ones keep five-fold symmetry)
    v, f = rr.icosphere(2)
    n, _ = rr.vertex_normals(v, f)
    assert np.abs(n[:12] - v[:12]).max() <= 1e-12
    # and under a rotation the normals rotate with the mesh
    R = np.array([[0.5, 0.0, np.sqrt(0.75)], [0.0, 1.0, 0.0], [-np.sqrt(0.75), 0.0, 0.5]])
    nr, _ = rr.vertex_normals(v, f, R)
    assert np.abs(nr - rr.apply_rotation(n, R)).max() <= 1e-12


def test_lighting_of_a_face_on_quad_in_closed_form():
    """n = (0, 0, -1) faces the camera: both lights give n . l = sqrt(1/2), lin = base (0.3 + 2 * 1.2 * sqrt(1/2) / pi)."""
    c = rr.shade(np.array([[0.0, 0.0, -1.0]]))[0]
    lin = rr.COLOR * (0.3 + 2.4 * np.sqrt(0.5) / np.pi)
    np.testing.assert_allclose(c, np.minimum(lin, 1.0) ** (1 / 2.2), rtol=0, atol=1e-15)
    # facing away: ambient only
    np.testing.assert_allclose(rr.shade(np.array([[0.0, 0.0, 1.0]]))[0], (rr.COLOR * 0.3) ** (1 / 2.2), rtol=0, atol=1e-15)
    verts = rr.verts_at_pixels([1.0, 7.0, 7.0, 1.0], [1.0, 1.0, 7.0, 7.0], 8, 8)
    faces = np.array([[0, 2, 1], [0, 3, 2]])
    n, _ = rr.vertex_normals(verts, faces)
    np.testing.assert_allclose(n, np.tile([0.0, 0.0, -1.0], (4, 1)), atol=1e-15)
    px, py, z = rr.project(verts, (1.0, 1.0, 0.0, 0.0), 8, 8)
    xy = rr.snap(px, py, verts)
    r = rr.rasterise([(xy, z)], faces, 8, 8)
    img = rr.resolve([(xy, z)], [n], faces, r['winner'])
    cov = r['winner'] >= 0
    assert cov.sum() == 36
    np.testing.assert_allclose(img[cov], np.tile(255.0 * c, (36, 1)), atol=1e-10)
    assert (img[~cov] == 0).all()


def test_projection_snap_and_sentinels():
    verts = np.array([[0.0, 0.0, 0.3], [0.25, -0.5, -0.2], [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [2.0 ** 21 / 32 * 2, 0.0, 0.0]])
    px, py, z = rr.project(verts, (1.0, 2.0, 0.5, 0.25), 64, 32)
    assert px[0] == 48.0 and py[0] == 24.0 and px[1] == 56.0 and py[1] == 8.0
    np.testing.assert_array_equal(z[:2], [0.3, -0.2])
    xy = rr.snap(px, py, verts)
    np.testing.assert_array_equal(xy[:2], [[48 * 256, 24 * 256], [56 * 256, 8 * 256]])
    assert (xy[2:] == rr.SENTINEL).all()
    assert rr.snap(np.array([0.001953125]), np.array([0.005859375]), np.zeros((1, 3))).tolist() == [[0, 2]]      # ties to even


def test_header_and_binding_declare_the_renderer():
    from gator_amd import _lib, kernel_resources
    names = ('gator_renderer_create', 'gator_renderer_destroy', 'gator_render_f32', 'gator_render_vertices_f32', 'gator_render_raster',
             'gator_render_resolve', 'gator_renderer_workspace', 'gator_renderer_set_small_box')
    header = open(os.path.join(ROOT, 'include', 'gator_hip.h')).read()
    for n in names:
        m = re.search(r'\bint %s\(([^;]*)\);' % n, header)
        assert m, n
        assert n in _lib.SIGNATURES, n
        assert len(_lib.SIGNATURES[n][1]) == m.group(1).count(',') + 1, n
    assert 'GATOR_RENDER_CULL_BACKFACES 1' in header
    for k in ('k_render_vertices', 'k_render_raster', 'k_render_resolve'):
        assert k in kernel_resources.HOT
    from gator_amd import build
    assert 'render.hip' in build.SOURCES
