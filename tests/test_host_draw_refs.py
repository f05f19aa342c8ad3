"""The 2D overlay's numpy reference (tests/draw_refs.py) checked on the CPU against closed forms, rainbow_colors against matplotlib's
recorded colours (tests/golden/vis_colors.npz, tools/gen_golden_vis.py), and the C ABI's declarations."""
import os
import re

import numpy as np
import pytest

from tests import draw_refs as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('L', [1, 2, 16, 19])
def test_rainbow_colors_equal_matplotlibs(L, golden_dir):
    from gator_amd import vis
    want = np.load(os.path.join(golden_dir, 'vis_colors.npz'))['L%d' % L]
    got = vis.rainbow_colors(L)
    assert got.shape == (L, 3) and got.dtype == np.float64
    np.testing.assert_array_equal(got, want)


def test_horizontal_thickness_2_line_covers_the_rows_the_formula_says():
    """h = 1: cov = clamp(1.5 - d), so the line's own row is fully covered, the rows one above and below half (q = floor(127.5 + 0.5) =
    128), the rows at distance 2 not at all; beyond the end points the cap falls off with the distance to the end point."""
    q = dr.coverage_q(dr.capsule((3, 5), (12, 5), 2, (0, 0, 0)), 11, 17)
    assert (q[5, 3:13] == 255).all() and (q[4, 3:13] == 128).all() and (q[6, 3:13] == 128).all()
    assert (q[:4] == 0).all() and (q[7:] == 0).all()
    assert q[5, 2] == 128 and q[5, 1] == 0 and q[5, 13] == 128 and q[5, 14] == 0          # d = 1 and d = 2 from an end point
    assert q[4, 2] == int(np.floor(255 * (1.5 - np.sqrt(2.0)) + 0.5)) == 22                # the cap's corner, d = sqrt(2)
    thin = dr.coverage_q(dr.capsule((3, 5), (12, 5), 1, (0, 0, 0)), 11, 17)                # thickness 1: cov = clamp(1 - d), one row
    assert (thin[5, 3:13] == 255).all() and thin.sum() == 255 * 10


def test_disc_coverage_has_the_8_lattice_symmetries():
    q = dr.coverage_q(dr.disc((6, 6), 3, (0, 0, 0)), 13, 13)
    for s in (q[::-1], q[:, ::-1], q.T, q[::-1, ::-1], q.T[::-1], q.T[:, ::-1], q.T[::-1, ::-1]):
        np.testing.assert_array_equal(q, s)
    assert q[6, 6] == 255 and q[6, 8] == 255 and q[6, 9] == 128 and q[6, 10] == 0          # cov = 3.5 - d at d = 0, 2, 3, 4
    assert q[7, 9] == int(np.floor(255 * (3.5 - np.sqrt(10.0)) + 0.5)) == 86 and q[8, 9] == 0          # d = sqrt(10), sqrt(13)
    r = dr.coverage_q(dr.ring((6, 6), 2, 3, (0, 0, 0)), 13, 13)
    np.testing.assert_array_equal(r, r.T[::-1])
    assert r[6, 6] == 0 and r[6, 8] == 255 and r[6, 10] == 0                               # |d - 2| = 2, 0, 2 against t/2 + 0.5 = 2


@pytest.mark.parametrize('t', [1, 2, 3, 6])
def test_zero_length_capsule_is_the_disc_of_half_its_thickness(t):
    cap = dr.coverage(dr.capsule((4, 7), (4, 7), t, (0, 0, 0)), 15, 11)
    yy, xx = np.mgrid[:15, :11]
    want = np.clip((t / 2 + 0.5) - np.sqrt(((xx - 4) ** 2 + (yy - 7) ** 2).astype(np.float64)), 0, 1)
    np.testing.assert_array_equal(cap, want)
    if t % 2 == 0:
        np.testing.assert_array_equal(dr.quantise(cap), dr.coverage_q(dr.disc((4, 7), t // 2, (0, 0, 0)), 15, 11))


def test_q_is_monotone_in_distance():
    """Along a ray from a disc's centre, from a capsule's axis and from a ring's circle outwards, q never grows."""
    q = dr.coverage_q(dr.disc((0, 0), 3, (0, 0, 0)), 1, 8)[0]
    assert (np.diff(q) <= 0).all() and q[0] == 255 and q[-1] == 0
    yy, xx = np.mgrid[:40, :40]
    for a, b in (((5, 5), (30, 17)), ((20, 3), (7, 33)), ((8, 8), (31, 31))):
        prim = dr.capsule(a, b, 2, (0, 0, 0))
        q = dr.coverage_q(prim, 40, 40).ravel()
        ab = np.array(b, np.float64) - a
        ap = np.stack([xx.ravel() - a[0], yy.ravel() - a[1]], 1).astype(np.float64)
        tt = np.clip(ap @ ab / (ab @ ab), 0, 1)
        d = np.linalg.norm(ap - tt[:, None] * ab, axis=1)
        order = np.argsort(d, kind='stable')
        sep = np.diff(d[order]) > 1e-9              # only pairs whose distances really differ
        assert (np.diff(q[order])[sep] <= 0).all()
        assert (q[d <= 0.5] == 255).all() and (q[d >= 1.5 + 1e-9] == 0).all()
    q = dr.coverage_q(dr.ring((0, 0), 2, 3, (0, 0, 0)), 1, 8)[0]
    assert (np.diff(q[2:]) <= 0).all() and (np.diff(q[:3]) >= 0).all()


def test_blend_and_alpha_end_points():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (9, 14, 3), dtype=np.uint8)
    prims = [dr.capsule((1, 1), (12, 7), 2, (10, 200, 255)), dr.disc((5, 4), 3, (255, 0, 0))]
    canvas = dr.draw_prims(img, prims, 1.0)
    assert (canvas != img).any()
    np.testing.assert_array_equal(dr.draw_prims(img, prims, 0.0), img)
    np.testing.assert_array_equal(dr.mix(img, canvas.astype(np.int64), 1.0), canvas)
    for a in np.linspace(0, 1, 41):                 # a canvas equal to the image stays the image: untouched tiles may be copied
        np.testing.assert_array_equal(dr.mix(img, img.astype(np.int64), a), img)
    full = np.full((2, 2), 255)
    assert (dr.blend(np.zeros((2, 2, 3), np.int64), full, (7, 8, 9)) == (7, 8, 9)).all()    # q = 255 replaces, q = 0 keeps
    keep = img.astype(np.int64)
    np.testing.assert_array_equal(dr.blend(keep.copy(), np.zeros((9, 14), np.int64), (1, 2, 3)), keep)
    half = dr.mix(np.full((1, 1, 3), 1, np.uint8), np.full((1, 1, 3), 2, np.int64), 0.5)    # 1.5 rounds to even
    assert (half == 2).all()
    assert dr.to_c8((0.5, 1.5, 300.0)) == (0, 2, 255) and dr.to_c8((-3.0, np.nan, 254.5)) == (0, 0, 254)


def test_person_prims_follow_the_reference_order_and_skips():
    sk = ((0, 1), (1, 2))
    col = np.array([(1, 2, 3), (4, 5, 6)], np.float32)
    j = np.array([(1.9, 2.9, 1.0), (-3.9, 4.2, 0.3), (7, 8, 0.5)], np.float32)
    kinds = lambda ps: [(p['kind'], p['a']) for p in ps]      # noqa: E731
    assert kinds(dr.person_prims(j, sk, col)) == [('disc', (1, 2)), ('disc', (7, 8))]      # joint 1 is below 0.4: both lines go, and its marks
    allp = dr.person_prims(j[:, :2], sk, col)
    assert kinds(allp) == [('capsule', (1, 2)), ('disc', (1, 2)), ('disc', (-3, 4)), ('capsule', (-3, 4)), ('disc', (-3, 4)), ('disc', (7, 8))]
    assert allp[0]['c8'] == (1, 2, 3) and allp[3]['c8'] == (4, 5, 6)
    j[0, 0] = np.inf
    assert kinds(dr.person_prims(j[:, :2], sk, col)) == [('disc', (-3, 4)), ('capsule', (-3, 4)), ('disc', (-3, 4)), ('disc', (7, 8))]
    box = np.array([(0, 0), (5, 0), (5, 5), (np.nan, 5)], np.float32)
    boxed = dr.person_prims(j[:, :2], sk, col, bbox=box, style=dr.COCO)
    assert [(p['kind'], p['a'], p.get('b')) for p in boxed[:2]] == [('capsule', (0, 0), (5, 0)), ('capsule', (5, 0), (5, 5))]
    assert boxed[0]['c8'] == (255, 255, 0) and boxed[0]['t'] == 1 and boxed[2]['kind'] == 'ring'
    far, ok = dr.to_pixel(np.array([3e9, -2.0 ** 20 - 5, 2.0 ** 20 - 0.5], np.float32))
    assert far.tolist() == [2 ** 20, -2 ** 20, 2 ** 20 - 1] and ok.all()      # (2^20 - 0.5 is a float32)


def test_draw2d_symbols_are_declared_and_listed():
    from gator_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'gator_hip.h')).read()
    for n, nargs in (('gator_draw2d_create', 4), ('gator_draw2d_destroy', 1), ('gator_draw2d_u8', 3), ('gator_draw2d_workspace', 3),
                     ('gator_draw2d_set_tile_rows', 2)):
        m = re.search(r'\bint %s\(([^;]*)\);' % n, header)
        assert m, n
        assert n in _lib.SIGNATURES, n
        assert len(_lib.SIGNATURES[n][1]) == m.group(1).count(',') + 1 == nargs, n
    fields = re.search(r'typedef struct \{([^}]*)\} gator_draw2d_args;', header).group(1)
    fields = re.sub(r'/\*.*?\*/', '', fields, flags=re.S)
    names = [w.strip(' *') for decl in fields.split(';') if decl.strip() for w in decl.strip().split(None, 1)[1].replace('float', '').replace('uint8_t', '').replace('int32_t', '').replace('const', '').split(',')]
    assert names == [f[0] for f in _lib.Draw2dArgs._fields_]
    assert 'GATOR_DRAW_KEYPOINTS 0' in header and 'GATOR_DRAW_COCO 1' in header and (_lib.DRAW_KEYPOINTS, _lib.DRAW_COCO) == (0, 1)
