"""The device's 2D pose overlay (gator_amd/vis.py, csrc/draw2d.hip) against tests/draw_refs.py: every output byte equals the numpy
restatement -- no tolerance anywhere in this file.  Frames are small (37 x 29, 1 x 1, 64 x 16, one tile, one tile row): the tile is
64 x 4 pixels in the kernel's one-row form and 64 x 16 in its tall form, so they have edge tiles on both axes.  Every comparison is
made for both forms and for the built-in choice between them; the tile shapes, the LDS list's capacity and the grid size at which
the choice changes are read from the source."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import draw_refs as dr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, 'gator_amd', 'csrc', 'draw2d.hip')).read()
TILE_W, TILE_H = (int(v) for v in re.search(r'kTileW = (\d+), kTileH = (\d+);', SRC).groups())
LIST_CAP = int(re.search(r'kListCap = (\d+);', SRC).group(1))
TALL_ROWS = int(re.search(r'kTallRows = (\d+);', SRC).group(1))
TALL_FROM = int(re.search(r'kTallTileFrom = (\d+);', SRC).group(1))
TALL_H = TILE_H * TALL_ROWS
SIZES = [(37, 29), (1, 1), (64, 16), (TILE_W, TILE_H), (3 * TILE_W + 8, TILE_H), (TILE_W, TALL_H), (TILE_W + 1, TALL_H + 1)]      # (W, H)
STYLE = {'keypoints': dr.KEYPOINTS, 'coco': dr.COCO}

# six limbs on twelve joints in a 37 x 29 frame: slopes 0, infinity, +1, -1, 7/17 and -13/5, some ends off the frame
SLOPES_SK = tuple((2 * k, 2 * k + 1) for k in range(6))
SLOPES_J = np.array([(2.7, 4.2), (33.1, 4.9), (20.5, -3.0), (20.2, 27.9), (3, 3), (25, 25), (30.9, 2.2), (8.1, 25.0),
                     (1.0, 9.0), (35.4, 23.3), (11.0, 27.6), (16.8, 1.4)], np.float32)


def T(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


_DRAWERS = {}


def drawer(skeleton, J):
    from gator_amd import vis
    key = (tuple(map(tuple, skeleton)), J)
    if key not in _DRAWERS:
        _DRAWERS[key] = vis.SkeletonDrawer(skeleton, J, DEV)
    return _DRAWERS[key]


def frames(N, W, H, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (N, H, W, 3), dtype=np.uint8)


def colors(L, seed=1):
    return np.random.default_rng(seed).uniform(0, 255, (L, 3)).astype(np.float32)


def check(images, joints, skeleton, col, bbox=None, image_index=None, kp_thre=0.4, alpha=1.0, style='keypoints'):
    """Draw on the device -- both forms of the tile kernel, then the built-in choice -- and in numpy; every byte equal.  -> the picture."""
    joints = np.asarray(joints, np.float32)
    d = drawer(skeleton, joints.shape[1])
    want = dr.draw(images, joints, skeleton, col, bbox, image_index, kp_thre, alpha, STYLE[style])
    for rows in (1, TALL_ROWS, 0):
        d.set_tile_rows(rows)
        got = d.draw(T(images, torch.uint8), T(joints), colors=T(col), bbox=None if bbox is None else T(bbox), image_index=image_index,
                     kp_thre=kp_thre, alpha=alpha, style=style).cpu().numpy()
        np.testing.assert_array_equal(got, want, err_msg='rows = %d' % rows)
    return got


@pytest.mark.parametrize('style', ['keypoints', 'coco'])
@pytest.mark.parametrize('size', SIZES)
def test_slopes_in_every_frame_size(size, style):
    W, H = size
    img = frames(2, W, H)
    j = np.stack([SLOPES_J, SLOPES_J[::-1] * [1.7, 0.4] + [3, 1], SLOPES_J * 0 + [0.5, 0.2]]).astype(np.float32)      # the third: all on pixel (0, 0)
    out = check(img, j, SLOPES_SK, colors(6), image_index=[0, 1, 1], style=style)
    assert (out[0] != img[0]).any() == (W > 1) and (out[1] != img[1]).any()


def test_line_through_a_tile_corner_crosses_four_tiles():
    W, H = 2 * TILE_W + 3, 2 * TALL_H + 1
    for cx, cy in ((TILE_W, TILE_H), (TILE_W, TALL_H)):      # pixels (cx - 1, cy - 1), (cx, cy - 1), (cx - 1, cy), (cx, cy) lie in four tiles
        j = np.array([[(cx - 4, cy - 4), (cx + 3, cy + 3), (cx + 3, cy - 4), (cx - 4, cy + 3)]], np.float32)
        img = frames(1, W, H)
        out = check(img, j, ((0, 1), (2, 3)), colors(2))
        for x, y in ((cx - 1, cy - 1), (cx, cy - 1), (cx - 1, cy), (cx, cy)):
            assert (out[0, y, x] != img[0, y, x]).any()


def test_primitives_off_the_frame_and_clamped_coordinates():
    W, H = 37, 29
    sk = ((0, 1), (2, 3), (4, 5), (6, 7), (8, 9))
    j = np.array([[(-50, -50), (-20, -30),                      # wholly outside
                   (-10, 5), (20, 40),                          # partly outside
                   (-3e9, 10), (3e9, 12),                       # far beyond 2^20 on both sides: clamped, still crosses the frame
                   (2.0 ** 20, 2.0 ** 20), (5, 6),              # at the clamp
                   (-2.0 ** 20 - 3, 20), (30, -2.0 ** 20)]], np.float32)
    img = frames(1, W, H)
    out = check(img, j, sk, colors(5))
    assert (out[0, 10:13] != img[0, 10:13]).any()
    only_outside = check(img, j, ((0, 1),), colors(1))
    np.testing.assert_array_equal(only_outside, img)


@pytest.mark.parametrize('style', ['keypoints', 'coco'])
def test_zero_length_limbs(style):
    j = np.array([[(5.2, 7.9), (5.7, 7.1), (20, 20)]], np.float32)        # joints 0 and 1 truncate to the same pixel; limb (2, 2) is one joint twice
    check(frames(1, 37, 29), j, ((0, 1), (2, 2)), colors(2), style=style)


def test_overdraw_depends_on_the_order_as_the_reference_says():
    j = np.array([[(3, 3), (30, 20), (30, 4), (4, 21)]], np.float32)
    img, col = frames(1, 37, 29), colors(2)
    ab = check(img, j, ((0, 1), (2, 3)), col)
    ba = check(img, j, ((2, 3), (0, 1)), col[::-1])
    assert (ab != ba).any()
    twice = check(img, np.concatenate([j, j]), ((0, 1), (2, 3)), col, image_index=[0, 0])      # the same person again is not idempotent on soft edges
    assert (twice != ab).any()


def crowd(target, seed):
    """People in a 37 x 29 frame, skeleton ((0, 1), (2, 2)), three-column joints: exactly `target` of their primitives touch the first
    tile -- of either form: they lie in its first TILE_H rows -- interleaved with people that draw nothing and people below the tall tile."""
    far = TALL_H + 4
    assert far < 28
    rng = np.random.default_rng(seed)
    plan = [6] * (target // 6) + {0: [], 1: [1], 2: [1, 1], 3: [3], 4: [4], 5: [4, 1]}[target % 6]
    plan += [0] * 7 + [-1] * 40                       # 0: nobody confident; -1: a full person outside the tile
    plan = [plan[i] for i in rng.permutation(len(plan))]
    conf = {6: (1, 1, 1), 4: (1, 0, 1), 3: (1, 1, 0), 1: (1, 0, 0), 0: (0, 0, 0), -1: (1, 1, 1)}
    people = []
    for n in plan:
        xy = np.stack([rng.uniform(0, 36.9, 3), rng.uniform(far, 28.9, 3) if n < 0 else rng.uniform(0, TILE_H - 0.1, 3)], 1)
        people.append(np.concatenate([xy, np.array(conf[n], np.float64)[:, None]], 1))
    return np.array(people, np.float32)


@pytest.mark.parametrize('delta', [-1, 0, 1, 300])
def test_more_primitives_in_one_tile_than_the_list_holds(delta):
    """LIST_CAP - 1, LIST_CAP and LIST_CAP + 1 primitives touch one tile (then a second wrap's worth): the list is drawn and refilled,
    the order carries over."""
    target = LIST_CAP + delta if delta < 300 else 2 * LIST_CAP + 5
    j = crowd(target, 7 + delta)
    sk = ((0, 1), (2, 2))
    tops = np.array([q['a'][1] - 3 for p in j for q in dr.person_prims(p, sk, colors(2))])      # a footprint reaches up to 3 rows above its point
    assert (tops <= TILE_H - 1).sum() == target and (tops <= TALL_H - 1).sum() == target
    img = frames(2, 37, 29)
    check(img, j, sk, colors(2), image_index=[1] * len(j))


def test_the_built_in_choice_on_both_sides_of_its_grid_size():
    """One workgroup short of kTallTileFrom the one-row form is launched, at it the tall form: the same bytes (check() also forces both)."""
    per_frame = -(-29 // TILE_H)                     # workgroups of the one-row form in a 37 x 29 frame
    assert TALL_FROM % per_frame == 0
    N = TALL_FROM // per_frame
    img = np.broadcast_to(frames(1, 37, 29), (N, 29, 37, 3)).copy()
    img[:, 0, 0, 0] = np.arange(N) % 251
    j = np.stack([SLOPES_J, SLOPES_J + 2, SLOPES_J * 0.5, SLOPES_J[::-1], SLOPES_J + 1]).astype(np.float32)
    for n in (N - 1, N):
        check(img[:n], j, SLOPES_SK, colors(6), image_index=[0, n - 1, n // 2, n - 1, n - 2], alpha=0.25)


def test_an_image_does_not_depend_on_its_batch():
    img = frames(3, 37, 29)
    j = np.stack([SLOPES_J, SLOPES_J + 2, SLOPES_J * 0.5, SLOPES_J[::-1]]).astype(np.float32)
    col = colors(6)
    whole = check(img, j, SLOPES_SK, col, image_index=[2, 1, 1, 0])
    alone = check(img[1:2], j[1:3], SLOPES_SK, col, image_index=[0, 0])
    np.testing.assert_array_equal(whole[1], alone[0])
    other = img.copy()
    other[0], other[2] = 255 - other[0], 0
    again = check(other, j * [[[1]], [[1]], [[1]], [[3]]], SLOPES_SK, col, image_index=[2, 1, 1, 0])
    np.testing.assert_array_equal(again[1], whole[1])
    np.testing.assert_array_equal(check(img, j[:2], SLOPES_SK, col)[2], img[2])       # image_index None: a frame without a person is copied


def test_skipped_joints_remove_the_references_primitives():
    sk = ((0, 1), (1, 2), (2, 3), (3, 4))
    base = np.array([(4, 4, 0.9), (30, 6, 0.9), (28, 24, 0.9), (6, 22, 0.9), (18, 14, 0.9)], np.float32)
    img, col = frames(1, 37, 29), colors(4)
    full = check(img, base[None], sk, col)
    for joint, comp, value in ((1, 0, np.nan), (2, 1, np.inf), (3, 0, -np.inf), (4, 2, 0.4), (0, 2, 0.39), (2, 2, np.nan)):
        j = base.copy()
        j[joint, comp] = value
        out = check(img, j[None], sk, col)
        assert (out != full).any(), (joint, comp, value)
        less = [l for l in sk if joint not in l]                      # what is left: the limbs without that joint, and the other joints' marks
        prims = []
        for l, (a, b) in enumerate(sk):
            c8 = dr.to_c8(col[l])
            xy = dr.to_pixel(base[:, :2])[0]
            if (a, b) in less:
                prims.append(dr.capsule(xy[a], xy[b], 2, c8))
            prims += [dr.disc(xy[i], 3, c8) for i in (a, b) if i != joint]
        np.testing.assert_array_equal(out[0], dr.draw_prims(img[0], prims))
    j = base.copy()
    j[:, 2] = 0.400001
    np.testing.assert_array_equal(check(img, j[None], sk, col), full)


def test_two_column_joints_draw_everything():
    sk = ((0, 1), (1, 2))
    j = np.array([[(4, 4, 0.0), (30, 6, np.nan), (28, 24, -1.0)]], np.float32)
    img, col = frames(1, 37, 29), colors(2)
    np.testing.assert_array_equal(check(img, j, sk, col), img)
    out = check(img, j[:, :, :2], sk, col, kp_thre=np.nan)
    assert (out != img).any()
    d = drawer(sk, 3)
    conf = d.draw(T(img, torch.uint8), T(j[:, :, :2]), colors=T(col), conf=T(np.ones((1, 3))))
    np.testing.assert_array_equal(conf.cpu().numpy(), out)


@pytest.mark.parametrize('style', ['keypoints', 'coco'])
def test_box_on_and_off(style):
    j = np.stack([SLOPES_J, SLOPES_J + 1]).astype(np.float32)
    box = np.array([[(2.5, 3.5), (33.9, 3.2), (34.0, 26.0), (2, 26)], [(-5, 10), (20, -4), (50, 12), (np.nan, 40)]], np.float32)
    img, col = frames(2, 37, 29), colors(6)
    on = check(img, j, SLOPES_SK, col, bbox=box, style=style)
    off = check(img, j, SLOPES_SK, col, style=style)
    assert (on != off).any()
    at = np.full((2, 12, 2), (18, 3), np.float32)                      # every joint on the box's top edge (2, 3) - (33, 3)
    under = check(img, at, SLOPES_SK, col, bbox=box, style=style)
    assert tuple(under[0, 3, 10]) == (255, 255, 0) and tuple(under[0, 3, 18]) == dr.to_c8(col[5])      # the skeleton lies on top of the box


@pytest.mark.parametrize('alpha', [0.0, 0.25, 1.0])
def test_alpha(alpha):
    img = frames(2, 3 * TILE_W + 8, 2 * TILE_H + 1)
    j = np.stack([SLOPES_J, SLOPES_J * [5, 0.3]]).astype(np.float32)
    out = check(img, j, SLOPES_SK, colors(6), alpha=alpha)
    if alpha == 0.0:
        np.testing.assert_array_equal(out, img)


def test_in_place_repeat_and_workspace():
    from gator_amd import vis
    sk, col = SLOPES_SK, T(colors(6))
    d = vis.SkeletonDrawer(sk, 12, DEV)
    assert d.workspace() == (0, 0)
    img = T(frames(3, 37, 29), torch.uint8)
    j = T(np.stack([SLOPES_J, SLOPES_J + 2, SLOPES_J * 0.5]))
    for alpha in (1.0, 0.25):
        a = d.draw(img, j, colors=col, alpha=alpha)
        b = d.draw(img, j, colors=col, alpha=alpha)
        assert torch.equal(a, b)
        same = img.clone()
        ret = d.draw(same, j, colors=col, alpha=alpha, out=same)
        assert ret is same and torch.equal(same, a)
    small = d.workspace()
    assert small[0] > 0 and small[1] == 1                             # the records; no tables without image_index
    big_j, idx = j.repeat(40, 1, 1), [k % 3 for k in range(120)]
    d.draw(img, big_j, colors=col, image_index=idx)
    largest = d.workspace()
    assert largest[0] > small[0]
    for _ in range(3):
        d.draw(img, big_j, colors=col, image_index=idx)
        d.draw(img, j, colors=col)
        d.draw(img, big_j[:50], colors=col, image_index=idx[:50], bbox=None)
    assert d.workspace() == largest
    d.close()


def test_graph_capture_replays_to_the_same_bytes():
    from gator_amd import vis
    d = vis.SkeletonDrawer(SLOPES_SK, 12, DEV)
    img = T(frames(2, 37, 29), torch.uint8)
    j = T(np.stack([SLOPES_J, SLOPES_J + 2]))
    col = T(colors(6))
    out = torch.zeros_like(img)
    want = d.draw(img, j, colors=col, alpha=0.25).clone()             # the warm-up: the workspace is there before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        d.draw(img, j, colors=col, alpha=0.25, out=out)
    for shift in (0, 3):
        j.add_(shift)
        want = d.draw(img, j, colors=col, alpha=0.25).clone()
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)
    np.testing.assert_array_equal(out.cpu().numpy(), dr.draw(img.cpu().numpy(), j.cpu().numpy(), SLOPES_SK, col.cpu().numpy(), alpha=0.25))
    d.close()


def test_argument_errors_name_the_field_and_leave_out_untouched():
    from gator_amd import _lib
    lib = _lib.load()
    sk = np.array(SLOPES_SK, np.int32)
    h = ctypes.c_void_p()
    for bad, n_limbs, n_joints, word in ((sk, 0, 12, b'n_limbs'), (sk, 6, 11, b'joint index 11'), (sk * -1, 6, 12, b'joint index'), (None, 6, 12, b'null')):
        rc = lib.gator_draw2d_create(None if bad is None else bad.ctypes.data_as(ctypes.c_void_p), n_limbs, n_joints, ctypes.byref(h))
        assert rc == -1 and word in lib.gator_last_error() and not h.value, word
    assert lib.gator_draw2d_create(sk.ctypes.data_as(ctypes.c_void_p), 6, 12, ctypes.byref(h)) == 0
    N, H, W = 2, 29, 37
    img = T(frames(N, W, H), torch.uint8)
    out = torch.full_like(img, 77)
    j, col = T(np.stack([SLOPES_J, SLOPES_J])), T(colors(6))
    idx = np.array([0, 1], np.int32)
    good = dict(struct_size=ctypes.sizeof(_lib.Draw2dArgs), n_people=2, n_images=N, H=H, W=W, joint_dim=2, style=0, kp_thre=0.4, alpha=1.0,
                joints=j.data_ptr(), colors=col.data_ptr(), bbox=None, images=img.data_ptr(), out=out.data_ptr(), image_index=idx.ctypes.data)
    st = _lib.stream_ptr(torch.device(DEV))
    past, before = np.array([0, 2], np.int32), np.array([-1, 0], np.int32)
    cases = [(dict(joints=None), b'joints is NULL'), (dict(colors=None), b'colors is NULL'), (dict(images=None), b'images is NULL'),
             (dict(out=None), b'out is NULL'), (dict(H=0), b'H = 0'), (dict(W=0), b'W = 0'), (dict(H=-3), b'H = -3'), (dict(W=8193), b'W = 8193'),
             (dict(struct_size=ctypes.sizeof(_lib.Draw2dArgs) - 8), b'struct_size'), (dict(struct_size=0), b'struct_size'),
             (dict(image_index=past.ctypes.data), b'image_index[1] = 2'), (dict(image_index=before.ctypes.data), b'image_index[0] = -1'),
             (dict(image_index=None, n_images=1), b'image_index is NULL'), (dict(joint_dim=4), b'joint_dim'), (dict(style=2), b'style'),
             (dict(alpha=1.5), b'alpha'), (dict(alpha=float('nan')), b'alpha'), (dict(n_people=0), b'n_people'), (dict(n_images=0), b'n_images')]
    for change, word in cases:
        a = _lib.Draw2dArgs(**dict(good, **change))
        assert lib.gator_draw2d_u8(h, ctypes.byref(a), st) == -1, change
        msg = lib.gator_last_error()
        assert b'gator_draw2d_u8' in msg and word in msg, (change, msg)
    assert lib.gator_draw2d_u8(None, ctypes.byref(_lib.Draw2dArgs(**good)), st) == -1 and b'handle' in lib.gator_last_error()
    assert lib.gator_draw2d_u8(h, None, st) == -1 and b'args' in lib.gator_last_error()
    torch.cuda.synchronize()
    assert (out == 77).all()
    assert lib.gator_draw2d_u8(h, ctypes.byref(_lib.Draw2dArgs(**good)), st) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), dr.draw(img.cpu().numpy(), j.cpu().numpy(), SLOPES_SK, col.cpu().numpy()))
    assert lib.gator_draw2d_destroy(h) == 0 and lib.gator_draw2d_destroy(None) == 0
    with pytest.raises(RuntimeError, match='image_index'):
        drawer(SLOPES_SK, 12).draw(img, j, colors=col, image_index=[0, 5])


def test_numpy_mirrors_of_the_reference_functions():
    from gator_amd import vis
    rng = np.random.default_rng(3)
    img = frames(1, 64, 48)[0]
    sk = ((0, 7), (7, 8), (8, 9), (9, 10), (8, 11), (11, 12), (12, 13), (8, 14), (14, 15), (15, 16), (0, 1), (1, 2), (2, 3), (0, 4), (4, 5), (5, 6))
    kps = np.concatenate([rng.uniform(2, 60, (1, 17)), rng.uniform(2, 46, (1, 17)), rng.uniform(0.2, 1.0, (1, 17))])        # [3,J], float64
    kps[2, 5] = 0.3
    box = np.array([(1.5, 1.5), (62, 2), (62, 46), (1, 46)])
    got = vis.vis_2d_keypoints(img, kps, sk, bbox=box, kp_thre=0.4, alpha=1, device=DEV)
    j = np.concatenate([np.trunc(kps[:2].T), (kps[2] > 0.4)[:, None]], 1).astype(np.float32)
    c8 = np.rint(vis.rainbow_colors(16))
    np.testing.assert_array_equal(got, dr.draw(img[None], j[None], sk, c8, bbox=box[None].astype(np.float32), kp_thre=0.5)[0])
    assert got.dtype == np.uint8 and (got != img).any() and (kps[2] <= 0.4).any()
    default = vis.vis_2d_keypoints(img, kps, sk, device=DEV)          # the demo's call (demo/run.py:218)
    np.testing.assert_array_equal(default, dr.draw(img[None], j[None], sk, c8, kp_thre=0.5)[0])
    coco = vis.vis_coco_skeleton(img, kps, sk, (0.2, 0.9, 0.35), alpha=0.25, device=DEV)
    want = dr.draw(img[None], j[None, :, :2], sk, np.rint(np.array([[0.2 * 255, 0.9 * 255, 0.35 * 255]] * 16)), alpha=0.25, style=dr.COCO)[0]
    np.testing.assert_array_equal(coco, want)


def test_draw_fit_on_a_fit_mesh_to_image_dict():
    from gator_amd import camera, vis
    from tests.helpers import build_model, load_golden
    _, m = build_model('coco19_alpha')
    jr = load_golden('j_regressors')
    R = np.zeros((17, 6890), np.float32)
    R[jr['coco_row'], jr['coco_col']] = jr['coco_val']
    m.set_joint_regressor(R)
    raw = load_golden('cam_fit')['raw'][:1, :, :2].astype(np.float32)
    raw = np.concatenate([raw, raw + 40]) * np.float32(0.1)            # two detections in a frame a tenth of the demo's
    W, H = 192, 108
    conf = np.ones((2, 17, 1), np.float32)
    conf[1, 9] = 0.1                                                   # a wrist the detector was unsure of
    raw3 = np.concatenate([raw, conf], 2)
    fit = camera.fit_mesh_to_image(m, T(raw3), 'coco', image_size=(W, H), steps=5)
    sk = ((1, 2), (0, 1), (0, 2), (2, 4), (1, 3), (6, 8), (8, 10), (5, 7), (7, 9), (12, 14), (14, 16), (11, 13), (13, 15), (17, 11), (17, 12), (17, 18),
          (18, 5), (18, 6), (18, 0))
    img = frames(2, W, H)
    out = camera.draw_fit(fit, T(raw3), sk, T(img, torch.uint8), add_pelvis_neck=True, box=True).cpu().numpy()
    pelvis = np.concatenate([(raw[:, 11] + raw[:, 12]) * np.float32(0.5), conf[:, 11] * conf[:, 12]], 1)
    neck = np.concatenate([(raw[:, 5] + raw[:, 6]) * np.float32(0.5), conf[:, 5] * conf[:, 6]], 1)
    j19 = np.concatenate([raw3, pelvis[:, None], neck[:, None]], 1)
    b = fit['bbox'].cpu().numpy()
    corners = np.stack([np.stack([b[:, 0], b[:, 1]], 1), np.stack([b[:, 0] + b[:, 2], b[:, 1]], 1), np.stack([b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], 1),
                        np.stack([b[:, 0], b[:, 1] + b[:, 3]], 1)], 1)
    np.testing.assert_array_equal(out, dr.draw(img, j19, sk, vis.rainbow_colors(19), bbox=corners))
    plain = camera.draw_fit(fit, T(raw), vis.SkeletonDrawer(sk, 19, DEV), T(img, torch.uint8), add_pelvis_neck=True).cpu().numpy()
    np.testing.assert_array_equal(plain, dr.draw(img, j19[:, :, :2], sk, vis.rainbow_colors(19)))
    assert (plain != out).any() and (plain != img).any()
