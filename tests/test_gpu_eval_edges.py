"""The evaluation and preprocessing kernels at their edges, against fp64 references on the host (oracle.gator_oracle, plain numpy):
gator_rigid_align_f32 / gator_joint_errors_f32 (k_rigid_align, k_joint_errors: rigid_fit, svd3), gator_preprocess_pose2d_f32 /
gator_preprocess_chain_f32 and gator_regress_joints_f32.  Every sample of every batch is compared; no second device path serves as a
reference.  Every bad-argument case below is one the library (csrc/caller_kernels.hip, csrc/api.hip: the checks in front of each
launch) or the Python wrapper refuses before anything is launched.

`python -m pytest tests/test_gpu_eval_edges.py -q -s -m gpu` prints the figures kept in profiles/eval_edge_tests.txt."""
import ctypes

import numpy as np
import pytest
import torch

from gator_amd import _lib
from gator_amd import eval as geval
from gator_amd import preprocess
from oracle import gator_oracle as go
from tests import eval_edge_refs as er
from tests.helpers import _joint_setting

pytestmark = pytest.mark.gpu

COCO19_PAIRS = _joint_setting(19)[1]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def align(a32, b32):
    return geval.rigid_align(dev(a32), dev(b32)).cpu().numpy()


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- 2a: shapes ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('N', [3, 4, 13, 14, 17, 31, 32])
@pytest.mark.parametrize('B', [1, 63, 64, 65, 129, 4097])
def test_rigid_align_shapes(B, N):
    """One thread per sample in 64-thread blocks, points in a [point][axis][thread] LDS image sized for 32 points: every point count
    next to a limit and every batch next to a block edge, all samples against the oracle."""
    rs = np.random.RandomState(B * 100 + N)
    a = (rs.randn(B, N, 3) * 300.0).astype(np.float32)
    b = er.image_of(rs, a.astype(np.float64)).astype(np.float32)
    got = align(a, b)
    ref = er.oracle_align(a, b)
    err = np.abs(got - ref).max((1, 2))
    bound = er.points_bound(b, ref)
    print('\nrigid_align B=%d N=%d: worst |ours - oracle| / bound %.3f' % (B, N, (err / bound).max()))
    assert (err <= bound).all(), (B, N, int(np.argmax(err / bound)))


@pytest.mark.parametrize('B,N', [(129, 17), (65, 32), (63, 3)])
def test_results_move_with_their_samples_bit_for_bit(B, N):
    """The same samples in another order: each result is the same bits at its sample's new place, in the last partial block too."""
    rs = np.random.RandomState(B + N)
    a = (rs.randn(B, N, 3) * 300.0).astype(np.float32)
    b = er.image_of(rs, a.astype(np.float64)).astype(np.float32)
    perm = rs.permutation(B)
    assert np.array_equal(bits(align(a[perm], b[perm])), bits(align(a, b)[perm]))
    e = geval.joint_errors(dev(a), dev(b), eval_joints=None).cpu().numpy()
    assert np.array_equal(bits(geval.joint_errors(dev(a[perm]), dev(b[perm]), eval_joints=None).cpu().numpy()), bits(e[perm]))


# ---- 2b - 2d: input families ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,N', er.family_cases())
def test_rigid_align_family(name, N):
    """65 samples of one family.  Compared per sample: the aligned points where the optimum is unique; |aligned - b| where only that is
    (collinear target); the target centroid where H = 0.  Then, reference-free, the residual sum of squares: Procrustes is an optimum,
    so the device's may exceed the oracle's by the float32 rounding of its output only (er.rss_floor), and no small perturbation of the
    oracle's fit may get below it -- which a non-orthogonal R cannot satisfy whatever the reference does.  The PA column of
    gator_joint_errors_f32 is held to the oracle on the same samples.

    The bounds are the suite's own (3e-7 max|b| + 1e-6 max|ref| per sample; 2e-5 max(1, want)); no family needed another.  For
    `b == a` and the exact image the residual itself is bounded: the optimum leaves sum|r|^2 <= sum|rounding of b|^2 <= 3N (2^-24 max|b|)^2,
    so every coordinate of the fp64 fit is within sqrt(3N) 2^-24 max|b| of b, and its float32 store within 2^-24 max|b| more."""
    a32, b32, a64, b64, mode = er.make_family(name, N)
    got = align(a32, b32)
    ref = er.oracle_align(a32, b32)
    assert np.isfinite(got).all() and np.isfinite(ref).all()
    bound = er.points_bound(b32, ref)
    bmax = np.abs(b32).max((1, 2)).astype(np.float64)
    noise = np.abs(er.oracle_align(a64, b64) - ref).max((1, 2)) if mode == 'points' else None
    if mode == 'points':
        err = np.abs(got - ref).max((1, 2))
    elif mode == 'dist':
        err = np.abs(np.linalg.norm(got.astype(np.float64) - b32, axis=2) - np.linalg.norm(ref - b32, axis=2)).max(1)
    else:
        assert mode == 'centroid'
        err = np.abs(got - b32).max((1, 2))
    print('\n%-46s N=%2d %-8s worst |ours - oracle| / max|b| %.2e   bound / max|b| %.2e   oracle f32 - f64 inputs / max|b| %s'
          % (name, N, mode, (err / bmax).max(), (bound / bmax).min(), 'n/a' if noise is None else '%.2e' % (noise / bmax).max()))
    if mode == 'centroid':
        assert np.array_equal(got, b32), 'H = 0 with var(a) > 0: c = 0, aligned = the target centroid exactly'
    else:
        assert (err <= bound).all(), (name, N, int(np.argmax(err / bound)), float((err / bound).max()))
    if name in ('b == a', 'b = exact similarity image of a'):
        assert (np.abs(got - b32).max((1, 2)) <= (np.sqrt(3.0 * N) + 1.0) * er.F32_EPS * bmax).all()
    # 2d: the optimum, reference-free
    r_dev, r_ref = er.rss(got, b32), er.rss(ref, b32)
    floor = er.rss_floor(ref, r_ref)
    over = (r_dev - (1 + 1e-6) * r_ref) / floor
    print('%-46s N=%2d          worst (rss ours - (1 + 1e-6) rss oracle) / float32 floor %.3f' % ('', N, over.max()))
    assert (r_dev <= (1 + 1e-6) * r_ref + floor).all(), (name, N, int(np.argmax(over)), float(over.max()))
    r_pert = er.perturbed_fits(np.random.RandomState(N), a32, b32)
    assert (r_pert >= r_dev - floor).all(), (name, N)
    # the PA column of joint_errors (root 0, all joints; the kernel root-aligns in float32, and so does the oracle's input here)
    e = geval.joint_errors(dev(a32), dev(b32), eval_joints=None).cpu().numpy().astype(np.float64)
    want0, want1 = er.oracle_joint_errors(a32 - a32[:, :1], b32 - b32[:, :1], None, 0, 1.0)
    print('%-46s N=%2d          worst |PA-MPJPE ours - oracle| / bound %.3f' % ('', N, (np.abs(e[:, 1] - want1) / er.errors_bound(want1)).max()))
    assert (np.abs(e[:, 1] - want1) <= er.errors_bound(want1)).all(), (name, N)
    assert (np.abs(e[:, 0] - want0) <= er.errors_bound(want0)).all(), (name, N)


def _contained(a32, b32, bad, a_bad, b_bad):
    """Samples `bad` replaced by (a_bad, b_bad): -> (aligned, errors) of the batch with them, after checking that every OTHER sample is
    bit-identical to the run without them."""
    a2, b2 = a32.copy(), b32.copy()
    a2[bad], b2[bad] = a_bad, b_bad
    clean, dirty = align(a32, b32), align(a2, b2)
    e_clean = geval.joint_errors(dev(a32), dev(b32), eval_joints=None).cpu().numpy()
    e_dirty = geval.joint_errors(dev(a2), dev(b2), eval_joints=None).cpu().numpy()
    torch.cuda.synchronize()                                  # the calls returned
    keep = np.ones(len(a32), bool)
    keep[bad] = False
    assert np.isfinite(clean).all() and np.isfinite(e_clean).all()
    assert np.array_equal(bits(dirty[keep]), bits(clean[keep])) and np.array_equal(bits(e_dirty[keep]), bits(e_clean[keep]))
    return a2, b2, dirty, e_dirty


@pytest.mark.parametrize('N', [3, 14])
def test_identical_source_points_are_non_finite_in_their_sample_only(N):
    """var(a) = 0: the oracle's c = sum(s) / var(a) is 0 / 0 and every aligned point NaN.  So is the device's, in that sample; its batch
    neighbours (same block, next block) keep their bits."""
    a32, b32, _, _, _ = er.make_family('generic', N, B=130, seed=1)
    bad = [0, 37, 63, 64, 129]
    a_bad = np.repeat(a32[bad][:, :1], N, axis=1)
    a2, b2, got, e = _contained(a32, b32, bad, a_bad, b32[bad])
    ref = er.oracle_align(a2, b2)
    assert not np.isfinite(ref[bad]).any()
    assert not np.isfinite(got[bad]).any() and not np.isfinite(e[bad, 1]).any()
    assert np.array_equal(e[bad, 0], geval.joint_errors(dev(a2[bad]), dev(b2[bad]), eval_joints=None).cpu().numpy()[:, 0]) and np.isfinite(e[bad, 0]).all()


@pytest.mark.parametrize('value', [np.nan, np.inf, -np.inf])
def test_a_non_finite_sample_stays_in_its_sample(value):
    """One NaN / Inf coordinate in the source of one sample and in the target of another: the call returns, those samples are non-finite,
    all others keep their bits."""
    a32, b32, _, _, _ = er.make_family('generic', 14, B=130, seed=2)
    bad = [5, 64]
    a_bad, b_bad = a32[bad].copy(), b32[bad].copy()
    a_bad[0, 3, 1] = value
    b_bad[1, 13, 2] = value
    a2, b2, got, e = _contained(a32, b32, bad, a_bad, b_bad)
    assert not np.isfinite(got[bad]).any() and not np.isfinite(e[bad, 1]).any()


# ---- 2e: joint_errors --------------------------------------------------------------------------------------------------------------

def _eval_sets(nj, root):
    rs = np.random.RandomState(nj + root)
    sets = {'none': None, 'permuted': tuple(rs.permutation(nj)[:11]), 'three': (nj - 1, 0, 7),
            'without root': tuple(j for j in range(nj) if j != root)[:14]}
    if nj >= 17:
        sets['h36m'] = geval.H36M_EVAL_JOINTS
    if nj == 32:
        sets['all 32, permuted'] = tuple(rs.permutation(32))
    return sets


@pytest.mark.parametrize('pred_scale', [1.0, 1000.0])
@pytest.mark.parametrize('nj,root', [(17, 0), (17, 5), (17, 16), (32, 0), (32, 5), (32, 31)])
def test_joint_errors_roots_index_sets_and_scale(nj, root, pred_scale):
    """Both columns of gator_joint_errors_f32 against the oracle on every sample, for each root and evaluation set, and against
    geval.mpjpe / geval.pa_mpjpe of the single sample."""
    B = 65
    rs = np.random.RandomState(nj * 7 + root)
    tgt = (rs.randn(B, nj, 3) * 250.0 + rs.randn(B, 1, 3) * 500.0).astype(np.float32)                       # mm
    pred = ((tgt + rs.randn(B, nj, 3) * 40.0 + rs.randn(B, 1, 3) * 30.0) / pred_scale).astype(np.float32)   # mm, or m for 1000
    dp, dt = dev(pred), dev(tgt)
    for label, ev in _eval_sets(nj, root).items():
        err = geval.joint_errors(dp, dt, eval_joints=ev, root=root, pred_scale=pred_scale).cpu().numpy().astype(np.float64)
        want0, want1 = er.oracle_joint_errors(pred, tgt, ev, root, pred_scale)
        r0, r1 = np.abs(err[:, 0] - want0) / er.errors_bound(want0), np.abs(err[:, 1] - want1) / er.errors_bound(want1)
        print('\njoint_errors nj=%d root=%d scale=%g %-18s worst error / bound: MPJPE %.3f  PA-MPJPE %.3f' % (nj, root, pred_scale, label, r0.max(), r1.max()))
        assert (r0 <= 1).all() and (r1 <= 1).all(), (label, int(np.argmax(r0)), int(np.argmax(r1)))
        scaled = dp * float(pred_scale)
        ev_all = tuple(range(nj)) if ev is None else ev
        m = np.array([float(geval.mpjpe(scaled[i:i + 1], dt[i:i + 1], ev, root)) for i in range(B)])
        pa = np.array([float(geval.pa_mpjpe(scaled[i:i + 1], dt[i:i + 1], ev_all)) for i in range(B)])
        # geval.pa_mpjpe aligns the joints where they are, not root-aligned: its float32 store of an aligned point and its float32
        # `aligned - target` each round at the size of the absolute coordinates, 2^-24 max|target| per coordinate, sqrt(3) of it per distance
        f32_abs = np.sqrt(3.0) * 2.0 ** -23 * np.abs(tgt).max((1, 2))
        assert (np.abs(err[:, 0] - m) <= er.errors_bound(want0)).all() and (np.abs(err[:, 1] - pa) <= er.errors_bound(want1) + f32_abs).all(), label


# ---- 2f: arguments -----------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_before_any_launch():
    """gator_rigid_align_f32 / gator_joint_errors_f32 return GATOR_EINVAL in front of the launch (csrc/caller_kernels.hip) for a point
    count outside 3..32, an evaluation count outside 3..32, a root outside the joints, a null pointer and an empty batch; the output
    buffer keeps its contents."""
    lib = _lib.load()
    x = torch.randn(4, 40, 3, device='cuda')
    out = torch.full((4, 40, 3), 7.0, device='cuda')
    idx = torch.arange(32, dtype=torch.int32, device='cuda')
    p, o, ix, st = x.data_ptr(), out.data_ptr(), idx.data_ptr(), stream()
    for n in (0, 1, 2, 33, 40, -1):
        assert lib.gator_rigid_align_f32(p, p, 4, n, o, st) == -1
    for batch in (0, -1):
        assert lib.gator_rigid_align_f32(p, p, batch, 14, o, st) == -1
        assert lib.gator_joint_errors_f32(p, p, batch, 17, ix, 14, 0, 1.0, o, st) == -1
    for args in ((None, p, 4, 14, o), (p, None, 4, 14, o), (p, p, 4, 14, None)):
        assert lib.gator_rigid_align_f32(*args, st) == -1
    for args in ((None, p, 4, 17, ix, 14, 0), (p, None, 4, 17, ix, 14, 0)):
        assert lib.gator_joint_errors_f32(*args, 1.0, o, st) == -1
    assert lib.gator_joint_errors_f32(p, p, 4, 17, ix, 14, 0, 1.0, None, st) == -1
    for n_eval in (0, 1, 2, 33, -3):
        assert lib.gator_joint_errors_f32(p, p, 4, 40, ix, n_eval, 0, 1.0, o, st) == -1
    for nj in (0, 2, 33, 40):                                  # no index list: all joints are evaluated, so they must be 3..32
        assert lib.gator_joint_errors_f32(p, p, 4, nj, None, 0, 0, 1.0, o, st) == -1
    for root in (-1, 17, 1000):
        assert lib.gator_joint_errors_f32(p, p, 4, 17, ix, 14, root, 1.0, o, st) == -1
    assert b'gator_joint_errors_f32' in lib.gator_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(RuntimeError):
        geval.rigid_align(x[:, :2].contiguous(), x[:, :2].contiguous())
    with pytest.raises(ValueError):
        geval.rigid_align(x[:, :14], x[:, :15])
    with pytest.raises(RuntimeError):
        geval.joint_errors(x[:, :17].contiguous(), x[:, :17].contiguous(), root=17)


@pytest.mark.parametrize('ev', [(0, 1, -1), (0, 1, 17), (3, 4, 5, 1 << 20), (-17, 2, 3)])
def test_evaluation_indices_are_validated_on_the_host(ev):
    """An evaluation index is a raw offset in k_joint_errors: the wrappers refuse one outside [0, n_joint) from the Python list, with a
    ValueError, before any tensor of it exists on the device."""
    x = torch.randn(4, 17, 3, device='cuda')
    with pytest.raises(ValueError):
        geval.joint_errors(x, x, eval_joints=ev)
    with pytest.raises(ValueError):
        geval.pa_mpjpe(x, x, eval_joints=ev)


# ---- 4: preprocessing ----------------------------------------------------------------------------------------------------------------

ROTS = (0.0, 17.5, -17.5, 90.0, -90.0, 180.0, 359.0)
RESOLUTIONS = ((288, 384), (256, 256), (384, 288))


def _with_pelvis_neck(raw):
    """The device appends pelvis and neck (csrc/caller_kernels.hip); the oracle is fed the same joints, via its own add_pelvis_neck_coco."""
    j = raw.astype(np.float64)
    j3 = np.concatenate([j[:, :2], np.ones((len(j), 1))], 1)
    return go.add_pelvis_neck_coco(j3)[:, :2]


def _chain_reference(raw, add, rot, flip, pairs, res):
    """go.preprocess_pose2d per sample -> (pose2d with zeros where the box is rejected, valid)."""
    B, J = raw.shape[0], raw.shape[1] + (2 if add else 0)
    out, valid = np.zeros((B, J, 2)), np.zeros(B, np.int32)
    for i in range(B):
        j = _with_pelvis_neck(raw[i]) if add else raw[i, :, :2].astype(np.float64)
        with np.errstate(all='ignore'):
            r = go.preprocess_pose2d(j, rot=float(rot[i]), flip=bool(flip[i]), flip_pairs=pairs, res=res)
        if r is not None:
            out[i], valid[i] = r, 1
    return out, valid


def _check_chain(raw, add, rot, flip, pairs, res, what, tol=2e-5):
    out, valid = preprocess.preprocess_chain(dev(raw), rot_deg=rot, flip=flip, flip_pairs=pairs, add_pelvis_neck=add, res=res)
    out, valid = out.cpu().numpy(), valid.cpu().numpy()
    ref, want = _chain_reference(raw, add, rot, flip, pairs, res)
    assert np.array_equal(valid, want), (what, np.nonzero(valid != want)[0][:8])
    assert np.all(out[want == 0] == 0)
    err = np.abs(out - ref).max((1, 2)) if len(out) else np.zeros(0)
    print('\npreprocess_chain %-60s kept %3d of %3d   worst |ours - oracle| %.2e' % (what, int(want.sum()), len(want), err.max()))
    assert (err <= tol).all(), (what, int(np.argmax(err)), float(err.max()))
    return out, valid


def _pairs_for(J, kind):
    if kind == 'none':
        return ()
    if J == 19:
        return COCO19_PAIRS
    return tuple((2 * k + 1, 2 * k + 2) for k in range((J - 1) // 2))[:8]


@pytest.mark.parametrize('J_in,add', [(2, False), (13, True), (17, True), (19, False), (30, True), (32, False)])
@pytest.mark.parametrize('B', [1, 63, 64, 65, 257])
def test_preprocess_chain_shapes_rotations_and_flips(B, J_in, add):
    """Every sample against go.preprocess_pose2d: each batch / joint-count edge with every component count, resolution, pair table; the
    rotations of ROTS and both flip values are spread over the samples of each batch."""
    J = J_in + (2 if add else 0)
    rs = np.random.RandomState(B * 64 + J)
    for k, (comps, res, kind) in enumerate(((2, RESOLUTIONS[0], 'pairs'), (3, RESOLUTIONS[1], 'none'), (5, RESOLUTIONS[2], 'pairs'))):
        raw = rs.rand(B, J_in, comps) * 400.0 + rs.rand(B, 1, comps) * 600.0
        if J_in == 2:
            # two joints: the segment is kept 35 .. 55 degrees off the image axes, at least 17 degrees after any rotation of ROTS.  Lined up
            # with an axis the other one has no spread, and the reference's own float32 cast of the two coordinates decides the result.
            th = np.deg2rad(rs.uniform(35.0, 55.0, B))
            raw[:, 1, :2] = raw[:, 0, :2] + rs.uniform(100.0, 400.0, B)[:, None] * np.stack([np.cos(th), rs.choice([-1.0, 1.0], B) * np.sin(th)], 1)
        raw = raw.astype(np.float32)
        rot = np.array([ROTS[(i + k) % len(ROTS)] for i in range(B)], np.float32)
        flip = ((np.arange(B) // len(ROTS) + k) % 2).astype(np.int32)
        if B == 1:
            rot[0], flip[0] = ROTS[1 + k], k % 2
        _check_chain(raw, add, rot, flip, _pairs_for(J, kind), res, 'B=%d J=%d%s comps=%d res=%s pairs=%s' % (B, J_in, '+2' if add else '', comps, res, kind))


@pytest.mark.parametrize('rot', ROTS)
@pytest.mark.parametrize('flip', [0, 1])
def test_preprocess_chain_every_rotation_with_and_without_flip(rot, flip):
    rs = np.random.RandomState(int(rot * 10) % 1000 + flip)
    raw = (rs.rand(65, 19, 2) * np.array([300.0, 500.0]) + 100.0).astype(np.float32)
    for pairs, label in ((COCO19_PAIRS, 'coco19 pairs'), ((), 'no pairs')):
        for res in RESOLUTIONS:
            _check_chain(raw, False, np.full(65, rot, np.float32), np.full(65, flip, np.int32), pairs, res, 'rot=%g flip=%d %s res=%s' % (rot, flip, label, res))


def _box_sample(rs, J, x0, y0, w, h):
    """J joints whose tight box is exactly [x0, x0 + w] x [y0, y0 + h]; all coordinates dyadic (multiples of 2^-10 below 2^12), so the
    float32 box the reference and the device derive is exact."""
    q = 2.0 ** -10
    p = np.stack([x0 + np.floor(rs.rand(J) * w / q) * q, y0 + np.floor(rs.rand(J) * h / q) * q], 1)
    p[0], p[1] = (x0, y0 + h), (x0 + w, y0)
    return p


def test_preprocess_chain_box_edges():
    """process_bbox keeps a box of exactly one pixel in width or height, and of 1 + 2^-10; it rejects 1 - 2^-10, and a wide box lower
    than a pixel.  The three aspect branches: wider than the input shape, higher, and equal (4 x 5 at 288 x 384: (4-1) = 0.75 (5-1)).
    The ONLY input kept out: a box of exactly one pixel in BOTH directions -- its scale is zero, the reference's affine solve is singular
    and the oracle raises."""
    d = 2.0 ** -10
    boxes = [(1.0, 40.0, 1), (40.0, 1.0, 1), (1.0 - d, 40.0, 0), (40.0, 1.0 - d, 0), (1.0 + d, 40.0, 1), (40.0, 1.0 + d, 1), (1.0 + d, 1.0 + d, 1),
             (1.0, 1.0 + d, 1), (1.0 + d, 1.0, 1), (900.0, 0.5, 0), (0.5, 900.0, 0), (900.0, 1.0 - d, 0), (4.0, 5.0, 1), (5.0, 4.0, 1), (400.0, 30.0, 1),
             (30.0, 400.0, 1), (3.25, 4.0, 1), (4.0, 4.0, 1), (1.0 - d, 1.0 - d, 0), (0.0, 50.0, 0), (50.0, 0.0, 0)]
    rs = np.random.RandomState(5)
    for res in RESOLUTIONS:
        for J in (2, 19):
            raw, keep = [], []
            for rep in range(4):
                for w, h, kept in boxes:
                    raw.append(_box_sample(rs, J, float(rs.randint(0, 2000)) + rep * 0.25, float(rs.randint(0, 2000)), w, h))
                    keep.append(kept)
            raw = np.stack(raw).astype(np.float32)
            B = len(raw)
            rot = np.array([ROTS[i % len(ROTS)] for i in range(B)], np.float32)
            flip = (np.arange(B) % 2).astype(np.int32)
            out, valid = _check_chain(raw, False, rot, flip, _pairs_for(J, 'pairs'), res, 'box edges J=%d res=%s' % (J, res))
            assert np.array_equal(valid, np.array(keep, np.int32))


@pytest.mark.parametrize('size', [2.0, 3.5, 17.0, 250.0, 4000.0])
def test_preprocess_chain_large_image_coordinates(size):
    """Boxes of 2 .. 4000 px anywhere in an 8192 px image: the device solves the affine by Cramer's rule in absolute coordinates, the
    oracle by LU; both are held to the chain's 2e-5."""
    rs = np.random.RandomState(int(size * 2))
    B, J = 129, 19
    origin = np.floor(rs.rand(B, 1, 2) * (8192.0 - size))
    origin[0], origin[1], origin[2] = 0.0, 8192.0 - size, (8192.0 - size, 0.0)
    raw = origin + rs.rand(B, J, 2) * size * np.array([1.0, 0.5 + rs.rand()])
    raw[:, 0], raw[:, 1] = origin[:, 0], origin[:, 0] + size
    raw = raw.astype(np.float32)
    rot = np.array([ROTS[i % len(ROTS)] for i in range(B)], np.float32)
    flip = (np.arange(B) // 3 % 2).astype(np.int32)
    for res in RESOLUTIONS:
        _check_chain(raw, False, rot, flip, COCO19_PAIRS, res, 'box %g px in 8192 px, res=%s' % (size, res))


def test_preprocess_chain_refuses_a_negative_flip_pair_on_the_host():
    x = torch.rand(3, 19, 2, device='cuda') * 100
    for pairs in (((1, 2), (-1, 3)), ((4, -2),)):
        with pytest.raises(ValueError):
            preprocess.preprocess_chain(x, flip=np.ones(3, np.int32), flip_pairs=pairs)


@pytest.mark.parametrize('J_in,add', [(1, False), (2, False), (13, True), (17, True), (19, False), (30, True), (32, False)])
@pytest.mark.parametrize('B', [1, 63, 64, 65, 257])
def test_reduced_preprocess_shapes(B, J_in, add):
    """gator_preprocess_pose2d_f32 against go.normalise_pose2d, every sample, 2e-6.  One joint has no spread: 0 / 0 on both axes, NaN
    exactly where numpy has it."""
    rs = np.random.RandomState(B * 64 + J_in)
    for comps in (2, 3, 5):
        raw = (rs.rand(B, J_in, comps) * 400.0 + rs.rand(B, 1, comps) * 6000.0).astype(np.float32)
        out = preprocess.normalise_pose2d(dev(raw), add_pelvis_neck=add).cpu().numpy()
        with np.errstate(all='ignore'):
            ref = np.stack([go.normalise_pose2d(_with_pelvis_neck(raw[i]) if add else raw[i]) for i in range(B)])
        assert out.shape == ref.shape
        assert np.array_equal(np.isnan(out), np.isnan(ref)) and np.isnan(ref).all() == (J_in == 1)
        if J_in > 1:
            err = np.abs(out - ref).max()
            print('\npreprocess B=%d J=%d%s comps=%d: worst |ours - oracle| %.2e' % (B, J_in, '+2' if add else '', comps, err))
            assert err <= 2e-6


def test_reduced_preprocess_degenerate_axis_stays_in_its_sample():
    """All x equal in some samples: their x column is 0 / 0 = NaN exactly where numpy's is, their y column and every other sample are
    as without them, bit for bit."""
    rs = np.random.RandomState(9)
    raw = (rs.rand(130, 19, 3) * 400.0 + 50.0).astype(np.float32)
    bad = [0, 63, 64, 129]
    raw2 = raw.copy()
    raw2[bad, :, 0] = raw[bad, :1, 0]
    clean = preprocess.normalise_pose2d(dev(raw)).cpu().numpy()
    got = preprocess.normalise_pose2d(dev(raw2)).cpu().numpy()
    with np.errstate(all='ignore'):
        ref = np.stack([go.normalise_pose2d(j) for j in raw2])
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(got[bad, :, 0]).all() and np.isnan(got).sum() == len(bad) * 19
    assert np.abs(np.nan_to_num(got) - np.nan_to_num(ref)).max() <= 2e-6
    keep = np.ones(130, bool)
    keep[bad] = False
    assert np.array_equal(bits(got[keep]), bits(clean[keep])) and np.array_equal(bits(got[bad][:, :, 1]), bits(clean[bad][:, :, 1]))


# ---- 5: joint regression ---------------------------------------------------------------------------------------------------------------

def _regress(verts, row, col, val, nj):
    B = verts.shape[0]
    dv, dr, dc, dw = dev(verts), dev(row.astype(np.int32)), dev(col.astype(np.int32)), dev(val.astype(np.float32))
    out = torch.full((B, nj, 3), 7.0, device='cuda')
    _lib.check(_lib.load().gator_regress_joints_f32(dv.data_ptr(), B, dr.data_ptr(), dc.data_ptr(), dw.data_ptr(), len(row), nj, out.data_ptr(), stream()),
               'gator_regress_joints_f32')
    return out.cpu().numpy()


@pytest.mark.parametrize('nnz', [1, 63, 64, 65, 1000])
@pytest.mark.parametrize('nj', [1, 17, 33])
@pytest.mark.parametrize('B', [1, 65])
def test_regress_joints_with_synthetic_coo(B, nj, nnz):
    """k_regress against an fp64 einsum over the same COO list: unsorted entries, duplicate (row, col) entries, the first and the last
    vertex, a joint without any entry (exactly 0), and terms of ~1e3 that cancel to ~1e-3.  Bound per output: 2e-6 sum|val vert|, the
    float32 rounding of a sum the kernel accumulates in fp64."""
    rs = np.random.RandomState(B + nj * 3 + nnz)
    verts = rs.randn(B, 6890, 3).astype(np.float32)
    empty = nj - 1 if nj > 1 else None                          # this joint gets no entry
    row = rs.randint(0, max(1, nj - 1), nnz)
    col = rs.randint(0, 6890, nnz)
    val = rs.rand(nnz).astype(np.float32)
    col[0] = 6889
    if nnz >= 63:
        col[1], col[2:6], row[2:6] = 0, col[6], row[6]           # duplicates of entry 6
        k = nnz // 2 // 2 * 2                                    # cancellation on joint 0: pairs (v, -(v - 1e-3 / pairs)) of ~1e3 on one vertex
        row[nnz - k:] = 0
        col[nnz - k:] = 3445
        big = (1e3 * (0.5 + rs.rand(k // 2))).astype(np.float32)
        val[nnz - k::2], val[nnz - k + 1::2] = big, -(big - np.float32(1e-3))
        verts[:, 3445] = 1.0
    dense = np.zeros((nj, 6890))
    mag = np.zeros((nj, 6890))
    np.add.at(dense, (row, col), val.astype(np.float64))
    np.add.at(mag, (row, col), np.abs(val.astype(np.float64)))
    ref = np.einsum('jv,bvk->bjk', dense, verts.astype(np.float64))
    bound = 2e-6 * np.einsum('jv,bvk->bjk', mag, np.abs(verts.astype(np.float64)))
    got = _regress(verts, row, col, val, nj)
    err = np.abs(got - ref)
    print('\nregress B=%d nj=%d nnz=%d: worst |ours - ref64| / bound %.3f' % (B, nj, nnz, (err[bound > 0] / bound[bound > 0]).max()))
    assert (err <= bound).all()
    if empty is not None:
        assert np.all(got[:, empty] == 0.0) and np.all(bound[:, empty] == 0.0)


def test_joint_regressor_rejects_a_matrix_that_is_not_n_by_6890():
    """Nothing on the device validates a column before it is used as a vertex offset: the dense matrix must be [n_joint, 6890]."""
    for shape in ((17, 6891), (17, 6889), (6890, 17), (6890,), (2, 17, 6890)):
        with pytest.raises(ValueError):
            geval.JointRegressor(np.ones(shape, np.float32), 'cuda')
    reg = geval.JointRegressor(np.eye(3, 6890, k=6887, dtype=np.float32), 'cuda')       # joints = the last three vertices
    v = torch.randn(2, 6890, 3, device='cuda')
    assert torch.equal(reg(v), v[:, 6887:])
    lib = _lib.load()
    p, st = v.data_ptr(), stream()
    for args in ((None, 2, p, p, p, 3, 3, p), (p, 0, p, p, p, 3, 3, p), (p, 2, None, p, p, 3, 3, p), (p, 2, p, p, p, 0, 3, p), (p, 2, p, p, p, 3, 0, p), (p, 2, p, p, p, 3, 3, None)):
        assert lib.gator_regress_joints_f32(*args, st) == -1
