"""gator_batch_prepare_f32 / gator_camera_targets_f32 / gator_amd.batch on the device against the float64 restatements of
tests/batch_refs.py.  Every test prints its measured error as a multiple of its bound before it asserts (profiles/train_batch.txt).

Bounds, none of them measured:
  k_batch_prepare    exp(out) against R exp(root) element by element: sqrt(3) pi 2^-24 for the rounding of the three output components
                     (each at most pi in size; a change d of a rotation vector moves no matrix element by more than |d|), plus the
                     orthogonality defect |R^T R - I|_F of the float32 R of that sample (a non-orthogonal product has no rotation
                     vector: the kernel takes the nearest rotation, which lies within the defect).  Away from pi the vector itself
                     against scipy within 2^-23 pi.
  k_camera_targets   every element of every output within 2^-23 |ref| + 1e-10 * sum |w| |v * 1000| (batch_refs.tolerances): one rounding
                     to float32 plus fp64 accumulation; a pixel carries the second term through X / Z * f.  The masks are exact.
  end to end         the layer's own bound (tests/test_gpu_smpl.py: 3 x the case's float32 spread, in mm), the project's 10 float32
                     roundings at the values' size for the parent's float32 tail, and the root vector's rounding and R's defect turned
                     into millimetres at the mesh's largest distance from the origin.

Sizes: one case of 6890 vertices; the rest NV in {3, 255, 256, 257} (one vertex pass of 256 lanes: below, at and above it, and a mesh
smaller than a regressor row) with B in {1, 2, 65}."""
import ctypes
import functools

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

from gator_amd import _lib, batch, preprocess, smpl
from gator_amd import eval as gator_eval
from tests import batch_refs as br
from tests import smpl_refs as sr

pytestmark = pytest.mark.gpu

OUT_KEYS = ('mesh', 'reg_pose3d', 'lift_pose3d', 'joint_img', 'fit_error', 'valid')
ROUND3 = np.sqrt(3.0) * np.pi * 2.0 ** -24
EINVAL = -1


def dev(x, dtype=torch.float32):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to('cuda', dtype)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- k_batch_prepare ------------------------------------------------------------------------------------------------------------------

FAMILIES = ('zero_root', 'tiny_root', 'identity_product', 'near_pi', 'pi_x', 'pi_y', 'pi_z', 'pi_generic', 'five_rad', 'diag_1m1m1', 'generic')


@functools.lru_cache(maxsize=None)
def prepare_case():
    """65 samples: one per family first, generic ones after.  -> (pose f32 [65,72], R f32 [65,3,3], betas f32 [65,10])."""
    rs = np.random.RandomState(404)
    B = 65
    pose = (rs.randn(B, 72) * 0.4).astype(np.float32)
    R = Rotation.from_rotvec(rs.randn(B, 3) * 0.9).as_matrix()
    unit = lambda v: v / np.linalg.norm(v)  # noqa: E731
    pose[0, :3] = 0.0
    pose[1, :3] = (unit(rs.randn(3)) * 1e-8).astype(np.float32)
    R[2] = br.exp_rotvec(pose[2, :3].astype(np.float64)).T
    R[3] = br.exp_rotvec(unit(rs.randn(3)) * (np.pi - 1e-4)) @ br.exp_rotvec(pose[3, :3].astype(np.float64)).T
    for i, d in ((4, (1, -1, -1)), (5, (-1, 1, -1)), (6, (-1, -1, 1))):                  # exactly pi about x, y, z: a zero root, an exact R
        pose[i, :3] = 0.0
        R[i] = np.diag(np.array(d, np.float64))
    a = unit(rs.randn(3))
    pose[7, :3] = 0.0
    R[7] = 2 * np.outer(a, a) - np.eye(3)                                                 # pi about a generic axis
    pose[8, :3] = (unit(rs.randn(3)) * 5.0).astype(np.float32)
    R[9] = np.diag([1.0, -1.0, -1.0])
    betas = rs.uniform(-2.5, 2.5, (B, 10)).astype(np.float32)
    betas[0] = np.where(rs.rand(10) < 0.5, -3.0, 3.0)                                     # +-3 exactly: kept
    betas[1, 4] = np.nextafter(np.float32(3.0), np.float32(4.0))                          # just beyond: zeroed
    betas[2, 9] = -np.nextafter(np.float32(3.0), np.float32(4.0))
    betas[3, 0] = np.nan                                                                  # NaN > 3 is false: kept, bit for bit
    return pose, R.astype(np.float32), betas


def run_prepare(pose, R, betas, inplace=False):
    p, r, b = dev(pose), dev(R), dev(betas)
    po = p if inplace else torch.full_like(p, -7.0)
    bo = None if b is None else (b if inplace else torch.full_like(b, -7.0))
    batch._launch_prepare(p, r, b, 0, po, bo)
    return po.cpu().numpy(), None if bo is None else bo.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize('B', [1, 2, 65])
def test_prepare_against_fp64(B):
    pose, R, betas = (a[:B] for a in prepare_case())
    out, bout = run_prepare(pose, R, betas)
    assert np.array_equal(bits(out[:, 3:]), bits(pose[:, 3:]))                            # every other joint: bit for bit
    R64, root64 = R.astype(np.float64), pose[:, :3].astype(np.float64)
    M = R64 @ br.exp_rotvec(root64)
    defect = np.linalg.norm(np.swapaxes(R64, 1, 2) @ R64 - np.eye(3), axis=(1, 2))
    got = out[:, :3].astype(np.float64)
    angle = np.linalg.norm(got, axis=1)
    assert np.isfinite(got).all() and (angle <= np.pi * (1 + 2.0 ** -23)).all()
    err = np.abs(br.exp_rotvec(got) - M).max(axis=(1, 2))
    bound = ROUND3 + defect
    vec = br.log_rotmat(M)
    away = np.linalg.norm(vec, axis=1) < np.pi - 1e-3
    verr = np.abs(got - vec).max(axis=1)
    for i in range(B):
        fam = FAMILIES[min(i, len(FAMILIES) - 1)]
        if i < len(FAMILIES):
            print('batch prepare %-16s angle %.9f  |exp(out) - R exp(root)| %.3e = %.2f x bound (defect %.1e)  vector vs scipy %s'
                  % (fam, angle[i], err[i], err[i] / bound[i], defect[i], '%.3e = %.2f x 2^-23 pi' % (verr[i], verr[i] / (2.0 ** -23 * np.pi)) if away[i] else 'n/a (at pi)'))
    print('batch prepare B %2d: worst %.2f x bound; vector worst %.2f x 2^-23 pi over %d samples away from pi'
          % (B, (err / bound).max(), (verr[away] / (2.0 ** -23 * np.pi)).max() if away.any() else 0.0, away.sum()))
    assert (err <= bound).all()
    assert (verr[away] <= 2.0 ** -23 * np.pi).all()
    if B == 65:
        assert not away[3:8].any() and away[[0, 1, 2, 8]].all()                           # the families are what they claim to be
        assert abs(angle[3] - (np.pi - 1e-4)) < 1e-6 and angle[2] < 1e-6 and (np.abs(angle[4:8] - np.pi) < 1e-6).all()
    want = br.mean_shape_rule(betas)
    assert np.array_equal(bits(bout), bits(want))
    if B == 65:
        assert np.array_equal(bits(bout[0]), bits(betas[0])) and not bout[1].any() and not bout[2].any() and np.isnan(bout[3, 0])


def test_prepare_null_rotation_in_place_and_poison():
    pose, R, betas = prepare_case()
    out, bout = run_prepare(pose, None, betas)
    assert np.array_equal(bits(out), bits(pose))                                          # R == NULL: the whole pose, bit for bit
    out2, _ = run_prepare(pose, None, None)
    assert np.array_equal(bits(out2), bits(pose))
    ref, bref = run_prepare(pose, R, betas)
    inp, binp = run_prepare(pose, R, betas, inplace=True)
    assert np.array_equal(bits(inp), bits(ref)) and np.array_equal(bits(binp), bits(bref))
    for B, first in ((1, 3), (2, 3)):                                                     # a sample's row is the same bits in any batch
        o, b = run_prepare(pose[first:first + B], R[first:first + B], betas[first:first + B])
        assert np.array_equal(bits(o), bits(ref[first:first + B])) and np.array_equal(bits(b), bits(bref[first:first + B]))
    bad = pose.copy()
    bad[5, 1] = np.nan                                                                    # in the root
    bad[6, 40] = np.nan                                                                   # in another joint: copied, the root still computed
    bad[7, 2] = np.inf
    Rb = R.copy()
    Rb[8, 1, 1] = np.nan
    o, _ = run_prepare(bad, Rb, betas)
    assert np.isnan(o[[5, 7, 8], :3]).all()
    assert np.array_equal(bits(o[5, 3:]), bits(bad[5, 3:])) and np.array_equal(bits(o[6]), bits(np.concatenate([ref[6, :3], bad[6, 3:]])))
    keep = np.setdiff1d(np.arange(65), [5, 6, 7, 8])
    assert np.array_equal(bits(o[keep]), bits(ref[keep]))


def test_root_to_camera_is_the_kernel():
    pose, R, betas = prepare_case()
    ref, _ = run_prepare(pose, R, None)
    assert np.array_equal(bits(batch.root_to_camera(dev(pose), dev(R)).cpu().numpy()), bits(ref))
    one = batch.root_to_camera(dev(pose), dev(R[11]))                                    # one camera for the batch
    want, _ = run_prepare(pose, np.broadcast_to(R[11], R.shape), None)
    assert np.array_equal(bits(one.cpu().numpy()), bits(want))


# ---- k_camera_targets -----------------------------------------------------------------------------------------------------------------

def coo_of(c, which, nv):
    row, col, val, dense = c[which + '_coo']
    return gator_eval._Coo(row, col, val, dense.shape[0], nv, 'cuda', 'test')


def target_tensors(c, sl=slice(None), inplace=False, **kw):
    """The argument tuple of batch._launch_camera_targets for the samples c[sl], and the dict of its output tensors."""
    a = dict(trans=c['trans'], cam_t=c['cam_t'], R=None, compensate_root=False, joint_cam=c['joint_cam'], joint_img=c['joint_img'],
             rot_deg=c['rot_deg'], flip=c['flip'], flip_pairs=c['flip_pairs'], lift_set=c['lift_set'], fitting_thr=np.inf)
    a.update(kw)
    d = lambda x, dt=torch.float32: None if x is None else dev(np.asarray(x)[sl], dt)  # noqa: E731
    verts, joints = d(c['verts']), d(c['joints'])
    B, nv = verts.shape[:2]
    coco = a['lift_set'] == 'coco'
    reg_h, reg_c = coo_of(c, 'reg_h36m', nv), coo_of(c, 'reg_coco', nv) if coco else None
    Jh = reg_h.n_joint
    Jl = reg_c.n_joint + 2 if coco else Jh
    e = lambda *s: torch.full(s, -7.0, device='cuda')  # noqa: E731
    out = {'mesh': verts if inplace else e(B, nv, 3), 'reg_pose3d': e(B, Jh, 3), 'lift_pose3d': e(B, Jl, 3), 'joint_img': e(B, Jl, 2),
           'fit_error': e(B), 'valid': e(B, 3)}
    pairs = dev(np.asarray(a['flip_pairs'], np.int32).reshape(-1, 2), torch.int32) if len(a['flip_pairs']) else None
    ji = a['joint_img']
    args = (verts, joints, d(a['trans']), d(a['cam_t']), d(a['R']), a['compensate_root'], d(c['focal']), d(c['princpt']), reg_h, reg_c,
            batch.LIFT_SETS[a['lift_set']], d(a['joint_cam']), None if ji is None else d(np.asarray(ji)[:, :, :2]), d(a['rot_deg']),
            d(a['flip'], torch.int32), pairs, float(a['fitting_thr']), 0) + tuple(out[k] for k in OUT_KEYS)
    return args, out


def run_targets(c, sl=slice(None), inplace=False, **kw):
    args, out = target_tensors(c, sl, inplace, **kw)
    batch._launch_camera_targets(*args)
    return {k: t.cpu().numpy() for k, t in out.items()}


def check(got, ref, tol, sl, label):
    """Every element of every output: finite references within the bound, non-finite ones (Z = 0, an empty row's 0 / 0) the same IEEE
    value; the masks exactly.  Prints the worst multiple of the bound per output."""
    worst = {}
    for k in OUT_KEYS:
        g, r = got[k].astype(np.float64), ref[k][sl]
        assert g.shape == r.shape, (label, k, g.shape, r.shape)
        if k == 'valid':
            assert np.array_equal(g, r), (label, k)
            continue
        fin = np.isfinite(r)
        assert np.array_equal(np.isnan(g), np.isnan(r)), (label, k)
        assert np.array_equal(g[~fin & ~np.isnan(r)], r[~fin & ~np.isnan(r)]), (label, k)          # the infinities, with their signs
        with np.errstate(invalid='ignore'):
            err, t = np.abs(g - r)[fin], tol[k][sl][fin]
        worst[k] = float(np.max(np.where(t > 0, err / np.where(t > 0, t, 1), np.where(err > 0, np.inf, 0.0)))) if err.size else 0.0
        assert (err <= t).all(), (label, k, worst[k])
    print('camera targets %-44s worst error / bound: %s' % (label, '  '.join('%s %.3f' % (k, v) for k, v in worst.items())))
    return worst


@functools.lru_cache(maxsize=None)
def ccase(nv, lift_set, dataset_joints, special=True):
    return br.camera_case(nv, 65, 900 + nv, lift_set, dataset_joints, special)


def compare(c, label, sl=slice(None), **kw):
    ref = br.reference_of(c, **kw)
    coco = kw.get('lift_set', c['lift_set']) == 'coco'
    has_img = kw.get('joint_img', c['joint_img']) is not None
    tol = br.tolerances(ref, c['focal'], coco or not has_img)
    got = run_targets(c, sl, **kw)
    check(got, ref, tol, sl, label)
    return got, ref


@pytest.mark.parametrize('nv', [3, 255, 256, 257])
@pytest.mark.parametrize('lift_set', ['human36', 'coco'])
@pytest.mark.parametrize('dataset_joints', [False, True])
def test_targets_against_fp64(nv, lift_set, dataset_joints):
    """Both lift sets, with and without the dataset's joints, the translation compensated and not, rot in {0, 30, -90} x flip in {0, 1}
    over the batch; regressors with an empty row, a duplicated row and a negative weight; B = 65, 2 and 1."""
    c = ccase(nv, lift_set, dataset_joints)
    assert {(float(r), int(f)) for r, f in zip(c['rot_deg'], c['flip'])} == {(r, f) for r in (0.0, 30.0, -90.0) for f in (0, 1)}
    tag = 'nv %d %s ds %d' % (nv, lift_set, dataset_joints)
    got, ref = compare(c, tag + ' plain', fitting_thr=25.0)
    compare(c, tag + ' compensated', R=c['R'], compensate_root=True, fitting_thr=25.0)
    compare(c, tag + ' B 2', slice(7, 9), fitting_thr=25.0)
    compare(c, tag + ' B 1', slice(64, 65), R=c['R'], compensate_root=True)
    # rot and flip touch the lifter's target only: without them the mesh, the regressor's target and the pixels are the same bits
    still = run_targets(c, rot_deg=None, flip=None, fitting_thr=25.0)
    for k in ('mesh', 'reg_pose3d', 'joint_img', 'fit_error', 'valid'):
        assert np.array_equal(bits(still[k]), bits(got[k])), k
    assert not np.array_equal(still['lift_pose3d'][1], got['lift_pose3d'][1])


@pytest.mark.parametrize('missing', ['trans', 'cam_t', 'both', 'trans_compensated', 'cam_t_compensated', 'R_given_not_used'])
def test_translation_terms_missing_one_at_a_time(missing):
    c = ccase(257, 'coco', False)
    kw = {'trans': dict(trans=None), 'cam_t': dict(cam_t=None), 'both': dict(trans=None, cam_t=None),
          'trans_compensated': dict(trans=None, R=c['R'], compensate_root=True),
          'cam_t_compensated': dict(cam_t=None, R=c['R'], compensate_root=True), 'R_given_not_used': dict(R=c['R'])}[missing]
    if missing == 'both':                                  # nothing puts the body in front of the camera: Z straddles 0, all finite or IEEE
        kw['rot_deg'] = None
    compare(c, 'missing ' + missing, slice(0, 9), **kw)


def point_row(coo, j, v):
    """The regressor with row j replaced by two entries of weight 1/2 on vertex v."""
    row, col, val, dense = coo
    keep = row != j
    row, col, val = np.append(row[keep], [j, j]), np.append(col[keep], [v, v]), np.append(val[keep], np.float32([0.5, 0.5]))
    dense = dense.copy()
    dense[j] = 0
    dense[j, v] = 1.0
    return row, col, val, dense


@pytest.mark.parametrize('lift_set', ['human36', 'coco'])
def test_z_zero_and_z_negative_are_ieee_and_local(lift_set):
    """Sample 0: joint 7 sits on a vertex with Z = 0 exactly (x / 0 = +-inf); joint 9 / 3 is an empty row (0 / 0 = NaN); sample 1: the
    whole body behind the camera (Z < 0, finite pixels).  The other samples are the bits of a batch without them."""
    c = dict(ccase(257, lift_set, False))
    c['verts'], c['trans'] = c['verts'].copy(), (c['trans'] + np.float32([0, 0, 4.5])).astype(np.float32)
    for k in ('reg_h36m', 'reg_coco'):
        c[k + '_coo'] = point_row(c[k + '_coo'], 7, 0)
        c[k] = c[k + '_coo'][3]
    base = run_targets(c, slice(0, 9), cam_t=None)
    c['verts'][0, 0, 2] = -c['trans'][0, 2]
    c['trans'][1, 2] = np.float32(-4.5)
    got, ref = compare(c, 'Z = 0, Z < 0 ' + lift_set, slice(0, 9), cam_t=None)
    assert np.isinf(got['joint_img'][0, 7]).all() and np.isnan(got['joint_img'][0, 3 if lift_set == 'coco' else 9]).all()
    z1 = ref['joint_cam_abs'][1][:, 2]
    assert (z1[z1 != 0] < 0).all() and np.isfinite(got['joint_img'][1][z1 != 0]).all()
    assert np.isfinite(got['mesh']).all() and np.isfinite(got['lift_pose3d']).all()
    for k in OUT_KEYS:
        assert np.array_equal(bits(got[k][2:]), bits(base[k][2:])), k


def test_fitting_gate():
    """Convex rows only: a row that does not sum to 1 is not a joint of the mesh and its error is hundreds of mm (those rows are
    checked, far beyond the threshold, in test_targets_against_fp64)."""
    for lift_set in ('human36', 'coco'):
        c = ccase(256, lift_set, True, False)
        thr = 25.0
        ref = br.reference_of(c, fitting_thr=thr)
        e = ref['fit_error']
        assert (np.abs(e - thr) > 1e-6 * thr).all() and (e > thr).sum() >= 5 and (e < thr).sum() >= 5          # a condition on the inputs
        got, _ = compare(c, 'gate %s thr 25' % lift_set, fitting_thr=thr)
        far = e > thr
        assert np.array_equal(got['valid'][:, 0], np.where(far, 0, 1)) and (got['valid'][:, 2] == 1).all()
        assert np.array_equal(got['valid'][:, 1], np.where(far, 0, 1) if lift_set == 'coco' else np.ones(65))
        got, _ = compare(c, 'gate %s thr inf' % lift_set, fitting_thr=np.inf)
        assert (got['valid'] == 1).all() and np.isfinite(got['fit_error']).all()
        got, _ = compare(c, 'gate %s thr 0' % lift_set, fitting_thr=0.0)
        assert (got['valid'][:, 0] == 0).all()
        c2 = ccase(256, lift_set, False)
        got, _ = compare(c2, 'gate %s no dataset joints' % lift_set, fitting_thr=0.0)
        assert (got['valid'] == 1).all() and np.isnan(got['fit_error']).all()
    # the dataset's joint_cam with the coco lift set needs no joint_img
    c = ccase(256, 'coco', True, False)
    compare(c, 'gate coco, joint_cam without joint_img', slice(0, 4), joint_img=None, fitting_thr=25.0)


def test_fullsize_mesh():
    c = br.camera_case(6890, 3, 6890, 'coco', True, special=True)
    compare(c, 'nv 6890 coco ds compensated', R=c['R'], compensate_root=True, fitting_thr=25.0)
    c = br.camera_case(6890, 2, 6891, 'human36', False, special=True)
    compare(c, 'nv 6890 human36', fitting_thr=25.0)


@pytest.mark.parametrize('lift_set,dataset_joints', [('human36', True), ('coco', False)])
def test_batch_invariance_in_place_poison_and_replay(lift_set, dataset_joints):
    c = ccase(257, lift_set, dataset_joints)
    kw = dict(R=c['R'], compensate_root=True, fitting_thr=25.0)
    full = run_targets(c, **kw)
    for sl in (slice(5, 6), slice(5, 7)):                                                 # B = 1 and 2 against B = 65
        part = run_targets(c, sl, **kw)
        for k in OUT_KEYS:
            assert np.array_equal(bits(part[k]), bits(full[k][sl])), (k, sl)
    inp = run_targets(c, inplace=True, **kw)                                              # mesh == verts
    for k in OUT_KEYS:
        assert np.array_equal(bits(inp[k]), bits(full[k])), k
    bad = dict(c)
    bad['verts'] = c['verts'].copy()
    bad['verts'][4, 100, 1] = np.nan
    got = run_targets(bad, **kw)
    keep = np.arange(65) != 4
    for k in OUT_KEYS:
        assert np.array_equal(bits(got[k][keep]), bits(full[k][keep])), k
    assert np.isnan(got['mesh'][4, 100, 1]) and got['valid'][4, 2] == 1
    if dataset_joints:                                     # a NaN error is not above the threshold: the masks stay ones
        assert full['valid'][4, 0] == 0
        jc = c['joint_cam'].copy()
        jc[4, 3, 0] = np.nan
        got = run_targets(c, joint_cam=jc, **kw)
        assert np.isnan(got['fit_error'][4]) and (got['valid'][4] == 1).all()
        for k in OUT_KEYS:
            assert np.array_equal(bits(got[k][keep]), bits(full[k][keep])), k
    # capture and replay: the eager bits
    args, out = target_tensors(c, **kw)
    pose, R, betas = prepare_case()
    p, r, b = dev(pose), dev(R), dev(betas)
    po, bo = torch.full_like(p, -7.0), torch.full_like(b, -7.0)
    eager_p, eager_b = run_prepare(pose, R, betas)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        batch._launch_prepare(p, r, b, 0, po, bo)
        batch._launch_camera_targets(*args)
    for t in list(out.values()) + [po, bo]:
        t.fill_(-3.0)
    g.replay()
    torch.cuda.synchronize()
    for k in OUT_KEYS:
        assert np.array_equal(bits(out[k].cpu().numpy()), bits(full[k])), k
    assert np.array_equal(bits(po.cpu().numpy()), bits(eager_p)) and np.array_equal(bits(bo.cpu().numpy()), bits(eager_b))


def test_empty_batch_and_every_einval():
    lib = _lib.load()
    c = ccase(256, 'coco', True)
    args, out = target_tensors(c, slice(0, 2), R=c['R'], compensate_root=True)
    call = lambda a: lib.gator_camera_targets_f32(ctypes.byref(a), stream())  # noqa: E731
    make = lambda: batch._camera_targets_args(*args)  # noqa: E731
    assert call(make()) == 0
    torch.cuda.synchronize()
    before = {k: t.clone() for k, t in out.items()}

    def refused(text, **fields):
        a = make()
        for k, v in fields.items():
            setattr(a, k, v)
        assert call(a) == EINVAL, fields
        assert text in lib.gator_last_error().decode(), (fields, lib.gator_last_error().decode())

    assert lib.gator_camera_targets_f32(None, stream()) == EINVAL and 'null args' in lib.gator_last_error().decode()
    refused('struct_size', struct_size=8)
    for name in ('verts', 'focal', 'princpt', 'joints', 'mesh', 'reg_pose3d', 'lift_pose3d', 'joint_img_out', 'fit_error', 'valid'):
        refused('null', **{name: None})
    refused('n_verts', n_verts=0)
    refused('reg_h36m over', reg_h36m_n_verts=255)
    refused('reg_coco over', reg_coco_n_verts=257)
    empty = _lib.GatorCoo(None, None, None, 0, 0)
    refused('coco without reg_coco', reg_coco=empty)
    a = make()
    short = _lib.GatorCoo(a.reg_coco.row, a.reg_coco.col, a.reg_coco.val, 0, 12)
    refused('reg_coco', reg_coco=short)
    refused('reg_coco', reg_coco=_lib.GatorCoo(a.reg_coco.row, a.reg_coco.col, a.reg_coco.val, 0, 63))
    refused('reg_h36m', reg_h36m=_lib.GatorCoo(a.reg_h36m.row, a.reg_h36m.col, a.reg_h36m.val, 0, 65))
    refused('reg_h36m', reg_h36m=_lib.GatorCoo(None, a.reg_h36m.col, a.reg_h36m.val, 5, 17))
    refused('joint_cam without', lift_set=_lib.LIFT_HUMAN36, joint_img=None)
    refused('compensate_root without R', R=None)
    refused('root_idx', root_idx=24)
    refused('root_idx', root_idx=-1)
    refused('lift_set', lift_set=2)
    refused('batch', batch=-1)
    refused('n_pairs', flip_pairs=None)
    torch.cuda.synchronize()
    for k, t in out.items():
        assert torch.equal(t.view(torch.int32), before[k].view(torch.int32)), k           # no refused call launched anything
    # batch == 0: GATOR_OK, nothing launched, no pointer looked at
    a = make()
    a.batch = 0
    for name in ('verts', 'mesh', 'focal'):
        setattr(a, name, None)
    assert call(a) == 0
    z = torch.empty((0, 72), device='cuda')
    assert lib.gator_batch_prepare_f32(z.data_ptr(), None, None, 0, 72, 0, 0, z.data_ptr(), None, stream()) == 0
    p = torch.zeros((2, 72), device='cuda')
    for bad in ((None, None, None, 2, 72, 0, 0, p.data_ptr(), None), (p.data_ptr(), None, None, 2, 72, 0, 0, None, None),
                (p.data_ptr(), None, None, 2, 71, 0, 0, p.data_ptr(), None), (p.data_ptr(), None, None, 2, 72, 0, 24, p.data_ptr(), None),
                (p.data_ptr(), None, None, 2, 72, 0, -1, p.data_ptr(), None), (p.data_ptr(), None, p.data_ptr(), 2, 72, 10, 0, p.data_ptr(), None),
                (p.data_ptr(), None, p.data_ptr(), 2, 72, 0, 0, p.data_ptr(), p.data_ptr()), (p.data_ptr(), None, None, -1, 72, 0, 0, p.data_ptr(), None)):
        assert lib.gator_batch_prepare_f32(*bad, stream()) == EINVAL, bad
        assert 'gator_batch_prepare_f32' in lib.gator_last_error().decode()
    torch.cuda.synchronize()
    assert not p.any()


# ---- camera_frame_batch, end to end ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def e2e_setup():
    """The 6890-vertex golden model of the layer's tests (its float32 spread is recorded), three samples, stand-in regressors."""
    from tests.test_gpu_smpl import case, make_layer
    c = case('nv6890')
    rs = np.random.RandomState(78)
    B = 3
    pose, betas, trans = (a[:B].copy() for a in c.np_in)
    betas[1, 4] = 3.5
    h = br.sparse_regressor(17, 6890, rs)
    k = br.sparse_regressor(17, 6890, rs)
    R = Rotation.from_rotvec(rs.randn(B, 3) * 0.6).as_matrix().astype(np.float32)
    cam_t = (rs.randn(B, 3) * 0.3 + np.array([0, 0, 5.0])).astype(np.float32)
    focal, princpt = np.float32([[1145.0, 1143.8]] * B), np.float32([[512.5, 515.4]] * B)
    return c, make_layer(c.m), pose, betas, trans, R, cam_t, focal, princpt, h, k


def full_chain(c, pose, betas, trans, R, cam_t, focal, princpt, h, k, lift_set, compensate, rot, flip, pairs, joint_cam=None, joint_img=None, thr=np.inf):
    p64 = pose.astype(np.float64) if R is None else br.root_to_camera(pose, R)[0]
    v, j = sr.lbs_forward(c.m, p64, br.mean_shape_rule(betas.astype(np.float64)), None)
    return br.camera_targets(v, j, focal, princpt, h[3], k[3], lift_set, trans, cam_t, R, compensate, joint_cam, joint_img, rot, flip, pairs, thr), v


@pytest.mark.parametrize('lift_set', ['human36', 'coco'])
def test_camera_frame_batch_end_to_end(lift_set):
    c, layer, pose, betas, trans, R, cam_t, focal, princpt, h, k = e2e_setup()
    B = 3
    pairs = br.COCO_FLIP_PAIRS if lift_set == 'coco' else br.H36M_FLIP_PAIRS
    rot, flip = np.float32([0.0, 30.0, -90.0]), np.int32([1, 0, 1])
    regs = [gator_eval._Coo(*x[:3], 17, 6890, 'cuda', 'test') for x in (h, k)]
    # dataset joints near the fp64 chain's regressed ones
    ref0, _ = full_chain(c, pose, betas, trans, R, cam_t, focal, princpt, h, k, lift_set, True, rot, flip, pairs)
    rs = np.random.RandomState(3)
    jc = (h[3] @ ref0['mesh_cam'] + rs.randn(B, 17, 3) * np.array([5.0, 20.0, 40.0])[:, None, None]).astype(np.float32)
    ji = np.stack([br.cam2pixel(jc[b].astype(np.float64), focal[b], princpt[b])[:, :2] for b in range(B)]).astype(np.float32)
    kw = dict(trans=dev(trans), cam_R=dev(R), cam_t=dev(cam_t), compensate_root=True, focal=dev(focal), princpt=dev(princpt[0]),
              regressor_h36m=regs[0], regressor_coco=regs[1], input_joint_name=lift_set, joint_cam=dev(jc), joint_img=dev(ji),
              fitting_thr=25.0, rot_deg=dev(rot), flip=dev(flip, torch.int32), flip_pairs=pairs)
    inputs, targets, meta = batch.camera_frame_batch(layer, dev(pose), dev(betas), **kw)
    assert layer.out_scale == 1.0 and layer.center_idx is None
    Jl = 19 if lift_set == 'coco' else 17
    # the reference's triple: keys and shapes (data/Human36M/dataset.py:403-405)
    assert sorted(inputs) == ['pose2d'] and sorted(targets) == ['lift_pose3d', 'mesh', 'reg_pose3d']
    assert {'mesh_valid', 'lift_pose3d_valid', 'reg_pose3d_valid'} <= set(meta) and set(meta) - {'mesh_valid', 'lift_pose3d_valid', 'reg_pose3d_valid'} == {'fit_error', 'input_valid', 'joint_img'}
    shapes = {'pose2d': (B, Jl, 2), 'mesh': (B, 6890, 3), 'lift_pose3d': (B, Jl, 3), 'reg_pose3d': (B, 17, 3), 'mesh_valid': (B, 6890, 1),
              'lift_pose3d_valid': (B, Jl, 1), 'reg_pose3d_valid': (B, 17, 1), 'fit_error': (B,), 'input_valid': (B,), 'joint_img': (B, Jl, 2)}
    for k_, s in shapes.items():
        t = {**inputs, **targets, **meta}[k_]
        assert tuple(t.shape) == s and t.is_cuda, k_
    for k_ in ('mesh_valid', 'lift_pose3d_valid', 'reg_pose3d_valid'):
        assert meta[k_].stride(1) == 0 and meta[k_].dtype == torch.float32             # broadcast views, not materialised
    # bit-equal to the three stages by hand
    p, b_ = dev(pose), dev(betas)
    pc, bc = batch._launch_prepare(p, dev(R), b_, 0, torch.empty_like(p), torch.empty_like(b_))
    verts, joints = layer(pc, bc, None)
    o = {'reg': torch.empty(B, 17, 3, device='cuda'), 'lift': torch.empty(B, Jl, 3, device='cuda'), 'img': torch.empty(B, Jl, 2, device='cuda'),
         'fit': torch.empty(B, device='cuda'), 'valid': torch.empty(B, 3, device='cuda'), 'mesh': torch.empty_like(verts)}
    batch._launch_camera_targets(verts, joints, dev(trans), dev(cam_t), dev(R), True, dev(focal), dev(np.broadcast_to(princpt[0], (B, 2))), regs[0],
                                 regs[1] if lift_set == 'coco' else None, batch.LIFT_SETS[lift_set], dev(jc), dev(ji), dev(rot), dev(flip, torch.int32),
                                 dev(np.asarray(pairs, np.int32), torch.int32), 25.0, 0, o['mesh'], o['reg'], o['lift'], o['img'], o['fit'], o['valid'])
    assert torch.equal(targets['mesh'], o['mesh']) and torch.equal(targets['reg_pose3d'], o['reg']) and torch.equal(targets['lift_pose3d'], o['lift'])
    assert torch.equal(meta['joint_img'], o['img']) and torch.equal(meta['fit_error'], o['fit'])
    assert torch.equal(meta['mesh_valid'][:, 0, 0], o['valid'][:, 0]) and torch.equal(meta['lift_pose3d_valid'][:, 0, 0], o['valid'][:, 1])
    p2d, ok = preprocess.preprocess_chain(meta['joint_img'], dev(rot), dev(flip, torch.int32), pairs, res=(288, 384))
    assert torch.equal(inputs['pose2d'], p2d) and torch.equal(meta['input_valid'], ok) and torch.isfinite(p2d).all()
    # against the full fp64 chain
    ref, v64 = full_chain(c, pose, betas, trans, R, cam_t, focal, np.broadcast_to(princpt[0], (B, 2)), h, k, lift_set, True, rot, flip, pairs, jc, ji, 25.0)
    R64 = R.astype(np.float64)
    defect = np.linalg.norm(np.swapaxes(R64, 1, 2) @ R64 - np.eye(3), axis=(1, 2)).max()
    reach = np.linalg.norm(v64, axis=2).max()                                            # metres from the model's origin, about which the root turns
    tol = 3e3 * c.spread_v + 10 * 2.0 ** -24 * np.abs(ref['mesh_cam']).max() + 1000 * (ROUND3 + defect) * reach
    got = {'mesh': targets['mesh'], 'reg_pose3d': targets['reg_pose3d'], 'lift_pose3d': targets['lift_pose3d'], 'fit_error': meta['fit_error']}
    for k_, t in got.items():
        err = np.abs(t.cpu().numpy() - ref[k_]).max()
        bound = tol / 1000 if k_ == 'mesh' else (2 * tol if k_ == 'lift_pose3d' else tol)
        print('camera_frame_batch %-8s %-12s err %.3e bound %.3e' % (lift_set, k_, err, bound))
        assert err <= bound, k_
    if lift_set == 'coco':
        P = ref['joint_cam_abs']
        gain = (focal[:, None, :] * (1 + np.abs(P[:, :, :2] / P[:, :, 2:])) / np.abs(P[:, :, 2:]))
        err = np.abs(meta['joint_img'].cpu().numpy() - ref['joint_img'])
        bound = tol * gain + 2.0 ** -23 * np.abs(ref['joint_img'])
        print('camera_frame_batch %-8s joint_img     worst err / bound %.3f' % (lift_set, (err / bound).max()))
        assert (err <= bound).all()
    else:
        assert torch.equal(meta['joint_img'], dev(ji))
    far = ref['fit_error'] > 25.0
    assert (np.abs(ref['fit_error'] - 25.0) > tol).all() and far.any() and not far.all()
    assert np.array_equal(meta['mesh_valid'][:, 0, 0].cpu().numpy(), np.where(far, 0, 1))


@pytest.mark.parametrize('lift_set', ['human36', 'coco'])
def test_camera_frame_batch_agrees_with_targets_from_smpl(lift_set):
    """No R, no rotation, no flip, no dataset joints: the configuration the parent's targets_from_smpl can express."""
    c, layer, pose, betas, trans, R, cam_t, focal, princpt, h, k = e2e_setup()
    jr = [gator_eval.JointRegressor(x[3].astype(np.float32), 'cuda') for x in (h, k)]
    inputs, targets, meta = batch.camera_frame_batch(layer, dev(pose), dev(betas), trans=dev(trans), focal=dev(focal), princpt=dev(princpt),
                                                     regressor_h36m=jr[0], regressor_coco=jr[1], input_joint_name=lift_set)
    old = smpl.targets_from_smpl(layer, dev(pose), dev(betas), dev(trans), jr[0], jr[1], input_joint_name=lift_set)
    ref, _ = full_chain(c, pose, betas, trans, None, None, focal, princpt, h, k, lift_set, False, None, None, ())
    tol = 3e3 * c.spread_v + 10 * 2.0 ** -24 * np.abs(ref['mesh_cam']).max()
    for k_ in ('mesh', 'reg_pose3d', 'lift_pose3d'):
        t = tol / 1000 if k_ == 'mesh' else tol
        new, par = targets[k_].cpu().numpy(), old[k_].cpu().numpy()
        e_new, e_old, e_diff = np.abs(new - ref[k_]).max(), np.abs(par - ref[k_]).max(), np.abs(new.astype(np.float64) - par).max()
        print('camera_frame_batch vs targets_from_smpl %-8s %-12s new-fp64 %.3e parent-fp64 %.3e new-parent %.3e bound %.3e' % (lift_set, k_, e_new, e_old, e_diff, t))
        assert e_new <= t and e_diff <= t, k_
    assert (meta['mesh_valid'] == 1).all() and torch.isnan(meta['fit_error']).all() and (meta['input_valid'] == 1).all()
    # the same through a dense array and a _Coo
    again = batch.camera_frame_batch(layer, dev(pose), dev(betas), trans=dev(trans), focal=dev(focal[0]), princpt=dev(princpt[0]),
                                     regressor_h36m=h[3].astype(np.float32), regressor_coco=gator_eval._Coo.from_dense(k[3].astype(np.float32), 'cuda'),
                                     input_joint_name=lift_set)
    assert torch.equal(again[1]['mesh'], targets['mesh']) and torch.equal(again[0]['pose2d'], inputs['pose2d'])
