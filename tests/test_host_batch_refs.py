"""CPU checks of the camera-frame batch (-m "not gpu"): tests/batch_refs.py against the reference's own functions
(tests/golden/train_batch.npz, tools/gen_golden_batch.py) and against scipy; the float32-literal chain against the float64 one (printed:
the reference's own noise, shown in profiles/train_batch.txt beside the device's errors, not used as a bound); every host-side refusal
of gator_amd.batch; the build list and the two signatures."""
import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

from gator_amd import _lib, batch, build
from tests import batch_refs as br
from tests.helpers import load_golden


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def test_restatement_equals_the_reference_functions():
    z = load_golden('train_batch')
    cam, f, c = z['cam'], z['focal'], z['princpt']
    assert cam[3, 2] == 0 and cam[4, 2] < 0
    got = br.cam2pixel(cam, f, c)
    assert same(got, z['cam2pixel'])                                                      # float64, bit for bit, the IEEE specials included
    assert np.isinf(got[3, :2]).all() and np.isfinite(got[4]).all()
    assert same(br.cam2pixel(cam.astype(np.float32), f.astype(np.float32), c.astype(np.float32)), z['cam2pixel_f32'])
    assert same(br.world2cam(cam, z['R'], z['t']), z['world2cam'])
    for name, pairs in (('h36m', br.H36M_FLIP_PAIRS), ('coco', br.COCO_FLIP_PAIRS)):
        S = z['S_' + name]
        assert same(br.flip_3d_joint(S, pairs), z['flip3d_' + name])
        for r in z['rots']:
            for fl in z['flips']:
                want = z['j3d_%s_%g_%d' % (name, r, fl)]
                assert same(br.j3d_processing(S, float(r), int(fl), pairs).astype(np.float32), want), (name, r, fl)
    assert same(br.j3d_processing(z['S_h36m'], 0.0, 0, ()), z['S_h36m'])                  # rot 0, no flip: the identity, exactly


def rodrigues(r):
    """exp of one rotation vector, the closed form, written out here: a second route beside scipy's."""
    t = np.linalg.norm(r)
    if t == 0:
        return np.eye(3)
    k = r / t
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def test_root_rotation_restatement_against_scipy_and_the_closed_form():
    rs = np.random.RandomState(5)
    B = 64
    pose = rs.randn(B, 72) * 0.5
    pose[0, :3] = 0.0                                                                     # zero root: the identity, not NaN
    pose[1, :3] = pose[1, :3] / np.linalg.norm(pose[1, :3]) * 1e-8
    pose[2, :3] = pose[2, :3] / np.linalg.norm(pose[2, :3]) * 5.0
    R = Rotation.from_rotvec(rs.randn(B, 3)).as_matrix()
    R[3] = np.diag([1.0, -1.0, -1.0])
    R[4] = br.exp_rotvec(pose[4, :3]).T                                                   # the product is the identity
    out, M = br.root_to_camera(pose, R)
    assert np.array_equal(out[:, 3:], pose[:, 3:])
    for b in range(B):
        assert np.abs(M[b] - R[b] @ rodrigues(pose[b, :3])).max() <= 1e-14
        assert np.abs(rodrigues(out[b, :3]) - M[b]).max() <= 1e-12
    ang = np.linalg.norm(out[:, :3], axis=1)
    assert (ang >= 0).all() and (ang <= np.pi + 1e-15).all()
    assert np.abs(out[0, :3] - Rotation.from_matrix(R[0]).as_rotvec()).max() <= 1e-15
    assert np.abs(out[4, :3]).max() <= 1e-15
    b = np.array([[3.0, -3.0, 0.5], [3.0000002, 0.0, 0.0], [0.0, -3.5, 1.0], [np.nan, 0.0, 0.0]], np.float32)
    want = b.copy()
    want[1:3] = 0
    assert np.array_equal(br.mean_shape_rule(b), want, equal_nan=True)                    # +-3 kept, beyond zeroed, a NaN row kept


@pytest.mark.parametrize('lift_set', ['human36', 'coco'])
@pytest.mark.parametrize('dataset_joints', [False, True])
def test_float32_literal_chain_against_float64(lift_set, dataset_joints):
    """The reference's own float32 noise on a 6890-vertex case with a compensated translation; printed, not asserted beyond sanity."""
    c = br.camera_case(6890, 4, 31, lift_set, dataset_joints, special=False)
    kw = dict(R=c['R'], compensate_root=True, fitting_thr=25.0)
    r64, r32 = br.reference_of(c, **kw), br.reference_of(c, fn=br.camera_targets_f32, **kw)
    tol = br.tolerances(r64, c['focal'], lift_set == 'coco' or not dataset_joints)
    for k in ('mesh', 'reg_pose3d', 'lift_pose3d', 'joint_img', 'fit_error'):
        err = np.abs(r32[k].astype(np.float64) - r64[k])
        with np.errstate(divide='ignore', invalid='ignore'):
            ratio = np.nanmax(np.where(tol[k] > 0, err / tol[k], 0.0)) if np.isfinite(err).any() else float('nan')
        print('train_batch float32-literal %-8s ds=%d %-12s max |f32 - f64| %.3e = %.1f x the device bound' % (lift_set, dataset_joints, k, np.nanmax(err) if np.isfinite(err).any() else np.nan, ratio))
        assert r32[k].shape == r64[k].shape
    assert np.abs(r32['mesh'].astype(np.float64) - r64['mesh']).max() < 1e-5              # metres: sanity, far above float32 noise at ~5 m
    assert np.array_equal(r32['valid'], r64['valid'])


class StubLayer:
    """What camera_frame_batch reads of a layer before any device work."""
    num_verts, num_joints, num_betas, out_scale, center_idx = 5, 24, 10, 1.0, None

    def forward(self, *a, **k):
        raise AssertionError('the layer must not run: the inputs are refused first')


def good():
    rs = np.random.RandomState(0)
    B = 2
    t = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32))  # noqa: E731
    return dict(layer=StubLayer(), pose=t(B, 72), shape=t(B, 10), trans=t(B, 3), cam_R=torch.eye(3).repeat(B, 1, 1), cam_t=t(B, 3),
                focal=torch.tensor([1000.0, 1000.0]), princpt=t(B, 2), regressor_h36m=np.abs(rs.randn(17, 5)).astype(np.float32),
                regressor_coco=np.abs(rs.randn(17, 5)).astype(np.float32), input_joint_name='coco', joint_cam=t(B, 17, 3), joint_img=t(B, 17, 3),
                fitting_thr=25.0, rot_deg=t(B), flip=torch.tensor([0, 1]), flip_pairs=((1, 2), (17, 18)), res=(288, 384))


def call(**kw):
    a = good()
    a.update(kw)
    return batch.camera_frame_batch(a.pop('layer'), a.pop('pose'), a.pop('shape'), **a)


REFUSALS = [
    (dict(layer=object()), 'SMPLLayer'),
    (dict(pose=torch.zeros(2, 71)), 'pose must be'),
    (dict(pose=torch.zeros(2, 72, dtype=torch.int64)), 'pose must be'),
    (dict(pose=np.zeros((2, 72), np.float32)), 'pose must be a tensor'),
    (dict(pose=torch.zeros(0, 72)), 'pose must be'),
    (dict(input_joint_name='smpl'), "'coco' or 'human36'"),
    (dict(regressor_coco=None), 'needs regressor_coco'),
    (dict(compensate_root=True, cam_R=None), 'compensate_root needs cam_R'),
    (dict(regressor_h36m=None), 'regressor_h36m is required'),
    (dict(shape=torch.zeros(2, 9)), 'shape must be'),
    (dict(trans=torch.zeros(2, 4)), 'trans must be'),
    (dict(cam_t=torch.zeros(3)), 'cam_t must be'),
    (dict(cam_R=torch.zeros(2, 9)), 'cam_R must be'),
    (dict(cam_R=torch.zeros(2, 3, 3, dtype=torch.int32)), 'floating-point'),
    (dict(focal=torch.zeros(3)), 'focal must be'),
    (dict(focal=None), 'focal and princpt'),
    (dict(princpt=torch.zeros(3, 2)), 'princpt must be'),
    (dict(regressor_h36m=np.zeros((17, 6), np.float32)), 'over 6 vertices'),
    (dict(regressor_h36m=np.zeros((65, 5), np.float32)), '65 joints'),
    (dict(regressor_coco=np.zeros((12, 5), np.float32)), 'coco regressor of 12 joints'),
    (dict(regressor_coco=np.zeros((63, 5), np.float32)), 'coco regressor of 63 joints'),
    (dict(joint_cam=torch.zeros(2, 16, 3)), 'joint_cam must be'),
    (dict(joint_img=torch.zeros(2, 17, 4)), 'joint_img must be'),
    (dict(joint_img=torch.zeros(2, 16, 2)), 'joint_img must be'),
    (dict(input_joint_name='human36', joint_img=None, flip_pairs=()), 'needs its joint_img'),
    (dict(fitting_thr=float('nan')), 'fitting_thr is NaN'),
    (dict(rot_deg=torch.zeros(3)), 'rot_deg must be'),
    (dict(flip=torch.zeros(2)), 'flip must be boolean or integer'),
    (dict(flip=torch.zeros(3, dtype=torch.int32)), 'flip must be'),
    (dict(flip_pairs=((1, 19),)), 'outside the 19 joints'),
    (dict(flip_pairs=((-1, 2),)), 'outside the 19 joints'),
    (dict(flip_pairs=(1, 2)), 'pairs of joint indices'),
    (dict(input_joint_name='human36', flip_pairs=((1, 17),)), 'outside the 17 joints'),
    (dict(res=(0, 384)), 'must be positive'),
    (dict(res=288), 'res must be'),
]


@pytest.mark.parametrize('kw,text', REFUSALS, ids=[t for _, t in REFUSALS])
def test_camera_frame_batch_refuses(kw, text):
    with pytest.raises(ValueError, match=text):
        call(**kw)


def test_there_is_no_cpu_path():
    with pytest.raises(RuntimeError, match='HIP device'):
        call()                                                                            # every value is fine; the tensors live on the host
    with pytest.raises(RuntimeError, match='HIP device'):
        batch.root_to_camera(torch.zeros(2, 72), torch.eye(3))


@pytest.mark.parametrize('args,text', [
    ((torch.zeros(2, 71), torch.eye(3)), 'pose must be'),
    ((torch.zeros(2, 72, dtype=torch.int32), torch.eye(3)), 'pose must be'),
    ((torch.zeros(2, 72), None), 'R is required'),
    ((torch.zeros(2, 72), torch.zeros(3, 3, 3)), 'R must be'),
    ((torch.zeros(2, 72), torch.eye(3), 24), 'root joint 24'),
    ((torch.zeros(2, 72), torch.eye(3), -1), 'root joint -1'),
])
def test_root_to_camera_refuses(args, text):
    with pytest.raises(ValueError, match=text):
        batch.root_to_camera(*args)


def test_build_list_and_signatures():
    assert 'train_batch.hip' in build.SOURCES
    assert len(_lib.SIGNATURES['gator_batch_prepare_f32'][1]) == 10
    assert len(_lib.SIGNATURES['gator_camera_targets_f32'][1]) == 2
    from gator_amd import kernel_resources as kr
    assert 'k_batch_prepare' in kr.HOT and 'k_camera_targets' in kr.HOT
    names = [n for n, _ in _lib.CameraTargetsArgs._fields_]
    assert names[0] == 'struct_size' and {'reg_h36m', 'reg_coco', 'flip_pairs', 'n_pairs', 'fitting_thr'} <= set(names)
