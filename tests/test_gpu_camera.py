"""gator_crop_joints_f32 / gator_fit_camera_f32 (gator_amd.camera, models.project_net.fit) against the reference's golden run
(tests/golden/cam_fit.npz) and the float64 numpy restatement (tests/camfit_ref.py).

Bounds are 3x the spreads between the golden's own fp32 and fp64 columns (torch's CPU fit, 48 samples):
    cam after 1 / 10 steps                   3.6e-8 / 1.6e-7    -> 1e-6 (the kernel's reduction order is not torch's)
    cam after 1500 steps, 42 well-conditioned samples  5.3e-4  -> 1.6e-3
    final loss, the same samples                       2.0e-3 px -> 0.006 px
    final loss, all samples                            0.016 px  -> 0.3 px (256 random samples on the CPU reached 0.13 px where the
                                                                   scale collapses to ~0; 48 do not sample that tail)"""
import ctypes

import numpy as np
import pytest
import torch

from gator_amd import _lib, camera, models
from tests import camfit_ref as cr
from tests.helpers import load_golden
from tests.test_host_camera import well_conditioned

pytestmark = pytest.mark.gpu

CAM_STEP_1_10 = 1e-6
CAM_1500 = 1.6e-3
LOSS_GOOD = 0.006
LOSS_ALL = 0.3


def _golden():
    z = load_golden('cam_fit')
    return z, torch.from_numpy(z['joints3d']).cuda(), torch.from_numpy(z['xy'][:, :17].copy()).cuda()


def test_crop_joints_matches_reference_chain():
    z = load_golden('cam_fit')
    coco = z['is_coco'] == 1
    for sel, add, nj in ((coco, True, 19), (~coco, False, 17)):
        xy, bbox, valid = camera.crop_joints(torch.from_numpy(z['raw'][sel]).cuda(), 500, add_pelvis_neck=add)
        xy, bbox, valid = xy.cpu().numpy(), bbox.cpu().numpy(), valid.cpu().numpy()
        assert xy.shape[1] == nj
        np.testing.assert_array_equal(valid, z['valid'][sel])
        assert np.abs(xy - z['xy'][sel, :nj]).max() <= 1e-4          # fp32 ulp at 500 px: 3e-5
        assert np.abs(bbox - z['bbox'][sel]).max() <= 1e-4
        assert not xy[valid == 0].any() and not bbox[valid == 0].any()


@pytest.mark.parametrize('k', [0, 1])
def test_fit_first_steps_match_golden_fp32(k):
    z, p, t = _golden()
    steps = int(z['snap_steps'][k])
    cam, loss = camera.fit_camera(p, t, init=torch.from_numpy(z['init']).cuda(), steps=steps)
    assert np.abs(cam.cpu().numpy() - z['cam_f32'][k]).max() <= CAM_STEP_1_10


def test_fit_1500_steps_against_golden():
    z, p, t = _golden()
    cam, loss = camera.fit_camera(p, t, init=torch.from_numpy(z['init']).cuda())
    cam, loss = cam.cpu().numpy().astype(np.float64), loss.cpu().numpy().astype(np.float64)
    good = well_conditioned(z)
    assert np.abs(cam - z['cam_f64'][-1])[good].max() <= CAM_1500
    assert (loss[good] <= z['loss_f64'][good] + LOSS_GOOD).all()
    assert (loss <= z['loss_f64'] + LOSS_ALL).all()


def test_orig_cam_matches_demo_conversion():
    """steps = 0 from the golden's fitted fp32 camera: cam is init exactly, orig_cam is convert_crop_cam_to_orig_img's."""
    z, p, t = _golden()
    init = torch.from_numpy(z['cam_f32'][-1].astype(np.float32)).cuda()
    w, h = (int(x) for x in z['image_size'])
    cam, loss, oc = camera.fit_camera(p, t, init=init, steps=0, bbox=torch.from_numpy(z['bbox']).cuda(), image_size=(w, h))
    assert torch.equal(cam, init)
    v = z['valid'] == 1
    ref = z['orig_cam'][v]
    assert (np.abs(oc.cpu().numpy()[v] - ref) <= 1e-5 * np.abs(ref)).all()


def _random_batch(B, seed, nj=17):
    """Detections in crop pixels and 3D joints that project near them (the golden's recipe)."""
    rs = np.random.RandomState(seed)
    c = 250 + (rs.rand(B, 1, 2) - 0.5) * 100
    tg = (c + (rs.rand(B, nj, 2) - 0.5) * rs.uniform(150, 400, (B, 1, 2))).astype(np.float32)
    s = rs.uniform(0.7, 1.2, (B, 1, 1))
    p = (tg - 250) / (s * 250) - rs.uniform(-0.1, 0.1, (B, 1, 2)) + rs.randn(B, nj, 2) * 0.03
    j3 = np.concatenate([p, rs.randn(B, nj, 1) * 0.1], 2).astype(np.float32)
    return j3, tg, rs.rand(B, 3).astype(np.float32)


def test_large_batch_is_per_sample_and_deterministic():
    B = 4097
    j3, tg, init = _random_batch(B, 11)
    P, T, I = (torch.from_numpy(a).cuda() for a in (j3, tg, init))
    cam, loss = camera.fit_camera(P, T, init=I)
    cam2, loss2 = camera.fit_camera(P, T, init=I)
    assert torch.equal(cam, cam2) and torch.equal(loss, loss2)
    for i in (0, 63, 64, 2048, 4096):
        c1, l1 = camera.fit_camera(P[i:i + 1], T[i:i + 1], init=I[i:i + 1])
        assert torch.equal(c1[0], cam[i]) and torch.equal(l1[0], loss[i])
    _, loss64 = cr.fit(j3, tg, init, dtype=np.float64)
    excess = loss.cpu().numpy().astype(np.float64) - loss64
    assert np.percentile(excess, 99) <= LOSS_GOOD, np.percentile(excess, 99)
    assert excess.max() <= LOSS_ALL


# 99th percentile of (fp32 - fp64) final loss of tests/camfit_ref.py's two restatements on _random_batch(300, 5, nj=19): fewer
# joints, a noisier fit (12: 0.0079 px, 19: 0.0023 px); the bound is 3x
LOSS_P99_GENERIC = {12: 0.024, 19: 0.007}


@pytest.mark.parametrize('n_fit', [12, 19])
def test_generic_joint_count(n_fit):
    """n_fit != 17 runs the LDS form of the kernel: against the fp32 restatement after 10 steps and the fp64 one after 1500."""
    j3, tg, init = _random_batch(300, 5, nj=19)
    P, T, I = (torch.from_numpy(a).cuda() for a in (j3, tg, init))
    cam10, _ = camera.fit_camera(P, T, init=I, steps=10, n_fit=n_fit)
    ref10, _ = cr.fit(j3, tg, init, steps=10, n_fit=n_fit, dtype=np.float32)
    assert np.abs(cam10.cpu().numpy() - ref10).max() <= CAM_STEP_1_10
    _, loss = camera.fit_camera(P, T, init=I, n_fit=n_fit)
    _, loss64 = cr.fit(j3, tg, init, n_fit=n_fit, dtype=np.float64)
    excess = loss.cpu().numpy().astype(np.float64) - loss64
    assert np.percentile(excess, 99) <= LOSS_P99_GENERIC[n_fit] and excess.max() <= LOSS_ALL


def test_custom_schedule_follows_the_milestone_rule():
    j3, tg, init = _random_batch(64, 9)
    sched = ((0, 0.2), (3, 0.02), (7, 0.3))
    cam, _ = camera.fit_camera(*(torch.from_numpy(a).cuda() for a in (j3, tg)), init=torch.from_numpy(init).cuda(), steps=12, schedule=sched)
    ref, _ = cr.fit(j3, tg, init, steps=12, schedule=sched, dtype=np.float32)
    assert np.abs(cam.cpu().numpy() - ref).max() <= CAM_STEP_1_10


def test_non_finite_input_stays_in_its_sample(coco_model):
    m, _ = coco_model
    from gator_amd import preprocess
    raw = torch.from_numpy(load_golden('cam_fit')['raw'][:2]).cuda()
    m.forward_joints(preprocess.normalise_pose2d(raw, add_pelvis_neck=True))        # the model's context exists before the fits
    j3, tg, init = _random_batch(130, 3)
    P, T, I = (torch.from_numpy(a).cuda() for a in (j3, tg, init))
    cam, loss = camera.fit_camera(P, T, init=I)
    P2 = P.clone()
    P2[70, 4, 0] = float('nan')
    cam2, loss2 = camera.fit_camera(P2, T, init=I)
    assert torch.isnan(cam2[70]).all() and torch.isnan(loss2[70])
    keep = torch.arange(130, device='cuda') != 70
    assert torch.equal(cam2[keep], cam[keep]) and torch.equal(loss2[keep], loss[keep])
    m.device_status()                                   # the fit raises no device status on the model's context
    c0, _ = camera.fit_camera(P, T, init=I, steps=0)
    assert torch.equal(c0, I)


def test_bad_arguments_are_einval():
    lib = _lib.load()
    p = torch.zeros(2, 17, 3, device='cuda')
    t = torch.zeros(2, 17, 2, device='cuda')
    i = torch.zeros(2, 3, device='cuda')
    cam = torch.empty(2, 3, device='cuda')
    ms = (ctypes.c_int32 * 2)(0, 5)
    lrs = (ctypes.c_double * 2)(0.1, 0.01)
    args = dict(n_fit=17, steps=10, n_sched=2, ms=ms)

    def call(n_fit=17, steps=10, n_sched=2, ms=ms):
        return lib.gator_fit_camera_f32(p.data_ptr(), 2, 17, t.data_ptr(), 17, n_fit, i.data_ptr(), 500, steps, ms, lrs, n_sched,
                                        None, 0.0, 0.0, cam.data_ptr(), None, None, None)
    assert call(**args) == 0
    torch.cuda.synchronize()
    for bad in (dict(n_fit=0), dict(n_fit=18), dict(steps=-1), dict(n_sched=0), dict(n_sched=9), dict(ms=(ctypes.c_int32 * 2)(0, -1))):
        assert call(**dict(args, **bad)) == -1, bad
        assert b'gator_fit_camera_f32' in lib.gator_last_error()
    rc = lib.gator_crop_joints_f32(t.data_ptr(), 2, 17, 2, 0, ctypes.c_float(0.0), ctypes.c_float(1.25), 500, 500, t.data_ptr(),
                                   i.data_ptr(), None, None)
    assert rc == -1 and b'gator_crop_joints_f32' in lib.gator_last_error()
    with pytest.raises(RuntimeError, match=r'\(-1\)'):
        camera.fit_camera(p, t, n_fit=40)


@pytest.fixture(scope='module')
def coco_model():
    from tests.helpers import build_model
    _, m = build_model('coco19_alpha')
    jr = load_golden('j_regressors')
    R = np.zeros((17, 6890), np.float32)
    R[jr['coco_row'], jr['coco_col']] = jr['coco_val']
    m.set_joint_regressor(R)
    return m, R


def test_fit_mesh_to_image_on_the_demo_input(coco_model):
    """The demo's flow on its own detection, batched with copies of it from three inits: against the float64 restatement of the fit
    of the device's own joints and target.  The seeded weights' joints do not look like the detection (a ~89 px fit), so the
    fit is ill-conditioned: the camera is held to the 1500-step bound where the fitted scale is >= 0.1 (the golden's
    well-conditioned rule; one of the three inits collapses it to ~0.09), the loss to the all-sample bound."""
    m, _ = coco_model
    z = load_golden('cam_fit')
    raw = torch.from_numpy(np.repeat(z['raw'][:1], 3, 0)).cuda()
    init = torch.from_numpy(z['init'][:3]).cuda()
    out = camera.fit_mesh_to_image(m, raw, 'coco', image_size=(1920, 1080), init=init)
    assert out['mesh'].shape == (3, 6890, 3) and out['joints'].shape == (3, 17, 3) and out['orig_cam'].shape == (3, 4)
    assert out['valid'].cpu().tolist() == [1, 1, 1]
    tg, bbox, _ = camera.crop_joints(raw, 500, add_pelvis_neck=True)
    assert torch.equal(out['bbox'], bbox)
    j3 = out['joints'].cpu().numpy()
    cam64, loss64 = cr.fit(j3, tg.cpu().numpy(), z['init'][:3], dtype=np.float64)
    fitted = np.abs(cam64[:, 0]) >= 0.1
    assert fitted.sum() >= 2
    assert np.abs(out['cam'].cpu().numpy() - cam64)[fitted].max() <= CAM_1500
    assert (out['loss'].cpu().numpy() <= loss64 + LOSS_ALL).all()
    oc = cr.crop_cam_to_image(out['cam'].cpu().numpy(), bbox.cpu().numpy(), 1920, 1080)
    assert np.abs(out['orig_cam'].cpu().numpy() - oc).max() <= 1e-5 * np.abs(oc).max()


def test_project_net_adam_on_the_device_against_fit(coco_model):
    """B = 1, the demo's way: models.project_net driven by torch.optim.Adam on the GPU for 1500 steps, and the same layer's fit(),
    both from the golden's first init (a fit whose scale stays away from 0; torch.rand's draw can collapse it, see above)."""
    m, _ = coco_model
    z = load_golden('cam_fit')
    raw = torch.from_numpy(z['raw'][:1]).cuda()
    from gator_amd import preprocess
    joints, _ = m.forward_joints(preprocess.normalise_pose2d(raw, add_pelvis_neck=True))
    target, _, _ = camera.crop_joints(raw, 500, add_pelvis_neck=True)
    a = models.project_net.get_model(crop_size=500).cuda()
    b = models.project_net.get_model(crop_size=500).cuda()
    with torch.no_grad():
        a.cam_param.copy_(torch.from_numpy(z['init'][:1]))
        b.cam_param.copy_(a.cam_param)
    crit = torch.nn.L1Loss()
    opt = torch.optim.Adam(a.parameters(), lr=0.1)
    for j in range(1500):
        loss = crit(a(joints.detach()), target[:, :17, :])
        opt.zero_grad()
        loss.backward()
        opt.step()
        if j == 500:
            for g in opt.param_groups:
                g['lr'] = 0.05
        if j == 1000:
            for g in opt.param_groups:
                g['lr'] = 0.001
    with torch.no_grad():
        loss_a = float(crit(a(joints), target[:, :17, :]))
    loss_b = float(b.fit(joints, target))
    assert b.cam_param.shape == (1, 3)
    assert abs(float(b.cam_param[0, 0])) >= 0.1
    assert np.abs(a.cam_param.detach().cpu().numpy() - b.cam_param.detach().cpu().numpy()).max() <= CAM_1500
    assert abs(loss_a - loss_b) <= LOSS_ALL
