"""gator_smpl_forward_f32 / gator_amd.smpl on the device against the float64 restatement (tests/smpl_refs.py) on the golden inputs
(tests/golden/smpl_layer.npz: the real smplpytorch layer's fp32 run on synthetic models).

Bounds.  Each golden case records max |reference fp32 - fp64 restatement| over its 65 samples, for verts and for joints: the
reference's own fp32 error (4.5e-7 .. 8.4e-7 m on verts, 1.7e-7 .. 5.0e-7 m on joints at |trans| ~ 2 m; 1000 x that in mm).  The
device is held to 3x that figure against the restatement -- the project's convention for an fp32 reference, tests/test_gpu_camera.py
-- and to 4x against the stored fp32 outputs themselves (the reference's 1x plus the device's 3x).  A run on the first B samples of a
case is held to the case's figure.  Every test prints its measured errors before it asserts (profiles/smpl_layer_tests.txt).

Sizes: the kernel's tile is 32 samples x 128 vertices, so B takes 31 / 32 / 33 and 65 (three tiles, the last with one sample), NV
takes 127 / 128 / 129 beside the issue's 1 / 63 / 64 / 65 / 257 / 6890 (54 vertex tiles)."""
import functools

import numpy as np
import pytest
import torch

from gator_amd import eval as gator_eval
from gator_amd import smpl
from tests import smpl_refs as sr
from tests.helpers import load_golden
from tests.test_host_smpl import case_options

pytestmark = pytest.mark.gpu

PARITY_CASES = ('nv1', 'nv63', 'nv64', 'nv65', 'nv127', 'nv128', 'nv129', 'nv257', 'nv6890')
OPTION_CASES = ('no_betas_no_trans', 'center0', 'center23', 'scale1000', 'dense', 'nb0')
BATCHES = (1, 2, 31, 32, 33, 65)


def make_layer(m, **kw):
    return smpl.SMPLLayer.from_arrays(m['v_template'], m['shapedirs'], m['posedirs'], m['weights'], m['J_regressor'], m['parents'],
                                      faces=m['faces'], **kw)


class Case:
    """A golden case on the device: model, layer, inputs (numpy and device), the fp64 restatement of all 65 samples, the spreads."""

    def __init__(self, name):
        z = load_golden('smpl_layer')
        self.name, self.o = name, case_options(name)
        self.m = sr.synthetic_model(*sr.CASES[name][0])
        self.layer = make_layer(self.m, center_idx=self.o['center_idx'], out_scale=self.o['out_scale'])
        self.np_in = (z[name + '.pose'], z[name + '.betas'] if self.o['betas'] else None, z[name + '.trans'] if self.o['trans'] else None)
        self.dev_in = tuple(None if a is None else torch.from_numpy(a).cuda() for a in self.np_in)
        self.ref_v, self.ref_j = sr.lbs_forward(self.m, *self.np_in, self.o['center_idx'], self.o['out_scale'])
        self.gold_v, self.gold_j = z[name + '.verts32'], z[name + '.joints32']
        self.spread_v, self.spread_j = (float(x) for x in z[name + '.spread'])

    def run(self, B=sr.N_SAMPLES, first=0, **kw):
        sl = slice(first, first + B)
        return self.layer(*(None if a is None else a[sl] for a in self.dev_in), **kw)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def check_parity(c, B, verts, joints):
    v, j = verts.cpu().numpy().astype(np.float64), joints.cpu().numpy().astype(np.float64)
    assert v.shape == (B,) + c.ref_v.shape[1:] and j.shape == (B,) + c.ref_j.shape[1:]
    ev, ej = np.abs(v - c.ref_v[:B]).max(), np.abs(j - c.ref_j[:B]).max()
    k = min(B, c.gold_v.shape[0])
    gv, gj = np.abs(v[:k] - c.gold_v[:k]).max(), np.abs(j[:k] - c.gold_j[:k]).max()
    print('smpl parity %-18s B %2d  verts: device %.3e reference %.3e (vs golden fp32 %.3e)  joints: device %.3e reference %.3e (vs golden fp32 %.3e)'
          % (c.name, B, ev, c.spread_v, gv, ej, c.spread_j, gj))
    assert ev <= 3 * c.spread_v and ej <= 3 * c.spread_j
    assert gv <= 4 * c.spread_v and gj <= 4 * c.spread_j


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('name', PARITY_CASES)
def test_parity_with_the_fp64_restatement(name, B):
    c = case(name)
    check_parity(c, B, *c.run(B))


@pytest.mark.parametrize('name', OPTION_CASES)
def test_options_and_models(name):
    """betas = None and trans = None, center_idx 0 and 23, out_scale 1000, a dense-weights model (24 influences: the looped form of
    the epilogue), a model without betas."""
    c = case(name)
    if name == 'dense':
        assert (c.m['weights'] != 0).sum(1).min() == 24
    for B in (1, 65):
        check_parity(c, B, *c.run(B))


@pytest.mark.parametrize('i,family', list(enumerate(sr.FAMILIES)))
def test_pose_families(i, family):
    """One sample per family, run alone and inside the batch: finite, within the case's bound, the same bits both ways."""
    c = case('families')
    verts, joints = c.run(65)
    v1, j1 = c.run(1, first=i)
    assert torch.isfinite(v1).all() and torch.isfinite(j1).all()
    assert torch.equal(v1[0], verts[i]) and torch.equal(j1[0], joints[i])
    ev = np.abs(v1[0].cpu().numpy() - c.ref_v[i]).max()
    ej = np.abs(j1[0].cpu().numpy() - c.ref_j[i]).max()
    print('smpl family %-10s verts: device %.3e reference(case) %.3e  joints: device %.3e reference(case) %.3e' % (family, ev, c.spread_v, ej, c.spread_j))
    assert ev <= 3 * c.spread_v and ej <= 3 * c.spread_j
    assert np.abs(v1[0].cpu().numpy() - c.gold_v[i]).max() <= 4 * c.spread_v
    if family == 'zero':                       # identity rotations: the joints are the shaped rest joints plus trans, not NaN
        J = c.m['J_regressor'].astype(np.float64) @ (c.m['v_template'] + c.m['shapedirs'].astype(np.float64) @ c.np_in[1][i].astype(np.float64))
        assert np.abs(j1[0].cpu().numpy() - (J + c.np_in[2][i])).max() <= 3 * c.spread_j


def test_families_batch_parity():
    c = case('families')
    check_parity(c, 65, *c.run(65))


def test_mano_sized_model_against_the_restatement():
    """NJ = 16, NV = 778, NB = 10: the reference layer cannot run it (its pose map is hard-wired to 23 joints), so there is no golden;
    the bound is 3x the spread of the nv257 case -- the same input distribution through the same arithmetic with a shorter chain."""
    m = sr.synthetic_model(778, 16, 10, 31)
    layer = make_layer(m)
    rs = np.random.RandomState(32)
    pose = (rs.randn(33, 48) * 0.4).astype(np.float32)
    betas = rs.uniform(-2.5, 2.5, (33, 10)).astype(np.float32)
    trans = (rs.randn(33, 3) * 1.2).astype(np.float32)
    rv, rj = sr.lbs_forward(m, pose, betas, trans)
    verts, joints = layer(*(torch.from_numpy(a).cuda() for a in (pose, betas, trans)))
    ev, ej = np.abs(verts.cpu().numpy() - rv).max(), np.abs(joints.cpu().numpy() - rj).max()
    ref = case('nv257')
    print('smpl mano-sized NV 778 NJ 16: verts %.3e (bound %.3e)  joints %.3e (bound %.3e)' % (ev, 3 * ref.spread_v, ej, 3 * ref.spread_j))
    assert verts.shape == (33, 778, 3) and joints.shape == (33, 16, 3)
    assert ev <= 3 * ref.spread_v and ej <= 3 * ref.spread_j


@pytest.mark.parametrize('name', ['nv129', 'nv6890'])
def test_a_sample_does_not_depend_on_its_batch(name):
    c = case(name)
    verts, joints = c.run(65)
    for i in (range(65) if name == 'nv129' else (0, 31, 32, 64)):
        v1, j1 = c.run(1, first=i)
        assert torch.equal(v1[0], verts[i]) and torch.equal(j1[0], joints[i]), i
    v33, j33 = c.run(33, first=20)             # another tiling of the same samples
    assert torch.equal(v33, verts[20:53]) and torch.equal(j33, joints[20:53])


def test_poison_stays_in_its_sample():
    c = case('nv129')
    pose, betas, trans = (a.clone() for a in c.dev_in)
    verts, joints = c.layer(pose, betas, trans)
    pose[7, 1] = float('nan')                  # the root's rotation: by the chain alone the root joint itself would stay finite
    betas[40, 3] = float('inf')
    v2, j2 = c.layer(pose, betas, trans)
    bad = torch.zeros(65, dtype=torch.bool, device='cuda')
    bad[[7, 40]] = True
    assert not torch.isfinite(v2[bad]).any() and not torch.isfinite(j2[bad]).any()
    assert torch.equal(v2[~bad], verts[~bad]) and torch.equal(j2[~bad], joints[~bad])
    pose2 = c.dev_in[0].clone()
    pose2[33, 20 * 3] = float('nan')           # an elbow: the reference keeps its ancestors' joints finite, here the whole sample is marked
    v3, j3 = c.layer(pose2, c.dev_in[1], c.dev_in[2])
    only = torch.arange(65, device='cuda') != 33
    assert not torch.isfinite(v3[33]).any() and not torch.isfinite(j3[33]).any()
    assert torch.equal(v3[only], verts[only]) and torch.equal(j3[only], joints[only])


def test_either_output_may_be_left_out_and_batch_zero():
    c = case('nv65')
    verts, joints = c.run(33)
    v, none = c.run(33, want_joints=False)
    assert none is None and torch.equal(v, verts)
    none, j = c.run(33, want_verts=False)
    assert none is None and torch.equal(j, joints)
    v0, j0 = c.layer(torch.empty(0, 72, device='cuda'), torch.empty(0, 10, device='cuda'), torch.empty(0, 3, device='cuda'))
    assert v0.shape == (0, 65, 3) and j0.shape == (0, 24, 3)
    with pytest.raises(ValueError):
        c.layer(c.dev_in[0][:4], c.dev_in[1][:3], None)
    with pytest.raises(RuntimeError, match='must live on'):
        c.layer(c.dev_in[0][:4].cpu())


def test_centre_with_translation_is_einval_on_a_live_ctx():
    import ctypes
    from gator_amd import _lib
    c = case('nv65')
    lib = _lib.load()
    p, b, t = (a[:2].contiguous() for a in c.dev_in)
    out = torch.empty(2, 65, 3, device='cuda')
    one = ctypes.c_float(1.0)
    assert lib.gator_smpl_forward_f32(c.layer._ctx, p.data_ptr(), b.data_ptr(), t.data_ptr(), 2, 0, one, out.data_ptr(), None, None) == -1
    assert b'center_idx' in lib.gator_last_error()
    assert lib.gator_smpl_forward_f32(c.layer._ctx, p.data_ptr(), b.data_ptr(), None, 2, 24, one, out.data_ptr(), None, None) == -1
    assert lib.gator_smpl_forward_f32(c.layer._ctx, p.data_ptr(), b.data_ptr(), None, -1, -1, one, out.data_ptr(), None, None) == -1
    assert lib.gator_smpl_forward_f32(c.layer._ctx, p.data_ptr(), b.data_ptr(), None, 2, 23, one, out.data_ptr(), None, None) == 0
    torch.cuda.synchronize()


def test_a_smaller_batch_reuses_the_workspace():
    c = case('nv257')
    c.run(65)
    torch.cuda.synchronize()
    base, cap = c.layer.workspace()
    assert base and cap >= 65
    for B in (8, 65, 1):
        c.run(B)
        assert c.layer.workspace() == (base, cap)
    fresh = make_layer(c.m)
    assert fresh.workspace() == (0, 0)
    fresh(*(a[:4] for a in c.dev_in))
    b4 = fresh.workspace()
    assert b4[0] and b4[1] == 4
    fresh(*(a[:40] for a in c.dev_in))                       # a larger batch grows it, once
    assert fresh.workspace()[1] == 40
    v, j = fresh(*(a[:4] for a in c.dev_in))
    assert fresh.workspace()[1] == 40
    ve, je = c.run(4)
    assert torch.equal(v, ve) and torch.equal(j, je)


def test_capture_and_replay_give_the_eager_bits():
    c = case('nv257')
    eager_v, eager_j = c.run(33)
    torch.cuda.synchronize()
    args = tuple(a[:33].clone() for a in c.dev_in)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c.layer(*args)                                       # the workspace exists before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    base = c.layer.workspace()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gv, gj = c.layer(*args)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(gv, eager_v) and torch.equal(gj, eager_j)
    assert c.layer.workspace() == base
    for a, src in zip(args, c.dev_in):                       # new inputs in the captured buffers: the replay computes them
        a.copy_(src[32:65])
    g.replay()
    torch.cuda.synchronize()
    v2, j2 = c.run(33, first=32)
    assert torch.equal(gv, v2) and torch.equal(gj, j2)


@functools.lru_cache(maxsize=None)
def dataset_setup():
    c = case('nv6890')
    rs = np.random.RandomState(77)
    regs = []
    for nj in (17, 17):                                      # stand-ins for the H36M and COCO regressors: 8-vertex convex rows
        R = np.zeros((nj, 6890), np.float32)
        for j in range(nj):
            R[j, rs.randint(0, 6890, 8)] = rs.dirichlet(np.ones(8)).astype(np.float32)
        regs.append(R)
    pose, betas, trans = (a[:3].copy() for a in c.np_in)
    betas[1, 4] = 3.5                                        # beyond 3: the datasets fall back to the mean shape
    return c, regs, pose, betas, trans


def test_get_smpl_coord_is_the_datasets_wrapper():
    c, regs, pose, betas, trans = dataset_setup()
    layer = make_layer(c.m)
    mesh, joints = smpl.get_smpl_coord(layer, *(torch.from_numpy(a).cuda() for a in (pose, betas, trans)))
    assert layer.out_scale == 1.0
    b2 = betas.copy()
    b2[1] = 0.0
    rv, rj = sr.lbs_forward(c.m, pose, b2, trans, out_scale=1000.0)
    rj = np.concatenate([rj, rv[:, list(smpl.FACE_KPS_VERTEX)]], 1)
    assert mesh.shape == (3, 6890, 3) and joints.shape == (3, 29, 3)
    ev, ej = np.abs(mesh.cpu().numpy() - rv).max(), np.abs(joints.cpu().numpy()[:, :24] - rj[:, :24]).max()
    print('smpl get_smpl_coord (mm): mesh %.3e joints %.3e, bound %.3e / %.3e' % (ev, ej, 3e3 * c.spread_v, 3e3 * c.spread_j))
    assert ev <= 3e3 * c.spread_v and ej <= 3e3 * c.spread_j          # millimetres: 1000 x the case's metres (cf. the scale1000 case)
    assert torch.equal(joints[:, 24:], mesh[:, list(smpl.FACE_KPS_VERTEX)])
    m2, j2 = smpl.get_smpl_coord(layer, torch.from_numpy(pose).cuda(), None)
    rv2, _ = sr.lbs_forward(c.m, pose, None, None, out_scale=1000.0)
    assert np.abs(m2.cpu().numpy() - rv2).max() <= 3e3 * c.spread_v


@pytest.mark.parametrize('joint_set', ['human36', 'coco'])
def test_targets_from_smpl(joint_set):
    """Against numpy on the restatement's mesh.  Tolerance: the mesh's 3x spread in mm, plus the fp32 rounding of an 8-term convex
    sum and of the root subtraction at the values' magnitude (10 roundings of 2^-24 relative)."""
    c, regs, pose, betas, trans = dataset_setup()
    layer = make_layer(c.m)
    jr = [gator_eval.JointRegressor(R, 'cuda') for R in regs]
    out = smpl.targets_from_smpl(layer, *(torch.from_numpy(a).cuda() for a in (pose, betas, trans)), jr[0], jr[1], input_joint_name=joint_set)
    assert sorted(out) == ['lift_pose3d', 'mesh', 'reg_pose3d']
    b2 = betas.copy()
    b2[1] = 0.0
    mesh, _ = sr.lbs_forward(c.m, pose, b2, trans, out_scale=1000.0)
    h36m = np.einsum('jv,bvc->bjc', regs[0].astype(np.float64), mesh)
    coco = np.einsum('jv,bvc->bjc', regs[1].astype(np.float64), mesh)
    coco = np.concatenate([coco, (coco[:, 11:12] + coco[:, 12:13]) * 0.5, (coco[:, 5:6] + coco[:, 6:7]) * 0.5], 1)
    want = {'mesh': (mesh - h36m[:, :1]) / 1000, 'reg_pose3d': h36m - h36m[:, :1],
            'lift_pose3d': coco - coco[:, -2:-1] if joint_set == 'coco' else h36m - h36m[:, :1]}
    tol = 3e3 * c.spread_v + 10 * 2.0 ** -24 * np.abs(mesh).max()
    for k, w in want.items():
        got = out[k].cpu().numpy()
        assert got.shape == w.shape, k
        err = np.abs(got - w).max()
        t = tol / 1000 if k == 'mesh' else tol
        print('smpl targets %-8s %-12s err %.3e tol %.3e' % (joint_set, k, err, t))
        assert err <= t, k
    assert out['lift_pose3d'].shape[1] == (19 if joint_set == 'coco' else 17)
