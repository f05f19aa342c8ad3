"""Digest of the forward's outputs for a few (variant, batch, encoder pin) cases.
  * A/B of two builds: run it under each (GATOR_AMD_LIB=...) and compare the lines -- equal digests = bitwise equal results.
  * `--write tests/golden/fp32_digests.json` records the digests of the CURRENT library (on a GPU box); tests/test_gpu_digest.py then
    holds every later build to them, so that a change that is meant to be a schedule only (round 4: dead token rows, C-layout GELU,
    zero operands on dead lanes) is checked bit for bit by the suite instead of by hand.  Re-record only with a change that is MEANT to
    move bits, together with the error budget (tests/error_budget.py).
  * `--forms --write tests/golden/mdr_form_digests.json` does the same for form_digests(): the MDR kernels' non-default arithmetic forms
    and whole-head kernels at B = 11, which the fp32 digests above never reach.
  * `--caller --write tests/golden/caller_side_digests.json` does the same for caller_digests(): the kernels around the forward
    (preprocess, camera crop, Procrustes / joint / mesh / sequence errors, camera targets) on small seeded shapes.
  * `--encoder --write tests/golden/encoder_form_digests.json` does the same for encoder_digests(): every form of the GAT encoder kernels
    (k_gat8, k_gat, k_gat_tiled, the tail launches, the stand-alone encoder entry, the block taps) at batches the fp32 digests never reach.
  * `--handles --write tests/golden/handle_digests.json` does the same for handle_digests(): the auxiliary libraries behind a handle (mesh
    renderer, 2D overlay, SMPL layer, fit and backward) on small seeded shapes, with each handle's workspace() after a small, the largest and the small
    call again.
  * `--regressor --write tests/golden/regressor_form_digests.json` does the same for regressor_digests(): every form of the vertex regressor
    (fp32-input, three bf16 planes, two fp16 planes, bf16, config 3's three) through the stage entry and its packers, the head-written
    operand, the joint epilogue and a rescaled weight, at the batches where a tile, a workgroup or a kernel choice changes.
python tools/ab_digest.py [tag] [--forms | --caller | --encoder | --handles | --regressor] [--write path [--commit hash-of-the-recorded-build]]"""
import contextlib, hashlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gator_amd import synthetic
from tests.helpers import build_model

VARIANTS = (('h36m17_bn', 17), ('coco19_alpha', 19))
CASES = [(name, J, B, pin) for name, J in VARIANTS for B, pin in ((5, 'auto'), (256, 'auto'), (700, 'auto'), (700, 'tiled'))]


def digests():
    out = {}
    models = {}
    for name, J, B, pin in CASES:
        if name not in models:
            models[name] = build_model(name, 'fused')[1]
        m = models[name]
        m.set_encoder(pin)
        x = torch.from_numpy(synthetic.synthetic_pose2d(B, J, seed=B)).cuda()
        v, p = m(x)
        torch.cuda.synchronize()
        m.set_encoder('auto')
        assert bool(torch.isfinite(v).all())
        out['%s B=%d %s' % (name, B, pin)] = hashlib.sha256(v.cpu().numpy().tobytes() + p.cpu().numpy().tobytes()).hexdigest()[:32]
    return out


# The MDR kernels' forms (mdr_fused.hip / mdr_head.hip): operand arithmetic XA = 2 (default), 1 (exact split), 0 (fp32-input MFMA), 3 (config 3:
# precision 'bf16'), and the whole-head kernels instead of the tiles' partial sums + k_mdr_head_finish.
FORMS = {'default': ({}, 'f32'), 'x3_1': ({'GATOR_MDR_X3': '1'}, 'f32'), 'x3_0': ({'GATOR_MDR_X3': '0'}, 'f32'), 'bf16': ({}, 'bf16'),
         'head_partials0': ({'GATOR_MDR_HEAD_PARTIALS': '0'}, 'f32')}
FORM_SWITCHES = ('GATOR_MDR_X3', 'GATOR_MDR_HEAD_PARTIALS', 'GATOR_MDR_PERSIST')
FORM_B = 11     # XCD queues 0-2 hold two samples and 3-7 one (a last ticket with two dead waves), the four-launch grid of 39 workgroups ends half empty, token tile 13 lacks 17 keys
FORM_B_ROLLED = 513     # k_mdr_head<512, false> (the rolled whole head) is planned only above 2 x 256 CUs' worth of samples


@contextlib.contextmanager
def _switches(env, names=FORM_SWITCHES):
    old = {k: os.environ.get(k) for k in names}
    try:
        for k in names:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _sha(*tensors):
    return hashlib.sha256(b''.join(t.cpu().numpy().tobytes() for t in tensors)).hexdigest()[:32]


def form_digests(forms=None):
    """{'<form> persist=<0|1> <variant> B=<B> <forward|pose2mesh>': digest}.  'forward' is the whole forward (vertices + pose3d);
    'pose2mesh' is the MDR entry point on a seeded randn pose_combine (k_mdr_joint and the pc branch of tile mode 0, both JointArgs::x2).
    The switches are read when a context is created, so every case drops the models' contexts first."""
    out = {}
    models = {name: build_model(name, 'fused')[1] for name, _ in VARIANTS}
    for form in (forms or FORMS):
        env, precision = FORMS[form]
        for persist in ('0', '1'):
            for name, J in VARIANTS:
                batches = (FORM_B, FORM_B_ROLLED) if form == 'head_partials0' and name == 'h36m17_bn' else (FORM_B,)
                for B in batches:
                    m = models[name]
                    with _switches(dict(env, GATOR_MDR_PERSIST=persist)):
                        m.invalidate()
                        m.pose2mesh.invalidate()
                        m.precision = precision
                        x = torch.from_numpy(synthetic.synthetic_pose2d(B, J, seed=B)).cuda()
                        v, p = m(x)
                        pc = torch.randn((B, J, 133), generator=torch.Generator().manual_seed(B)).cuda()
                        w = m.pose2mesh(pc)
                        torch.cuda.synchronize()
                        m.precision = 'f32'
                        m.invalidate()
                        m.pose2mesh.invalidate()
                    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(w).all())
                    key = '%s persist=%s %s B=%d ' % (form, persist, name, B)
                    out[key + 'forward'], out[key + 'pose2mesh'] = _sha(v, p), _sha(w)
    return out


# The GAT encoder's forms (gat_roles.hip + gat8_*.h / gat_fused.hip / gat_tiled.hip / gat_tail.hip).  name: (entry, environment, precision, batches, taps)
#   entry 'sample': the whole forward with the per-sample encoder pinned.  B = 3, and B = 65 = nine workgroups per XCD group, where both L2
#       warm-ups and the tail warm-up are on (below 64 they are off).  With the two variants (LR 10 / 12) the eight forms reach all eleven
#       k_gat8 instantiations and k_gat<true|false, false>.
#   entry 'tiled': the whole forward with the sample-tiled encoder pinned, B = 8: two workgroups, the second with one sample (J = 17) or two (J = 19).
#   entry 'gat': the stand-alone encoder (models/GAT.py -> gator_gat_forward_f32, k_gat<., true>): digest of pose3d + feat.
#   taps: a second forward with enable_block_taps(True); the six block taps join the digest.
ENCODER_FORMS = {
    'default': ('sample', {}, 'f32', (3, 65), False),
    'tail0': ('sample', {'GATOR_GAT8_TAIL': '0'}, 'f32', (3, 65), False),
    'lobyte0': ('sample', {'GATOR_GAT8_LOBYTE': '0'}, 'f32', (3, 65), False),
    'h4_0': ('sample', {'GATOR_GAT8_H4': '0'}, 'f32', (3, 65), False),
    'gat8_0': ('sample', {'GATOR_GAT8': '0'}, 'f32', (3, 65), False),
    'x3_0': ('sample', {'GATOR_GAT_X3': '0'}, 'f32', (3, 65), False),
    'bf16': ('sample', {}, 'bf16', (3, 65), False),
    'bf16_tail0': ('sample', {'GATOR_GAT8_TAIL': '0'}, 'bf16', (3, 65), False),
    'tiled': ('tiled', {}, 'f32', (8,), False),
    'tiled_h4_0': ('tiled', {'GATOR_GAT_TILED_H4': '0'}, 'f32', (8,), False),
    'tiled_bf16': ('tiled', {}, 'bf16', (8,), False),
    'gat': ('gat', {}, 'f32', (3,), False),
    'gat_x3_0': ('gat', {'GATOR_GAT_X3': '0'}, 'f32', (3,), False),
    'taps': ('sample', {}, 'f32', (3,), True),
    'tiled_taps': ('tiled', {}, 'f32', (8,), True),
}
ENCODER_SWITCHES = ('GATOR_GAT_X3', 'GATOR_GAT8', 'GATOR_GAT8_H4', 'GATOR_GAT8_LOBYTE', 'GATOR_GAT8_TAIL', 'GATOR_GAT8_DBG', 'GATOR_GAT_TILED',
                    'GATOR_GAT_TILED_H4', 'GATOR_GAT_TILED_MIN_BATCH', 'GATOR_C3_ENCODER')


def encoder_digests(forms=None):
    """{'<form> <variant> B=<B>': digest} of (vertices, pose3d[, gat_block0..5]), or of (pose3d, feat) for the stand-alone encoder entry.
    The switches are read when a context is created, so every case drops the models' contexts first."""
    out = {}
    models = {name: build_model(name, 'fused')[1] for name, _ in VARIANTS}
    for form in (forms or ENCODER_FORMS):
        entry, env, precision, batches, taps = ENCODER_FORMS[form]
        for name, J in VARIANTS:
            for B in batches:
                m = models[name]
                x = torch.from_numpy(synthetic.synthetic_pose2d(B, J, seed=B)).cuda()
                with _switches(env, ENCODER_SWITCHES):
                    m.invalidate()
                    m.pose_lifter.invalidate()
                    if entry == 'gat':
                        got = list(m.pose_lifter(x.reshape(B, 2 * J)))
                    else:
                        m.precision = precision
                        m.set_encoder(entry)
                        got = list(m(x))
                        if taps:
                            m.enable_block_taps(True)
                            got = list(m(x)) + [m.get_tap('gat_block%d' % i, (B, J, 128)).clone() for i in range(6)]
                        m.set_encoder('auto')
                        m.precision = 'f32'
                    torch.cuda.synchronize()
                    m.invalidate()
                    m.pose_lifter.invalidate()
                assert all(bool(torch.isfinite(t).all()) for t in got)
                out['%s %s B=%d' % (form, name, B)] = _sha(*got)
    return out


# The caller-side kernels (preprocess / camera crop / Procrustes and joint errors / sequence errors / mesh errors / camera targets): small
# seeded shapes at the edges of their shared pieces -- the 64-lane block edge, the 32-joint column limit, a rejected box, every rotation
# and flip, 3 and 32 fitted points, videos shorter than a triple.
COCO_FLIP_PAIRS = ((1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16))
H36M_FLIP_PAIRS = ((1, 4), (2, 5), (3, 6), (14, 11), (15, 12), (16, 13))
CALLER_B = (1, 64, 65, 130)
CALLER_JOINTS = ((17, True), (17, False), (30, True))      # (J_in, add pelvis / neck): 19 joints, 17, and 32 = the column limit
CALLER_ROT = (0.0, 30.0, -90.0, 180.0)


def _sha_canon(*tensors):
    """sha256[:32] of the raw bytes, every NaN first replaced by numpy's one NaN so that no digest depends on a payload."""
    import numpy as np
    h = hashlib.sha256()
    for t in tensors:
        a = t.detach().cpu().numpy().copy()
        if a.dtype.kind == 'f':
            a[np.isnan(a)] = np.nan
        h.update(a.tobytes())
    return h.hexdigest()[:32]


def _raw_joints(rs, B, J, comps, reject):
    """Pixel joints of B people in a 640 x 480 image (comps 3: a score column); reject: sample B // 2 has all joints on one point."""
    import numpy as np
    centre = rs.rand(B, 1, 2) * np.array([400.0, 250.0]) + np.array([120.0, 110.0])
    x = centre + (rs.rand(B, J, 2) - 0.5) * (rs.rand(B, 1, 2) * np.array([150.0, 200.0]) + 20.0)
    if comps == 3:
        x = np.concatenate([x, rs.rand(B, J, 1)], 2)
    if reject:
        x[B // 2, :, :2] = x[B // 2, :1, :2]
    return torch.from_numpy(x.astype(np.float32)).cuda()


def _rotations(rs, B):
    import numpy as np
    q, _ = np.linalg.qr(rs.randn(B, 3, 3))
    q[:, :, 0] *= np.sign(np.linalg.det(q))[:, None]
    return q


def _sparse_regressor(rs, n_joint, nv):
    import numpy as np
    d = np.zeros((n_joint, nv), np.float32)
    for j in range(n_joint):
        d[j, rs.choice(nv, 6, replace=False)] = rs.dirichlet(np.ones(6)).astype(np.float32)
    return d


def caller_digests():
    """{'<entry point> <case>': digest} of the raw output bytes of the caller-side entry points, inputs from np.random.RandomState."""
    import numpy as np
    from gator_amd import batch, camera, eval as gator_eval, preprocess, temporal
    f32 = np.float32
    dev = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)).cuda() if dt is None else torch.from_numpy(np.ascontiguousarray(a)).cuda().to(dt)  # noqa: E731
    out = {}

    # the 2D joint chain: normalise_pose2d, preprocess_chain, crop_joints
    for B in CALLER_B:
        for J, pn in CALLER_JOINTS:
            for comps in (2, 3):
                case = 'B=%d J=%d%s comps=%d' % (B, J, '+2' if pn else '', comps)
                rs = np.random.RandomState(1000 * B + 10 * J + comps + (5 if pn else 0))
                out['normalise_pose2d ' + case] = _sha_canon(preprocess.normalise_pose2d(_raw_joints(rs, B, J, comps, False), add_pelvis_neck=pn))
                # one sample whose box is rejected; at B = 1 that is the only sample, so B = 1 runs both ways
                for reject in ((False, True) if B == 1 else (True,)):
                    x = _raw_joints(rs, B, J, comps, reject)
                    got = list(preprocess.preprocess_chain(x, add_pelvis_neck=pn))
                    # per-sample augmentation: the four rotations cycle fastest, the flip every four samples; B = 1 takes all eight in turn
                    for shift in (range(8) if B == 1 else (0,)):
                        i = np.arange(B) + shift
                        rot, flip = np.asarray(CALLER_ROT, f32)[i % 4], ((i // 4) % 2).astype(np.int32)
                        got += preprocess.preprocess_chain(x, rot_deg=rot, flip=flip, flip_pairs=COCO_FLIP_PAIRS, add_pelvis_neck=pn)
                    got += preprocess.preprocess_chain(x, rot_deg=np.zeros(B, f32), flip=np.ones(B, np.int32), flip_pairs=COCO_FLIP_PAIRS,
                                                       add_pelvis_neck=pn, res=(256, 256))
                    valid = got[1].cpu().numpy()
                    assert reject == (int(valid.sum()) == B - 1) and (not reject or valid[B // 2] == 0), (case, valid)
                    tag = case + (' rejected' if B == 1 and reject else '')
                    out['preprocess_chain ' + tag] = _sha_canon(*got)
                    crops = []
                    for aspect in (1.0, 0.75):
                        for size in (500, (288, 384)):
                            crops += camera.crop_joints(x, crop_size=size, box_aspect=aspect, add_pelvis_neck=pn)
                    assert int(crops[2].sum()) == B - int(reject)
                    out['crop_joints ' + tag] = _sha_canon(*crops)

    # Procrustes and the joint errors
    for N in (3, 14, 32):
        for B in (1, 65):
            rs = np.random.RandomState(7000 + 100 * N + B)
            a, b = dev((rs.randn(B, N, 3) * 0.3).astype(f32)), dev((rs.randn(B, N, 3) * 0.3).astype(f32))
            out['rigid_align N=%d B=%d' % (N, B)] = _sha_canon(gator_eval.rigid_align(a, b))
            got = []
            for nj, idx in ((N, None), (N + 3, [int(i) for i in rs.permutation(N + 3)[:N]])):
                t = (rs.randn(B, nj, 3) * 300.0).astype(f32)
                p = (t / 1000.0 + rs.randn(B, nj, 3) * 0.03).astype(f32)
                for root in (0, nj - 1):
                    got.append(gator_eval.joint_errors(dev(p), dev(t), eval_joints=idx, root=root, pred_scale=1000.0))
                    got.append(gator_eval.joint_errors(dev(p * f32(1000.0)), dev(t), eval_joints=idx, root=root, pred_scale=1.0))
            out['joint_errors N=%d B=%d' % (N, B)] = _sha_canon(*got)

    # the per-video errors: videos of 1, 2, 3 and 70 frames in one call
    lengths = (1, 2, 3, 70)
    F = sum(lengths)
    for ne in (3, 14):
        rs = np.random.RandomState(8000 + ne)
        g = rs.randn(F, ne, 3) * 200.0
        p64 = g + np.cumsum(rs.randn(F, ne, 3), 0) * 3.0
        valid = (rs.rand(F) > 0.15)
        for dt in (torch.float32, torch.float64):
            for smooth in (False, True):
                got = []
                for v in (None, valid):
                    got += temporal._errors(dev(p64, dt), dev(g.astype(f32)), lengths, None, v, smooth, [0.004, 0.005, 1.0, 1.0], 'caller_digests')
                out['sequence_errors ne=%d %s smooth=%d' % (ne, str(dt).split('.')[1], smooth)] = _sha_canon(*got)

    # the whole-mesh errors
    for N in (50, 300):
        rs = np.random.RandomState(9000 + N)
        t = (rs.rand(3, N, 3) - 0.5) * np.array([0.9, 1.7, 0.4])
        p = t + rs.randn(3, N, 3) * 0.02 + rs.randn(3, 1, 3) * 0.1
        root_reg, eval_reg = _sparse_regressor(rs, 17, N), _sparse_regressor(rs, 17, N)
        for ev in (None, eval_reg):
            got = gator_eval.mesh_errors(dev(p.astype(f32)), dev(t.astype(f32)), root_reg, root=2, eval_regressor=ev, pred_scale=1000.0, target_scale=1000.0)
            out['mesh_errors N=%d eval=%d' % (N, ev is not None)] = _sha_canon(got)

    # the camera-frame targets (k_camera_targets), with the dataset's own joints so that the fitting error is formed
    B, N = 2, 50
    for lift_set, pairs in (('human36', H36M_FLIP_PAIRS), ('coco', COCO_FLIP_PAIRS)):
        rs = np.random.RandomState(9500 + len(lift_set))
        verts = ((rs.rand(B, N, 3) - 0.5) * np.array([0.9, 1.7, 0.4])).astype(f32)
        joints = (rs.randn(B, 24, 3) * 0.3).astype(f32)
        trans, cam_t = (rs.randn(B, 3) * 0.5).astype(f32), (rs.randn(B, 3) * 0.3 + np.array([0, 0, 4.5])).astype(f32)
        R = _rotations(rs, B).astype(f32)
        focal, princpt = (1145.0 + rs.randn(B, 2) * 5).astype(f32), (np.array([512.0, 515.0]) + rs.randn(B, 2) * 3).astype(f32)
        dh, dc = _sparse_regressor(rs, 17, N), _sparse_regressor(rs, 17, N)
        reg_h = gator_eval._Coo.from_dense(dh, 'cuda', 'caller_digests')
        reg_c = gator_eval._Coo.from_dense(dc, 'cuda', 'caller_digests') if lift_set == 'coco' else None
        mesh_cam = (verts.astype(np.float64) + (trans.astype(np.float64) + cam_t)[:, None]) * 1000.0
        jc = (np.einsum('jv,bvc->bjc', dh.astype(np.float64), mesh_cam) + rs.randn(B, 17, 3) * 20.0).astype(f32)
        ji = (jc[:, :, :2] / jc[:, :, 2:] * focal[:, None] + princpt[:, None]).astype(f32)
        Jl = 19 if lift_set == 'coco' else 17
        got = []
        for compensate in (False, True):
            o = [torch.empty(s, device='cuda') for s in ((B, N, 3), (B, 17, 3), (B, Jl, 3), (B, Jl, 2), (B,), (B, 3))]
            batch._launch_camera_targets(dev(verts), dev(joints), dev(trans), dev(cam_t), dev(R), compensate, dev(focal), dev(princpt), reg_h, reg_c,
                                         batch.LIFT_SETS[lift_set], dev(jc), dev(ji), dev(np.asarray([30.0, -90.0], f32)),
                                         dev(np.asarray([1, 0], np.int32)), dev(np.asarray(pairs, np.int32)), 25.0, 0, *o)
            got += o
        out['camera_targets %s B=%d N=%d' % (lift_set, B, N)] = _sha_canon(*got)
    torch.cuda.synchronize()
    return out


# The auxiliary libraries' handles (render.hip, draw2d.hip, smpl_lbs.hip, smpl_fit.hip): small seeded calls, and per handle the sequence
# small call / largest call / small call again with the workspace() tuple after each, so that the host side of a handle (growth rule,
# staged tables, accounting) is pinned against the build that recorded the file.
HANDLE_LIBS = ('renderer', 'draw2d', 'smpl', 'fit', 'backward')
HANDLE_SMPL_CASE = 'nv257'


def _renderer_digests(out):
    import numpy as np
    from gator_amd import render
    from tests import render_refs
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    base, faces = render_refs.icosphere(1)                  # 42 vertices, 80 faces
    rs = np.random.RandomState(11000)
    spheres = np.stack([base * 0.55, base * np.array([0.35, 0.5, 0.4])])      # two spheres; three meshes are placed from them
    verts = (spheres[[0, 1, 0]] + rs.uniform(-0.15, 0.15, (3, 1, 3))).astype(np.float32)
    cam = np.concatenate([rs.uniform(0.7, 1.1, (3, 2)), rs.uniform(-0.2, 0.2, (3, 2))], 1).astype(np.float32)
    W, H = 65, 33
    bg = dev(rs.randint(0, 256, (2, H, W, 3)).astype(np.uint8))
    color = rs.uniform(0.2, 1.0, (3, 3)).astype(np.float32)
    large = dict(verts=dev(verts), cam=dev(cam), background=bg, color=color, image_index=[1, 0, 1], size=(W, H), return_face_id=True, return_depth=True)
    small = dict(verts=dev(verts[:1]), cam=dev(cam[:1]), size=(16, 9), return_face_id=True, return_depth=True)
    r = render.MeshRenderer(faces, 'cuda:0', n_verts=base.shape[0])
    seq, ws = [], []
    for kw in (small, large, small):
        seq.append(_sha_canon(*r.render(**kw)))
        ws.append(list(r.workspace()))
    out['renderer render M=3 N=2 index=[1,0,1]'] = seq[1]
    out['renderer render M=2 index=None'] = _sha_canon(*r.render(dev(verts[:2]), dev(cam[:2]), size=(W, H), return_face_id=True, return_depth=True))
    xy, z, n = r.project(large['verts'], large['cam'], size=(W, H))
    keys = r.rasterise(xy, z, image_index=[1, 0, 1], n_images=2, size=(W, H))
    staged = r.resolve(keys, xy, n, background=bg, color=color, image_index=[1, 0, 1], return_face_id=True, return_depth=True)
    out['renderer project rasterise resolve M=3 N=2'] = _sha_canon(xy, z, n, keys, *staged)
    fresh = _sha_canon(*render.MeshRenderer(faces, 'cuda:0', n_verts=base.shape[0]).render(**small))
    assert seq[0] == seq[2] == fresh, 'the renderer depends on its workspace history'
    out['renderer sequence small'], out['renderer sequence workspace'] = seq[0], ws


def _draw2d_digests(out):
    import numpy as np
    from gator_amd import vis
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    skeleton = [(0, 1), (1, 2), (2, 3), (1, 4)]
    rs = np.random.RandomState(12000)
    W, H = 70, 37
    joints = np.concatenate([rs.uniform(-5, W + 5, (3, 5, 1)), rs.uniform(-5, H + 5, (3, 5, 1)), rs.uniform(0.2, 1.0, (3, 5, 1))], 2).astype(np.float32)
    lo, hi = joints[:, :, :2].min(1), joints[:, :, :2].max(1)
    bbox = np.stack([lo, np.stack([hi[:, 0], lo[:, 1]], 1), hi, np.stack([lo[:, 0], hi[:, 1]], 1)], 1).astype(np.float32)
    frames = dev(rs.randint(0, 256, (2, H, W, 3)).astype(np.uint8))
    tiny = dev(rs.randint(0, 256, (1, 9, 16, 3)).astype(np.uint8))
    d = vis.SkeletonDrawer(skeleton, 5, 'cuda:0')
    large = dict(images=frames, joints=dev(joints), bbox=dev(bbox), image_index=[1, 0, 1], alpha=0.6)
    small = dict(images=tiny, joints=dev(joints[:1] * np.array([0.2, 0.2, 1.0], np.float32)))
    seq, ws = [], []
    for kw in (small, large, small):
        seq.append(_sha_canon(d.draw(**kw)))
        ws.append(list(d.workspace()))
    for style, colors in (('keypoints', None), ('coco', (40.0, 200.0, 120.0))):
        for bb in (None, large['bbox']):
            got = {}
            for rows in (1, 4):
                d.set_tile_rows(rows)
                got[rows] = _sha_canon(d.draw(frames, large['joints'], colors=colors, bbox=bb, image_index=[1, 0, 1], alpha=0.6, style=style))
            d.set_tile_rows(0)
            inplace = frames.clone()
            d.draw(inplace, large['joints'], colors=colors, bbox=bb, image_index=[1, 0, 1], alpha=0.6, style=style, out=inplace)
            assert got[1] == got[4] == _sha_canon(inplace), 'draw2d: tile rows or in-place drawing change the bytes'
            out['draw2d %s bbox=%d P=3 N=2' % (style, bb is not None)] = got[1]
    fresh = _sha_canon(vis.SkeletonDrawer(skeleton, 5, 'cuda:0').draw(**small))
    assert seq[0] == seq[2] == fresh and seq[1] == out['draw2d keypoints bbox=1 P=3 N=2'], 'the drawer depends on its workspace history'
    out['draw2d sequence small'], out['draw2d sequence workspace'] = seq[0], ws


def _smpl_case():
    from gator_amd import smpl
    from tests import smpl_refs
    from tests.helpers import load_golden
    m = smpl_refs.synthetic_model(*smpl_refs.CASES[HANDLE_SMPL_CASE][0])
    z = load_golden('smpl_layer')
    pose, betas, trans = (torch.from_numpy(z['%s.%s' % (HANDLE_SMPL_CASE, k)]).cuda() for k in ('pose', 'betas', 'trans'))
    make = lambda **kw: smpl.SMPLLayer.from_arrays(m['v_template'], m['shapedirs'], m['posedirs'], m['weights'], m['J_regressor'],  # noqa: E731
                                                   m['parents'], faces=m['faces'], **kw)
    return make, pose, betas, trans


def _smpl_workspace(layer, before):
    """[batch capacity, 1 if the workspace's block is another one than after the previous call] -- the address itself is no constant"""
    base, cap = layer.workspace()
    return base, [cap, int(base != before)]


def _smpl_digests(out):
    make, pose, betas, trans = _smpl_case()
    layer, centred = make(), make(center_idx=3)
    seq, ws, base = [], [], 0
    for B in (1, 33, 1):
        seq.append(_sha_canon(*layer(pose[:B], betas[:B], trans[:B])))
        base, w = _smpl_workspace(layer, base)
        ws.append(w)
    for B in (1, 33):
        out['smpl forward B=%d' % B] = seq[0] if B == 1 else seq[1]
        out['smpl forward B=%d center_idx=3' % B] = _sha_canon(*centred(pose[:B], betas[:B]))
    fresh = _sha_canon(*make()(pose[:1], betas[:1], trans[:1]))
    assert seq[0] == seq[2] == fresh, 'the SMPL layer depends on its workspace history'
    out['smpl sequence workspace'] = ws


def _fit_digests(out):
    make, pose, betas, trans = _smpl_case()
    layer = make()
    target = layer(pose[:2], betas[:2], trans[:2])[0].clone()
    seq, ws, base = [], [], 0
    for B in (1, 2, 1):
        seq.append(_sha_canon(*layer.fit(target[:B], iters=3)))
        base, w = _smpl_workspace(layer, base)
        ws.append(w)
    out['fit cold B=2 iters=3'] = seq[1]
    warm = (pose[:2] + 0.05, betas[:2] * 0.5, trans[:2] + 0.01)
    out['fit warm B=2 iters=3'] = _sha_canon(*layer.fit(target, iters=3, init=warm))
    M = layer.fit_normal(*warm, target)
    P, N = layer.fit_width()
    iu = torch.triu_indices(N, N, device=M.device)
    out['fit normal B=2'] = _sha_canon(M[:, iu[0], iu[1]])              # only the upper triangle is specified
    fresh = _sha_canon(*make().fit(target[:1], iters=3))
    assert seq[0] == seq[2] == fresh, 'the SMPL fit depends on its workspace history'
    out['fit sequence small'], out['fit sequence workspace'] = seq[0], ws


def _grad_case(name):
    """A golden case as tests/test_gpu_smpl_backward.py takes it: (make a layer, device inputs with None for the absent ones,
    device upstream gradients (grad_verts, grad_joints))."""
    from gator_amd import smpl
    from tests import smpl_grad_refs as gr, smpl_refs
    m = smpl_refs.synthetic_model(*smpl_refs.CASES[name][0])
    make = lambda: smpl.SMPLLayer.from_arrays(m['v_template'], m['shapedirs'], m['posedirs'], m['weights'], m['J_regressor'], m['parents'])  # noqa: E731
    ins = tuple(None if a is None else torch.from_numpy(a).cuda() for a in gr.case_arguments(name))
    return make, ins, tuple(torch.from_numpy(a).cuda() for a in gr.upstream(name))


def _backward(layer, ins, ups, B, which='full', center=-1, needs=(True, True, True)):
    """gator_smpl_backward_f32 itself on the first B samples -> the digest of the gradients that were asked for."""
    from gator_amd import _lib
    from tests import smpl_grad_refs as gr
    ins = [None if a is None else a[:B].contiguous() for a in ins]
    gV, gJ = gr.select_upstream(which, *(g[:B].contiguous() for g in ups))
    outs = [torch.full_like(a, 7.0) if (a is not None and n) else None for a, n in zip(ins, needs)]
    ptr = _lib.ptr
    _lib.check(_lib.load().gator_smpl_backward_f32(layer._ctx, ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), B, center, 1.0, ptr(gV), ptr(gJ),
                                                   ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), _lib.stream_ptr(layer.device)),
               'gator_smpl_backward_f32')
    return _sha_canon(*(o for o in outs if o is not None))


def _backward_digests(out):
    """B = 1 and 33 (one lane of a sample tile; a full tile and a one-sample tile), nv257 (three vertex tiles, the last nearly all padding)
    and dense (24 influences: the looped MI_T = 0 kernels), every upstream subset, centring, an output subset, the workspace's growth."""
    make, ins, ups = _grad_case(HANDLE_SMPL_CASE)
    layer = make()
    seq, ws = [], []
    for B in (1, 33, 1):
        seq.append(_backward(layer, ins, ups, B))
        ws.append(list(layer.workspace_bytes()))
    for B in (1, 33):
        out['backward %s B=%d full' % (HANDLE_SMPL_CASE, B)] = seq[0] if B == 1 else seq[1]
        for which in ('verts', 'joints'):
            out['backward %s B=%d %s' % (HANDLE_SMPL_CASE, B, which)] = _backward(layer, ins, ups, B, which)
    out['backward %s B=33 full center_idx=3' % HANDLE_SMPL_CASE] = _backward(layer, (ins[0], ins[1], None), ups, 33, center=3)
    out['backward %s B=33 full grad_pose only' % HANDLE_SMPL_CASE] = _backward(layer, ins, ups, 33, needs=(True, False, False))
    dmake, dins, dups = _grad_case('dense')
    out['backward dense B=33 full'] = _backward(dmake(), dins, dups, 33)
    # the layer's own looped kernel (k_smpl_skin<0>), verts + joints; kept in this group: the 'smpl' group's keys are the set recorded before
    out['backward dense B=33 forward'] = _sha_canon(*dmake()(*(a[:33] for a in dins)))
    fresh = _backward(make(), ins, ups, 1)
    assert seq[0] == seq[2] == fresh, 'the SMPL backward depends on its workspace history'
    out['backward sequence small'], out['backward sequence workspace'] = seq[0], ws


def handle_digests(libs=None):
    """{'<library> <case>': digest, '<library> sequence workspace': the workspace() tuple after each of the three calls}."""
    out = {}
    for lib in (libs or HANDLE_LIBS):
        {'renderer': _renderer_digests, 'draw2d': _draw2d_digests, 'smpl': _smpl_digests, 'fit': _fit_digests, 'backward': _backward_digests}[lib](out)
    torch.cuda.synchronize()
    return out


# The vertex regressor's forms (upsample_*.hip behind upsample_common.h).  name: (environment, stage precision or None, stage batches, extras)
#   stage: pose2mesh.upsample on randn(B, 431, 3) * 0.3 seeded with B -- the stage packers and the regressor kernel.  33: a second tile and a
#       ragged one; 129: x2's second 128-sample workgroup with three dead waves; 257: x3's ninth tile (second workgroup, seven shadow waves)
#       and fp32's ragged pair; 224 / 225: fp32's one-tile -> two-tile switch; 65 (bf16): an odd tile count, the last pair repeats its tile.
#   extras: 'forward' the whole forward at B = 33 (the head-written operand); 'joints' forward_joints at B = 33 with and without the vertex
#       store, a seeded sparse regressor with an entry at vertex 0 and at 6889; 'scaled' the stage entry with the regressor's weights
#       times 2^12 (another pack-time shift than the golden one); 'c3' gator_forward_bf16 at B = 33; 'sequence' one context through B = 33,
#       257, 1 (the x3 plane stride follows the capacity; the row-subset digests of the first and third call must not depend on history).
REGRESSOR_FORMS = {
    'fp32': ({'GATOR_UPSAMPLE_X3': '0'}, 'f32', (1, 33, 129, 257, 224, 225), ('forward', 'sequence')),
    'x3': ({'GATOR_UPSAMPLE_X3': '1'}, 'f32', (1, 33, 129, 257), ('forward', 'joints', 'scaled', 'sequence')),
    'x2': ({'GATOR_UPSAMPLE_X3': '2'}, 'f32', (1, 33, 129, 257), ('joints', 'scaled', 'sequence')),
    'bf16': ({}, 'bf16', (1, 33, 65), ('sequence',)),
    'c3_default': ({}, None, (), ('c3',)),
    'c3_w1_0': ({'GATOR_C3_UPSAMPLE_W1': '0'}, None, (), ('c3',)),
    'c3_bf16': ({'GATOR_C3_UPSAMPLE_BF16': '1'}, None, (), ('c3',)),
}
REGRESSOR_SWITCHES = ('GATOR_UPSAMPLE_X3', 'GATOR_C3_UPSAMPLE_W1', 'GATOR_C3_UPSAMPLE_BF16')
REGRESSOR_B = 33
REGRESSOR_SEQUENCE = (33, 257, 1)
REGRESSOR_VARIANT = ('h36m17_bn', 17)


def _coarse(B, seed=None):
    return (torch.randn((B, 431, 3), generator=torch.Generator().manual_seed(B if seed is None else seed)) * 0.3).float().cuda()


def regressor_digests(forms=None):
    """{'<form> <case>': digest}.  The switches are read when a context is created, so every form drops the model's contexts first."""
    import numpy as np
    out = {}
    name, J = REGRESSOR_VARIANT
    for form in (forms or REGRESSOR_FORMS):
        env, precision, batches, extras = REGRESSOR_FORMS[form]
        m = build_model(name, 'fused')[1]

        def renew():
            torch.cuda.synchronize()
            m.invalidate()
            m.pose2mesh.invalidate()

        def note(case, *tensors):
            torch.cuda.synchronize()
            assert all(bool(torch.isfinite(t).all()) for t in tensors), (form, case)
            out['%s %s' % (form, case)] = _sha(*tensors)

        with _switches(env, REGRESSOR_SWITCHES):
            renew()
            for B in batches:
                note('stage B=%d' % B, m.pose2mesh.upsample(_coarse(B), precision=precision))
            x = torch.from_numpy(synthetic.synthetic_pose2d(REGRESSOR_B, J, seed=REGRESSOR_B)).cuda()
            if 'forward' in extras:
                note('forward B=%d' % REGRESSOR_B, *m(x))
            if 'c3' in extras:
                m.precision = 'bf16'
                note('forward_bf16 B=%d' % REGRESSOR_B, *m(x))
                m.precision = 'f32'
            if 'joints' in extras:
                rs = np.random.RandomState(13000)
                dense = _sparse_regressor(rs, 17, 6890)
                dense[0, 0], dense[16, 6889] = 0.25, -0.5
                m.set_joint_regressor(dense)
                for with_verts in (True, False):
                    note('joints B=%d with_verts=%d' % (REGRESSOR_B, with_verts), *m.forward_joints(x, with_verts=with_verts))
            if 'sequence' in extras:
                renew()
                vc = _coarse(max(REGRESSOR_SEQUENCE), seed=14000)
                seq = [_sha(m.pose2mesh.upsample(vc[:B].contiguous(), precision=precision)[:1]) for B in REGRESSOR_SEQUENCE]
                assert seq[0] == seq[2], 'the regressor depends on its workspace history'
                for B, h in zip(REGRESSOR_SEQUENCE[:2], seq):
                    out['%s sequence B=%d row 0' % (form, B)] = h
            if 'scaled' in extras:
                with torch.no_grad():
                    m.pose2mesh.upsample_conv.weight.mul_(2.0 ** 12)
                renew()
                note('stage B=%d weights * 2^12' % REGRESSOR_B, m.pose2mesh.upsample(_coarse(REGRESSOR_B), precision=precision))
            renew()
    return out


def main_regressor():
    write = sys.argv[sys.argv.index('--write') + 1] if '--write' in sys.argv else None
    d = regressor_digests()
    for k, h in d.items():
        print('%-56s %s' % (k, h), flush=True)
    if write:
        commit = sys.argv[sys.argv.index('--commit') + 1] if '--commit' in sys.argv else 'unknown'
        what = ('sha256[:32] per vertex-regressor form (tools/ab_digest.py: regressor_digests), gfx950, golden weights of h36m17_bn: the stage '
                'entry on randn(B, 431, 3) * 0.3 seeded with B, the whole forward and forward_joints on synthetic_pose2d(33, 17, seed=33), '
                'gator_forward_bf16 under its three regressor switches, weights times 2^12, and row 0 of one context run through B = 33, 257, 1.  '
                'Recorded with the library of commit %s' % commit)
        with open(write, 'w') as f:
            json.dump({'what': what, 'digests': d}, f, indent=1)


def main_handles():
    write = sys.argv[sys.argv.index('--write') + 1] if '--write' in sys.argv else None
    d = handle_digests()
    for k, h in d.items():
        print('%-56s %s' % (k, h), flush=True)
    if write:
        commit = sys.argv[sys.argv.index('--commit') + 1] if '--commit' in sys.argv else 'unknown'
        what = ('sha256[:32] of the raw output bytes of the auxiliary libraries (tools/ab_digest.py: handle_digests: renderer, draw2d, SMPL layer, '
                'fit and backward), gfx950, NaNs canonicalised, seeded inputs; "sequence workspace": workspace() after a small, the largest and '
                'the small call again on one handle (SMPL: [capacity, block replaced]; backward: [bytes, allocations]).  Recorded with the library of commit %s' % commit)
        with open(write, 'w') as f:
            json.dump({'what': what, 'digests': d}, f, indent=1)


def main_caller():
    write = sys.argv[sys.argv.index('--write') + 1] if '--write' in sys.argv else None
    d = caller_digests()
    for k, h in d.items():
        print('%-56s %s' % (k, h), flush=True)
    if write:
        commit = sys.argv[sys.argv.index('--commit') + 1] if '--commit' in sys.argv else 'unknown'
        what = ('sha256[:32] of the raw output bytes of the caller-side entry points (tools/ab_digest.py: caller_digests), gfx950, NaNs '
                'canonicalised, inputs from np.random.RandomState with fixed seeds.  Recorded with the library of commit %s' % commit)
        with open(write, 'w') as f:
            json.dump({'what': what, 'digests': d}, f, indent=1)


def main():
    if '--forms' in sys.argv:
        return main_forms()
    if '--caller' in sys.argv:
        return main_caller()
    if '--encoder' in sys.argv:
        return main_encoder()
    if '--handles' in sys.argv:
        return main_handles()
    if '--regressor' in sys.argv:
        return main_regressor()
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    write = sys.argv[sys.argv.index('--write') + 1] if '--write' in sys.argv else None
    if write in args:
        args.remove(write)
    tag = args[0] if args else os.path.basename(os.environ.get('GATOR_AMD_LIB', 'default'))
    d = digests()
    for k, h in d.items():
        print('%-24s %-32s %s' % (tag, k, h), flush=True)
    if write:
        with open(write, 'w') as f:
            json.dump({'what': 'sha256[:32] of (vertices, pose3d) bytes of gator_forward_f32, default arithmetic, gfx950; inputs synthetic_pose2d(B, J, seed=B), golden weights',
                       'digests': d}, f, indent=1)


def main_forms():
    write = sys.argv[sys.argv.index('--write') + 1] if '--write' in sys.argv else None
    d = form_digests()
    for k, h in d.items():
        print('%-56s %s' % (k, h), flush=True)
    if write:
        commit = sys.argv[sys.argv.index('--commit') + 1] if '--commit' in sys.argv else 'unknown'
        what = ('sha256[:32] per MDR form (tools/ab_digest.py: form_digests), gfx950, golden weights: forward = (vertices, pose3d) bytes on '
                'synthetic_pose2d(B, J, seed=B); pose2mesh = vertices of the MDR entry point on randn(B, J, 133) seeded with B.  Recorded with '
                'the library of commit %s' % commit)
        with open(write, 'w') as f:
            json.dump({'what': what, 'digests': d}, f, indent=1)


def main_encoder():
    write = sys.argv[sys.argv.index('--write') + 1] if '--write' in sys.argv else None
    d = encoder_digests()
    for k, h in d.items():
        print('%-40s %s' % (k, h), flush=True)
    if write:
        commit = sys.argv[sys.argv.index('--commit') + 1] if '--commit' in sys.argv else 'unknown'
        what = ('sha256[:32] per GAT encoder form (tools/ab_digest.py: encoder_digests), gfx950, golden weights, inputs synthetic_pose2d(B, J, '
                'seed=B): (vertices, pose3d) bytes of the forward, with the six block taps where the form records them; (pose3d, feat) of the '
                'stand-alone encoder entry.  Recorded with the library of commit %s' % commit)
        with open(write, 'w') as f:
            json.dump({'what': what, 'digests': d}, f, indent=1)


if __name__ == '__main__':
    main()
