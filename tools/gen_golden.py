#!/usr/bin/env python3
"""Generate the golden fixtures under tests/golden/ by running the REAL reference (kasvii/GATOR,
mounted read-only at /root/reference) on CPU with import shims.  Dev-container only: the reference
never travels to the GPU box; only the small data fixtures written here do.

Usage:  python tools/gen_golden.py            (re-creates tests/golden/*.npz)
        python tools/gen_golden.py camfit     (one section only: base, scale, train, train_drop, rigid, preprocess, camfit)

Shims: timm DropPath/Mlp stubs, easydict stub, a pre-seeded core.config.cfg (the real
one mkdirs under the read-only tree at import), funcs_utils stub (imports cv2/matplotlib), a 3-point
affine solve standing in for cv2.getAffineTransform, identity .cuda(), Mesh default device -> cpu,
chdir to a scratch dir holding seeded stand-ins for the licence-gated data/base_data files.
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = '/root/reference'
sys.path.insert(0, REPO)

from gator_amd import synthetic  # noqa: E402
from oracle import graph_consts as gc  # noqa: E402  (Floyd-Warshall output = the path files fed to the reference)

OUT = os.path.join(REPO, 'tests', 'golden')


class _EasyDict(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        self[k] = v


def install_shims(scratch, alpha):
    # timm
    timm = types.ModuleType('timm')
    tm = types.ModuleType('timm.models')
    tl = types.ModuleType('timm.models.layers')
    tv = types.ModuleType('timm.models.vision_transformer')

    class DropPath(nn.Module):
        def __init__(self, p=0.):
            super().__init__()
            self.drop_prob = p                              # kept for train_drop_golden's hook; the forward stays the identity

        def forward(self, x):
            return x

    class Mlp(nn.Module):
        def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
            super().__init__()
            out_features = out_features or in_features
            self.fc1 = nn.Linear(in_features, hidden_features)
            self.act = act_layer()
            self.fc2 = nn.Linear(hidden_features, out_features)
            self.drop = nn.Dropout(drop)

        def forward(self, x):
            return self.drop(self.fc2(self.drop(self.act(self.fc1(x)))))

    tl.DropPath = DropPath
    tv.Mlp = Mlp
    sys.modules.update({'timm': timm, 'timm.models': tm, 'timm.models.layers': tl,
                        'timm.models.vision_transformer': tv})
    ed = types.ModuleType('easydict')
    ed.EasyDict = _EasyDict
    sys.modules['easydict'] = ed
    # core.config
    cfg = _EasyDict()
    cfg.DATASET = _EasyDict(BASE_DATA_DIR=os.path.join(scratch, 'data', 'base_data'))
    cfg.MODEL = _EasyDict(alpha=alpha, posenet_pretrained=False, posenet_path='', input_shape=(384, 288))
    core = types.ModuleType('core')
    cc = types.ModuleType('core.config')
    cc.cfg = cfg
    core.config = cc
    sys.modules.update({'core': core, 'core.config': cc})
    fu = types.ModuleType('funcs_utils')
    fu.load_checkpoint = lambda *a, **k: (_ for _ in ()).throw(ValueError('No checkpoint exists'))
    fu.stop = sys.exit
    sys.modules['funcs_utils'] = fu
    # cv2: only getAffineTransform is reached (lib/aug_utils.py:164-167)
    cv2 = types.ModuleType('cv2')

    def get_affine_transform(src, dst):
        a = np.concatenate([np.asarray(src, np.float64), np.ones((3, 1))], 1)
        return np.linalg.solve(a, np.asarray(dst, np.float64)).T

    cv2.getAffineTransform = get_affine_transform
    sys.modules['cv2'] = cv2
    torch.Tensor.cuda = lambda self, *a, **k: self
    nn.Module.cuda = lambda self, *a, **k: self
    for p in (os.path.join(REF, 'lib'),):
        if p not in sys.path:
            sys.path.insert(0, p)
    return cfg


def write_base_data(scratch, base, sp, path, tag):
    d = os.path.join(scratch, 'data', 'base_data')
    os.makedirs(d, exist_ok=True)
    np.save(os.path.join(d, 'smpl_mean_vertices.npy'), base['smpl_mean_vertices'])
    np.save(os.path.join(d, 'J_regressor_h36m.npy'), base['J_regressor_h36m'])
    import scipy.sparse as sps
    D = np.empty(2, dtype=object)
    D[0], D[1] = base['D'][0].tocoo(), base['D'][1].tocoo()
    U = np.empty(2, dtype=object)
    U[0], U[1] = base['D'][0].T.tocoo(), base['D'][1].T.tocoo()
    A = np.empty(3, dtype=object)
    A[0], A[1], A[2] = sps.identity(6890).tocoo(), sps.identity(1723).tocoo(), sps.identity(431).tocoo()
    np.savez(os.path.join(d, 'mesh_downsampling.npz'), A=A, U=U, D=D)
    np.save(os.path.join(d, 'shortest_path_%s.npy' % tag), sp)
    np.save(os.path.join(d, 'path_%s.npy' % tag), path)


def dump_jregressors():
    z = {}
    for name, f in (('h36m', 'data/Human36M/J_regressor_h36m_correct.npy'), ('coco', 'data/COCO/J_regressor_coco.npy')):
        m = np.load(os.path.join(REF, f))
        r, c = np.nonzero(m)
        z[name + '_row'], z[name + '_col'], z[name + '_val'] = r.astype(np.int32), c.astype(np.int32), m[r, c]
    np.savez(os.path.join(OUT, 'j_regressors.npz'), **z)


def run_variant(name, J, alpha, seed, B=4, upsample_gain=0.2, subset=None, out_name=None):
    import scipy.sparse as sps
    scratch = tempfile.mkdtemp(prefix='gator_golden_')
    for m in [k for k in sys.modules if k.split('.')[0] in ('models', 'graph_utils', 'coarsening', 'core', 'funcs_utils')]:
        del sys.modules[m]
    install_shims(scratch, alpha)
    base = synthetic.make_base_data(seed)
    rs = base['rs']
    skeleton, flips = gc.joint_setting(J)
    adj0 = gc.build_adj(J, skeleton, flips)
    sp, path = gc.floyd_warshall(gc.delete_symmetric_edges(adj0))
    tag = '3dpw' if J == 19 else 'h36m'
    write_base_data(scratch, base, sp, path, tag)
    os.chdir(scratch)
    import models  # noqa  (reference lib/models)
    from models.backbones import mesh as ref_mesh
    ref_mesh.Mesh.__init__.__defaults__ = ('data/base_data/mesh_downsampling.npz', 1, 1, torch.device('cpu'))
    import graph_utils
    ref_adj = graph_utils.build_adj(J, skeleton, flips)            # the reference's own adjacency builder
    assert np.array_equal(ref_adj, adj0)
    graph_adj = [None, sps.csr_matrix(ref_adj)]
    jreg = synthetic.model_j_regressor(J)
    model = models.GATOR.get_model(J, 128, 6, graph_adj, 1, torch.Tensor(jreg))
    model.eval()
    sd = model.state_dict()
    new = synthetic.seeded_state_dict(synthetic.shapes_of(sd), rs, upsample_gain=upsample_gain)
    sd.update({k: torch.from_numpy(v) for k, v in new.items()})
    model.load_state_dict(sd)
    pose2d = synthetic.synthetic_pose2d(B, J, seed + 1 if subset is None else seed + 17)
    x = torch.from_numpy(pose2d)

    taps = {}
    hooks = []

    def tap(mod, key, sel=lambda o: o):
        hooks.append(mod.register_forward_hook(lambda m, i, o: taps.__setitem__(key, sel(o).detach().clone())))

    tap(model.pose_lifter.get_hop_path_encoding, 'hop_path_bias')
    tap(model.pose_lifter, 'feat', lambda o: o[1])
    for i, blk in enumerate(model.pose_lifter.blocks):
        tap(blk, 'gat_block%d' % i, lambda o: o[0])
    tap(model.pose2mesh.selfatt, 'mdr_attn0')
    tap(model.pose2mesh.norm_2, 'mdr_norm2')
    tap(model.pose2mesh.upsample_conv, 'vert431_in')
    up_in = {}
    hooks.append(model.pose2mesh.upsample_conv.register_forward_hook(
        lambda m, i, o: up_in.__setitem__('vert431', i[0].detach().clone())))
    # verts tokens after the 3rd LBF layer = input of motion_linear
    hooks.append(model.pose2mesh.motion_linear.register_forward_hook(
        lambda m, i, o: taps.__setitem__('mdr_lbf2', i[0].detach().clone())))
    with torch.no_grad():
        verts, pose3d = model(x)
    for h in hooks:
        h.remove()
    # fp64 re-evaluation of the same weights (tolerance anchor): cast plain-attribute tensors by hand
    m64 = model.double()
    for blk in m64.pose_lifter.blocks:
        blk.adj = blk.adj.double()
        blk.gcn.adj = blk.gcn.adj.double()
    hp = m64.pose_lifter.get_hop_path_encoding
    hp.edg_adj = hp.edg_adj.double()
    hp.spatial = hp.spatial.double()
    with torch.no_grad():
        verts64, pose3d64 = m64(x.double())
    if subset is not None:
        # scale-free parity fixture: a fixed vertex subset of a larger batch, reference fp32 output and its fp64 anchor
        v32, v64 = verts.float().numpy()[:, subset], verts64.numpy()[:, subset]
        noise = np.abs(verts.double().numpy() - verts64.numpy()).max() * 1e3
        np.savez(os.path.join(OUT, out_name + '.npz'), variant=name, seed=np.int64(seed), upsample_gain=np.float64(upsample_gain),
                 pose2d=pose2d, vertex_subset=subset.astype(np.int32), verts_f64=v64,
                 ref32_minus_f64=(v32.astype(np.float64) - v64).astype(np.float32),
                 pose3d_f64=pose3d64.numpy(), ref32_noise_mm_all_vertices=np.float64(noise),
                 verts_absmax=np.float64(np.abs(verts64.numpy()).max()))
        print('%s: gain %.1f B=%d  |verts| max %.3f m  ref fp32-vs-fp64 max %.3e mm (all vertices), %.3e mm (subset)'
              % (out_name, upsample_gain, B, np.abs(verts64.numpy()).max(), noise, np.abs(v32 - v64).max() * 1e3))
        os.chdir(REPO)
        return
    gat = model.pose_lifter
    out = dict(
        seed=np.int64(seed), alpha=np.bool_(alpha), num_joint=np.int64(J),
        pose2d=pose2d, verts=verts.float().numpy(), pose3d=pose3d.float().numpy(),
        verts_f64=verts64.numpy(), pose3d_f64=pose3d64.numpy(),
        hop_path_bias=taps['hop_path_bias'].float().numpy(), feat=taps['feat'].float().numpy(),
        gat_block0=taps['gat_block0'].float().numpy(), gat_block5=taps['gat_block5'].float().numpy(),
        mdr_lbf2=taps['mdr_lbf2'].float().numpy(), vert431=up_in['vert431'].float().numpy(),
        graph_adj=gat.graph_adj.float().numpy(), shortest_path=sp, path=path,
        edge_input=hp.edg_adj.float().numpy(),
        vj_relation=np.asarray(model.pose2mesh.vj_relation, np.int64),
        init_vertices_431=sd['pose2mesh.init_vertices'].float().numpy(),
        state_dict_keys=np.array(sorted(sd.keys())),
        state_dict_shapes=np.array([str(tuple(sd[k].shape)) for k in sorted(sd.keys())]),
        # spot checks of the seeded weights so a recipe drift is caught without storing 46 MB
        w_probe_lifter=sd['pose_lifter.lifter.weight'].float().numpy()[:2, :8],
        w_probe_upconv=sd['pose2mesh.upsample_conv.weight'].float().numpy()[:2, :3],
    )
    err = np.abs(out['verts'].astype(np.float64) - out['verts_f64']).max() * 1000
    print('%s: J=%d alpha=%s  |verts| max %.3f m  fp32-vs-fp64 max %.2e mm' % (name, J, alpha, np.abs(out['verts']).max(), err))
    np.savez(os.path.join(OUT, name + '.npz'), **out)
    os.chdir(REPO)


def train_golden(name, J, alpha, seed, B=4):
    """One training step's loss and gradients from the REAL reference: model.train() with every nn.Dropout at p = 0 (DropPath
    is the identity stub) - the reference's RNG stream cannot be reproduced elsewhere - so BatchNorm1d runs on batch statistics;
    loss = lib/core/base.py:137-148 incl. the edge term, criteria = lib/core/loss.py get_loss(faces) loaded from its file.
    Stores loss parts and, per parameter, the gradient's max / norm and 48 fixed entries, from the fp32 run and an fp64 run."""
    _train_recording('train_' + name, J, alpha, seed, B, None)


def train_drop_golden(name, J, alpha, seed, mask_seed, B=4):
    """train_golden with the reference's dropout and DropPath ON, the masks drawn on the host: the reference modules stay as they
    are, every nn.Dropout gets p = 0 after its value is remembered, the DropPath stub is the identity with its drop_prob stored,
    and a forward hook on each of them multiplies the module's output by the keep factor of tests/train_refs.py::DropSites - in
    call order the next Philox offset from 1 on, step word 0; nn.Dropout per element at the flat index of the contiguous output,
    DropPath one decision per sample / (1 - p) (timm's).  nn.Identity (block 0's DropPath) and p == 0 draw nothing.  The fp32 and
    the fp64 run get the same masks.  `mask_seed` is the first candidate: the seed used and recorded is the first one from there
    on whose masks are not inert (train_refs.live_path_families: each of the four DropPath families has a site that keeps one
    sample and drops another), judged from the host masks alone.  Adds `mask_seed` and the site log to what train_golden stores."""
    _train_recording('train_drop_' + name, J, alpha, seed, B, mask_seed)


def _train_recording(out_name, J, alpha, seed, B, mask_seed):
    import importlib.util
    import scipy.sparse as sps
    scratch = tempfile.mkdtemp(prefix='gator_golden_')
    for m in [k for k in sys.modules if k.split('.')[0] in ('models', 'graph_utils', 'coarsening', 'core', 'funcs_utils')]:
        del sys.modules[m]
    install_shims(scratch, alpha)
    base = synthetic.make_base_data(seed)
    rs = base['rs']
    skeleton, flips = gc.joint_setting(J)
    adj0 = gc.build_adj(J, skeleton, flips)
    sp, path = gc.floyd_warshall(gc.delete_symmetric_edges(adj0))
    write_base_data(scratch, base, sp, path, '3dpw' if J == 19 else 'h36m')
    os.chdir(scratch)
    import models  # noqa
    from models.backbones import mesh as ref_mesh
    ref_mesh.Mesh.__init__.__defaults__ = ('data/base_data/mesh_downsampling.npz', 1, 1, torch.device('cpu'))
    spec = importlib.util.spec_from_file_location('ref_core_loss', os.path.join(REF, 'lib', 'core', 'loss.py'))
    ref_loss = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_loss)
    graph_adj = [None, sps.csr_matrix(adj0)]
    model = models.GATOR.get_model(J, 128, 6, graph_adj, 1, torch.Tensor(synthetic.model_j_regressor(J)))
    sd = model.state_dict()
    new = synthetic.seeded_state_dict(synthetic.shapes_of(sd), rs)
    sd.update({k: torch.from_numpy(v) for k, v in new.items()})
    model.load_state_dict(sd)
    model.train()
    remembered = {}
    for qual, m in model.named_modules():
        if isinstance(m, nn.Dropout):
            remembered[qual] = (m, float(m.p), False)
            m.p = 0.0
        elif isinstance(m, sys.modules['timm.models.layers'].DropPath):
            remembered[qual] = (m, float(m.drop_prob), True)
    sites = {'cur': None}
    if mask_seed is not None:
        from tests.train_refs import DropSites, live_path_families

        def make_hook(qual, p, per_sample):
            def hook(mod, inputs, out):
                f = sites['cur'].factor(qual, out.shape, p, per_sample)
                return None if f is None else out * f.to(out.dtype)
            return hook

        for qual, (m, p, per_sample) in remembered.items():
            m.register_forward_hook(make_hook(qual, p, per_sample))
    faces = synthetic.synthetic_faces(seed)
    jreg_t = synthetic.load_j_regressors()['h36m'].astype(np.float32)          # target_joint_set regressor (base.py:104)
    pose2d = synthetic.synthetic_pose2d(B, J, seed + 3)
    tg = synthetic.training_targets(B, J, base, jreg_t, seed)
    crit = ref_loss.get_loss(faces=faces)

    if mask_seed is not None:
        sites['cur'] = DropSites(mask_seed)                 # which sites draw, in which order, does not depend on the seed
        with torch.no_grad():
            model(torch.from_numpy(pose2d))
        order = sites['cur'].log
        while len(live_path_families(mask_seed, order, B)) < 4:
            mask_seed += 1

    def step(mdl, dt):
        if mask_seed is not None:
            sites['cur'] = DropSites(mask_seed)
        t = {k: torch.from_numpy(v).to(dt) for k, v in tg.items()}
        mdl.zero_grad()
        pred_mesh, lift_pose = mdl(torch.from_numpy(pose2d).to(dt))
        pred_pose = torch.matmul(torch.from_numpy(jreg_t).to(dt)[None, :, :], pred_mesh * 1000)
        l1 = crit[0](pred_mesh, t['mesh'], t['mesh_valid'])
        l2 = 1e-1 * crit[1](pred_mesh, t['mesh'])
        l4 = 1e-3 * crit[3](pred_pose, t['reg_pose3d'], t['reg_pose3d_valid'])
        l5 = 1e-3 * crit[4](lift_pose, t['lift_pose3d'], t['lift_pose3d_valid'])
        l3 = 20 * crit[2](pred_mesh, t['mesh'])
        loss = l1 + l2 + l4 + l5 + l3
        loss.backward()
        grads = {k: p.grad.detach().clone() for k, p in mdl.named_parameters()}
        parts = np.array([float(v) for v in (l1, l2, l3, l4, l5, loss)])
        return parts, grads, pred_mesh.detach(), lift_pose.detach()

    parts32, g32, mesh32, _ = step(model, torch.float32)
    log32 = sites['cur'].log if mask_seed is not None else None
    m64 = model.double()
    for blk in m64.pose_lifter.blocks:
        blk.adj = blk.adj.double()
        blk.gcn.adj = blk.gcn.adj.double()
    hp = m64.pose_lifter.get_hop_path_encoding
    hp.edg_adj = hp.edg_adj.double()
    hp.spatial = hp.spatial.double()
    parts64, g64, mesh64, lift64 = step(m64, torch.float64)
    names = sorted(g64.keys())
    prs = np.random.RandomState(1234)
    out = dict(seed=np.int64(seed), alpha=np.bool_(alpha), num_joint=np.int64(J), batch=np.int64(B), pose2d=pose2d,
               loss_parts_f32=parts32, loss_parts_f64=parts64, param_names=np.array(names),
               mesh_f64_probe=mesh64.numpy()[:, ::97], lift_pose_f64=lift64.numpy())
    probe_idx, probe64, probe32, gmax, gnorm, noise = [], [], [], [], [], []
    for k in names:
        a64, a32 = g64[k].reshape(-1).numpy(), g32[k].reshape(-1).double().numpy()
        idx = np.sort(prs.choice(a64.size, size=min(48, a64.size), replace=False))
        pad = np.full(48, -1, np.int64)
        pad[:idx.size] = idx
        v64, v32 = np.zeros(48), np.zeros(48)
        v64[:idx.size], v32[:idx.size] = a64[idx], a32[idx]
        probe_idx.append(pad); probe64.append(v64); probe32.append(v32)
        gmax.append(np.abs(a64).max()); gnorm.append(np.sqrt((a64 ** 2).sum())); noise.append(np.abs(a32 - a64).max())
    out.update(probe_idx=np.stack(probe_idx), grad_f64=np.stack(probe64), grad_f32=np.stack(probe32), grad_absmax=np.array(gmax),
               grad_norm=np.array(gnorm), ref32_minus_f64_max=np.array(noise))
    if mask_seed is not None:
        log = sites['cur'].log
        assert log == log32 == order
        shapes = np.full((len(log), 4), -1, np.int64)
        for i, e in enumerate(log):
            shapes[i, :len(e[3])] = e[3]
        out.update(mask_seed=np.int64(mask_seed), site_name=np.array([e[0] for e in log]), site_kind=np.array([e[1] for e in log]),
                   site_p=np.array([e[2] for e in log], np.float64), site_shape=shapes, site_offset=np.array([e[4] for e in log], np.int64))
        print('%s: mask seed %d, %d draws (%d per sample), live DropPath families %s'
              % (out_name, mask_seed, len(log), sum(e[1] == 'path' for e in log), sorted(live_path_families(mask_seed, log, B))))
    np.savez(os.path.join(OUT, out_name + '.npz'), **out)
    rel = np.array(noise) / np.maximum(np.array(gmax), 1e-300)
    print('%s: loss %.6f (fp32 %.6f) parts %s; %d parameter tensors, ref fp32-vs-fp64 gradient error / max|g|: median %.1e max %.1e'
          % (out_name, parts64[-1], parts32[-1], parts64[:5].round(5).tolist(), len(names), np.median(rel), rel.max()))
    os.chdir(REPO)


def demo_preprocess_golden():
    """Config 1 plumbing (demo/run.py:193-198,124-133): raw COCO-17 joints -> [1,19,2] normalised input."""
    scratch = tempfile.mkdtemp(prefix='gator_golden_')
    install_shims(scratch, True)
    for m in [k for k in sys.modules if k in ('coord_utils', 'aug_utils')]:
        del sys.modules[m]
    import aug_utils
    import coord_utils
    raw = np.load(os.path.join(REF, 'demo', 'coco_joint_input.npy'))
    names = ('Nose', 'L_Eye', 'R_Eye', 'L_Ear', 'R_Ear', 'L_Shoulder', 'R_Shoulder', 'L_Elbow', 'R_Elbow', 'L_Wrist',
             'R_Wrist', 'L_Hip', 'R_Hip', 'L_Knee', 'R_Knee', 'L_Ankle', 'R_Ankle', 'Pelvis', 'Neck')
    j = raw.copy()

    def add(jc, a, b):
        n = (jc[names.index(a)] + jc[names.index(b)]) * 0.5
        n[2] = jc[names.index(a), 2] * jc[names.index(b), 2]
        return np.concatenate((jc, n.reshape(1, 3)))

    j = add(j, 'L_Hip', 'R_Hip')
    j = add(j, 'L_Shoulder', 'R_Shoulder')
    j = j[:, :2]
    bbox = coord_utils.get_bbox(j)
    bbox2 = coord_utils.process_bbox(bbox.copy())
    ji, _ = aug_utils.j2d_processing(j.copy(), (288, 384), bbox2, 0, 0, None)
    ji = ji[:, :2]
    ji /= np.array([[288, 384]])
    mean, std = np.mean(ji, axis=0), np.std(ji, axis=0)
    ji = (ji.copy() - mean) / std
    np.savez(os.path.join(OUT, 'demo_preprocess.npz'), raw_coco17=raw, pose2d=ji[None].astype(np.float32))
    print('demo: normalised rows 0-3', ji[:4].round(4).tolist(), 'min %.4f max %.4f' % (ji.min(), ji.max()))


COCO19_FLIP_PAIRS = ((1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16))     # data/PW3D/dataset.py:33-34


def preprocess_chain_golden():
    """The GENERAL input chain run as it is (lib/coord_utils.py:21-66, lib/aug_utils.py:51-64,140-179; call order of
    data/PW3D/dataset.py:236-250): random 19-joint detections, rotation in +-30 degrees, random flips, plus boxes that
    process_bbox rejects (None)."""
    scratch = tempfile.mkdtemp(prefix='gator_golden_')
    install_shims(scratch, True)
    for m in [k for k in sys.modules if k in ('coord_utils', 'aug_utils')]:
        del sys.modules[m]
    import aug_utils
    import coord_utils
    rs = np.random.RandomState(777)
    N, J = 48, 19
    joints = np.zeros((N, J, 2), np.float64)
    rot = np.zeros(N)
    flip = np.zeros(N, np.int32)
    out = np.zeros((N, J, 2), np.float32)
    valid = np.ones(N, np.int32)
    for i in range(N):
        c = rs.rand(2) * np.array([1200, 800]) + 100
        ext = np.array([rs.rand() * 300 + 20, rs.rand() * 500 + 40]) * (0.3 + rs.rand())
        joints[i] = c + (rs.rand(J, 2) - 0.5) * ext
        if i % 3:
            rot[i] = np.clip(rs.randn() * 30, -60, 60)
        flip[i] = int(i % 4 == 1)
        if i in (7, 23):
            joints[i] = joints[i, :1]                       # all joints coincide: w = h = 0
        if i == 31:
            joints[i, :, 0] = joints[i, 0, 0] + np.linspace(0, 0.5, J)      # narrower than one pixel
        bbox = coord_utils.get_bbox(joints[i])
        bbox = coord_utils.process_bbox(bbox.copy())
        if bbox is None:
            valid[i] = 0
            continue
        ji, _ = aug_utils.j2d_processing(joints[i].copy(), (288, 384), bbox, rot[i], int(flip[i]), COCO19_FLIP_PAIRS)
        ji = ji[:, :2]
        ji /= np.array([[288, 384]])
        mean, std = np.mean(ji, axis=0), np.std(ji, axis=0)
        out[i] = (ji.copy() - mean) / std
    np.savez(os.path.join(OUT, 'preprocess_chain.npz'), joints=joints, rot=rot, flip=flip, flip_pairs=np.array(COCO19_FLIP_PAIRS, np.int32),
             pose2d=out, valid=valid)
    print('preprocess chain: %d samples, %d rejected by process_bbox' % (N, int((valid == 0).sum())))


def rigid_align_golden():
    """lib/coord_utils.py:127-149 run as it is: random, mirrored (det < 0 branch), near-coplanar and scaled point sets, plus the
    PA-MPJPE reduction of data/PW3D/dataset.py:337-375 (per-sample rigid_align on the 14 evaluation joints, mean distance)."""
    scratch = tempfile.mkdtemp(prefix='gator_golden_')
    install_shims(scratch, True)
    for m in [k for k in sys.modules if k in ('coord_utils',)]:
        del sys.modules[m]
    import coord_utils
    rs = np.random.RandomState(4242)
    A, B = [], []
    for i in range(24):
        a = rs.randn(14, 3) * 120
        q, _ = np.linalg.qr(rs.randn(3, 3))
        b = (0.5 + rs.rand()) * a @ q.T + rs.randn(3) * 40 + rs.randn(14, 3) * (8 if i % 2 else 0.0)
        if i % 4 == 1:
            b[:, 0] = -b[:, 0]                      # mirror image: forces the reflection fix
        if i % 6 == 2:
            a[:, 2] *= 1e-3                         # nearly coplanar: smallest singular value ~ 0
        A.append(a)
        B.append(b)
    A, B = np.stack(A), np.stack(B)
    out = np.stack([coord_utils.rigid_align(a, b) for a, b in zip(A, B)])
    pa = float(np.mean([np.sqrt(((o - b) ** 2).sum(1)).mean() for o, b in zip(out, B)]))
    A32, B32 = A.astype(np.float32), B.astype(np.float32)      # the reference feeds float32 arrays from the model
    out32 = np.stack([coord_utils.rigid_align(a, b) for a, b in zip(A32, B32)])
    np.savez(os.path.join(OUT, 'rigid_align.npz'), A=A, B=B, aligned=out, pa_mpjpe=np.float64(pa), aligned_from_f32=out32)
    print('rigid_align: 24 sets, PA error %.4f mm' % pa)


def _import_demo_run():
    """demo/run.py as a module, with stand-ins for what it imports but the camera step does not reach (renderer, vis, smpl, the
    checkpoint and .obj helpers); lib/ is on the path already (install_shims)."""
    import importlib.util
    for name, attrs in (('__init_path', {}), ('renderer', {'Renderer': object}), ('vis', {'vis_2d_keypoints': None}),
                        ('smpl', {'SMPL': object})):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
    sys.modules['funcs_utils'].save_obj = None
    spec = importlib.util.spec_from_file_location('demo_run', os.path.join(REF, 'demo', 'run.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def camfit_golden():
    """The demo's camera step run as it is (demo/run.py:123-164, lib/models/project_net.py, convert_crop_cam_to_orig_img :21-39):
    the crop target through the real get_bbox / process_bbox(aspect 1.0, scale 1.25) / j2d_processing at 500 x 500, then one
    OptimzeCamLayer per sample with cam_param overwritten by the recorded init, torch.optim.Adam and nn.L1Loss with the demo's
    schedule on the CPU, in fp32 and fp64.  Sample 0 is demo/coco_joint_input.npy; 1-23 random COCO detections (pelvis and neck
    appended, the fit on the first 17), 24-47 random H36M-17 ones.  joints3d projects near its target (s in [0.7, 1.2], |t| <= 0.1,
    3 cm noise) except for four samples whose joints are shuffled (ill-conditioned fits) and two whose detections collapse to one
    point (valid = 0, target 0).  Raw joints are float32 values (what the device reads)."""
    scratch = tempfile.mkdtemp(prefix='gator_golden_')
    install_shims(scratch, True)
    for m in [k for k in sys.modules if k in ('coord_utils', 'aug_utils')]:
        del sys.modules[m]
    import aug_utils
    import coord_utils
    demo = _import_demo_run()
    import models  # noqa: F401  (reference lib/models)
    import models.project_net as ref_pn
    N, crop, img_w, img_h = 48, 500, 1920, 1080
    shuffled, collapsed = (5, 17, 30, 41), (20, 44)
    rs = np.random.RandomState(2027)
    raw = np.zeros((N, 17, 2), np.float32)
    raw[0] = np.load(os.path.join(REF, 'demo', 'coco_joint_input.npy'))[:, :2]
    for i in range(1, N):
        c = rs.rand(2) * np.array([1200, 500]) + np.array([350, 280])
        ext = np.array([rs.rand() * 250 + 60, rs.rand() * 450 + 120])
        raw[i] = c + (rs.rand(17, 2) - 0.5) * ext
        if i in collapsed:
            raw[i] = raw[i, :1]
    is_coco = (np.arange(N) < 24).astype(np.int32)
    xy = np.zeros((N, 19, 2), np.float32)
    bbox = np.zeros((N, 4), np.float32)
    valid = np.ones(N, np.int32)
    for i in range(N):
        j = raw[i].astype(np.float64)
        if is_coco[i]:
            j = np.concatenate([j, (j[11:12] + j[12:13]) * 0.5, (j[5:6] + j[6:7]) * 0.5])    # demo/run.py:103-121 (pelvis, neck)
        b1 = coord_utils.process_bbox(coord_utils.get_bbox(j).copy(), aspect_ratio=1.0, scale=1.25)
        if b1 is None:
            valid[i] = 0
            continue
        out, _ = aug_utils.j2d_processing(j.copy(), (crop, crop), b1, 0, 0, None)
        xy[i, :len(j)] = out[:, :2]
        bbox[i] = b1
    target = xy[:, :17]
    s_true = 0.7 + rs.rand(N) * 0.5
    t_true = (rs.rand(N, 2) - 0.5) * 0.2
    p = (target - crop / 2) / (s_true[:, None, None] * (crop / 2)) - t_true[:, None, :] + rs.randn(N, 17, 2) * 0.03
    for i in shuffled:
        p[i] = p[i, rs.permutation(17)]
    joints3d = np.concatenate([p, rs.randn(N, 17, 1) * 0.1], 2).astype(np.float32)
    torch.manual_seed(7)
    init = torch.rand(N, 3).numpy()
    snaps = (1, 10, 1500)
    cams = {}
    losses = {}
    for dt, tag in ((torch.float32, 'f32'), (torch.float64, 'f64')):
        cams[tag] = np.zeros((len(snaps), N, 3), np.float64)
        losses[tag] = np.zeros(N, np.float64)
        for i in range(N):
            layer = ref_pn.get_model(crop_size=crop).to(dt)
            with torch.no_grad():
                layer.cam_param.copy_(torch.from_numpy(init[i:i + 1]).to(dt))
            pred_3d_joint = torch.from_numpy(joints3d[i:i + 1]).to(dt)
            target_joint = torch.from_numpy(xy[i:i + 1]).to(dt)
            criterion = nn.L1Loss()
            optimizer = torch.optim.Adam(layer.parameters(), lr=0.1)
            layer.train()
            for j in range(0, 1500):                    # demo/run.py:150-157
                pred_2d_joint = layer(pred_3d_joint.detach())
                loss = criterion(pred_2d_joint, target_joint[:, :17, :])
                optimizer.zero_grad()
                loss.backward()
                optimizer.step()
                if j == 500:
                    for param_group in optimizer.param_groups:
                        param_group['lr'] = 0.05
                if j == 1000:
                    for param_group in optimizer.param_groups:
                        param_group['lr'] = 0.001
                if j + 1 in snaps:
                    cams[tag][snaps.index(j + 1), i] = layer.cam_param[0].detach().double().numpy()
            with torch.no_grad():
                losses[tag][i] = float(criterion(layer(pred_3d_joint), target_joint[:, :17, :]))
    cam32 = cams['f32'][-1].astype(np.float32)
    orig_cam = demo.convert_crop_cam_to_orig_img(cam=cam32, bbox=bbox, img_width=img_w, img_height=img_h).astype(np.float32)
    np.savez_compressed(os.path.join(OUT, 'cam_fit.npz'), raw=raw, is_coco=is_coco, crop_size=np.int32(crop), xy=xy, bbox=bbox,
                        valid=valid, joints3d=joints3d, init=init, snap_steps=np.array(snaps, np.int32), cam_f32=cams['f32'],
                        cam_f64=cams['f64'], loss_f32=losses['f32'], loss_f64=losses['f64'], image_size=np.array([img_w, img_h], np.int32),
                        orig_cam=orig_cam, shuffled=np.array(shuffled, np.int32))
    d = np.abs(cams['f32'][-1] - cams['f64'][-1]).max(1)
    print('camfit: %d samples (%d invalid), 1500-step |f32 - f64| max %.2e, median loss %.3f px'
          % (N, int((valid == 0).sum()), d.max(), float(np.median(losses['f64']))))


if __name__ == '__main__':
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(8)
    only = sys.argv[1:]
    if not only or 'base' in only:
        dump_jregressors()
        run_variant('h36m17_bn', 17, False, seed=0)
        run_variant('coco19_alpha', 19, True, seed=100)
        demo_preprocess_golden()
    if not only or 'scale' in only:
        sub = np.sort(np.random.RandomState(99).permutation(6890)[:512])
        run_variant('h36m17_bn', 17, False, seed=0, B=64, upsample_gain=0.2, subset=sub, out_name='scale_gain02')
        run_variant('h36m17_bn', 17, False, seed=0, B=64, upsample_gain=1.0, subset=sub, out_name='scale_gain10')
    if not only or 'train' in only:
        train_golden('h36m17_bn', 17, False, seed=0)
        train_golden('coco19_alpha', 19, True, seed=100)
    if not only or 'train_drop' in only:
        train_drop_golden('h36m17_bn', 17, False, seed=0, mask_seed=2024)
        train_drop_golden('coco19_alpha', 19, True, seed=100, mask_seed=2025)
    if not only or 'rigid' in only:
        rigid_align_golden()
    if not only or 'preprocess' in only:
        preprocess_chain_golden()
    if not only or 'camfit' in only:
        camfit_golden()
