"""References of the SMPL layer's backward tests: the layer once more in torch float64 (a restatement of smpl_refs.lbs_forward, which
restates smplpytorch's SMPL_Layer.forward; it shares no code with the kernels), its vector-Jacobian product by torch.autograd.grad, and
the seeded upstream gradients of the golden cases.  The upstream gradients are generated, not stored: [65,6890,3] is too large to
commit.  tests/golden/smpl_layer_grad.npz (tools/gen_golden_smpl_grad.py) pins the VJP to the real layer's fp32 autograd."""
import numpy as np
import torch

from tests import smpl_refs as sr

OUTPUTS = ('pose', 'betas', 'trans')
UPSTREAMS = ('full', 'verts', 'joints')


def case_options(name):
    """The forward options of a golden case, as tests/test_host_smpl.py reads them."""
    (nv, nj, nb, seed, dense), opt, keep = sr.CASES[name]
    return {'betas': opt.get('betas', True) and nb > 0, 'trans': opt.get('trans', True), 'center_idx': opt.get('center_idx'),
            'out_scale': opt.get('out_scale', 1.0), 'keep': keep}


def case_arguments(name):
    """(pose, betas | None, trans | None) of a golden case, float32, with the inputs the case does not use left out."""
    o = case_options(name)
    pose, betas, trans = sr.case_inputs(name)
    return pose, betas if o['betas'] else None, trans if o['trans'] else None


def upstream(name):
    """The case's upstream gradients, float32 standard normal: grad_verts [65,NV,3], grad_joints [65,NJ,3]."""
    (nv, nj, nb, seed, dense), _, _ = sr.CASES[name]
    rs = np.random.RandomState(2000 + seed)
    return rs.randn(sr.N_SAMPLES, nv, 3).astype(np.float32), rs.randn(sr.N_SAMPLES, nj, 3).astype(np.float32)


def rodrigues64(a):
    """[..., 3] axis-angles -> [..., 3, 3]: batch_rodrigues with its `+ 1e-8` inside the norm, then quat2mat with its normalisation."""
    angle = torch.sqrt(((a + 1e-8) ** 2).sum(-1, keepdim=True))
    half = angle * 0.5
    q = torch.cat([torch.cos(half), torch.sin(half) * (a / angle)], -1)
    q = q / torch.sqrt((q * q).sum(-1, keepdim=True))
    w, x, y, z = q.unbind(-1)
    rows = [w * w + x * x - y * y - z * z, 2 * x * y - 2 * w * z, 2 * w * y + 2 * x * z,
            2 * w * z + 2 * x * y, w * w - x * x + y * y - z * z, 2 * y * z - 2 * w * x,
            2 * x * z - 2 * w * y, 2 * w * x + 2 * y * z, w * w - x * x - y * y + z * z]
    return torch.stack(rows, -1).reshape(a.shape[:-1] + (3, 3))


def lbs_forward64(m, pose, betas=None, trans=None, center_idx=None, out_scale=1.0):
    """torch float64 tensors in, (verts [B,NV,3], joints [B,NJ,3]) out; differentiable in pose, betas and trans."""
    t = lambda k: torch.from_numpy(np.asarray(m[k], np.float64))      # noqa: E731
    vt, sd, pd, w, jr = t('v_template'), t('shapedirs'), t('posedirs'), t('weights'), t('J_regressor')
    nj = w.shape[1]
    B = pose.shape[0]
    R = rodrigues64(pose.reshape(B, nj, 3))
    pose_map = (R[:, 1:] - torch.eye(3, dtype=torch.float64)).reshape(B, (nj - 1) * 9)
    v_shaped = vt.expand(B, -1, -1)
    if betas is not None and sd.shape[2]:
        v_shaped = v_shaped + torch.einsum('vck,bk->bvc', sd, betas)
    J = torch.einsum('jv,bvc->bjc', jr, v_shaped)
    v_posed = v_shaped + torch.einsum('vck,bk->bvc', pd, pose_map)
    GR, Gt = [R[:, 0]], [J[:, 0]]
    for j in range(1, nj):
        p = int(m['parents'][j])
        GR.append(GR[p] @ R[:, j])
        Gt.append(torch.einsum('brc,bc->br', GR[p], J[:, j] - J[:, p]) + Gt[p])
    GR, Gt = torch.stack(GR, 1), torch.stack(Gt, 1)                  # [B,NJ,3,3], [B,NJ,3]
    At = Gt - torch.einsum('bjrc,bjc->bjr', GR, J)
    TR = torch.einsum('vj,bjrc->bvrc', w, GR)
    Tt = torch.einsum('vj,bjr->bvr', w, At)
    verts = torch.einsum('bvrc,bvc->bvr', TR, v_posed) + Tt
    joints = Gt
    if trans is not None:
        if center_idx is not None:
            raise ValueError('center_idx goes with trans = None')
        off = trans[:, None, :]
    elif center_idx is not None:
        off = -joints[:, center_idx:center_idx + 1]
    else:
        off = 0.0
    return (verts + off) * out_scale, (joints + off) * out_scale


def vjp64(model, inputs, options, gV, gJ):
    """inputs: (pose, betas | None, trans | None) as numpy; options: {'center_idx', 'out_scale'}; gV [B,NV,3] | None, gJ [B,NJ,3] | None.
    -> {'pose', 'betas', 'trans'}: float64 numpy gradients of sum(verts * gV) + sum(joints * gJ), None for an input that is absent."""
    leaves = [None if a is None else torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(True) for a in inputs]
    verts, joints = lbs_forward64(model, *leaves, options.get('center_idx'), options.get('out_scale', 1.0))
    outs, grads = [], []
    if gV is not None:
        outs.append(verts)
        grads.append(torch.from_numpy(np.asarray(gV, np.float64)))
    if gJ is not None:
        outs.append(joints)
        grads.append(torch.from_numpy(np.asarray(gJ, np.float64)))
    have = [x for x in leaves if x is not None]
    got = iter(torch.autograd.grad(outs, have, grads, allow_unused=True))
    res = {}
    for name, leaf in zip(OUTPUTS, leaves):
        if leaf is None:
            res[name] = None
        else:
            g = next(got)
            res[name] = np.zeros(leaf.shape) if g is None else g.numpy()
    return res


def select_upstream(which, gV, gJ):
    return (gV if which in ('full', 'verts') else None), (gJ if which in ('full', 'joints') else None)
