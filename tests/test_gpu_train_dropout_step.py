"""The training step with every dropout and DropPath site ON, end to end on the GPU: gator_amd/train/model.py must use the
dropout kernels where, in the order and at the rates the reference's modules do in .train().  The kernels' masks are pinned to the
host Philox (tests/test_gpu_train_dropout_ref.py); here the whole step is - against (a) the REAL reference's step recorded under
host-drawn masks (tests/golden/train_drop_*.npz, tools/gen_golden.py::train_drop_golden) and (b) float64 autograd of the oracle
with the same masks handed in (oracle/gator_oracle.py `drop=`, tests/train_refs.py::DropSites), which the host test
tests/test_oracle_train_golden.py pins to that recording site by site.  The masks are fixed, so the step is as smooth a function
as with dropout off: every bound is the one of the dropout-off sibling in tests/test_gpu_train_step.py."""
import functools

import numpy as np
import pytest
import torch

from gator_amd import synthetic
from gator_amd.train import model as M
from gator_amd.train import ops
from oracle import gator_oracle as go
from tests.helpers import build_model, load_golden, oracle_setup
from tests.test_gpu_train_step import batch_of, make_trainer
from tests.train_refs import PATH_FAMILIES, DropSites, check_close, live_path_families

pytestmark = pytest.mark.gpu

PART_KEYS = ('vertice', 'normal', 'edge', 'mesh2joint3d', 'liftedjoint3d')


@functools.lru_cache(maxsize=None)
def _oracle_inputs(name):
    z, c, sd = oracle_setup(name)
    seed = int(load_golden('train_drop_' + name)['seed'])
    return c, sd, seed, synthetic.make_base_data(seed), synthetic.load_j_regressors()['h36m'].astype(np.float32), synthetic.synthetic_faces(seed)


def oracle_drop_step(name, sites, rates=None, batch=None, shift=0, grads=True, dtype=torch.float64):
    """One step of the oracle under the masks of `sites` on the batch batch_of(z, batch, shift) builds -> (loss parts + total as
    a list, {name: gradient} or None, mesh, pose3d)"""
    c, sd, seed, base, jreg, faces = _oracle_inputs(name)
    z = load_golden('train_drop_' + name)
    B = int(z['batch']) if batch is None else batch
    pose2d = torch.from_numpy(z['pose2d'] if batch is None else synthetic.synthetic_pose2d(B, c.J, seed + 3 + shift))
    tg = {k: torch.from_numpy(v) for k, v in synthetic.training_targets(B, c.J, base, jreg, seed + shift).items()}
    P = {k: (v.to(dtype).requires_grad_(grads) if (v.is_floating_point() and not M.is_buffer(k)) else v) for k, v in sd.items()}
    with torch.set_grad_enabled(grads):
        mesh, pose3d = go.gator_forward_train(P, c, pose2d, dtype, drop=sites, rates=rates)
        loss, parts = go.training_loss(mesh, pose3d, tg, jreg, faces, with_edge=True)
    out = None
    if grads:
        names = [k for k in P if torch.is_tensor(P[k]) and P[k].requires_grad]
        out = dict(zip(names, torch.autograd.grad(loss, [P[k] for k in names], allow_unused=True)))
    return [float(parts[k].detach()) for k in PART_KEYS] + [float(loss.detach())], out, mesh.detach(), pose3d.detach()


def parts_of(loss, parts):
    return [float(parts[k]) for k in PART_KEYS] + [float(loss)]


def check_whole_gradients(tag, tr, grad, ograds, only=None):
    """test_training_step_matches_oracle_autograd_other_batch's criterion on whole tensors: 1e-4 max|g| + 3e-6 sibling + 1e-9"""
    g = grad.cpu().double()
    worst, worst_k, seen = 0.0, None, 0
    for k, (a, b, shape) in zip(tr.params.names, tr.params.slots):
        if only is not None and k not in only:
            continue
        seen += 1
        og = ograds[k]
        og = torch.zeros(shape, dtype=torch.float64) if og is None else og
        scale = float(og.abs().max())
        sib = ograds.get(k[:-4] + 'weight') if k.endswith('.bias') else None          # (a softmax's key bias has an exactly-zero gradient)
        sibling = float(sib.abs().max()) if sib is not None else 0.0
        err = float((g[a:b].view(shape) - og).abs().max())
        if scale > 1e-9 and err / scale > worst:
            worst, worst_k = err / scale, k
        assert err <= 1e-4 * scale + 3e-6 * sibling + 1e-9, '%s: %.3e vs max|g| %.3e' % (k, err, scale)
    assert seen == (len(tr.params.names) if only is None else len(only))
    print('[%s] %d gradient tensors; worst error / max|g| = %.2e (%s)' % (tag, seen, worst, worst_k))


def assert_live(seed, log, B, step=0, families=PATH_FAMILIES):
    """a check of the TEST's masks, from the host Philox alone: every DropPath family keeps one sample and drops another somewhere"""
    assert set(families) <= live_path_families(seed, log, B, step), (seed, step, sorted(live_path_families(seed, log, B, step)))


@pytest.mark.parametrize('name', ['h36m17_bn', 'coco19_alpha'])
def test_dropout_step_matches_reference_recording(name):
    """Trainer with the reference's rates and seed = the recording's mask seed, on the recorded batch, against the real reference's
    step under the same masks: test_training_step_matches_reference_recording's criterion per parameter tensor,
    |ours - ref fp64| <= 4 x |ref fp32 - ref fp64| + 2e-5 max|g| + 3e-6 sibling + 1e-12 with the noise of THIS recording."""
    z = load_golden('train_drop_' + name)
    _, m, tr, _ = make_trainer(name, rates=M.Rates(), seed=int(z['mask_seed']))
    tr.epoch = 16                                                    # > edge_loss_start: all five losses (base.py:145-147)
    x, tg = batch_of(z)
    loss, parts, grad = tr.loss_and_grad(x, tg)
    want = z['loss_parts_f64']
    got = parts_of(loss, parts)
    print('\n[%s] loss parts ours %s\n%s reference fp64 %s' % (name, np.round(got, 6).tolist(), ' ' * len(name), np.round(want, 6).tolist()))
    assert np.allclose(got, want, rtol=2e-5)
    g = grad.cpu().double().numpy()
    names = [str(k) for k in z['param_names']]
    assert sorted(tr.params.names) == names
    slot = dict(zip(tr.params.names, tr.params.slots))
    worst, worst_k = 0.0, None
    absmax = dict(zip(names, z['grad_absmax']))
    for i, k in enumerate(names):
        a, b, shape = slot[k]
        idx = z['probe_idx'][i]
        n = int((idx >= 0).sum())
        got = g[a:b][idx[:n]]
        scale, noise = float(z['grad_absmax'][i]), float(z['ref32_minus_f64_max'][i])
        err = np.abs(got - z['grad_f64'][i][:n]).max()
        sibling = float(absmax.get(k[:-4] + 'weight', 0.0)) if k.endswith('.bias') else 0.0
        tol = 4.0 * noise + 2e-5 * scale + 3e-6 * sibling + 1e-12
        if scale > 1e-9 and err / scale > worst:
            worst, worst_k = err / scale, k
        assert err <= tol, '%s: err %.3e tol %.3e (max|g| %.3e, ref fp32 noise %.3e)' % (k, err, tol, scale, noise)
        assert abs(np.abs(g[a:b]).max() - scale) <= 4.0 * noise + 1e-4 * scale + 3e-6 * sibling + 1e-12, k
    print('[%s] %d parameter tensors; worst probe error / max|g| = %.2e (%s)' % (name, len(names), worst, worst_k))
    assert tr.gen.offset == 58                                        # 34 draws in the lifter, 24 in MDR


def distinct_rates():
    """eight different probabilities, none the reference's: a field used where its neighbour belongs changes a mask and a scale"""
    r = M.Rates()
    r.gat_attn, r.gat_proj, r.gat_mlp = 0.35, 0.45, 0.15
    r.gat_path = [0.0, 0.28, 0.12, 0.22, 0.27, 0.17]
    r.mdr_attn, r.mdr_drop, r.mdr_path, r.mdr_self = 0.25, 0.3, 0.33, 0.05
    vals = [r.gat_attn, r.gat_proj, r.gat_mlp, r.mdr_attn, r.mdr_drop, r.mdr_path, r.mdr_self] + r.gat_path
    assert len(set(vals)) == len(vals) and not set(vals) & {0.4, 0.1, 0.2}
    return r


DISTINCT_SEED = 3


def test_distinct_rates_match_oracle_autograd_other_batch():
    """J = 17 with BatchNorm, B = 3, another batch, eight different rates: every whole gradient tensor, the mesh and the lifted
    pose against float64 autograd of the oracle with the same rates and masks."""
    name, B, shift, seed = 'h36m17_bn', 3, 5, DISTINCT_SEED
    rates = distinct_rates()
    z = load_golden('train_drop_' + name)
    _, m, tr, _ = make_trainer(name, rates=rates, seed=seed)
    tr.epoch = 16
    x, tg = batch_of(z, B, shift=shift)
    loss, parts, grad = tr.loss_and_grad(x, tg)
    assert tr.gen.offset == 58
    mesh, pose3d = M.gator_forward(tr.params.views(), tr.consts, x, ops.Generator(seed), rates, True, tr.params.buffers)    # the same masks again
    sites = DropSites(seed)
    oparts, ograds, omesh, opose = oracle_drop_step(name, sites, rates, B, shift)
    assert len(sites.log) == 58
    assert_live(seed, sites.log, B)
    print()
    assert np.allclose(parts_of(loss, parts), oparts, rtol=2e-5), (parts_of(loss, parts), oparts)
    check_close('mesh (m)', mesh, omesh)
    check_close('pose3d (mm)', pose3d, opose)
    check_whole_gradients('distinct rates, B=3', tr, grad, ograds)


def test_offsets_run_on_over_eager_steps():
    """Without a device step counter the Philox offset runs on: the second loss_and_grad of a trainer draws 59 .. 116."""
    name, B, shift, seed = 'coco19_alpha', 3, 7, 7
    z = load_golden('train_drop_' + name)
    _, m, tr, _ = make_trainer(name, rates=M.Rates(), seed=seed)
    tr.epoch = 16
    x, tg = batch_of(z, B, shift=shift)
    tr.loss_and_grad(x, tg)
    assert tr.gen.offset == 58
    loss, parts, grad = tr.loss_and_grad(x, tg)
    assert tr.gen.offset == 116
    sites = DropSites(seed, first_offset=59)
    oparts, ograds, _, _ = oracle_drop_step(name, sites, None, B, shift)
    assert [e[4] for e in sites.log] == list(range(59, 117))
    assert_live(seed, sites.log, B)
    print()
    assert np.allclose(parts_of(loss, parts), oparts, rtol=2e-5), (parts_of(loss, parts), oparts)
    check_whole_gradients('second eager step', tr, grad, ograds,
                          only=('pose_lifter.blocks.3.attn.qkv.weight', 'pose2mesh.encoder_1.attn.wq.weight', 'pose2mesh.selfatt_2.linears.0.weight'))


def test_eval_draws_nothing():
    """training=False with the reference's rates: no site takes an offset, and the forward, the loss and the gradient are, bit for
    bit, those of a trainer whose rates are all 0."""
    name = 'h36m17_bn'
    z = load_golden('train_drop_' + name)
    _, m, on, _ = make_trainer(name, rates=M.Rates(), seed=9)
    _, m, off, _ = make_trainer(name)
    on.epoch = off.epoch = 16
    x, tg = batch_of(z, 3, shift=2)
    l1, p1, g1 = on.loss_and_grad(x, tg, training=False)
    assert on.gen.offset == 0
    l0, p0, g0 = off.loss_and_grad(x, tg, training=False)
    assert float(l1) == float(l0) and torch.equal(g1, g0) and all(torch.equal(p1[k], p0[k]) for k in p0)
    mesh1, pose1 = M.gator_forward(on.params.views(), on.consts, x, on.gen, on.rates, False, on.params.buffers)
    mesh0, pose0 = M.gator_forward(off.params.views(), off.consts, x, off.gen, off.rates, False, off.params.buffers)
    assert on.gen.offset == 0 and torch.equal(mesh1, mesh0) and torch.equal(pose1, pose0)
    assert float(g1.abs().max()) > 0


def test_lift_trainer_with_dropout_matches_oracle_autograd():
    """LiftTrainer with the reference's rates: 34 draws, all gradients against float64 autograd of the oracle's gat_forward under
    the same masks (test_lift_trainer_matches_oracle_autograd's bounds)."""
    from gator_amd.train.trainer import LiftTrainer
    name, B, J, seed = 'coco19_alpha', 3, 19, 5
    zz, m = build_model(name, 'fused')
    lt = LiftTrainer.from_module(m.pose_lifter, rates=M.Rates(), seed=seed)
    x = torch.from_numpy(synthetic.synthetic_pose2d(B, J, 21))
    cam = torch.from_numpy(np.random.RandomState(3).randn(B, J, 3).astype(np.float32) * 250)
    valid = torch.ones(B, J, 1)
    valid[1] = 0
    loss, grad = lt.loss_and_grad(x.cuda().reshape(B, -1), cam.cuda(), valid.cuda())
    assert lt.gen.offset == 34
    c, sd = _oracle_inputs(name)[:2]
    P = {k: (v.double().requires_grad_(True) if (v.is_floating_point() and not M.is_buffer(k)) else v) for k, v in sd.items() if k.startswith('pose_lifter.')}
    sites = DropSites(seed)
    x_out, _ = go.gat_forward(P, c, x.reshape(B, -1), torch.float64, drop=sites)
    assert len(sites.log) == 34
    assert_live(seed, sites.log, B, families=PATH_FAMILIES[:2])
    oloss = go.coord_loss(x_out.reshape(B, J, 3), cam.double(), valid.double())
    assert abs(float(loss) - float(oloss.detach())) <= 1e-5 * float(oloss.detach())
    g = grad.cpu().double()
    keys = ['pose_lifter.' + k for k in lt.params.names]
    ograds = torch.autograd.grad(oloss, [P[k] for k in keys], allow_unused=True)
    worst, worst_k = 0.0, None
    for k, (a, b, shape), og in zip(lt.params.names, lt.params.slots, ograds):
        og = torch.zeros(shape, dtype=torch.float64) if og is None else og
        scale = float(og.abs().max())
        err = float((g[a:b].view(shape) - og).abs().max())
        if scale > 1e-9 and err / scale > worst:
            worst, worst_k = err / scale, k
        assert err <= 1e-4 * scale + 1e-9, (k, err, scale)
    print('\n[lifter, dropout on] %d gradient tensors; worst error / max|g| = %.2e (%s)' % (len(keys), worst, worst_k))


@pytest.mark.parametrize('eager_steps', [0, 2])
def test_captured_step_draws_the_promised_masks(eager_steps):
    """Trainer.capture's docstring: replay n draws offsets 1 .. 58 in the step word optim.step_count (before capture) + n.  lr = 0
    keeps the weights at their initial values, so the oracle needs no state from the device."""
    name, B, shift, seed = 'h36m17_bn', 3, 4, 13
    z = load_golden('train_drop_' + name)
    _, m, tr, _ = make_trainer(name, rates=M.Rates(), seed=seed, lr=0.0)
    tr.epoch = 16
    x, tg = batch_of(z, B, shift=shift)
    for _ in range(eager_steps):
        tr.step(x, tg)
    before = tr.optim.step_count
    assert before == eager_steps
    tr.capture(x, tg)
    print()
    for n in (1, 2):
        loss, parts = tr.step(x, tg)
        sites = DropSites(seed, first_offset=1, step=before + n)
        oparts = oracle_drop_step(name, sites, None, B, shift, grads=False)[0]
        assert [e[4] for e in sites.log] == list(range(1, 59))
        assert_live(seed, sites.log, B, step=before + n)
        got = parts_of(loss, parts)
        print('[captured after %d eager steps] replay %d: worst relative loss-part error %.2e' % (eager_steps, n, max(abs(a - b) / abs(b) for a, b in zip(got, oparts))))
        assert np.allclose(got, oparts, rtol=2e-5), (n, got, oparts)
