"""Pins the oracle's TRAINING restatement (oracle/gator_oracle.py: gator_forward_train, training_loss) to the real reference:
loss parts and per-parameter gradients of one training step recorded by tools/gen_golden.py::train_golden (reference modules in
.train() with dropout p = 0, lib/core/loss.py criteria, lib/core/base.py:137-148 weighting, torch autograd), and by
train_drop_golden with every dropout and DropPath site ON under host-drawn Philox masks (tests/train_refs.py::DropSites): the
oracle must call the same sites, in the same order, with the same probabilities and shapes, as the reference's modules did."""
import numpy as np
import pytest
import torch

from gator_amd import synthetic
from gator_amd.train.model import is_buffer
from oracle import gator_oracle as go
from tests.helpers import load_golden, oracle_setup
from tests.train_refs import PATH_FAMILIES, DropSites, keep_mask, live_path_families, path_families


def oracle_step(name, dtype=torch.float64, batch=None, seed_shift=0, golden='train_', drop=None, rates=None):
    z = load_golden(golden + name)
    zz, c, sd = oracle_setup(name)
    J, seed = int(z['num_joint']), int(z['seed'])
    B = int(z['batch']) if batch is None else batch
    base = synthetic.make_base_data(seed)
    P = {k: (v.to(dtype).requires_grad_(True) if (v.is_floating_point() and not is_buffer(k)) else v) for k, v in sd.items()}
    pose2d = torch.from_numpy(z['pose2d'] if batch is None else synthetic.synthetic_pose2d(B, J, seed + 3 + seed_shift))
    jreg = synthetic.load_j_regressors()['h36m'].astype(np.float32)
    tg = {k: torch.from_numpy(v) for k, v in synthetic.training_targets(B, J, base, jreg, seed + seed_shift).items()}
    if drop is None:
        mesh, pose3d = go.gator_forward_train(P, c, pose2d, dtype)
    else:
        mesh, pose3d = go.gator_forward_train(P, c, pose2d, dtype, drop=drop, rates=rates)
    loss, parts = go.training_loss(mesh, pose3d, tg, jreg, synthetic.synthetic_faces(seed), with_edge=True)
    names = [k for k in P if torch.is_tensor(P[k]) and P[k].requires_grad]
    grads = dict(zip(names, torch.autograd.grad(loss, [P[k] for k in names], allow_unused=True)))
    return z, loss, parts, grads, (pose2d, tg, jreg, mesh.detach(), pose3d.detach())


def check_against_recording(name, z, loss, parts, grads, what):
    want = z['loss_parts_f64']                                            # vertice, normal, edge, mesh2joint3d, liftedjoint3d, total
    got = [float(parts[k].detach()) for k in ('vertice', 'normal', 'edge', 'mesh2joint3d', 'liftedjoint3d')] + [float(loss.detach())]
    assert np.allclose(got, want, rtol=5e-9, atol=0)      # (the reference's fp64 run keeps a few float32 constants)
    names = [str(k) for k in z['param_names']]
    assert sorted(grads) == names                                         # the same parameter set as model.named_parameters()
    worst = 0.0
    for i, k in enumerate(names):
        idx = z['probe_idx'][i]
        n = int((idx >= 0).sum())
        g = grads[k]
        g = torch.zeros_like(g) if g is None else g
        got = g.reshape(-1).numpy()[idx[:n]]
        scale = max(float(z['grad_absmax'][i]), 1e-300)
        err = np.abs(got - z['grad_f64'][i][:n]).max()
        assert abs(float(g.abs().max()) - float(z['grad_absmax'][i])) <= 1e-7 * scale + 1e-16, k
        assert err <= 1e-7 * scale + 1e-16, (k, err, scale)
        if scale > 1e-9:                                                  # (exactly-zero gradients have no relative error to report)
            worst = max(worst, err / scale)
    print('\n[%s] oracle training step %s vs reference fp64: %d tensors, worst probe error / max|g| = %.1e' % (name, what, len(names), worst))


def recorded_log(z):
    """the site log of a train_drop_*.npz as DropSites keeps it: (site, kind, rate, shape, offset) per draw"""
    return [(str(n), str(k), float(p), tuple(int(d) for d in s if d >= 0), int(o))
            for n, k, p, s, o in zip(z['site_name'], z['site_kind'], z['site_p'], z['site_shape'], z['site_offset'])]


@pytest.mark.parametrize('name', ['h36m17_bn', 'coco19_alpha'])
def test_oracle_training_step_matches_reference(name):
    z, loss, parts, grads, _ = oracle_step(name)
    check_against_recording(name, z, loss, parts, grads, '(dropout off)')


@pytest.mark.parametrize('name', ['h36m17_bn', 'coco19_alpha'])
def test_oracle_dropout_step_matches_reference(name):
    """Every dropout / DropPath site on: the oracle under DropSites(mask_seed) against the real reference's fp64 step under the
    same host masks, at the bounds of the dropout-off test; and the oracle's site log equals the reference's, entry by entry."""
    z = load_golden('train_drop_' + name)
    sites = DropSites(int(z['mask_seed']))
    z, loss, parts, grads, _ = oracle_step(name, golden='train_drop_', drop=sites)
    want = recorded_log(z)
    assert len(want) == 58 and len(sites.log) == 58
    assert sum(e[0].startswith('pose_lifter.') for e in want) == 34 and sum(e[0].startswith('pose2mesh.') for e in want) == 24
    for got, ref in zip(sites.log, want):
        assert got == ref, (got, ref)                                     # module name, kind, p, shape, offset
    assert [e[4] for e in want] == list(range(1, 59)) and sites.next_offset == 59
    check_against_recording(name, z, loss, parts, grads, '(dropout on, seed %d)' % int(z['mask_seed']))
    off = load_golden('train_' + name)                                    # and it is another function than the dropout-off step
    assert np.array_equal(off['pose2d'], z['pose2d']) and abs(z['loss_parts_f64'][-1] - off['loss_parts_f64'][-1]) > 1e-3 * off['loss_parts_f64'][-1]


@pytest.mark.parametrize('name', ['h36m17_bn', 'coco19_alpha'])
def test_recorded_masks_are_not_inert(name):
    """Each of the four DropPath families (GAT attention + MGCN branch, GAT MLP, MDR cross-attention, MDR MLP) has a recorded site
    that keeps one of the B = 4 samples and drops another - judged from the host masks alone - so a per-batch or per-element
    decision, a reused mask or a missing DropPath cannot reproduce the recording."""
    z = load_golden('train_drop_' + name)
    log, seed, B = recorded_log(z), int(z['mask_seed']), int(z['batch'])
    fam = path_families(log)
    assert [len(fam[f]) for f in PATH_FAMILIES] == [5, 5, 3, 3]           # block 0 of the lifter has nn.Identity (GAT.py:25)
    assert live_path_families(seed, log, B) == set(PATH_FAMILIES)
    for site, kind, rate, shape, offset in log:                           # every draw of the step both keeps and drops
        assert shape[0] == B
        n = B if kind == 'path' else int(np.prod(shape))
        kept = int(keep_mask(seed, offset, n, rate).sum())
        assert kind == 'path' or 0 < kept < n, (site, kept, n)


def test_drop_sites_offsets_and_step_word():
    a = DropSites(7)
    x = torch.ones(3, 5, 4, dtype=torch.float64)
    y0 = a('s0', x, 0.4)
    assert a('skip', x, 0.0) is x and len(a.log) == 1                     # rate 0 draws nothing
    y1 = a('s1', x, 0.25, True)
    assert a.log == [('s0', 'element', 0.4, (3, 5, 4), 1), ('s1', 'path', 0.25, (3, 5, 4), 2)] and a.next_offset == 3
    assert np.array_equal(y0.reshape(-1).numpy() != 0, keep_mask(7, 1, 60, 0.4).astype(bool))
    assert set(np.unique(y0.numpy())) == {0.0, 1.0 / 0.6}
    rows = y1.reshape(3, -1)
    assert bool((rows == rows[:, :1]).all())                              # one decision per sample, scaled by the keep probability
    assert np.array_equal(rows[:, 0].numpy(), keep_mask(7, 2, 3, 0.25).astype(np.float64) / 0.75)
    b = DropSites(7, first_offset=a.next_offset)                          # the second step of an eager stream runs on
    z0 = b('s0', x, 0.4)
    b('s1', x, 0.25, True)
    assert [e[4] for e in b.log] == [3, 4] and b.next_offset == 5
    assert np.array_equal(z0.reshape(-1).numpy() != 0, keep_mask(7, 3, 60, 0.4).astype(bool)) and not torch.equal(z0, y0)
    c = DropSites(7, step=2)                                              # the step word: same offsets, every mask another one
    w0 = c('s0', x, 0.4)
    w1 = c('s1', torch.ones(64, 2, dtype=torch.float64), 0.25, True)
    assert [e[4] for e in c.log] == [1, 2]
    assert np.array_equal(w0.reshape(-1).numpy() != 0, keep_mask(7, 1 + (2 << 32), 60, 0.4).astype(bool)) and not torch.equal(w0, y0)
    assert not np.array_equal(w1[:, 0].numpy() != 0, keep_mask(7, 2, 64, 0.25).astype(bool))
    f32 = DropSites(7)('s0', x.float(), 0.4)                              # the factor takes the run's dtype
    assert f32.dtype == torch.float32 and torch.equal(f32 != 0, y0 != 0)


@pytest.mark.parametrize('name', ['h36m17_bn', 'coco19_alpha'])
def test_oracle_without_drop_is_unchanged(name):
    """drop = None (bench.py's CPU baseline, every dropout-off reference) does no new work: gator_forward_train gives, bit for
    bit, what the site-aware branches give under a `drop` that returns its input, the eval forward ignores `drop`, and the
    dropout-off recording still holds for it (test_oracle_training_step_matches_reference)."""
    z = load_golden('train_' + name)
    zz, c, sd = oracle_setup(name)
    x = torch.from_numpy(z['pose2d'])
    calls = []

    def identity(site, t, rate, per_sample=False):
        calls.append(site)
        return t

    with torch.no_grad():
        mesh, pose3d = go.gator_forward_train(sd, c, x, torch.float64)
        mesh_i, pose3d_i = go.gator_forward_train(sd, c, x, torch.float64, drop=identity)
        assert len(calls) == 60                                           # block 0's DropPath is asked too, with rate 0
        assert torch.equal(mesh, mesh_i) and torch.equal(pose3d, pose3d_i)
        for got, want in ((mesh.numpy()[:, ::97], z['mesh_f64_probe']), (pose3d.numpy(), z['lift_pose_f64'])):
            assert float(np.abs(got - want).max()) <= 5e-9 * float(np.abs(want).max())       # the recorded outputs, at this file's rtol for the loss parts
        pc = torch.cat((x.double(), pose3d / 1000, go.gat_forward(sd, c, x.reshape(len(x), -1), torch.float64)[1]), dim=2)
        calls.clear()
        assert torch.equal(go.mdr_forward(sd, c, pc, torch.float64), go.mdr_forward(sd, c, pc, torch.float64, drop=identity)) and not calls
