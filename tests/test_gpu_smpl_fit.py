"""gator_smpl_fit_f32 / gator_smpl_fit_normal_f32 (SMPLLayer.fit, fit_normal) on the device against the float64 restatement of the
iteration, tests/smpl_fit_refs.py.  Every bound comes from that file: the stage's D(NV) u sum|J_a J_b| + floor is derived in its
docstring; K_FLOOR and EPS_NOISY are the figures of the float32-emulated reference (host test 4, profiles/smpl_fit.txt).  Every test
prints its measured figures before it asserts.

Sizes.  The normal kernel's tile is 64 vertices and a workgroup's chunk 512, so NV takes 1 / 63 / 64 / 65 / 127 / 128 / 129 / 257 and 6890
(14 chunks, the last one partial); B takes 1 / 2 / 33 / 65."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from gator_amd import _lib, smpl
from tests import smpl_fit_refs as fr
from tests import smpl_refs as sr

pytestmark = pytest.mark.gpu

BATCHES = (1, 2, 33, 65)
STAGE_NV = (1, 63, 64, 65, 127, 128, 129, 257, 6890)


def make_layer(m):
    return smpl.SMPLLayer.from_arrays(m['v_template'], m['shapedirs'], m['posedirs'], m['weights'], m['J_regressor'], m['parents'], faces=m['faces'])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    return t.cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def table_layer(name):
    return make_layer(fr.model(name))


@functools.lru_cache(maxsize=None)
def stage_case(nv):
    """65 states and targets on a model of nv vertices: sample 0 at zero, sample 1 from the pi family (two joints turned by fp32's pi),
    the rest generic (axis-angle entries ~0.4 rad, betas in +-2.5, |trans| ~ 1 m); the target is another draw's mesh."""
    m = sr.synthetic_model(nv, 24, 10, 300 + nv % 1000)
    rs = np.random.RandomState(nv)
    B = 65
    pose = (rs.randn(B, 72) * 0.4).astype(np.float32)
    betas = rs.uniform(-2.5, 2.5, (B, 10)).astype(np.float32)
    trans = rs.randn(B, 3).astype(np.float32)
    pose[0], betas[0], trans[0] = 0.0, 0.0, 0.0
    pose[1] = 0.0
    pose[1, 3:6] = (np.float32(np.pi), 0.0, 0.0)
    pose[1, 48:51] = (0.0, 0.0, np.float32(np.pi))
    n_t = 65 if nv <= 257 else 2
    tv, _ = sr.lbs_forward(m, (rs.randn(n_t, 72) * 0.4), rs.uniform(-2.5, 2.5, (n_t, 10)), rs.randn(n_t, 3))
    target = np.ascontiguousarray(tv[np.arange(B) % n_t].astype(np.float32))
    return m, make_layer(m), (pose, betas, trans), target


@pytest.mark.parametrize('nv', STAGE_NV)
def test_stage_against_the_fp64_normal_matrix(nv):
    m, layer, st, target = stage_case(nv)
    P, N = layer.fit_width()
    assert (P, N) == fr.widths(m) == (85, 96)
    runs = {B: layer.fit_normal(dev(st[0][:B]), dev(st[1][:B]), dev(st[2][:B]), dev(target[:B])) for B in BATCHES}
    for B in BATCHES:                                       # a sample's M does not depend on the batch around it
        assert torch.equal(runs[B], runs[65][:B]), B
    M = host(runs[65])
    iu = np.triu_indices(N)
    assert np.isfinite(M[:, iu[0], iu[1]]).all()
    for b in (0, 1, 2, 64):
        s = tuple(a[b] for a in st)
        tg = target[b].astype(np.float64)
        ref = fr.normal_matrix(m, *(a[b:b + 1] for a in st), tg[None])[0]
        bound = fr.stage_bound(m, *s, tg)
        err = np.abs(M[b] - ref)[iu]
        bd = bound[iu]
        worst = (err[bd > 0] / bd[bd > 0]).max()
        print('smpl fit stage NV %4d sample %2d: max |dev - ref| %.3e, worst err / bound %.3e, err (M[P][P]) %.6e ref %.6e'
              % (nv, b, err.max(), worst, M[b, P, P], ref[P, P]))
        assert (err <= bd).all()


def run_fit(layer, target, init=None, iters=fr.ITERS):
    out = layer.fit(dev(target), iters=iters, init=None if init is None else tuple(dev(a) for a in init))
    return tuple(t.cpu().numpy() for t in out)


def check_floor(label, name, truth, tgt, out):
    """bound 2: the returned parameters, pushed through fp64 lbs_forward, reproduce the target within K_FLOOR e32, and out_rms agrees
    with that fp64-evaluated rms within the same bound."""
    m = fr.model(name)
    pose, betas, trans, rms = out
    for i in range(len(tgt)):
        e32 = fr.e32_of(m, tuple(a[i] for a in truth), tgt[i])
        ev = fr.rms_of(m, (pose[i], betas[i], trans[i]), tgt[i])
        print('smpl fit %-12s sample %d: fp64-evaluated rms %.3e m, out_rms %.3e m, e32 %.3e m, bound K e32 = %.3e m'
              % (label, i, ev, rms[i], e32, fr.K_FLOOR * e32))
        assert ev <= fr.K_FLOOR * e32
        assert abs(float(rms[i]) - ev) <= fr.K_FLOOR * e32


@functools.lru_cache(maxsize=None)
def table_rows():
    return list(fr.table())


@pytest.mark.parametrize('row', range(10))
def test_whole_fit_reaches_the_float32_floor(row):
    label, name, truth, tgt, init = table_rows()[row]
    check_floor(label, name, truth, tgt, run_fit(table_layer(name), tgt, init))


@pytest.mark.parametrize('row', range(1, 10, 2))
def test_warm_start_in_eight_iterations(row):
    label, name, truth, tgt, init = table_rows()[row]
    assert init is not None
    check_floor(label + '/warm8', name, truth, tgt, run_fit(table_layer(name), tgt, init, fr.WARM_ITERS))


def test_noisy_target_reaches_the_reference_minimum():
    name, tgt = fr.noisy_target()
    m = fr.model(name)
    st64, _ = fr.fit(m, tgt[0], None, fr.ITERS)
    r64 = fr.rms_of(m, st64, tgt[0])
    pose, betas, trans, rms = run_fit(table_layer(name), tgt)
    ev = fr.rms_of(m, (pose[0], betas[0], trans[0]), tgt[0])
    print('smpl fit noisy: device fp64-evaluated rms %.12e m, float64 reference %.12e m, excess %.3e (eps %.3e), out_rms %.9e'
          % (ev, r64, ev / r64 - 1, fr.EPS_NOISY, rms[0]))
    assert ev <= r64 * (1 + fr.EPS_NOISY)


@functools.lru_cache(maxsize=None)
def batch_case():
    name = 'nv65'
    truth = fr.case_truth(name, fr.ZERO_INIT_MAX, n=65)
    tgt, _ = sr.lbs_forward(fr.model(name), *truth)
    return table_layer(name), np.ascontiguousarray(tgt.astype(np.float32))


def equal_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def test_rows_do_not_depend_on_the_batch_and_repeat():
    layer, tgt = batch_case()
    full = layer.fit(dev(tgt), iters=10)
    assert all(torch.isfinite(t).all() for t in full)
    assert equal_bits(full, layer.fit(dev(tgt), iters=10))
    for B in BATCHES:
        part = layer.fit(dev(tgt[:B]), iters=10)
        assert equal_bits(part, tuple(t[:B] for t in full)), B


def test_a_bad_sample_stays_alone():
    layer, tgt = batch_case()
    tgt = tgt[:33]
    good = layer.fit(dev(tgt), iters=6)
    bad_t = tgt.copy()
    bad_t[3, 17, 1] = np.nan
    bad_t[31, 0, 0] = np.inf
    out = layer.fit(dev(bad_t), iters=6)
    keep = [i for i in range(33) if i not in (3, 31)]
    for o, g in zip(out, good):
        assert torch.isnan(o[3]).all() and torch.isnan(o[31]).all()
        assert torch.equal(o[keep], g[keep])
    init = [t.clone() for t in good[:3]]                    # a non-finite start
    init[0][5, 10] = float('nan')
    init[1][6, 2] = float('inf')
    init[2][7, 0] = float('nan')
    ref = layer.fit(dev(tgt), iters=3, init=tuple(good[:3]))
    out = layer.fit(dev(tgt), iters=3, init=tuple(init))
    keep = [i for i in range(33) if i not in (5, 6, 7)]
    for o, g in zip(out, ref):
        assert torch.isnan(o[[5, 6, 7]]).all()
        assert torch.equal(o[keep], g[keep])


def test_graph_capture_and_workspace():
    layer, tgt = batch_case()
    x = dev(tgt[:33])
    eager = layer.fit(dev(tgt), iters=5)                    # the largest call: the workspace is sized here
    ws = layer.workspace()
    assert ws[1] >= 65
    eager33 = layer.fit(x, iters=5)
    assert layer.workspace() == ws
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        layer.fit(x, iters=5)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = layer.fit(x, iters=5)
    for t in out:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert equal_bits(out, eager33)
    g.replay()
    torch.cuda.synchronize()
    assert equal_bits(out, eager33) and equal_bits(eager33, tuple(t[:33] for t in eager))
    assert layer.workspace() == ws


def test_argument_checks():
    layer, tgt = batch_case()
    lib = _lib.load()
    B = 2
    x = dev(tgt[:B])
    outs = [torch.full((B, 72), 7.0).cuda(), torch.full((B, 10), 7.0).cuda(), torch.full((B, 3), 7.0).cuda(), torch.full((B,), 7.0).cuda()]
    init = [torch.zeros(B, 72).cuda(), torch.zeros(B, 10).cuda(), torch.zeros(B, 3).cuda()]
    p = _lib.ptr

    def call(ctx, target, ini, iters, o):
        return lib.gator_smpl_fit_f32(ctx, target, ini[0], ini[1], ini[2], B, iters, o[0], o[1], o[2], o[3], None)

    none3, po, pi = [None] * 3, [p(t) for t in outs], [p(t) for t in init]
    bad = {'null ctx': (None, p(x), none3, 5, po), 'null target': (layer._ctx, None, none3, 5, po),
           'iters 0': (layer._ctx, p(x), none3, 0, po), 'iters 257': (layer._ctx, p(x), none3, 257, po),
           'partial init': (layer._ctx, p(x), [pi[0], None, pi[2]], 5, po), 'pose-only init': (layer._ctx, p(x), [pi[0], None, None], 5, po)}
    for k in range(4):
        o = list(po)
        o[k] = None
        bad['null output %d' % k] = (layer._ctx, p(x), none3, 5, o)
    for what, args in bad.items():
        assert call(*args) == -1, what                      # GATOR_EINVAL
        assert len(lib.gator_last_error()) > 20, what
    assert lib.gator_smpl_fit_normal_f32(layer._ctx, pi[0], pi[1], pi[2], p(x), B, None, None) == -1
    dense = make_layer(sr.synthetic_model(65, 24, 10, 19, True))
    assert call(dense._ctx, p(x), none3, 5, po) == -6       # GATOR_EUNSUPPORTED
    assert b'influences' in lib.gator_last_error()
    M = torch.full((B, 96, 96), 7.0).cuda()
    assert lib.gator_smpl_fit_normal_f32(dense._ctx, pi[0], pi[1], pi[2], p(x), B, p(M), None) == -6
    with pytest.raises(RuntimeError, match='influences'):
        dense.fit(x)
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs + [M])  # nothing was launched
    with pytest.raises(ValueError):
        layer.fit(x[:, :10])
    pose, betas, trans, rms = smpl.fit_to_mesh(layer, x, iters=3)
    assert pose.shape == (B, 72) and betas.shape == (B, 10) and trans.shape == (B, 3) and rms.shape == (B,)
