"""gator_mesh_errors_f32 (csrc/mesh_eval.hip: k_mesh_errors) at its edges, against the fp64 reference of tests/mesh_eval_refs.py (the
oracle's regress_joints, mpjpe and rigid_align per sample): vertex counts either side of the 64-lane wave and the 256-thread workgroup,
the input families of tests/eval_edge_refs.py, the regressor's edges, batch invariance, the C ABI's refusals, graph capture, and
gator_amd.eval.MeshEvaluator.  Every sample and every column is compared.

The bound is the suite's criterion for an error column plus the input-rounding term of its criterion for aligned points
(mesh_eval_refs.mesh_bound): 2e-5 max(1, want) + 3e-7 max|scaled coordinate of the sample|.

`python -m pytest tests/test_gpu_mesh_eval.py -q -s -m gpu` prints the ratios kept in profiles/mesh_eval.txt."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from gator_amd import _lib
from gator_amd import eval as geval
from tests import eval_edge_refs as er
from tests import mesh_eval_refs as mr

pytestmark = pytest.mark.gpu

EINVAL = -1
COLS = geval.MESH_ERROR_COLUMNS


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def run(p, t, *args, **kw):
    return geval.mesh_errors(dev(p), dev(t), *args, **kw).cpu().numpy()


def held(got, want, bound, what):
    """Every sample and column within its bound; NaN only where the reference has NaN.  Prints the worst ratio."""
    got = got.astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
    ok = ~np.isnan(want)
    ratio = np.zeros_like(want)
    ratio[ok] = np.abs(got - want)[ok] / np.broadcast_to(bound, want.shape)[ok]
    print('\n%-58s worst |ours - fp64 reference| / bound per column: %s' % (what, ' '.join('%.4f' % r for r in ratio.max(0))))
    assert (ratio <= 1.0).all(), (what, np.argwhere(ratio > 1.0)[:4].tolist(), float(ratio.max()))
    return ratio.max()


# ---- the vertex-count sweep -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def sweep_case(N):
    """65 body-like samples in metres (scale 1000 on both sides), a 24-row root regressor and a 17-row evaluation regressor, and the
    reference of every sample: computed once per N, shared by the batch sizes."""
    rs = np.random.RandomState(1000 + N)
    p, t = mr.body_like(rs, 65, N)
    jr, je = mr.sparse_rows(rs, 24, N), mr.sparse_rows(rs, 17, N)
    want = mr.oracle_mesh_errors(p, t, jr, 0, je, mr.H36M_EVAL, 0, 1000.0, 1000.0)
    assert np.isfinite(want).all()
    return p, t, jr, je, want


@pytest.mark.parametrize('N', [3, 4, 63, 64, 65, 255, 256, 257, 431, 513])
@pytest.mark.parametrize('B', [1, 2, 65])
def test_vertex_count_sweep(B, N):
    """One 256-thread workgroup per sample strides the vertices: counts under a wave, either side of a wave and of the workgroup, two
    and more strides, the coarse mesh's 431."""
    p, t, jr, je, want = sweep_case(N)
    got = run(p[:B], t[:B], jr, 0, je, pred_scale=1000.0, target_scale=1000.0)
    held(got, want[:B], mr.mesh_bound(want[:B], p[:B], t[:B], 1000.0, 1000.0), 'sweep B=%d N=%d' % (B, N))


@functools.lru_cache(maxsize=None)
def full_case():
    """Three 6890-vertex samples within 1 m of the origin with errors of ~10 cm; prediction in metres, target in mm (pred_scale 1000,
    target_scale 1); regressors of the shipped shapes, 24 and 17 sparse rows that each sum to 1."""
    rs = np.random.RandomState(6890)
    N = geval.N_VERTS
    t = rs.randn(3, N, 3) * 0.4 + rs.uniform(-0.5, 0.5, (3, 1, 3))
    p = (1.02 * t + rs.randn(3, 1, 3) * 0.03 + rs.randn(3, N, 3) * 0.06).astype(np.float32)
    t = (t * 1000.0).astype(np.float32)
    jr, je = mr.sparse_rows(rs, 24, N, per_row=5), mr.sparse_rows(rs, 17, N, per_row=6)
    want = mr.oracle_mesh_errors(p, t, jr, 0, je, mr.H36M_EVAL, 0, 1000.0, 1.0)
    return p, t, jr, je, want


def test_full_mesh_with_the_shipped_shapes_and_the_existing_entry_points():
    """N = 6890, B = 3, JointRegressor objects as regressors, against the reference; then columns 0 and 1 against
    joint_errors(JointRegressor(J)(mesh)) and column 3 against eval.mpvpe per sample, each within errors_bound."""
    p, t, jr, je, want = full_case()
    P, T = dev(p), dev(t)
    Jr, Je = geval.JointRegressor(jr, 'cuda'), geval.JointRegressor(je, 'cuda')
    got = geval.mesh_errors(P, T, Jr, 0, Je, pred_scale=1000.0).cpu().numpy()
    held(got, want, mr.mesh_bound(want, p, t, 1000.0, 1.0), 'full mesh B=3 N=6890')
    assert np.array_equal(bits(got), bits(run(p, t, jr, 0, je, pred_scale=1000.0))), 'a dense regressor and its JointRegressor differ'
    je_dev = geval.joint_errors(Je(P), Je(T), pred_scale=1000.0).cpu().numpy().astype(np.float64)
    for k in (0, 1):
        assert (np.abs(got[:, k] - je_dev[:, k]) <= er.errors_bound(want[:, k])).all(), (COLS[k], got[:, k], je_dev[:, k])
    rp, rt = Jr(P) * 1000.0, Jr(T)
    mp = np.array([float(geval.mpvpe(P[i:i + 1] * 1000.0, T[i:i + 1], rp[i:i + 1], rt[i:i + 1])) for i in range(3)])
    print('columns 0, 1 vs joint_errors / bound: %.4f %.4f   column 3 vs eval.mpvpe / bound: %.4f'
          % tuple([(np.abs(got[:, k] - je_dev[:, k]) / er.errors_bound(want[:, k])).max() for k in (0, 1)]
                  + [(np.abs(got[:, 3] - mp) / er.errors_bound(want[:, 3])).max()]))
    assert (np.abs(got[:, 3] - mp) <= er.errors_bound(want[:, 3])).all(), (got[:, 3], mp)


# ---- input families ---------------------------------------------------------------------------------------------------------------------

def _far(rs, B, N):
    """Both meshes 100 m (1e5 mm) from the origin, 200 m apart: what a pass over raw moments would lose to cancellation."""
    a = rs.randn(B, N, 3) * 300.0
    off = np.array([1e5, -1e5, 5e4])
    return a + off, er.image_of(rs, a) - off


FAMILY_CASES = [(name, ns[-1] if ns[-1] < 14 else 65) for name, (_, _, ns) in er.FAMILIES.items()] + [('far centroid (100 m)', 65)]


@pytest.mark.parametrize('name,N', FAMILY_CASES)
def test_input_family(name, N):
    """17 samples of every family of tests/eval_edge_refs.py as (prediction, target) meshes of 65 vertices (the polyhedra at their own
    6 and 8), in mm at scale 1: generic, mirrored, coplanar, collinear, thin, repeated singular values, b == a, exact images, far
    centroids, extreme scales, a target collapsed to a point.  All five columns are distances, which are unique in every family."""
    B = 17
    if name.startswith('far'):
        rs = np.random.RandomState(100)
        a, b = _far(rs, B, N)
        a32, b32 = a.astype(np.float32), b.astype(np.float32)
    else:
        a32, b32, _, _, _ = er.make_family(name, N, B=B)
    rs = np.random.RandomState(N + len(name))
    jr, je = mr.sparse_rows(rs, 24, N), mr.sparse_rows(rs, 17, N)
    want = mr.oracle_mesh_errors(a32, b32, jr, 0, je)
    assert np.isfinite(want).all(), name
    held(run(a32, b32, jr, 0, je), want, mr.mesh_bound(want, a32, b32), 'family %s N=%d' % (name, N))


def _nonfinite_setup():
    rs = np.random.RandomState(77)
    N, B = 65, 5
    a32, b32, _, _, _ = er.make_family('generic', N, B=B, seed=3)
    jr, je = mr.sparse_rows(rs, 24, N), mr.sparse_rows(rs, 17, N)
    used = int(np.nonzero(jr[0])[0][0])                   # a vertex under the root joint ...
    je[1, used] = 0.125                                   # ... and under evaluation joint 1
    free = int(np.nonzero(~(jr.any(0) | je.any(0)))[0][0])      # a vertex under no joint of either regressor
    return a32, b32, jr, je, used, free


@pytest.mark.parametrize('value', [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize('side', ['pred', 'target'])
def test_a_non_finite_sample_is_nan_and_stays_in_its_sample(value, side):
    """One non-finite coordinate at a vertex that every column depends on: that sample's row is NaN, its neighbours keep their bits.
    At a vertex under no joint, the joint columns keep their bits too and the two mesh columns are NaN."""
    a32, b32, jr, je, used, free = _nonfinite_setup()
    clean = run(a32, b32, jr, 0, je)
    assert np.isfinite(clean).all()
    for vertex, nan_cols in ((used, [0, 1, 2, 3, 4]), (free, [3, 4])):
        a2, b2 = a32.copy(), b32.copy()
        (a2 if side == 'pred' else b2)[2, vertex, 1] = value
        dirty = run(a2, b2, jr, 0, je)
        keep = [0, 1, 3, 4]
        assert np.array_equal(bits(dirty[keep]), bits(clean[keep])), (vertex, 'another sample changed')
        assert np.isnan(dirty[2, nan_cols]).all(), (vertex, dirty[2])
        rest = [k for k in range(5) if k not in nan_cols]
        assert np.array_equal(bits(dirty[2, rest]), bits(clean[2, rest])), (vertex, dirty[2], clean[2])


def test_a_prediction_of_zero_variance_gives_what_the_oracle_gives():
    """All predicted vertices identical: the oracle's scale is 0 / 0, column 4 NaN, on both sides; columns 0, 2, 3 are ordinary numbers.
    (Column 1 fits joints that differ by the float32 rounding of the rows' sums only, so it is compared within the bound as well:
    both sides start from the same fp64 joints to ~1e-16 relative.)"""
    a32, b32, jr, je, _, _ = _nonfinite_setup()
    a2 = a32.copy()
    a2[1] = a2[1, :1]
    want = mr.oracle_mesh_errors(a2, b32, jr, 0, je)
    assert np.isnan(want[1, 4]) and np.isfinite(want[1, [0, 2, 3]]).all() and np.isfinite(np.delete(want, 1, 0)).all()
    got = run(a2, b32, jr, 0, je)
    cols = [0, 2, 3, 4]
    held(got[:, cols], want[:, cols], mr.mesh_bound(want, a2, b32)[:, cols], 'zero variance of the prediction')
    assert np.array_equal(bits(np.delete(got, 1, 0)), bits(np.delete(run(a32, b32, jr, 0, je), 1, 0)))


# ---- the regressor's edges --------------------------------------------------------------------------------------------------------------

def _edge_coo(rs, n_joint, N):
    """(row, col, val) of an n_joint-row regressor with: row 0 on vertices 0 and N-1 only; an empty row; a row with a cancelling pair;
    every value of row 2 split into two entries; and the whole list shuffled."""
    d = mr.sparse_rows(rs, n_joint, N)
    d[0] = 0
    d[0, 0], d[0, N - 1] = 0.5, 0.5
    if n_joint > 5:
        d[5] = 0
    r, c = np.nonzero(d)
    v = d[r, c]
    dup = r == min(2, n_joint - 1)
    r, c, v = np.concatenate([r, r[dup]]), np.concatenate([c, c[dup]]), np.concatenate([np.where(dup, v * 0.25, v), v[dup] * 0.75]).astype(np.float32)
    j = min(3, n_joint - 1)
    r, c, v = np.concatenate([r, [j, j]]), np.concatenate([c, [N // 2, N // 2]]), np.concatenate([v, np.float32([0.3, -0.3])])
    order = rs.permutation(r.size)
    return r[order], c[order], v[order]


@pytest.mark.parametrize('nj_root,nj_eval,n_eval', [(64, 64, 32), (1, 3, 3), (24, 17, 14), (64, 40, 3)])
def test_regressor_edges(nj_root, nj_eval, n_eval):
    """Entries at vertex 0 and N-1, an empty joint row, unsorted, duplicated and cancelling entries, root = the last row, 1 and 64
    joints, 3 and 32 evaluation joints (a list in no particular order, or all joints when the regressor has 3); and the same call
    without the evaluation regressor: columns 0-1 NaN, columns 2-4 the same bits."""
    rs = np.random.RandomState(nj_root * 100 + nj_eval)
    N, B = 65, 3
    a32, b32, _, _, _ = er.make_family('generic', N, B=B, seed=4)
    rr, rc, rv = _edge_coo(rs, nj_root, N)
    e_r, e_c, e_v = _edge_coo(rs, nj_eval, N)
    root, eroot = nj_root - 1, nj_eval - 1
    ev = None if n_eval == nj_eval else [int(i) for i in rs.permutation(nj_eval)[:n_eval]]
    want = mr.oracle_mesh_errors(a32, b32, mr.dense_of(rr, rc, rv, nj_root, N), root, mr.dense_of(e_r, e_c, e_v, nj_eval, N), ev, eroot)
    root_coo = geval._Coo(rr, rc, rv, nj_root, N, 'cuda')
    eval_coo = geval._Coo(e_r, e_c, e_v, nj_eval, N, 'cuda')
    got = run(a32, b32, root_coo, root, eval_coo, ev, eroot)
    held(got, want, mr.mesh_bound(want, a32, b32), 'regressor edges %d / %d / %d' % (nj_root, nj_eval, n_eval))
    if nj_root > 5:
        assert not mr.dense_of(rr, rc, rv, nj_root, N)[5].any()          # the empty row is what it claims
    alone = run(a32, b32, root_coo, root)
    assert np.isnan(alone[:, :2]).all() and np.array_equal(bits(alone[:, 2:]), bits(got[:, 2:]))
    empty = run(a32, b32, geval._Coo([], [], [], 2, N, 'cuda'), 1)                        # no entry at all: both roots at the origin
    want0 = mr.oracle_mesh_errors(a32, b32, np.zeros((2, N)), 1)
    held(empty, want0, mr.mesh_bound(want0, a32, b32), 'an empty root regressor')


# ---- batch invariance -------------------------------------------------------------------------------------------------------------------

def test_a_row_does_not_depend_on_its_batch():
    """Sample 0's row is the same bits at B = 1, 2, 65 and among samples that are all NaN."""
    p, t, jr, je, _ = sweep_case(257)
    kw = dict(pred_scale=1000.0, target_scale=1000.0)
    root_coo, eval_coo = geval._Coo.from_dense(jr, 'cuda'), geval._Coo.from_dense(je, 'cuda')
    first = run(p[:1], t[:1], root_coo, 0, eval_coo, **kw)
    assert np.isfinite(first).all()
    for B in (2, 65):
        assert np.array_equal(bits(run(p[:B], t[:B], root_coo, 0, eval_coo, **kw)[:1]), bits(first)), B
    p2, t2 = p.copy(), t.copy()
    p2[1:], t2[1::2] = np.nan, np.nan
    got = run(p2, t2, root_coo, 0, eval_coo, **kw)
    assert np.array_equal(bits(got[:1]), bits(first)) and np.isnan(got[1:]).all()


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------

def _raw_call(lib, p, t, B, N, root_struct, root, eval_struct, eroot, idx, ne, out, ps=1.0, ts=1.0):
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.data_ptr())
    return lib.gator_mesh_errors_f32(ptr(p), ptr(t), B, N, ps, ts, None if root_struct is None else ctypes.byref(root_struct), root,
                                     None if eval_struct is None else ctypes.byref(eval_struct), eroot, ptr(idx), ne, ptr(out), st)


def test_bad_arguments_are_refused_before_any_launch():
    """Every GATOR_EINVAL case of include/gator_hip.h leaves a poisoned output as it was."""
    lib = _lib.load()
    rs = np.random.RandomState(9)
    B, N = 4, 40
    p, t = dev(rs.randn(B, N, 3).astype(np.float32)), dev(rs.randn(B, N, 3).astype(np.float32))
    rc, ec = geval._Coo.from_dense(mr.sparse_rows(rs, 24, N), 'cuda'), geval._Coo.from_dense(mr.sparse_rows(rs, 17, N), 'cuda')
    idx = torch.as_tensor(mr.H36M_EVAL, dtype=torch.int32, device='cuda')
    out = torch.full((B, 5), 123.0, device='cuda')
    R, E = rc.struct, ec.struct

    def coo(base, **kw):
        s = base()
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    good = dict(p=p, t=t, B=B, N=N, root_struct=R(), root=0, eval_struct=E(), eroot=0, idx=idx, ne=14, out=out)
    cases = {
        'null pred': dict(p=None), 'null target': dict(t=None), 'null root regressor': dict(root_struct=None),
        'batch 0': dict(B=0), 'batch -1': dict(B=-1), 'two vertices': dict(N=2),
        'root n_joint 0': dict(root_struct=coo(R, n_joint=0)), 'root n_joint 65': dict(root_struct=coo(R, n_joint=65)),
        'eval n_joint 0': dict(eval_struct=coo(E, n_joint=0)), 'eval n_joint 65': dict(eval_struct=coo(E, n_joint=65)),
        'root = n_joint': dict(root=24), 'root -1': dict(root=-1), 'eval root = n_joint': dict(eroot=17), 'eval root -1': dict(eroot=-1),
        '2 evaluation joints': dict(ne=2), '33 evaluation joints': dict(ne=33), 'all 40 joints': dict(idx=None, ne=0, eval_struct=coo(E, n_joint=40)),
        'root nnz -1': dict(root_struct=coo(R, nnz=-1)), 'eval nnz -1': dict(eval_struct=coo(E, nnz=-1)),
        'root null row': dict(root_struct=coo(R, row=None)), 'root null col': dict(root_struct=coo(R, col=None)),
        'root null val': dict(root_struct=coo(R, val=None)), 'eval null val': dict(eval_struct=coo(E, val=None)),
    }
    for what, kw in cases.items():
        assert _raw_call(lib, **dict(good, **kw)) == EINVAL, what
    assert _raw_call(lib, **dict(good, out=None)) == EINVAL
    torch.cuda.synchronize()
    assert (out == 123.0).all()
    assert _raw_call(lib, **good) == 0
    want = geval.mesh_errors(p, t, rc, 0, ec)
    assert torch.equal(out, want)
    # "absent" in both spellings: a null struct, and nnz = 0 with three null arrays
    a, b = torch.full((B, 5), 1.0, device='cuda'), torch.full((B, 5), 2.0, device='cuda')
    assert _raw_call(lib, **dict(good, eval_struct=None, idx=None, ne=0, out=a)) == 0
    assert _raw_call(lib, **dict(good, eval_struct=_lib.GatorCoo(None, None, None, 0, 0), idx=None, ne=0, out=b)) == 0
    assert torch.isnan(a[:, :2]).all() and torch.equal(a[:, 2:], want[:, 2:]) and torch.equal(a[:, 2:], b[:, 2:]) and torch.isnan(b[:, :2]).all()


def test_capture_and_replay_give_the_eager_bits():
    p, t, jr, je, _ = sweep_case(431)
    P, T = dev(p[:7]), dev(t[:7])
    rc, ec = geval._Coo.from_dense(jr, 'cuda'), geval._Coo.from_dense(je, 'cuda')
    idx = torch.as_tensor(mr.H36M_EVAL, dtype=torch.int32, device='cuda')
    eager = geval.mesh_errors(P, T, rc, 0, ec, pred_scale=1000.0, target_scale=1000.0)
    out = torch.full((7, 5), -1.0, device='cuda')
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        geval._launch_mesh_errors(P, T, rc, 0, ec, idx, 0, 1000.0, 1000.0, out)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    P.copy_(dev(p[7:14]))                                   # new inputs in the captured buffers: the replay computes them
    T.copy_(dev(t[7:14]))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, geval.mesh_errors(P, T, rc, 0, ec, pred_scale=1000.0, target_scale=1000.0))


# ---- MeshEvaluator ----------------------------------------------------------------------------------------------------------------------

def test_mesh_evaluator_collects_rows_and_reports_both_means():
    """Updates of 5, 5 and 2 samples into a buffer that starts at 4 rows (so it grows twice) == one call on the 12 samples, row for row;
    summary() = the per-sample means and the mean of the three batch means, which differ because the last batch is short."""
    p, t, jr, je, _ = sweep_case(431)
    P, T = dev(p[:12]), dev(t[:12])
    ev = geval.MeshEvaluator(jr, je, n_verts=431, pred_scale=1000.0, target_scale=1000.0, capacity=4)
    whole = geval.mesh_errors(P, T, jr, 0, je, pred_scale=1000.0, target_scale=1000.0).cpu().numpy()
    for s, n in ((0, 5), (5, 5), (10, 2)):
        rows = ev.update(P[s:s + n], T[s:s + n])
        assert rows.shape == (n, 5)
    assert len(ev) == 12 and np.array_equal(bits(ev.rows()), bits(whole))
    s = ev.summary()
    r = whole.astype(np.float64)
    assert set(s) == set(COLS) | {'MPVPE_batch_mean', 'MPJPE_batch_mean'}
    for k, name in enumerate(COLS):
        assert s[name] == pytest.approx(r[:, k].mean(), rel=1e-12)
    for name, k in (('MPVPE_batch_mean', 3), ('MPJPE_batch_mean', 0)):
        want = np.mean([r[0:5, k].mean(), r[5:10, k].mean(), r[10:12, k].mean()])
        assert s[name] == pytest.approx(want, rel=1e-12) and s[name] != s[COLS[k]]
    ev.reset()
    assert len(ev) == 0 and ev.rows().shape == (0, 5)
    with pytest.raises(RuntimeError):
        ev.summary()
    ev.update(P[:3], T[:3])
    assert np.array_equal(bits(ev.rows()), bits(whole[:3]))
    with pytest.raises(ValueError):
        ev.update(P[:3, :100], T[:3, :100])
    with pytest.raises(RuntimeError):
        ev.update(P[:3].cpu(), T[:3].cpu())
