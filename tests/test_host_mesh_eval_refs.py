"""The fp64 reference of the mesh-evaluation kernel (tests/mesh_eval_refs.py) on closed forms and against the reference's own
lib/coord_utils.rigid_align on 431-point sets (tests/golden/mesh_eval.npz, tools/gen_golden_mesh_eval.py), on the CPU; and the argument
checks of gator_amd.eval.mesh_errors that are decided on the host before any device is needed."""
import numpy as np
import pytest
import torch

from gator_amd import eval as geval
from oracle import gator_oracle as go
from tests import eval_edge_refs as er
from tests import mesh_eval_refs as mr
from tests.helpers import load_golden


def _setup(seed, B=4, N=40, nj=17):
    rs = np.random.RandomState(seed)
    t = (rs.randn(B, N, 3) * 300.0 + rs.randn(B, 1, 3) * 500.0).astype(np.float32)
    return rs, t, mr.sparse_rows(rs, 24, N), mr.sparse_rows(rs, nj, N)


def test_identical_meshes_give_zero():
    rs, t, jr, je = _setup(0)
    e = mr.oracle_mesh_errors(t, t.copy(), jr, 0, je)
    assert np.array_equal(e[:, [0, 2, 3]], np.zeros((4, 3)))
    assert np.abs(e[:, [1, 4]]).max() <= 1e-9                    # the fit of a set onto itself is the identity to rounding


def test_similarity_image_has_no_pa_error_and_a_pure_offset_has_a_known_mpvpe():
    """target = s R pred + shift: column 4 is 0 (and column 1: the joints of an affine image are the image of the joints when the rows
    sum to 1).  target = pred + shift: the roots move with the meshes, so column 3 is 0; when the root regressor's rows are empty the
    roots stay at the origin and column 3 is |shift| exactly."""
    rs, p, jr, je = _setup(1)
    R = er.rotations(rs, len(p))
    shift = rs.randn(len(p), 1, 3) * 80.0
    t = (0.8 * np.einsum('bnk,brk->bnr', p.astype(np.float64), R) + shift)
    e = mr.oracle_mesh_errors(p, t.astype(np.float32), jr, 0, je)
    scale = np.abs(t).max()
    assert e[:, 4].max() <= 3 * er.F32_EPS * scale               # the float32 rounding of the target is all that is left
    assert e[:, 1].max() <= 3 * er.F32_EPS * scale + 1e-6 * scale       # + the regressor rows' float32 sums (1 +- 1e-7)
    assert e[:, 3].min() > 10.0                                  # not aligned by the root alone: it is turned and scaled
    t2 = (p.astype(np.float64) + shift).astype(np.float32)
    e2 = mr.oracle_mesh_errors(p, t2, jr, 0, je)
    assert e2[:, 3].max() <= 3 * er.F32_EPS * scale + 1e-6 * scale
    e3 = mr.oracle_mesh_errors(p, t2, np.zeros_like(jr), 0, None)
    want = np.linalg.norm((t2.astype(np.float64) - p).reshape(len(p), -1, 3), axis=2).mean(1)
    assert np.abs(e3[:, 3] - want).max() <= 1e-9 and np.abs(want - np.linalg.norm(shift[:, 0], axis=1)).max() <= 3 * er.F32_EPS * scale
    assert np.isnan(e3[:, :2]).all() and np.array_equal(e3[:, 2], np.zeros(len(p)))


def test_mirrored_target_takes_the_reflection_branch():
    """A mirror image cannot be reached by a rotation: the fit's R has det +1 (go.rigid_transform_3d flips the last singular vector) and
    the PA error stays large, while the unmirrored image of the same points fits to rounding."""
    rs, p, jr, je = _setup(2)
    p64 = p.astype(np.float64)
    m = p64 * np.array([1.0, 1.0, -1.0])
    for b in range(len(p)):
        c, R, _ = go.rigid_transform_3d(p64[b], m[b])
        U, s, Vt = np.linalg.svd((p64[b] - p64[b].mean(0)).T @ (m[b] - m[b].mean(0)))
        assert np.linalg.det(Vt.T @ U.T) < 0 and abs(np.linalg.det(R) - 1.0) < 1e-9
    e = mr.oracle_mesh_errors(p, m.astype(np.float32), jr, 0, je)
    assert e[:, 4].min() > 50.0 and e[:, 1].min() > 1.0


def test_one_hot_regressor_row_is_that_vertex():
    rs, t, _, _ = _setup(3, N=9)
    p = (t + rs.randn(*t.shape).astype(np.float32) * 30.0).astype(np.float32)
    N = 9
    onehot = np.zeros((3, N), np.float32)
    onehot[0, 0], onehot[1, N - 1], onehot[2, 4] = 1.0, 1.0, 1.0
    for root in range(3):
        e = mr.oracle_mesh_errors(p, t, onehot, root, onehot, None, root)
        v = (0, N - 1, 4)[root]
        d = (p.astype(np.float64) - p[:, v:v + 1]) - (t.astype(np.float64) - t[:, v:v + 1])
        want3 = np.linalg.norm(d, axis=2).mean(1)
        want2 = np.linalg.norm(d[:, [0, N - 1, 4]], axis=2).mean(1)
        assert np.abs(e[:, 3] - want3).max() <= 1e-9 and np.abs(e[:, 2] - want2).max() <= 1e-9
        assert np.abs(e[:, 0] - want2).max() <= 1e-9             # the same three joints as the evaluation set


def test_duplicate_entries_add_and_cancelling_entries_vanish():
    d = mr.dense_of([1, 0, 1, 1], [2, 0, 2, 3], [0.25, 1.0, 0.5, -0.5], 3, 5)
    assert d[1, 2] == 0.75 and d[1, 3] == -0.5 and d[0, 0] == 1.0 and not d[2].any()
    d = mr.dense_of([0, 0], [1, 1], [0.3, -0.3], 1, 4)
    assert not d.any()


def test_column_4_is_the_references_rigid_align_on_a_431_point_mesh():
    """lib/coord_utils.py:127-149 itself on three 431-point float32 sets (generic, mirrored, 100 m from the origin): the per-vertex
    distances of the oracle's alignment and column 4 of the reference are the reference's fp64 run to rounding; its own float32 run is
    farther away than that, which is the error this project does not copy."""
    z = load_golden('mesh_eval')
    A, B = z['A'], z['B']
    assert A.dtype == np.float32 and A.shape == (3, 431, 3)
    for a, b, want in zip(A, B, z['pa_dist64']):
        got = np.linalg.norm(go.rigid_align(a.astype(np.float64), b.astype(np.float64)) - b, axis=1)
        assert np.abs(got - want).max() <= 1e-9 * np.abs(a).max()
    rs = np.random.RandomState(5)
    jr = mr.sparse_rows(rs, 24, 431)
    e = mr.oracle_mesh_errors(A, B, jr, 0, None)
    assert np.abs(e[:, 4] - z['pa_mpvpe64']).max() <= 1e-9 * np.abs(A).max()
    assert np.isnan(e[:, :2]).all()
    assert (np.abs(z['pa_mpvpe32'] - z['pa_mpvpe64']) <= 1e-6 * np.abs(A).max((1, 2))).all()       # the reference's float32 run, for scale


# ---- gator_amd.eval.mesh_errors: what is refused on the host ----------------------------------------------------------------------------

def _args(N=12, nj=17):
    rs = np.random.RandomState(7)
    p = torch.from_numpy(rs.randn(2, N, 3).astype(np.float32))
    return p, p.clone(), mr.sparse_rows(rs, 24, N), mr.sparse_rows(rs, nj, N)


@pytest.mark.parametrize('case', ['2-d mesh', 'xy mesh', 'shape mismatch', 'two vertices', 'empty batch', 'regressor width', '1-d regressor',
                                  '65 joints', 'root', 'negative root', 'eval root', 'eval index', 'negative eval index', '2 eval joints',
                                  '33 eval joints', 'all of 40 joints', 'eval regressor width', 'JointRegressor-sized'])
def test_mesh_errors_refuses_on_the_host(case):
    p, t, jr, je = _args()
    kw = dict(root_regressor=jr, eval_regressor=je)
    if case == '2-d mesh':
        p, t = p[0], t[0]
    elif case == 'xy mesh':
        p, t = p[:, :, :2], t[:, :, :2]
    elif case == 'shape mismatch':
        t = t[:, :11]
    elif case == 'two vertices':
        p, t, kw = p[:, :2], t[:, :2], dict(root_regressor=jr[:, :2], eval_regressor=je[:, :2])
    elif case == 'empty batch':
        p, t = p[:0], t[:0]
    elif case == 'regressor width':
        kw['root_regressor'] = jr[:, :11]
    elif case == '1-d regressor':
        kw['root_regressor'] = jr[0]
    elif case == '65 joints':
        kw['root_regressor'] = np.tile(jr, (3, 1))[:65]
    elif case == 'root':
        kw['root'] = 24
    elif case == 'negative root':
        kw['root'] = -1
    elif case == 'eval root':
        kw['eval_root'] = 17
    elif case == 'eval index':
        kw['eval_joints'] = (0, 1, 17)
    elif case == 'negative eval index':
        kw['eval_joints'] = (0, 1, -1)
    elif case == '2 eval joints':
        kw['eval_joints'] = (0, 1)
    elif case == '33 eval joints':
        kw['eval_joints'] = tuple(range(17)) + tuple(range(16))
    elif case == 'all of 40 joints':
        kw.update(eval_regressor=np.tile(je, (3, 1))[:40], eval_joints=None)
    elif case == 'eval regressor width':
        kw['eval_regressor'] = je[:, :5]
    elif case == 'JointRegressor-sized':
        kw['root_regressor'] = geval.JointRegressor(np.eye(3, geval.N_VERTS, dtype=np.float32), 'cpu')      # 6890 columns, 12 vertices
    with pytest.raises(ValueError):
        geval.mesh_errors(p, t, **kw)


def test_mesh_errors_needs_device_tensors_and_checks_before_it_says_so():
    p, t, jr, je = _args()
    with pytest.raises(RuntimeError, match='HIP device'):
        geval.mesh_errors(p, t, jr, eval_regressor=je, pred_scale=1000.0, target_scale=1000.0)
    with pytest.raises(RuntimeError, match='HIP device'):
        geval.mesh_errors(p, t, jr)
    with pytest.raises(ValueError):                      # JointRegressor keeps refusing anything but 6890 columns
        geval.JointRegressor(jr, 'cpu')
    assert geval.MESH_ERROR_COLUMNS == ('MPJPE', 'PA-MPJPE', 'MPJPE_SMPL', 'MPVPE', 'PA-MPVPE')


def test_private_coo_checks_rows_and_columns():
    with pytest.raises(ValueError):
        geval._Coo([0], [12], [1.0], 3, 12, 'cpu')
    with pytest.raises(ValueError):
        geval._Coo([0], [-1], [1.0], 3, 12, 'cpu')
    with pytest.raises(ValueError):
        geval._Coo([3], [0], [1.0], 3, 12, 'cpu')
    with pytest.raises(ValueError):
        geval._Coo([0, 1], [0], [1.0], 3, 12, 'cpu')
    c = geval._Coo([2, 0, 2], [11, 0, 11], [0.5, 1.0, 0.25], 3, 12, 'cpu')          # unsorted, duplicated: kept as given
    assert c.nnz == 3 and c.row[:3].tolist() == [2, 0, 2] and c.col[:3].tolist() == [11, 0, 11]
    assert geval._Coo([], [], [], 1, 12, 'cpu').nnz == 0
