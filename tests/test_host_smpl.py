"""The SMPL layer without a GPU: the float64 restatement (tests/smpl_refs.py) against the reference layer's golden run
(tests/golden/smpl_layer.npz, written by tools/gen_golden_smpl.py), the synthetic models' checksums, the model-file readers of
gator_amd.smpl, the models.smpl mirror's tables and the host-side argument checks of the C ABI."""
import ctypes
import json
import pickle

import numpy as np
import pytest
import torch

from gator_amd import _lib, smpl
from tests import smpl_refs as sr
from tests.helpers import load_golden


def golden_meta(z):
    return json.loads(str(z['meta']))


def case_options(name):
    (nv, nj, nb, seed, dense), opt, keep = sr.CASES[name]
    return {'betas': opt.get('betas', True) and nb > 0, 'trans': opt.get('trans', True), 'center_idx': opt.get('center_idx'),
            'out_scale': opt.get('out_scale', 1.0), 'keep': keep}


@pytest.mark.parametrize('name', sorted(sr.CASES))
def test_restatement_matches_the_reference_layer(name):
    """fp64 restatement vs the real layer's fp32 outputs, on the stored samples, within the spread recorded over all samples."""
    z = load_golden('smpl_layer')
    o = case_options(name)
    m = sr.synthetic_model(*sr.CASES[name][0])
    k = o['keep']
    pose, betas, trans = z[name + '.pose'][:k], z[name + '.betas'][:k], z[name + '.trans'][:k]
    v, j = sr.lbs_forward(m, pose, betas if o['betas'] else None, trans if o['trans'] else None, o['center_idx'], o['out_scale'])
    sv, sj = z[name + '.spread']
    assert z[name + '.verts32'].shape == v.shape and z[name + '.joints32'].shape == j.shape
    assert np.abs(z[name + '.verts32'] - v).max() <= sv * (1 + 1e-6)
    assert np.abs(z[name + '.joints32'] - j).max() <= sj * (1 + 1e-6)
    # the reference's own fp32 error is a few ulp of the output: metres at ~2 m (ulp 2.4e-7), millimetres at out_scale 1000
    assert 1e-8 * o['out_scale'] < sv < 2e-6 * o['out_scale'] and 1e-8 * o['out_scale'] < sj < 2e-6 * o['out_scale']


def test_generator_checksums_and_inputs():
    z = load_golden('smpl_layer')
    meta = golden_meta(z)
    assert sorted(meta) == sorted(sr.CASES)
    for name, (margs, opt, keep) in sr.CASES.items():
        assert meta[name]['model'] == list(margs) and meta[name]['stored'] == keep
        assert sr.model_sha256(sr.synthetic_model(*margs)) == meta[name]['sha256'], name
        for got, want in zip(sr.case_inputs(name), (z[name + '.pose'], z[name + '.betas'], z[name + '.trans'])):
            np.testing.assert_array_equal(got, want)


def test_synthetic_model_is_a_body_model():
    m = sr.synthetic_model(257, 24, 10, 3)
    assert m['v_template'].shape == (257, 3) and m['shapedirs'].shape == (257, 3, 10) and m['posedirs'].shape == (257, 3, 207)
    assert ((m['weights'] != 0).sum(1) == 4).all() and np.allclose(m['weights'].sum(1), 1, atol=1e-6)
    assert np.allclose(m['J_regressor'].sum(1), 1, atol=1e-6) and ((m['J_regressor'] != 0).sum(1) <= 8).all()
    assert tuple(m['parents']) == sr.SMPL_PARENTS
    assert ((sr.synthetic_model(65, 24, 10, 3, True)['weights'] != 0).sum(1) == 24).all()


def test_zero_pose_is_the_rest_pose_only_with_the_epsilon():
    m = sr.synthetic_model(65, 24, 10, 5)
    R = sr.rodrigues(np.zeros((24, 3)))
    np.testing.assert_array_equal(R, np.broadcast_to(np.eye(3), (24, 3, 3)))
    v, j = sr.lbs_forward(m, np.zeros((1, 72)))
    wsum = m['weights'].astype(np.float64).sum(1, keepdims=True)        # float32 weights sum to 1 within 1e-7, and the layer does not normalise
    assert np.abs(v[0] - wsum * m['v_template']).max() <= 1e-14          # posedirs x 0, identity transforms
    assert np.abs(j[0] - m['J_regressor'].astype(np.float64) @ m['v_template']).max() <= 1e-12


class _Ch:
    """Stands in for a chumpy array in a pickle: the value sits in .r"""

    def __init__(self, a):
        self.r = a


def _model_dict(m, sparse, wrapped):
    import scipy.sparse as sps
    wrap = _Ch if wrapped else (lambda a: a)
    kt = np.stack([np.where(m['parents'] < 0, 2 ** 32 - 1, m['parents']), np.arange(len(m['parents']))]).astype(np.uint32)
    return {'v_template': wrap(m['v_template'].astype(np.float64)), 'shapedirs': wrap(m['shapedirs'].astype(np.float64)),
            'posedirs': wrap(m['posedirs'].astype(np.float64)), 'weights': wrap(m['weights'].astype(np.float64)),
            'J_regressor': sps.csc_matrix(m['J_regressor'].astype(np.float64)) if sparse else m['J_regressor'],
            'kintree_table': kt, 'f': m['faces'].astype(np.uint32), 'bs_style': 'lbs', 'bs_type': 'lrotmin'}


@pytest.mark.parametrize('sparse,wrapped', [(True, False), (False, False), (True, True)])
def test_read_pkl_round_trip(tmp_path, sparse, wrapped):
    m = sr.synthetic_model(65, 24, 10, 6)
    path = tmp_path / 'model.pkl'
    with open(path, 'wb') as fh:
        pickle.dump(_model_dict(m, sparse, wrapped), fh, protocol=2)
    a = smpl.read_pkl(str(path))
    for k in ('v_template', 'shapedirs', 'posedirs', 'weights', 'J_regressor'):
        assert a[k].dtype == np.float32 and a[k].flags['C_CONTIGUOUS']
        np.testing.assert_array_equal(a[k], m[k])
    assert a['parents'][0] == 2 ** 32 - 1 and tuple(a['parents'][1:]) == sr.SMPL_PARENTS[1:]
    np.testing.assert_array_equal(a['faces'], m['faces'])


def test_read_npz_round_trip(tmp_path):
    m = sr.synthetic_model(63, 24, 10, 7)
    path = tmp_path / 'model.npz'
    np.savez(path, **{k: v for k, v in _model_dict(m, False, False).items() if not isinstance(v, str)})
    a = smpl.read_npz(str(path))
    for k in ('v_template', 'shapedirs', 'posedirs', 'weights', 'J_regressor', 'faces'):
        np.testing.assert_array_equal(a[k], m[k])
    np.savez(path, **m)                                     # the layer's own argument names are read as well
    b = smpl.read_npz(str(path))
    np.testing.assert_array_equal(b['parents'], m['parents'])
    np.testing.assert_array_equal(b['posedirs'], m['posedirs'])


def test_layer_has_no_cpu_path():
    m = sr.synthetic_model(8, 24, 10, 1)
    with pytest.raises(RuntimeError, match='HIP device'):
        smpl.SMPLLayer(m['v_template'], m['shapedirs'], m['posedirs'], m['weights'], m['J_regressor'], m['parents'], device='cpu')
    with pytest.raises(ValueError, match='inconsistent'):
        smpl.SMPLLayer(m['v_template'], m['shapedirs'], m['posedirs'][:, :, :9], m['weights'], m['J_regressor'], m['parents'], device='cpu')


def test_models_smpl_mirror_tables():
    from gator_amd import models

    class Layer:
        num_verts = 6890
        th_faces = None
        th_J_regressor = torch.zeros(24, 6890)
    s = models.smpl.SMPL(Layer())
    assert s.layer['male'] is s.layer['female'] is s.layer['neutral'] and s.get_layer('neutral') is s.layer['neutral']
    assert s.vertex_num == 6890 and s.joint_num == 29 == len(s.joints_name) and s.root_joint_idx == 0
    assert s.joint_regressor.shape == (29, 6890) and s.joint_regressor.dtype == np.float32
    assert [int(np.argmax(r)) for r in s.joint_regressor[24:]] == list(s.face_kps_vertex) == [331, 2802, 6262, 3489, 3990]
    assert s.joint_regressor[24:].sum() == 5
    assert s.joints_name[12] == 'Neck' and s.joints_name[24:] == ('Nose', 'L_Eye', 'R_Eye', 'L_Ear', 'R_Ear')
    assert all(s.joints_name[a][2:] == s.joints_name[b][2:] and s.joints_name[a][0] == 'L' for a, b in s.flip_pairs)
    assert len(s.skeleton) == 27 and max(max(e) for e in s.skeleton) == 28
    with pytest.raises(ValueError):
        models.smpl.SMPL({'male': Layer()})


def _create(m, nv=None, nj=None, nb=None, struct_size=None, parents=None, null=None):
    lib = _lib.load()
    par = np.ascontiguousarray(np.where(m['parents'] < 0, -1, m['parents']) if parents is None else parents, dtype=np.int32)
    arrs = {k: np.ascontiguousarray(m[k], dtype=np.float32) for k in ('v_template', 'shapedirs', 'posedirs', 'weights', 'J_regressor')}
    ptr = {k: (None if k == null else v.ctypes.data) for k, v in arrs.items()}
    mod = _lib.SmplModel(ctypes.sizeof(_lib.SmplModel) if struct_size is None else struct_size,
                         m['v_template'].shape[0] if nv is None else nv, m['weights'].shape[1] if nj is None else nj,
                         m['shapedirs'].shape[2] if nb is None else nb, ptr['v_template'], ptr['shapedirs'], ptr['posedirs'], ptr['weights'],
                         ptr['J_regressor'], par.ctypes.data)
    ctx = ctypes.c_void_p()
    rc = lib.gator_smpl_create(ctypes.byref(mod), ctypes.byref(ctx))
    return rc, ctx, lib.gator_last_error()


def test_create_refuses_bad_models_on_the_host():
    """Every refusal is decided before any device work: these pass on a machine without a GPU."""
    m = sr.synthetic_model(8, 24, 10, 2)
    bad_order = np.array(sr.SMPL_PARENTS, np.int32)
    bad_order[5] = 7                                                          # a parent after its joint
    self_parent = np.array(sr.SMPL_PARENTS, np.int32)
    self_parent[9] = 9
    negative = np.array(sr.SMPL_PARENTS, np.int32)
    negative[3] = -1                                                          # only parents[0] may be anything
    for kw, word in ((dict(parents=bad_order), b'parents[5]'), (dict(parents=self_parent), b'parents[9]'), (dict(parents=negative), b'parents[3]'),
                     (dict(nj=33), b'n_joints'), (dict(nj=1), b'n_joints'), (dict(nb=17), b'n_betas'), (dict(nb=-1), b'n_betas'),
                     (dict(nv=0), b'n_verts'), (dict(struct_size=ctypes.sizeof(_lib.SmplModel) - 8), b'struct_size'),
                     (dict(struct_size=0), b'struct_size'), (dict(null='posedirs'), b'NULL'), (dict(null='shapedirs'), b'NULL')):
        rc, ctx, msg = _create(m, **kw)
        assert rc == -1 and not ctx.value, kw
        assert b'gator_smpl_create' in msg and word in msg, (kw, msg)
    lib = _lib.load()
    assert lib.gator_smpl_create(None, None) == -1
    assert lib.gator_smpl_destroy(None) == 0


def test_forward_refuses_centre_with_translation_and_null_ctx():
    lib = _lib.load()
    one = ctypes.c_float(1.0)
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.gator_smpl_forward_f32(None, p, None, p, 1, 0, one, None, None, None) == -1
    assert b'center_idx goes with trans = NULL' in lib.gator_last_error()
    assert lib.gator_smpl_forward_f32(None, p, None, None, 1, 0, one, None, None, None) == -1
    assert b'null ctx' in lib.gator_last_error()
    assert lib.gator_smpl_workspace(None, None, None) == -1
