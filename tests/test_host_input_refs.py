"""CPU-only: the input batches of tests/input_refs.py are what they claim, and the bar tests/test_gpu_input_families.py holds the
device to is not vacuous on them.  Conditions on the inputs, not measurements: a draw that misses one is replaced, not excused.
Both golden variants, the 16 rows the GPU tests use."""
import numpy as np
import pytest
import torch

from tests import input_refs as ir
from tests.helpers import VARIANTS

REF_V_MAX, REF_P_MAX = 1.5e-3, 1e-3         # mm: the floors of the suite's bars (tests/test_gpu_softmax_edges.py); every row's reference error stays below them


def _show(name, batch, r):
    print('\n[%s %s]' % (name, batch))
    for i in range(ir.B):
        print(ir.fmt_row(r, i))


@pytest.mark.parametrize('name', VARIANTS)
def test_contract_rows_are_standardised(name):
    x = ir.run(name, 'contract').x.numpy().astype(np.float64)
    assert np.abs(x.mean(1)).max() <= 1e-6 and np.abs(x.std(1) - 1.0).max() <= 1e-6
    x = ir.run(name, 'ordinary').x.numpy().astype(np.float64)
    assert np.abs(x.mean(1)).max() <= 1e-6 and np.abs(x.std(1) - 1.0).max() <= 1e-6


@pytest.mark.parametrize('name', VARIANTS)
def test_contract_rows_are_the_shapes_they_claim(name):
    r = ir.run(name, 'contract')
    x, J = r.x.numpy().astype(np.float64), r.c.J
    top = np.sqrt(J - 1.0)
    for row, k in ((3, 0), (4, J - 1)):
        assert abs(abs(x[row, k, 0]) - top) <= 1e-6 * top and abs(abs(x[row, k, 1]) - top) <= 1e-6 * top
        rest = np.delete(x[row], k, 0)
        assert np.ptp(rest, 0).max() == 0.0                                    # the other joints coincide exactly
    assert abs(x[5, J // 2, 0] - top) <= 1e-2 and 0.0 < np.ptp(np.delete(x[5], J // 2, 0), 0).max() <= 1e-2
    assert len(np.unique(x[6], axis=0)) == 2
    assert np.array_equal(x[7, :, 0], x[7, :, 1]) and np.array_equal(x[8, :, 0], -x[8, :, 1])
    assert np.ptp(x[9, 0:6], 0).max() == 0.0
    assert np.abs(x[10]).max() > np.abs(x[0:3]).max()                          # the heavy tail reaches past the Gaussian rows
    assert all(len(np.unique(x[11, :, a])) == 2 for a in (0, 1))
    assert np.abs(x[3:12]).max() >= 4.0 > np.abs(x[[0, 1, 2, 12, 13, 14, 15]]).max()


@pytest.mark.parametrize('name', VARIANTS)
def test_units_rows_are_the_inputs_they_claim(name):
    r = ir.run(name, 'units')
    x = r.x.numpy()
    assert not x[3].any() and not np.signbit(x[3]).any()
    assert not x[4].any() and np.signbit(x[4]).all()
    assert x[5].all() and np.abs(x[5]).max() < np.finfo(np.float32).tiny       # every coordinate a non-zero denormal
    assert not x[6, :, 1].any() and abs(x[6, :, 0].astype(np.float64).std() - 1.0) <= 1e-6
    base = np.ldexp(x[ir.GAIN_ROWS[0]].astype(np.float64), -ir.GAINS[0])
    assert np.abs(base.mean(0)).max() <= 1e-6 and np.abs(base.std(0) - 1.0).max() <= 1e-6
    for row, k in zip(ir.GAIN_ROWS, ir.GAINS):
        assert np.array_equal(x[row].astype(np.float64), np.ldexp(base, k))     # the same pose, the gain exact
    px = x[ir.PIXEL_ROW]
    assert 0.0 < px[:, 0].min() and px[:, 0].max() < 1920.0 and 0.0 < px[:, 1].min() and px[:, 1].max() < 1080.0
    assert np.abs(x[ir.OFFSET_ROW] - 1e6).max() <= 0.1
    assert np.isfinite(x).all()


@pytest.mark.parametrize('batch', ir.BATCHES)
@pytest.mark.parametrize('name', VARIANTS)
def test_the_reference_maps_every_row_to_a_mesh_within_the_floors(name, batch):
    """Every row finite in the fp32 oracle and within the floors of the bars: on these inputs the bars of the GPU tests ARE their floors
    (or 2 x ref just above), so a device row outside them is the device's doing."""
    r = ir.run(name, batch)
    _show(name, batch, r)
    assert r.finite32.all() and np.isfinite(r.v64).all() and np.isfinite(r.p64).all()
    assert r.ref_v.max() <= REF_V_MAX, r.ref_v
    assert r.ref_p.max() <= REF_P_MAX, r.ref_p


@pytest.mark.parametrize('name', VARIANTS)
def test_rows_0_to_2_are_shared_and_the_oracle_is_row_independent(name):
    o = ir.run(name, 'ordinary')
    for batch in ('contract', 'units'):
        r = ir.run(name, batch)
        assert torch.equal(r.x[0:3], o.x[0:3])
        assert np.abs(r.v64[0:3] - o.v64[0:3]).max() * 1e3 <= 1e-9 and np.abs(r.p64[0:3] - o.p64[0:3]).max() <= 1e-9


@pytest.mark.parametrize('name', VARIANTS)
def test_the_joint_tokens_grow_as_the_gain_and_the_outputs_do_not(name):
    """max|mdr_jf| of the gain rows: flat below gain 1 (bias, position and feature terms), linear in the gain above 2^10; the offset
    and pixel rows carry their magnitude into it too.  The embedding's GroupNorm takes the gain out: max|gat_embed| stays where the
    Gaussian rows have it."""
    r = ir.run(name, 'units')
    jf = dict(zip(ir.GAINS, r.jf[list(ir.GAIN_ROWS)]))
    print('\n[%s] max|mdr_jf| per gain: %s | pixels %.3g | offset %.3g | Gaussian rows %.3g' % (
        name, '  '.join('2^%d: %.3g' % kv for kv in jf.items()), r.jf[ir.PIXEL_ROW], r.jf[ir.OFFSET_ROW], r.jf[0:3].max()))
    assert abs(jf[-100] / jf[-20] - 1.0) <= 1e-3
    for lo, hi in ((10, 15), (15, 40)):
        assert abs(jf[hi] / jf[lo] / 2.0 ** (hi - lo) - 1.0) <= 2e-2
    # 4 094: the documented operand range of the default arithmetic (include/gator_hip.h, "Operand range of that default"; 16 x value must
    # fit an fp16 plane, largest finite fp16 65 504).  A condition on the input: the 2^15 row would leave that range were jf carried on planes
    assert jf[15] >= 4094.0
    assert jf[40] >= 1e11 and r.jf[ir.OFFSET_ROW] >= 1e5 and r.jf[ir.PIXEL_ROW] >= 100.0
    assert r.embed.max() <= 4.0 * r.embed[0:3].max()


@pytest.mark.parametrize('name', VARIANTS)
def test_outlier_rows_reach_an_embedding_no_gaussian_row_does(name):
    r, o = ir.run(name, 'contract'), ir.run(name, 'ordinary')
    print('\n[%s] max|gat_embed|: outlier rows %s, sixteen Gaussian rows <= %.2f' % (name, np.round(r.embed[3:6], 2).tolist(), o.embed.max()))
    assert r.embed[3:6].min() > o.embed.max() and r.embed[3:6].max() >= 1.5 * o.embed.max()


@pytest.mark.parametrize('name', VARIANTS)
def test_the_mdr_stage_reference_is_within_the_floor(name):
    r = ir.run(name, 'units')
    v, ref = ir.mdr_run(name)
    print('\n[%s] mdr_forward on the rounded pose_combine: fp32 vs fp64 per row (mm) %s' % (name, ' '.join('%.1e' % e for e in ref)))
    assert np.isfinite(v).all() and ref.max() <= REF_V_MAX
    assert np.abs(v - r.v64).max() * 1e3 <= 1e-3             # rounding pose_combine to fp32 moves the mesh by less than the bar's floor


def test_runs_are_cached_and_builders_deterministic():
    assert ir.run('h36m17_bn', 'units') is ir.run('h36m17_bn', 'units')
    for J in (17, 19):
        for b in ir.BATCHES:
            a, c = ir.BUILDERS[b](J), ir.BUILDERS[b](J)
            assert a.dtype == np.float32 and a.shape == (ir.B, J, 2) and np.array_equal(a, c, equal_nan=False)
            assert len(ir.ROW_NAMES[b]) == ir.B
