"""The fp64 restatements of tests/temporal_refs.py against the reference's own lib/smooth_utils and lib/coord_utils.compute_error_accel
(tests/golden/temporal.npz, tools/gen_golden_temporal.py), on the CPU; the argument checks of gator_amd.temporal that are decided on the
host before any device is needed; and the build's and the binding's entries for csrc/temporal.hip."""
import numpy as np
import pytest
import torch

from gator_amd import _lib, build, temporal
from tests import temporal_refs as tr
from tests.helpers import load_golden


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def test_golden_is_what_the_generator_describes():
    z = load_golden('temporal')
    assert tuple(z['lengths']) == tr.LENGTHS and [tuple(p) for p in z['params']] == list(tr.PARAMS)
    F = sum(tr.LENGTHS)
    assert z['pred'].dtype == np.float32 and z['pred'].shape == (F, 14, 3) and z['gt'].dtype == np.float32 and z['gt'].shape == (F, 14, 3)
    assert all(z['smooth_%d' % k].dtype == np.float64 and z['smooth_%d' % k].shape == (F, 14, 3) for k in range(3))
    s, v = tr.seg_starts(tr.LENGTHS), z['valid']
    assert not v[s[4]] and not v[s[6] - 1] and not v[s[6] + 40] and v.dtype == np.uint8       # a first, a last and an interior frame
    assert len(z['accel']) == sum(max(0, T - 2) for T in tr.LENGTHS)


@pytest.mark.parametrize('k', [0, 1, 2])
def test_restated_filter_is_the_references_bit_for_bit(k):
    z = load_golden('temporal')
    mc, beta = z['params'][k]
    got = tr.one_euro_videos(z['pred'], z['lengths'], min_cutoff=mc, beta=beta)
    assert np.array_equal(bits(got), bits(z['smooth_%d' % k]))
    s = tr.seg_starts(z['lengths'])
    assert np.array_equal(got[s[:-1]], z['pred'][s[:-1]].astype(np.float64))       # a video's first frame is copied
    assert np.abs(got - z['pred']).max() > 1.0                                       # and the rest is filtered, by millimetres


def test_restated_filter_with_timestamps_is_the_references_dt_run():
    """OneEuroFilter called with t = idx * dt sees t_e = fl(idx dt) - fl((idx - 1) dt), which is dt only to rounding: the restatement
    given the same timestamps is the reference bit for bit.  With t_e = dt at every step (what the kernel computes) the result moves by
    rounding only.  Bound: |t_e - dt| <= 2 * half an ulp of T dt < 8, i.e. 2^-50, a relative 30 * 2^-50 = 2.7e-14 of dt; it enters r
    (twice), dx and through them a, each with a relative sensitivity <= 1, and x_hat = x_prev + a (x - x_prev) with 0 < a < 1 is a
    convex combination that does not amplify an earlier step's error: over T = 65 steps at most 65 * 4 * 2.7e-14 < 1e-11 of max|x|."""
    z = load_golden('temporal')
    s, v, dt = tr.seg_starts(z['lengths']), int(z['dt_video']), float(z['dt'])
    x = z['pred'][s[v]:s[v + 1]]
    mc, beta = z['dt_params']
    assert dt == 1.0 / 30.0 and len(x) == 65
    got = tr.one_euro(x, mc, beta, 1.0, dt, t=np.arange(len(x)) * dt)
    assert np.array_equal(bits(got), bits(z['smooth_dt']))
    const = tr.one_euro(x, mc, beta, 1.0, dt)
    assert np.abs(const - z['smooth_dt']).max() <= 1e-11 * np.abs(x).max()
    assert np.abs(const - tr.one_euro(x, mc, beta, 1.0, 1.0)).max() > 1.0            # dt matters: not the dt = 1 result


def test_restated_acceleration_error_is_the_references():
    z = load_golden('temporal')
    for valid, key in ((None, 'accel'), (z['valid'], 'accel_valid')):
        rows = tr.accel_rows(z['smooth_0'], z['gt'], z['lengths'], valid)
        got, want = rows[~np.isnan(rows)], z[key]
        assert got.shape == want.shape
        assert (np.abs(got - want) <= 1e-13 * np.abs(want)).all()
    # the mask removes every triple that holds an invalid frame, and nothing else
    rows, masked = tr.accel_rows(z['smooth_0'], z['gt'], z['lengths']), tr.accel_rows(z['smooth_0'], z['gt'], z['lengths'], z['valid'])
    gone = np.isnan(masked) & ~np.isnan(rows)
    bad = np.flatnonzero(z['valid'] == 0)
    s = tr.seg_starts(z['lengths'])
    want_gone = np.zeros(len(rows), bool)
    for b in bad:
        v = np.searchsorted(s, b, side='right') - 1
        for i in range(max(s[v], b - 2), b + 1):
            want_gone[i] = i + 2 < s[v + 1]
    assert np.array_equal(gone, want_gone) and gone.sum() == len(z['accel']) - len(z['accel_valid'])
    assert np.isnan(masked[s[3]:s[4]]).all()                  # the 5-frame video has no triple left


def test_error_rows_on_closed_forms():
    rs = np.random.RandomState(1)
    L = (1, 2, 3, 7)
    g = tr.walk(rs, L, ne=5).astype(np.float64)
    rows = tr.error_rows(g + np.array([3.0, 4.0, 0.0]), g, L)            # a pure offset: no acceleration error, |offset| = 5, PA removes it
    ok = ~np.isnan(rows[:, 0])
    assert ok.sum() == 1 + 5 and np.abs(rows[ok, 0]).max() <= 1e-9
    assert np.abs(rows[:, 1] - 5.0).max() <= 1e-9 and np.abs(rows[:, 2]).max() <= 1e-9
    t = np.arange(sum(L), dtype=np.float64)[:, None, None]
    rows = tr.error_rows(g + 0.5 * t * t * np.array([0.0, 0.0, 2.0]), g, (sum(L),))       # constant acceleration 2 along z
    assert np.abs(rows[:-2, 0] - 2.0).max() <= 1e-9 and np.isnan(rows[-2:, 0]).all()
    sums = tr.video_sums(rows, (sum(L),))
    assert sums[0, 3] == sum(L) - 2 and sums[0, 4] == sum(L) and sums[0, 5] == 0.0
    assert np.isnan(tr.summary(tr.error_rows(g + 1.0, g, L), L)['accel'])     # a video without a triple: np.mean of nothing


# ---- gator_amd.temporal: what is refused on the host --------------------------------------------------------------------------------------

def _joints(F=10, ne=14):
    rs = np.random.RandomState(3)
    return torch.from_numpy(rs.randn(F, ne, 3).astype(np.float32)), torch.from_numpy(rs.randn(F, ne, 3).astype(np.float32))


@pytest.mark.parametrize('case', ['lengths sum', 'zero length', 'negative length', 'no video', 'float lengths', 'both groupings', 'index too large',
                                  'negative index', 'index twice', 'index missing', 'empty index list', 'float indices', 'empty input', 'scalar',
                                  'integer input', 'out dtype', 'dt zero', 'nan cutoff'])
def test_smooth_pose_refuses_on_the_host(case):
    p, _ = _joints()
    kw = {}
    if case == 'lengths sum':
        kw['lengths'] = [4, 5]
    elif case == 'zero length':
        kw['lengths'] = [10, 0]
    elif case == 'negative length':
        kw['lengths'] = [11, -1]
    elif case == 'no video':
        kw['lengths'] = []
    elif case == 'float lengths':
        kw['lengths'] = [5.0, 5.0]
    elif case == 'both groupings':
        kw.update(lengths=[10], video_indices=[np.arange(10)])
    elif case == 'index too large':
        kw['video_indices'] = [np.arange(5), np.arange(6, 11)]      # 0..4 and 6..10: 10 is outside
    elif case == 'negative index':
        kw['video_indices'] = [np.arange(9), np.array([-1])]
    elif case == 'index twice':
        kw['video_indices'] = [np.arange(5), np.array([5, 6, 7, 8, 8])]
    elif case == 'index missing':
        kw['video_indices'] = [np.arange(5), np.arange(5, 9)]
    elif case == 'empty index list':
        kw['video_indices'] = []
    elif case == 'float indices':
        kw['video_indices'] = [np.arange(10) * 1.0]
    elif case == 'empty input':
        p = p[:0]
    elif case == 'scalar':
        p = torch.tensor(1.0)
    elif case == 'integer input':
        p = p.long()
    elif case == 'out dtype':
        kw['out_dtype'] = torch.float16
    elif case == 'dt zero':
        kw['dt'] = 0.0
    elif case == 'nan cutoff':
        kw['min_cutoff'] = float('nan')
    with pytest.raises(ValueError):
        temporal.smooth_pose(p, **kw)


def test_an_empty_video_among_the_index_arrays_is_refused():
    p, _ = _joints()
    with pytest.raises(ValueError, match='at least one frame'):
        temporal.smooth_pose(p, video_indices=[np.arange(10), np.array([], np.int64)])


@pytest.mark.parametrize('case', ['2 joints', '33 joints', 'shape mismatch', 'xy joints', '2-d', 'lengths sum', 'valid length', 'float valid',
                                  'index twice'])
def test_sequence_errors_and_accel_error_refuse_on_the_host(case):
    p, g = _joints()
    kw = {}
    if case == '2 joints':
        p, g = p[:, :2], g[:, :2]
    elif case == '33 joints':
        p, g = p.repeat(1, 3, 1)[:, :33], g.repeat(1, 3, 1)[:, :33]
    elif case == 'shape mismatch':
        g = g[:9]
    elif case == 'xy joints':
        p, g = p[:, :, :2], g[:, :, :2]
    elif case == '2-d':
        p, g = p[:, 0], g[:, 0]
    elif case == 'lengths sum':
        kw['lengths'] = [3, 3]
    elif case == 'valid length':
        kw['valid'] = torch.ones(9, dtype=torch.uint8)
    elif case == 'float valid':
        kw['valid'] = torch.ones(10)
    with pytest.raises(ValueError):
        if case == 'index twice':
            temporal.sequence_errors(p, g, video_indices=[np.array([0, 1, 2, 3, 4]), np.array([4, 5, 6, 7, 8])])
        else:
            temporal.sequence_errors(p, g, **kw)
    if case != 'index twice':
        with pytest.raises(ValueError):
            temporal.accel_error(g, p, **kw)


def test_host_tensors_are_refused_after_the_checks():
    p, g = _joints()
    with pytest.raises(RuntimeError, match='HIP device'):
        temporal.smooth_pose(p)
    with pytest.raises(RuntimeError, match='HIP device'):
        temporal.sequence_errors(p, g, lengths=[4, 6])
    with pytest.raises(RuntimeError, match='HIP device'):
        temporal.accel_error(g, p, valid=np.ones(10, bool))
    with pytest.raises(ValueError):                      # a bad grouping is reported first, device or not
        temporal.smooth_pose(p, lengths=[4, 5])


def test_segments_of_index_arrays():
    seg, order = temporal._segments(6, None, [np.array([4, 0]), np.array([5]), np.array([2, 1, 3])], 't')
    assert seg.tolist() == [0, 2, 3, 6] and order.tolist() == [4, 0, 5, 2, 1, 3]
    seg, order = temporal._segments(6, None, None, 't')
    assert seg.tolist() == [0, 6] and order is None
    seg, order = temporal._segments(6, (1, 2, 3), None, 't')
    assert seg.tolist() == [0, 1, 3, 6] and order is None


def test_temporal_unit_is_built_and_bound():
    assert 'temporal.hip' in build.SOURCES
    assert 'gator_one_euro_f32' in _lib.SIGNATURES and 'gator_sequence_errors' in _lib.SIGNATURES
    assert len(_lib.SIGNATURES['gator_one_euro_f32'][1]) == 12 and len(_lib.SIGNATURES['gator_sequence_errors'][1]) == 11
    assert temporal.SEQUENCE_ERROR_COLUMNS == ('accel', 'MPJPE', 'PA-MPJPE') and temporal.PREFETCH == 8
