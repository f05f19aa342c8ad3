"""csrc/temporal.hip through gator_amd.temporal, against the reference's own runs (tests/golden/temporal.npz) and the fp64 restatements
of tests/temporal_refs.py.

The filter's float64 output is compared BIT FOR BIT.  That is derived, not measured: every operation of the recursion is an IEEE
add, multiply, divide or abs on the same fp64 values in the same order as numpy's, so any difference is a bug -- typically a
multiply-add contracted into one FMA.  Columns 0 and 1 of the error rows are means of at most 32 square roots of sums of three squares
in fp64, about 40 roundings of 1.1e-16: a relative 1e-13 leaves a twenty-fold margin.  Column 2 (after the similarity fit) is held to
the suite's criterion for PA errors, eval_edge_refs.errors_bound.

`python -m pytest tests/test_gpu_temporal.py -q -s -m gpu` prints the ratios kept in profiles/temporal.txt."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from gator_amd import _lib, temporal
from tests import eval_edge_refs as er
from tests import temporal_refs as tr
from tests.helpers import load_golden

pytestmark = pytest.mark.gpu

PF = temporal.PREFETCH
REL = 1e-13


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64 if x.dtype == np.float64 else np.uint32)


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape
    bad = np.argwhere(bits(got) != bits(want))
    assert not len(bad), ('%d of %d values differ, first at %s: %r != %r'
                          % (len(bad), got.size, bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


def smooth(x, **kw):
    return temporal.smooth_pose(dev(x), **kw).cpu().numpy()


def within(got, want, bound, what):
    """NaN exactly where the reference has NaN, everything else within its bound; prints the worst ratio."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, np.argwhere(np.isnan(got) != np.isnan(want))[:4].tolist())
    ok = ~np.isnan(want)
    ratio = np.abs(got - want)[ok] / np.broadcast_to(bound, want.shape)[ok]
    worst = float(ratio.max()) if ratio.size else 0.0
    print('\n%-64s worst |ours - fp64 reference| / bound: %.4f' % (what, worst))
    assert worst <= 1.0, (what, worst)


# ---- the filter against the reference's own runs ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('k', [0, 1, 2])
def test_filter_is_the_references_smooth_pose_bit_for_bit(k):
    z = load_golden('temporal')
    mc, beta = z['params'][k]
    got = smooth(z['pred'], lengths=z['lengths'], min_cutoff=float(mc), beta=float(beta))
    assert got.dtype == np.float64 and got.shape == z['pred'].shape
    same_bits(got, z['smooth_%d' % k])


def test_filter_with_dt_one_thirtieth():
    """The kernel's t_e is dt at every step: the restatement with a constant t_e, bit for bit.  The reference's run (timestamps idx * dt,
    whose differences are dt to rounding only) is within the bound derived in tests/test_host_temporal_refs.py."""
    z = load_golden('temporal')
    s, v, dt = tr.seg_starts(z['lengths']), int(z['dt_video']), float(z['dt'])
    x = z['pred'][s[v]:s[v + 1]]
    mc, beta = (float(q) for q in z['dt_params'])
    got = smooth(x, min_cutoff=mc, beta=beta, dt=dt)
    same_bits(got, tr.one_euro(x, mc, beta, 1.0, dt))
    assert np.abs(got - z['smooth_dt']).max() <= 1e-11 * np.abs(x).max()
    got = smooth(x, min_cutoff=mc, beta=beta, dt=dt, d_cutoff=0.37)
    same_bits(got, tr.one_euro(x, mc, beta, 0.37, dt))


# ---- the filter's edges, against the restatement on fresh inputs --------------------------------------------------------------------------

def signal(rs, lengths, C):
    return tr.walk(rs, lengths, ne=C, spread=200.0).reshape(sum(lengths), C * 3)[:, :C].copy()


@pytest.mark.parametrize('C', [1, 42, 257])
def test_every_video_length_around_the_prefetch_ring(C):
    """Lengths 1 .. 2 PF + 1 in one launch: shorter than the ring, exactly one and two rings, one frame more."""
    L = tuple(range(1, 2 * PF + 2))
    x = signal(np.random.RandomState(10 + C), L, C)
    same_bits(smooth(x, lengths=L), tr.one_euro_videos(x, L))
    same_bits(smooth(x, lengths=L, min_cutoff=0.004, beta=0.005), tr.one_euro_videos(x, L, min_cutoff=0.004, beta=0.005))


def test_a_whole_mesh_of_channels():
    """C = 20670 (a [T,6890,3] mesh sequence): 323 channel chunks, the last one partly filled; the trailing shape is kept."""
    rs = np.random.RandomState(20)
    x = (rs.randn(1, 6890, 3) * 400.0 + np.cumsum(rs.randn(5, 6890, 3) * 6.0, 0)).astype(np.float32)
    got = smooth(x)
    assert got.shape == (5, 6890, 3)
    same_bits(got.reshape(5, -1), tr.one_euro(x.reshape(5, -1)))


@functools.lru_cache(maxsize=None)
def many_videos():
    """70 videos of mixed lengths (1 .. 40, the first a single frame, the last the longest), 42 channels, and the restatement's result."""
    rs = np.random.RandomState(30)
    L = (1,) + tuple(int(t) for t in rs.randint(1, 41, 68)) + (40,)
    x = signal(rs, L, 42)
    return L, x, tr.one_euro_videos(x, L)


def test_one_video_and_seventy():
    L, x, want = many_videos()
    same_bits(smooth(x, lengths=L), want)
    same_bits(smooth(x), tr.one_euro(x))                  # no grouping: one video of all the frames


@pytest.mark.parametrize('v', [0, 1, 35, 69])
def test_a_video_does_not_depend_on_its_neighbours(v):
    """Alone, first among others and last among others: the same bits as in its place among the seventy."""
    L, x, want = many_videos()
    s = tr.seg_starts(L)
    mine, ref = x[s[v]:s[v + 1]], want[s[v]:s[v + 1]]
    same_bits(smooth(mine), ref)
    others = np.concatenate([x[:s[v]], x[s[v + 1]:]])
    Lo = L[:v] + L[v + 1:]
    same_bits(smooth(np.concatenate([mine, others]), lengths=(L[v],) + Lo)[:L[v]], ref)
    same_bits(smooth(np.concatenate([others, mine]), lengths=Lo + (L[v],))[-L[v]:], ref)


def test_shuffled_video_indices_equal_the_contiguous_case():
    L, x, want = many_videos()
    rs = np.random.RandomState(31)
    s = tr.seg_starts(L)
    perm = rs.permutation(len(x))                         # frame k of the video order stands at perm[k] of the input
    shuffled = np.empty_like(x)
    shuffled[perm] = x
    vids = [perm[a:b] for a, b in zip(s[:-1], s[1:])]
    vids = [vids[i] for i in rs.permutation(len(vids))]   # and the videos are listed in another order
    got = smooth(shuffled, video_indices=vids)
    same_bits(got[perm], want)


def test_float32_output_is_the_rounding_of_the_float64_one():
    L, x, want = many_videos()
    got = smooth(x, lengths=L, out_dtype=torch.float32)
    assert got.dtype == np.float32
    same_bits(got, want.astype(np.float32))
    same_bits(smooth(x.astype(np.float64), lengths=L), want)          # a float64 input is read as float32


def test_a_non_finite_value_poisons_its_channel_from_its_frame_on_and_nothing_else():
    L, x, want = many_videos()
    s = tr.seg_starts(L)
    x = x.copy()
    v = [i for i, T in enumerate(L) if T >= 12][:3]
    spots = [(s[v[0]] + 3, 5, np.nan), (s[v[1]], 0, np.inf), (s[v[2]] + L[v[2]] - 1, 41, -np.inf), (s[v[0]] + 9, 17, np.nan)]
    mask = np.zeros(x.shape, bool)
    for (f, c, val), vid in zip(spots, (v[0], v[1], v[2], v[0])):
        x[f, c] = val
        mask[f:s[vid + 1], c] = True
    # an infinity at a video's FIRST frame is copied as it is; NaN follows from the next frame on
    got = smooth(x, lengths=L)
    ref = tr.one_euro_videos(x, L)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref))
    assert np.array_equal(~np.isfinite(got), mask) and np.isinf(got[s[v[1]], 0]) and np.isnan(got[s[v[1]] + 1, 0])
    same_bits(got[~mask], want[~mask])
    g32 = smooth(x, lengths=L, out_dtype=torch.float32)
    assert np.array_equal(np.isnan(g32), np.isnan(ref))
    same_bits(g32[~mask], want.astype(np.float32)[~mask])


# ---- the error columns ----------------------------------------------------------------------------------------------------------------------

def run_errors(pred, gt, L, valid=None):
    """gator_sequence_errors itself: rows [F,3] and sums [V,6], float64 on the host."""
    p, g = dev(pred), dev(gt)
    seg = dev(tr.seg_starts(L))
    v = None if valid is None else dev(np.asarray(valid, np.uint8))
    rows = torch.full((len(pred), 3), 7.0, device='cuda', dtype=torch.float64)
    sums = torch.full((len(L), 6), 7.0, device='cuda', dtype=torch.float64)
    temporal._launch_sequence_errors(p, g, v, seg, len(L), rows, sums)
    return rows.cpu().numpy(), sums.cpu().numpy()


def check_rows(rows, sums, want, L, what):
    within(rows[:, 0], want[:, 0], REL * np.abs(want[:, 0]), what + ': accel')
    within(rows[:, 1], want[:, 1], REL * np.abs(want[:, 1]), what + ': MPJPE')
    within(rows[:, 2], want[:, 2], er.errors_bound(want[:, 2]), what + ': PA-MPJPE')
    ws = tr.video_sums(rows, L)                            # the sums of OUR rows: the reduction alone is under test here
    assert np.array_equal(sums[:, 3:], ws[:, 3:]), (sums[:, 3:], ws[:, 3:])       # counts and the spare column: exact
    within(sums[:, :3], ws[:, :3], REL * np.abs(ws[:, :3]) + 1e-300, what + ': per-video sums')


@functools.lru_cache(maxsize=None)
def error_case(F, ne):
    """Videos of 1, 2 and 3 frames, then the rest split in two: F either side of the 64-frame block.  fp64 smoothed prediction."""
    rs = np.random.RandomState(100 * F + ne)
    rest = F - 6
    L = (1, 2, 3, rest // 2, rest - rest // 2)
    g = tr.walk(rs, L, ne=ne, jitter=0.0)
    p32 = (g.astype(np.float64) * 1.05 + rs.randn(F, ne, 3) * 15.0 + rs.randn(F, 1, 3) * 30.0).astype(np.float32)
    p64 = tr.one_euro_videos(p32, L, min_cutoff=0.004, beta=0.005)
    return L, g, p32, p64, tr.error_rows(p32, g, L), tr.error_rows(p64, g, L)


@pytest.mark.parametrize('ne', [3, 14, 32])
@pytest.mark.parametrize('F', [63, 64, 65])
def test_error_rows_and_video_sums(F, ne):
    L, g, p32, p64, want32, want64 = error_case(F, ne)
    assert np.isnan(want64[[0, 1, 2, 3, 4, 5], 0]).tolist() == [True, True, True, False, True, True]      # lengths 1, 2, 3: one triple
    rows, sums = run_errors(p64, g, L)
    check_rows(rows, sums, want64, L, 'F %d ne %d float64 pred' % (F, ne))
    rows, sums = run_errors(p32, g, L)
    check_rows(rows, sums, want32, L, 'F %d ne %d float32 pred' % (F, ne))


def test_valid_mask_against_the_references_vis_handling():
    z = load_golden('temporal')
    L, g, sm = tuple(int(t) for t in z['lengths']), z['gt'], z['smooth_0']
    for valid, key in ((None, 'accel'), (z['valid'], 'accel_valid')):
        got = temporal.accel_error(dev(g), dev(sm), lengths=L, valid=None if valid is None else dev(valid)).cpu().numpy()
        ref = tr.accel_rows(sm, g, L, valid)
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        kept = got[~np.isnan(got)]
        within(kept, z[key], REL * np.abs(z[key]), 'compute_error_accel of the reference, %s' % key)
    valid = z['valid']
    rows, sums = run_errors(sm, g, L, valid)
    check_rows(rows, sums, tr.error_rows(sm, g, L, valid), L, 'golden videos under the mask')
    assert sums[3, 3] == 0 and sums[:, 3].sum() == len(z['accel_valid'])          # the 5-frame video keeps no triple
    # a host mask (bool numpy) is the same as a device one
    got = temporal.accel_error(dev(g), dev(sm), lengths=L, valid=valid.astype(bool)).cpu().numpy()
    same_bits(got, rows[:, 0])


def test_rows_do_not_depend_on_the_batch():
    L, g, _, p64, _, _ = error_case(65, 14)
    rows, _ = run_errors(p64, g, L)
    s = tr.seg_starts(L)
    a, b = s[3], s[4]
    alone, _ = run_errors(p64[a:b], g[a:b], (b - a,))
    same_bits(alone, rows[a:b])
    again, _ = run_errors(p64, g, L)
    same_bits(again, rows)


def test_sequence_errors_is_the_commented_block_of_evaluate():
    """Smoothing, the rows, the per-video means and the three averages in one call, against the same chain on the host."""
    z = load_golden('temporal')
    L, g, p = tuple(int(t) for t in z['lengths']), z['gt'], z['pred']
    rows, per_video, summary = temporal.sequence_errors(dev(p), dev(g), lengths=L)
    rows = rows.cpu().numpy()
    want = tr.error_rows(z['smooth_0'], g, L)             # smooth_0: the reference's smooth_pose(min_cutoff=0.004, beta=0.005)
    check_rows(rows, tr.video_sums(rows, L), want, L, 'sequence_errors on the golden videos')
    ref = tr.summary(rows, L)
    assert np.isnan(summary['accel']) and np.isnan(ref['accel'])          # videos of 1 and 2 frames: np.mean of nothing, not hidden
    assert np.isnan(per_video[:2, 0]).all() and not np.isnan(per_video[2:, 0]).any()
    for k in ('MPJPE', 'PA-MPJPE'):
        assert abs(summary[k] - ref[k]) <= REL * abs(ref[k]), (k, summary[k], ref[k])
    # without the short videos all three are numbers, and the frames may come shuffled
    s = tr.seg_starts(L)
    keep = np.arange(s[2], s[-1])
    rs = np.random.RandomState(5)
    perm = rs.permutation(len(keep))
    ps, gs = np.empty_like(p[keep]), np.empty_like(g[keep])
    ps[perm], gs[perm] = p[keep], g[keep]
    vids = [perm[a - s[2]:b - s[2]] for a, b in zip(s[2:-1], s[3:])]
    rows2, per_video2, summary2 = temporal.sequence_errors(dev(ps), dev(gs), video_indices=vids)
    same_bits(rows2.cpu().numpy()[perm], rows[keep])
    ref2 = tr.summary(rows[keep], L[2:])
    for k in ('accel', 'MPJPE', 'PA-MPJPE'):
        assert np.isfinite(ref2[k]) and abs(summary2[k] - ref2[k]) <= REL * abs(ref2[k]), (k, summary2[k], ref2[k])
    within(per_video2, per_video[2:], REL * np.abs(per_video[2:]), 'per-video means, shuffled input')
    # smooth=False scores the raw prediction
    rows3, _, _ = temporal.sequence_errors(dev(p), dev(g), lengths=L, smooth=False)
    raw = tr.error_rows(p, g, L)
    within(rows3.cpu().numpy()[:, :2], raw[:, :2], REL * np.abs(raw[:, :2]), 'smooth=False')


def test_c_abi_refuses_before_any_launch():
    lib = _lib.load()
    x = torch.zeros((4, 9), device='cuda')
    seg = dev(np.array([0, 4], np.int64))
    out = torch.full((4, 9), 7.0, device='cuda', dtype=torch.float64)
    rows = torch.full((4, 3), 7.0, device='cuda', dtype=torch.float64)
    sums = torch.full((1, 6), 7.0, device='cuda', dtype=torch.float64)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: t.data_ptr()      # noqa: E731
    euro = [(None, P(seg), 4, 1, 9, 1.0, P(out)), (P(x), None, 4, 1, 9, 1.0, P(out)), (P(x), P(seg), 4, 1, 9, 1.0, None),
            (P(x), P(seg), 0, 1, 9, 1.0, P(out)), (P(x), P(seg), 4, 0, 9, 1.0, P(out)), (P(x), P(seg), 4, 5, 9, 1.0, P(out)),
            (P(x), P(seg), 4, 1, 0, 1.0, P(out)), (P(x), P(seg), 4, 1, 9, 0.0, P(out)), (P(x), P(seg), 4, 1, 9, float('nan'), P(out))]
    for xi, si, F, V, C, dt, oi in euro:
        assert lib.gator_one_euro_f32(xi, si, F, V, C, 0.004, 0.7, 1.0, dt, 1, oi, st) == -1
        assert b'gator_one_euro_f32' in lib.gator_last_error()
    seqs = [(None, P(x), P(seg), 4, 1, 3), (P(x), None, P(seg), 4, 1, 3), (P(x), P(x), None, 4, 1, 3), (P(x), P(x), P(seg), 0, 1, 3),
            (P(x), P(x), P(seg), 4, 0, 3), (P(x), P(x), P(seg), 4, 5, 3), (P(x), P(x), P(seg), 4, 1, 2), (P(x), P(x), P(seg), 4, 1, 33)]
    for pi, gi, si, F, V, ne in seqs:
        assert lib.gator_sequence_errors(pi, 0, gi, None, si, F, V, ne, P(rows), P(sums), st) == -1
    assert lib.gator_sequence_errors(P(x), 0, P(x), None, P(seg), 4, 1, 3, None, P(sums), st) == -1
    assert lib.gator_sequence_errors(P(x), 0, P(x), None, P(seg), 4, 1, 3, P(rows), None, st) == -1
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (rows == 7.0).all() and (sums == 7.0).all()
