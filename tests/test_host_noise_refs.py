"""CPU checks of the detector noise (-m "not gpu"): the numpy restatement (tests/noise_refs.py) against recorded runs of the reference's
own synthesize_pose and generate_syn_error (tests/golden/detector_noise.npz, tools/gen_golden_noise.py) in distribution; its zero-noise
form against the oracle's clean chain; the absence of undecided candidates in the inputs the GPU tests restate; the plumbing
(signature, build list, kernel registration) and every host-side refusal of gator_amd.noise."""
import ctypes

import numpy as np
import pytest
import torch
from scipy import stats as sps

from gator_amd import _lib, batch, build, kernel_resources, noise
from oracle import gator_oracle as go
from tests import noise_refs as nr
from tests.helpers import load_golden

FAMILY_ALPHA = 1e-3           # family-wise significance of the distribution test, Bonferroni over its comparisons
RESTATED_DRAWS = 1000         # per pose; the fixture holds 5000 of the reference's


def _merged(a, b):
    """Merge, from the right, the bins whose expected count in the smaller sample is below 5."""
    a, b = list(map(float, a)), list(map(float, b))
    small = min(sum(a), sum(b)) / (sum(a) + sum(b))
    i = len(a) - 1
    while len(a) > 1 and i >= 0:
        if (a[i] + b[i]) * small < 5.0:
            k = i - 1 if i > 0 else 1
            a[k] += a[i]
            b[k] += b[i]
            del a[i], b[i]
            i = min(i, len(a) - 1)
        else:
            i -= 1
    return np.array(a), np.array(b)


def two_sample_chi2(a, b):
    """-> (statistic, degrees of freedom, p) of the two-sample chi-square test for histograms of unequal totals."""
    a, b = _merged(a, b)
    if len(a) < 2:
        return 0.0, 0, 1.0
    na, nb = a.sum(), b.sum()
    stat = (((np.sqrt(nb / na) * a - np.sqrt(na / nb) * b) ** 2) / (a + b)).sum()
    return float(stat), len(a) - 1, float(sps.chi2.sf(stat, len(a) - 1))


def test_chi2_helper_on_known_tables():
    assert two_sample_chi2([50, 50], [500, 500])[2] == 1.0
    assert two_sample_chi2([90, 10], [500, 500])[2] < 1e-12
    a, b = _merged([100, 3, 2, 0], [1000, 20, 30, 0])
    assert a.sum() == 105 and b.sum() == 1050 and len(a) == len(b) < 4


@pytest.mark.parametrize('pose', [0, 1, 2, 3])
def test_restatement_has_the_reference_distribution(pose):
    """Per joint, the restatement's output histograms -- distance from the clean joint and from the clean partner, tests/noise_refs.py::
    histogram -- against the reference's recorded ones: two-sample chi-square, bins of expected count < 5 merged, family-wise 1e-3 over
    all 4 x (17 + 16) comparisons.  Fixed seeds: the outcome is deterministic."""
    z = load_golden('detector_noise')
    assert int(z['n_draws']) >= 5000
    p, area = z['poses'][pose], float(z['areas'][pose])
    out = np.stack([nr.synthesize_pose(p[:, :2], p[:, 2], area, (2024, pose, n))[0] for n in range(RESTATED_DRAWS)])
    alpha = FAMILY_ALPHA / (4 * (17 + 16))
    worst = 1.0
    for j in range(17):
        hs = nr.histogram(out[:, j], p[j, :2], area, j)
        assert hs.sum() == RESTATED_DRAWS and z['hist_self'][pose, j].sum() == int(z['n_draws'])
        pairs = [('joint', hs, z['hist_self'][pose, j])]
        q = nr.partner_of(j)
        if q >= 0:
            pairs.append(('partner', nr.histogram(out[:, j], p[q, :2], area, j), z['hist_partner'][pose, j]))
        for what, mine, theirs in pairs:
            stat, df, pv = two_sample_chi2(mine, theirs)
            worst = min(worst, pv)
            assert pv >= alpha, (pose, j, what, mine.tolist(), theirs.tolist(), stat, df, pv)
    print('\npose %d: smallest p over its comparisons %.3g (bound %.3g)' % (pose, worst, alpha))


def test_restated_stats_mode_has_the_tables_moments():
    """generate_syn_error restated: per joint the mean and standard deviation of the applied noise and the share of draws that applied it,
    each within 5 standard errors of the table's value for the n draws taken (se of a mean: std / sqrt(m); of a standard deviation of
    normal draws: std / sqrt(2 (m - 1)); of a rate: sqrt(w (1 - w) / n)), m = the draws that applied the noise."""
    table = load_golden('detector_noise')['stats_table']
    n = 4000
    draws, applied = zip(*(nr.syn_error(table, (31, 7, k)) for k in range(n)))
    draws, applied = np.stack(draws).astype(np.float64), np.stack(applied)
    for j in range(len(table)):
        w, m = table[j, 4], int(applied[:, j].sum())
        assert abs(m / n - w) <= 5 * np.sqrt(w * (1 - w) / n), (j, m / n, w)
        assert (draws[~applied[:, j], j] == 0).all()
        x = draws[applied[:, j], j]
        for ax in range(2):
            mean, std = table[j, ax], table[j, 2 + ax]
            assert abs(x[:, ax].mean() - mean) <= 5 * std / np.sqrt(m), (j, ax, x[:, ax].mean(), mean)
            assert abs(x[:, ax].std(ddof=1) - std) <= 5 * std / np.sqrt(2 * (m - 1)), (j, ax, x[:, ax].std(ddof=1), std)


def test_recorded_reference_stats_agree_with_the_table():
    """The fixture's own record of generate_syn_error: the same three criteria for the reference's draws."""
    z = load_golden('detector_noise')
    table, n = z['stats_table'], int(z['stats_n'])
    for j in range(len(table)):
        w = table[j, 4]
        m = z['stats_rate'][j] * n
        assert abs(z['stats_rate'][j] - w) <= 5 * np.sqrt(w * (1 - w) / n) + 1e-12
        for ax in range(2):
            assert abs(z['stats_mean'][j, ax] - table[j, ax]) <= 5 * table[j, 2 + ax] / np.sqrt(m) + 1e-6       # float32 draws
            assert abs(z['stats_std'][j, ax] - table[j, 2 + ax]) <= 5 * table[j, 2 + ax] / np.sqrt(2 * (m - 1)) + 1e-6


def test_zero_noise_is_the_clean_chain():
    """A zero-weight table leaves the clean crop joints untouched and gives the no-noise mode's result, bit for bit; against the
    oracle's chain pose2d is held to the chain's own 2e-5 (tests/test_gpu_eval_edges.py), not to the bit: the oracle flips in fp64
    before the float32 cast (j2d_processing(f=1)), the training order restated here flips the float32 joints after the noise step."""
    c = nr.gpu_case('stats17')
    table = load_golden('detector_noise')['stats_table'].copy()
    table[:, 4] = 0.0
    r = nr.noisy_input(c['joints'], 'stats', table=table, **c['kw'])
    clean = nr.noisy_input(c['joints'], 'clean', **c['kw'])
    assert np.array_equal(r['crop'], r['clean']) and np.array_equal(r['crop'], clean['crop'])
    assert np.array_equal(r['pose2d'], clean['pose2d']) and np.array_equal(r['valid'], clean['valid'])
    kw = c['kw']
    for b in range(len(c['joints'])):
        want = go.preprocess_pose2d(c['joints'][b].astype(np.float64), rot=float(kw['rot_deg'][b]), flip=bool(kw['flip'][b]),
                                    flip_pairs=kw['flip_pairs'], res=kw['res'])
        assert (want is not None) == bool(r['valid'][b])
        if want is None:
            assert not r['pose2d'][b].any() and not r['crop'][b].any()
        else:
            assert np.abs(r['pose2d'][b] - want).max() <= 2e-5
    assert r['valid'].sum() == len(r['valid']) - 1


@pytest.mark.parametrize('name', ['coco19', 'stats17', 'detections19'])
def test_gpu_cases_have_no_undecided_candidates(name):
    """The device is compared with the restatement decision for decision; that needs every candidate of these exact inputs and seeds
    to be farther than a relative 2^-40 from its threshold -- thousands of fp64 ulps, far above any libm's sine and cosine error."""
    r = nr.restated(name, table=load_golden('detector_noise')['stats_table'])
    assert r['undecided'] == 0
    c = nr.gpu_case(name)
    assert len(c['joints']) <= 16 and r['valid'].sum() == len(r['valid']) - 1
    if name == 'coco19':
        d = nr.decisions_array(r['decisions'])
        kept = d[r['valid'] == 1]
        assert set(np.unique(kept[:, :, 5])) >= {nr.CASE_JITTER, nr.CASE_MISS, nr.CASE_GOOD}            # the cases the inputs reach
        assert (kept[:, :, 5] >= 0).all()                  # no stable input zeroes a joint (partners would have to coincide)
        assert (kept[:, :, 7] >= 0).any()                  # a miss taken from the partner's resampled points
        assert (kept[:, 0, 2:4] == 0).all()                # the nose has no partner
        assert np.array_equal(r['crop'][:, 17:], r['clean'][:, 17:])
        tiers = {int((v[:17] > 0).sum()) for v in c['kw']['joint_valid']}
        assert tiers == {17, 10, 5}


def test_philox_words_are_the_dropout_generators():
    from tests.train_refs import philox4x32
    w = nr.words(0x0123456789ABCDEF, 9, 5, nr.SET_MISS1, 12, [0, 1999])
    want = philox4x32([[0, 12 | 2 << 8, 5, 9], [1999, 12 | 2 << 8, 5, 9]], [[0x89ABCDEF, 0x01234567]], 7)
    assert np.array_equal(w, want)
    assert nr.uniform(np.uint32(0)) == 2.0 ** -33 and nr.uniform(np.uint32(0xFFFFFFFF)) < 1.0
    assert nr.index_of(0xFFFFFFFF, 2000) == 1999 and nr.index_of(0, 2000) == 0


def test_signature_build_list_and_kernel_registration():
    assert 'detector_noise.hip' in build.SOURCES
    res, args = _lib.SIGNATURES['gator_preprocess_noise_f32']
    assert res is ctypes.c_int32 and args == [ctypes.POINTER(_lib.PreprocessNoiseArgs), ctypes.c_void_p]
    for k in ('k_noise_crop', 'k_noise_candidates', 'k_noise_finish'):
        assert k in kernel_resources.HOT
    assert _lib.ABI_VERSION == 2
    m = noise.CocoDetectorNoise().struct()
    assert ctypes.sizeof(m) == 1072 and ctypes.sizeof(_lib.PreprocessNoiseArgs) == 168
    assert np.array_equal(np.array(m.var[:]), (nr.SIGMAS * 2) ** 2)
    assert list(m.partner) == [nr.partner_of(j) for j in range(17)]
    assert [m.log_ks[k] for k in range(3)] == [float(np.log(k)) for k in nr.KS]
    for j in range(17):
        assert m.inv_prob[j] == nr.inv_prob(j)
        assert [m.jitter_prob[t][j] for t in range(2)] == [nr.jitter_prob(j, n) for n in (10, 11)]
        assert [m.miss_prob[t][j] for t in range(3)] == [nr.miss_prob(j, n) for n in (5, 10, 11)]
    assert (m.n_jitter, m.n_miss, m.n_inv, m.n_good) == (nr.N, 4 * nr.N, nr.N, nr.N // 4)


def test_host_side_refusals():
    """Every check that raises before a device is needed."""
    x = torch.zeros(2, 19, 2)
    coco = noise.CocoDetectorNoise()
    table = np.ones((17, 2))
    st = noise.ErrorStatsNoise(table, table, np.ones(17))
    bad = [dict(joint_img=torch.zeros(2, 19), model=coco, seed=0),
           dict(joint_img=torch.zeros(2, 19, 4), model=coco, seed=0),
           dict(joint_img=torch.zeros(2, 33, 2), model=coco, seed=0),
           dict(joint_img=torch.zeros(2, 16, 2), model=coco, seed=0),                       # coco needs 17 joints
           dict(joint_img=x, model=st, seed=0),                                            # a 17-joint table, 19 joints
           dict(joint_img=x, model=None, seed=0),                                          # neither model nor detections
           dict(joint_img=x, model=coco, seed=0, detections=torch.zeros(2, 19, 2)),
           dict(joint_img=x, model=None, seed=0, detections=torch.zeros(2, 17, 2)),
           dict(joint_img=x, model='coco', seed=0),
           dict(joint_img=x, model=coco, seed=-1),
           dict(joint_img=x, model=coco, seed=2 ** 64),
           dict(joint_img=x, model=coco, seed=0, step=-1),
           dict(joint_img=x, model=coco, seed=0, step=2 ** 32),
           dict(joint_img=x, model=coco, seed=0, step=torch.zeros(1, dtype=torch.int32)),
           dict(joint_img=x, model=coco, seed=0, sample_offset=-1),
           dict(joint_img=x, model=coco, seed=0, sample_offset=2 ** 32 - 1),
           dict(joint_img=x, model=coco, seed=0, flip_pairs=((1, -2),)),
           dict(joint_img=x, model=coco, seed=0, flip_pairs=(1, 2)),
           dict(joint_img=x, model=coco, seed=0, res=(0, 384)),
           dict(joint_img=x, model=coco, seed=0, rot_deg=np.zeros(3)),
           dict(joint_img=x, model=coco, seed=0, flip=torch.zeros(2)),
           dict(joint_img=x, model=coco, seed=0, joint_valid=torch.ones(2, 17)),
           dict(joint_img=torch.zeros(2, 17, 2), model=st, seed=0, return_decisions=True)]
    for kw in bad:
        kw = dict(kw)
        with pytest.raises(ValueError):
            noise.noisy_input(kw.pop('joint_img'), kw.pop('model'), **kw)
    with pytest.raises(RuntimeError, match='HIP device'):                                  # a host tensor: no CPU path
        noise.noisy_input(x, coco, seed=0)
    for args in ((np.ones((17, 3)), table, np.ones(17)), (table, np.ones((16, 2)), np.ones(17)), (table, table, np.ones(16)),
                 (table, -table, np.ones(17)), (table * np.nan, table, np.ones(17)), (np.ones((33, 2)), np.ones((33, 2)), np.ones(33))):
        with pytest.raises(ValueError):
            noise.ErrorStatsNoise(*args)
    assert 'noise' in batch.camera_frame_batch.__kwdefaults__ and batch.camera_frame_batch.__kwdefaults__['noise'] is None
