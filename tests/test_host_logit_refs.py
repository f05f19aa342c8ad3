"""CPU-only: the weight transforms of tests/logit_refs.py put the fp64 oracle's logits where tests/test_gpu_softmax_edges.py says
they are.  Conditions, not measurements: each bound below is what the GPU test needs of its input (beyond +-88.7 natural units an
exp() with no maximum subtracted overflows fp32 or flushes its row sum to zero; a row spread of 20 / 150 leaves a softmax one / no
key besides the maximum above fp32's / fp64's rounding), both golden variants, the 8 samples the GPU tests use."""
import numpy as np
import pytest
import torch

from tests import logit_refs as lr
from tests.helpers import VARIANTS

GAINS = (('enc_gain', 'enc'), ('cross_gain', 'cross'), ('head_gain', 'head'))
ALL = [('enc_gain', 3), ('enc_gain', 8), ('enc_bias_gain', 32), ('enc_kshift', lr.ENC_KSHIFT), ('cross_gain', 3), ('cross_gain', 8),
       ('self_kshift', lr.SELF_KSHIFT), ('head_gain', 3), ('head_gain', 8), ('head_shift', 100.0), ('head_shift', -100.0)]


def _show(name, tr, r):
    print('\n[%s %s] %s | fp32 oracle vs fp64: verts %.2e mm, pose3d %.2e mm' % (name, tr, lr.fmt_ranges(r.ranges), r.ref_v, r.ref_p))


@pytest.mark.parametrize('name', VARIANTS)
def test_the_seeded_weights_keep_every_softmax_comfortable(name):
    """The gap this module closes, as a condition: without a transform no site leaves |logit| <= 8, spread <= 8."""
    r = lr.run(name)
    _show(name, None, r)
    for site in lr.SITES:
        assert r.ranges[site]['absmax'] <= 8.0 and r.ranges[site]['spread'] <= 8.0, site


@pytest.mark.parametrize('tr,site', [(('enc_kshift', lr.ENC_KSHIFT), 'enc'), (('self_kshift', lr.SELF_KSHIFT), 'self')])
@pytest.mark.parametrize('name', VARIANTS)
def test_k_shifts_preserve_the_function_and_move_row_maxima_past_100(name, tr, site):
    base, r = lr.run(name), lr.run(name, tr)
    _show(name, tr, r)
    dv, dp = float(np.abs(r.v64 - base.v64).max() * 1e3), float(np.abs(r.p64 - base.p64).max())
    print('shifted fp64 oracle vs unshifted: verts %.2e mm, pose3d %.2e mm' % (dv, dp))
    assert dv <= 1e-9 and dp <= 1e-9
    assert r.ranges[site]['rowmax_min'] <= -100.0 and r.ranges[site]['rowmax_max'] >= 100.0
    assert r.ranges[site]['spread'] <= 1.0001 * base.ranges[site]['spread'] + 1e-9      # constant over the keys: the rows keep their shape


@pytest.mark.parametrize('c', [100.0, -100.0])
@pytest.mark.parametrize('name', VARIANTS)
def test_head_shift_moves_every_row_maximum_past_95(name, c):
    r = lr.run(name, ('head_shift', c))
    _show(name, ('head_shift', c), r)
    h = r.ranges['head']
    assert (h['rowmax_min'] >= 95.0) if c > 0 else (h['rowmax_max'] <= -95.0)


@pytest.mark.parametrize('fam,site', GAINS)
@pytest.mark.parametrize('name', VARIANTS)
def test_gains_reach_sharp_rows(name, fam, site):
    for g, need in ((3, 20.0), (8, 150.0)):
        r = lr.run(name, (fam, g))
        _show(name, (fam, g), r)
        assert r.ranges[site]['spread'] >= need


@pytest.mark.parametrize('name', VARIANTS)
def test_bias_gain_reaches_bias_dominated_rows(name):
    r = lr.run(name, ('enc_bias_gain', 32))
    _show(name, ('enc_bias_gain', 32), r)
    assert r.ranges['enc']['spread'] >= 100.0


@pytest.mark.parametrize('tr', ALL, ids=lambda t: '%s_%g' % t)
@pytest.mark.parametrize('name', VARIANTS)
def test_a_transform_leaves_the_other_sites_where_they_were(name, tr):
    base, r = lr.run(name), lr.run(name, tr)
    for site in lr.SITES:
        if site != lr.SITE_OF[tr[0]]:
            for q in ('absmax', 'spread'):
                assert r.ranges[site][q] <= 1.5 * base.ranges[site][q], (site, q)


@pytest.mark.parametrize('name', VARIANTS)
def test_sharp_cross_attention_peaks_at_both_ends_of_the_joint_mask(name):
    """Under cross_gain(8) some (sample, head, token) row has its argmax at joint 0 and some at joint J-1, the last key in front of
    the masked columns J..31 of the 32-row tile."""
    r = lr.run(name, ('cross_gain', 8))
    print('\n[%s] cross-attention argmax per joint: %s' % (name, r.cross_argmax.tolist()))
    assert r.cross_argmax[0] > 0 and r.cross_argmax[r.c.J - 1] > 0


def test_transforms_leave_their_input_alone_and_touch_only_their_tensors():
    c, sd, x = lr.setup('h36m17_bn')
    before = {k: t.clone() for k, t in sd.items()}
    n = {'enc_gain': 12, 'enc_bias_gain': 2, 'enc_kshift': 6, 'cross_gain': 6, 'self_kshift': 3, 'head_gain': 2, 'head_shift': 1}
    for tr in ALL:
        sd2 = lr.apply(sd, tr)
        assert sum(not torch.equal(sd2[k], sd[k]) for k in sd) == n[tr[0]], tr
    assert all(torch.equal(sd[k], before[k]) for k in sd)
    b = 'pose_lifter.blocks.2.attn.qkv.'
    sd2 = lr.enc_gain(sd, 3)
    assert torch.equal(sd2[b + 'weight'][256:], sd[b + 'weight'][256:]) and torch.equal(sd2[b + 'bias'][:256], sd[b + 'bias'][:256] * 3)
    sd2 = lr.enc_kshift(sd, 48.0)
    assert torch.equal(sd2[b + 'bias'][:128], sd[b + 'bias'][:128]) and torch.equal(sd2[b + 'bias'][256:], sd[b + 'bias'][256:])
    sd2 = lr.head_shift(sd, 100.0)
    assert torch.equal(sd2['pose2mesh.motion_linear.bias'][20:], sd['pose2mesh.motion_linear.bias'][20:])


def test_the_logit_taps_do_not_change_the_oracle():
    from oracle import gator_oracle as go
    c, sd, x = lr.setup('coco19_alpha')
    v, p = go.gator_forward(sd, c, x, torch.float32)
    v2, p2 = go.gator_forward(sd, c, x, torch.float32, {})
    assert torch.equal(v, v2) and torch.equal(p, p2)
