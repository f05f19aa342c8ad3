"""Every softmax of the forward, in every kernel form that computes it, under sharp and shifted logits.

The forward has four softmaxes (encoder J x J attention with the hop / path bias; MDR cross-attention over the J joint keys of a 32-row
tile masked at J; MDR 431-key self-attention; the head's 20-way mix), each hand-written in several forms.  With the seeded weights
every logit stays within +-7 and every row's spread within 8, where a softmax with no maximum subtracted, a running maximum exchanged
wrongly between half-waves or a masked key scored 0 instead of -1e30 passes every other test.  tests/logit_refs.py moves the logits:
gains (row spreads 20 .. 450: all but one key below fp32's rounding), exact k-shifts (row maxima beyond +-100, the function unchanged)
and the head's +-100 shift; tests/test_host_logit_refs.py proves those ranges on the fp64 oracle.

Every test: B = 8, a fresh module per form, the transform applied to the module's and to the oracle's state dict alike, and
  1. device_status() clean and m.arithmetic still what the test set (a heal must not silently swap the form under test),
  2. finite output,
  3. vertex error against the fp64 oracle ON THE SAME WEIGHTS <= max(1.5e-3 mm, 2 x ref), ref = the fp32 oracle's error on the same
     weights and samples (the criterion of test_attention_rescale_paths_under_large_logits); pose3d likewise with the suite's 1e-3 mm
     floor, for the encoder's transforms,
  4. under the two exact k-shifts, the same bound against the UNSHIFTED oracle,
  5. a second run and samples [2:5] run alone are bit-equal (the tiled encoder is forced for every batch size, so it compares within
     itself).
gator_create takes the softmax-invisible part of K's bias and of the mix biases out when it packs them (fused_api.hip), so under enc_kshift and
head_shift the encoder and head kernels see ordinary logits: those cases pin that removal (on the parent k_gat / k_gat_tiled came out at up to
2.5 x ref and the head at 2.7 x ref), the gains pin the kernels' maximum subtraction, self_kshift both.
Config 3 (precision = 'bf16') under the three gains: the bar of test_config3_guard_keeps_two_planes_under_sharp_attention (1 mm max,
0.2 mm rms), on one plane or after the guard took the context out of the mode.  Measured figures: profiles/softmax_edge_tests.txt."""
import numpy as np
import pytest
import torch

from tests import logit_refs as lr
from tests.helpers import build_model

pytestmark = pytest.mark.gpu

H, C = 'h36m17_bn', 'coco19_alpha'
SWITCHES = ('GATOR_GAT_X3', 'GATOR_GAT8', 'GATOR_GAT8_H4', 'GATOR_GAT_TILED', 'GATOR_GAT_TILED_H4', 'GATOR_MDR_X3', 'GATOR_UPSAMPLE_X3',
            'GATOR_MDR_PERSIST', 'GATOR_MDR_HEAD_PARTIALS', 'GATOR_C3_MDR', 'GATOR_C3_ENCODER', 'GATOR_C3_GUARD')
# form -> (environment read when the context is created, arithmetic)
ENC_FORMS = {
    'gat8': ({}, 'default'),                                                   # k_gat8, scores from fp16 planes
    'gat8_six': ({'GATOR_GAT8_H4': '0'}, 'default'),                           # k_gat8, the exact six products
    'gat': ({'GATOR_GAT8': '0'}, 'default'),                                   # k_gat (gat_fused.hip)
    'tiled_h4': ({'GATOR_GAT_TILED': '1', 'GATOR_GAT_TILED_H4': '1'}, 'default'),   # k_gat_tiled: VALU attention
    'tiled_six': ({'GATOR_GAT_TILED': '1', 'GATOR_GAT_TILED_H4': '0'}, 'default'),
    'gat_fp32': ({'GATOR_GAT_X3': '0'}, 'default'),                            # fp32-input MFMA
    'exact': ({}, 'exact'),
}
MDR_FORMS = {
    'x2': ({'GATOR_MDR_X3': '2'}, 'default'),                                  # JointX2 cross-attention, two-plane self-attention
    'x3': ({'GATOR_MDR_X3': '1'}, 'default'),                                  # JointF32 (XA 1), three-plane self-attention
    'mdr_fp32': ({'GATOR_MDR_X3': '0'}, 'default'),                            # JointF32 (XA 0), fp32-input MFMA
    'exact': ({}, 'exact'),
    'x2_launches': ({'GATOR_MDR_PERSIST': '0'}, 'default'),
    'x2_persist': ({'GATOR_MDR_PERSIST': '1'}, 'default'),
}
HEAD_FORMS = {'partials': ({'GATOR_MDR_HEAD_PARTIALS': '1'}, 'default'), 'whole': ({'GATOR_MDR_HEAD_PARTIALS': '0'}, 'default')}
ENC_TRANSFORMS = (('enc_gain', 3), ('enc_gain', 8), ('enc_bias_gain', 32), ('enc_kshift', lr.ENC_KSHIFT))
MDR_TRANSFORMS = (('cross_gain', 3), ('cross_gain', 8), ('self_kshift', lr.SELF_KSHIFT))
HEAD_TRANSFORMS = (('head_gain', 3), ('head_gain', 8), ('head_shift', 100.0), ('head_shift', -100.0))


def _cases(forms, transforms, both=('?',)):
    """Every transform on every form; both variants on the forms in `both`, one variant on the others, alternating."""
    out, n = [], 0
    for tr in transforms:
        for form in forms:
            if form in both or both == ('*',):
                names = (H, C)
            else:
                names = ((H, C)[n % 2],)
                n += 1
            out += [pytest.param(name, form, tr, id='%s-%s-%s_%g' % (name, form, tr[0], tr[1])) for name in names]
    return out


def _module(monkeypatch, name, forms, form, sd_oracle, precision='f32'):
    """A fresh module of `name` with the transformed weights, created under the form's switches."""
    env, arith = forms[form]
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    z, m = build_model(name, 'fused', device=None)
    sd = m.state_dict()
    sd.update({k: v for k, v in sd_oracle.items() if k in sd})
    m.load_state_dict(sd)
    m.arithmetic = arith
    m.precision = precision
    return m.cuda()


def _err(a, b, scale=1.0):
    return float(np.abs(a - b).max() * scale)


def _check(monkeypatch, name, forms, form, tr, pose):
    import warnings
    r = lr.run(name, tr)
    m = _module(monkeypatch, name, forms, form, r.sd)
    arith = forms[form][1]
    x = r.x.cuda()
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)                      # a heal (RuntimeWarning) would swap the form under test
        v, p = m(x)
        torch.cuda.synchronize()
        m.device_status()
        v2, p2 = m(x)
        vs, ps = m(x[2:5].contiguous())
        torch.cuda.synchronize()
        m.device_status()
    assert m.arithmetic == arith
    vn, pn = v.cpu().numpy().astype(np.float64), p.cpu().numpy().astype(np.float64)
    ours_v, ours_p = _err(vn, r.v64, 1e3), _err(pn, r.p64)
    site = lr.SITE_OF[tr[0]]
    g = r.ranges[site]
    line = '[softmax-edge] %-5s %-12s %-11s %-14s verts ours %.3e ref %.3e mm | pose3d ours %.3e ref %.3e mm | |l|<=%.1f spread %.1f rowmax [%.1f, %.1f]' % (
        site, name, form, '%s(%g)' % tr, ours_v, r.ref_v, ours_p, r.ref_p, g['absmax'], g['spread'], g['rowmax_min'], g['rowmax_max'])
    if tr[0] in lr.EXACT_SHIFTS:
        base = lr.run(name)
        inv_v, inv_p = _err(vn, base.v64, 1e3), _err(pn, base.p64)
        line += ' | vs the unshifted fp64 oracle: verts %.3e mm pose3d %.3e mm' % (inv_v, inv_p)
    print('\n' + line)
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(p).all())
    assert ours_v <= max(1.5e-3, 2.0 * r.ref_v)
    if pose:
        assert ours_p <= max(1e-3, 2.0 * r.ref_p)
    if tr[0] in lr.EXACT_SHIFTS:
        if pose:
            assert inv_p <= max(1e-3, 2.0 * r.ref_p)
        assert inv_v <= max(1.5e-3, 2.0 * r.ref_v)
    assert torch.equal(v, v2) and torch.equal(p, p2)
    assert torch.equal(vs, v[2:5]) and torch.equal(ps, p[2:5])


@pytest.mark.parametrize('name,form,tr', _cases(ENC_FORMS, ENC_TRANSFORMS, both=('gat8',)))
def test_encoder_softmax(monkeypatch, name, form, tr):
    _check(monkeypatch, name, ENC_FORMS, form, tr, pose=True)


@pytest.mark.parametrize('name,form,tr', _cases(MDR_FORMS, MDR_TRANSFORMS))
def test_mdr_attention_softmax(monkeypatch, name, form, tr):
    _check(monkeypatch, name, MDR_FORMS, form, tr, pose=False)


@pytest.mark.parametrize('name,form,tr', _cases(HEAD_FORMS, HEAD_TRANSFORMS, both=('*',)))
def test_head_mix_softmax(monkeypatch, name, form, tr):
    _check(monkeypatch, name, HEAD_FORMS, form, tr, pose=False)


@pytest.mark.parametrize('g', [3, 8])
@pytest.mark.parametrize('fam,name', [('enc_gain', H), ('cross_gain', C), ('head_gain', H)])
def test_config3_under_sharp_softmaxes(monkeypatch, fam, name, g):
    """gator_forward_bf16 on its default form: either the weights stay in the one-plane mode and meet its bar, or the guard took the
    context out of the mode (c3_state) and the bar is met there -- sharp attention costs speed, never millimetres."""
    r = lr.run(name, (fam, g))
    m = _module(monkeypatch, name, {'c3': ({}, 'default')}, 'c3', r.sd, precision='bf16')
    x = r.x.cuda()
    v, p = m(x)
    torch.cuda.synchronize()
    m.device_status()
    assert m.arithmetic == 'default'
    state, bound = m.c3_state()
    e = np.abs(v.cpu().numpy().astype(np.float64) - r.v64) * 1e3
    rms = float(np.sqrt((e ** 2).mean()))
    site = r.ranges[lr.SITE_OF[fam]]
    print('\n[softmax-edge] c3    %-12s %-11s %-14s bound %.0f -> %s | verts max %.3f mm rms %.4f mm | spread %.1f'
          % (name, 'config 3', '%s(%g)' % (fam, g), bound, 'one plane' if state else 'two planes', e.max(), rms, site['spread']))
    assert bool(torch.isfinite(v).all())
    assert (not state) or bound <= 1024.0
    assert e.max() < 1.0 and rms < 0.2
    v2, _ = m(x)
    vs, _ = m(x[2:5].contiguous())
    assert torch.equal(v, v2) and torch.equal(vs, v[2:5])
