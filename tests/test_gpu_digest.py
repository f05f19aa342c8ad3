"""Bit-identity of the fp32 forward against recorded digests (tests/golden/fp32_digests.json, written by tools/ab_digest.py on a GPU box).
Round 4 made several changes that were meant to be schedules only and checked them by hand with tools/ab_digest.py; this is that check
as a test: per-sample kernel and sample-tiled kernel, persistent and four-launch MDR forms (B = 5 / 256 / 700), both golden variants.
A change that is meant to move bits re-records the file (and re-runs the error budget); any other change must leave it green.
tests/golden/mdr_form_digests.json does the same for the MDR kernels' other forms (tools/ab_digest.py: form_digests): exact split, fp32-input
MFMA, config 3 and the whole-head kernels, four-launch and persistent, at B = 11.
tests/golden/caller_side_digests.json does it for the kernels around the forward (tools/ab_digest.py: caller_digests).
tests/golden/encoder_form_digests.json does it for every form of the GAT encoder kernels (tools/ab_digest.py: encoder_digests).
tests/golden/regressor_form_digests.json does it for every form of the vertex regressor (tools/ab_digest.py: regressor_digests)."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fp32_digests.json')
FORMS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mdr_form_digests.json')
CALLER_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'caller_side_digests.json')


def test_fp32_forward_digests_match_the_recorded_build():
    if not os.path.exists(PATH):
        pytest.skip('no recorded digests (tools/ab_digest.py --write tests/golden/fp32_digests.json on a GPU box)')
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tools.ab_digest import digests
    want = json.load(open(PATH))['digests']
    got = digests()
    bad = {k: (got.get(k), h) for k, h in want.items() if got.get(k) != h}
    assert not bad, 'outputs moved bits against tests/golden/fp32_digests.json: %s' % bad
ENCODER_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'encoder_form_digests.json')
ENCODER_FORMS = ['default', 'tail0', 'lobyte0', 'h4_0', 'gat8_0', 'x3_0', 'bf16', 'bf16_tail0', 'tiled', 'tiled_h4_0', 'tiled_bf16', 'gat', 'gat_x3_0',
                 'taps', 'tiled_taps']


@pytest.mark.parametrize('form', ['default', 'x3_1', 'x3_0', 'bf16', 'head_partials0'])
def test_mdr_form_digests_match_the_recorded_build(form):
    """Every MDR form bit for bit: GATOR_MDR_PERSIST = 0 and 1, both golden variants, the whole forward and the MDR entry point on a random
    pose_combine (k_mdr_joint, both K/V tile forms), B = 11; head_partials0 also at B = 513, where the plan picks the rolled k_mdr_head."""
    if not os.path.exists(FORMS_PATH):
        pytest.skip('no recorded digests (tools/ab_digest.py --forms --write tests/golden/mdr_form_digests.json on a GPU box)')
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tools.ab_digest import form_digests
    want = {k: h for k, h in json.load(open(FORMS_PATH))['digests'].items() if k.startswith(form + ' ')}
    got = form_digests([form])
    assert len(want) >= 8 and set(got) == set(want)
    bad = {k: (got.get(k), h) for k, h in want.items() if got.get(k) != h}
    assert not bad, 'outputs moved bits against tests/golden/mdr_form_digests.json: %s' % bad


@pytest.mark.parametrize('form', ENCODER_FORMS)
def test_encoder_form_digests_match_the_recorded_build(form):
    """Every form of the GAT encoder bit for bit against the build recorded before its kernels' shared steps were stated once: the eight
    per-sample forms at B = 3 and 65 (all eleven k_gat8 instantiations, k_gat<true|false, false>, both L2 warm-ups and the tail warm-up),
    the three sample-tiled forms at B = 8, the stand-alone encoder entry (k_gat<., true>) and the block taps of both encoders; both golden
    variants (tools/ab_digest.py: encoder_digests)."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tools.ab_digest import ENCODER_FORMS as forms, encoder_digests
    assert sorted(forms) == sorted(ENCODER_FORMS)
    want = {k: h for k, h in json.load(open(ENCODER_PATH))['digests'].items() if k.startswith(form + ' ')}
    got = encoder_digests([form])
    assert len(want) >= 2 and set(got) == set(want)
    bad = {k: (got.get(k), h) for k, h in want.items() if got.get(k) != h}
    assert not bad, 'outputs moved bits against tests/golden/encoder_form_digests.json: %s' % bad


def test_caller_side_digests_match_the_recorded_build():
    """The kernels around the forward (preprocess, camera crop, Procrustes / joint / mesh / sequence errors, camera targets) bit for bit
    against the build that was recorded before their shared steps moved into csrc/joints2d.h and csrc/procrustes.h: small seeded shapes
    at the 64-lane block edge, the 32-joint column limit, a rejected box, every rotation and flip, 3 and 32 fitted points, videos
    shorter than a triple (tools/ab_digest.py: caller_digests)."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tools.ab_digest import caller_digests
    want = json.load(open(CALLER_PATH))['digests']
    got = caller_digests()
    assert len(want) >= 100 and set(got) == set(want)
    bad = {k: (got.get(k), h) for k, h in want.items() if got.get(k) != h}
    assert not bad, 'outputs moved bits against tests/golden/caller_side_digests.json: %s' % bad


HANDLES_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'handle_digests.json')


@pytest.mark.parametrize('lib', ['renderer', 'draw2d', 'smpl', 'fit', 'backward'])
def test_handle_digests_match_the_recorded_build(lib):
    """The auxiliary libraries behind a handle bit for bit against the build recorded before their host scaffolding (growth rule, staged
    table, handle checks) was stated once in csrc/handle.h: small seeded calls of every entry point, and per handle a small call, the
    largest and the small one again, whose digests must not depend on the handle's history and whose workspace() tuples (bytes and
    allocation counts, the SMPL capacity) are the recorded ones (tools/ab_digest.py: handle_digests).  Every 'backward' key was
    recorded before the SMPL kernels' shared device steps moved into csrc/smpl_steps.h: gator_smpl_backward_f32 at B = 1 and 33 on three
    vertex tiles, every upstream subset, centring, an output subset, and 24 influences per vertex (the looped MI_T = 0 kernels) in
    both directions; the layer's dense forward is in this group so that the earlier groups keep their key sets."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tools.ab_digest import HANDLE_LIBS, handle_digests
    assert lib in HANDLE_LIBS
    want = {k: h for k, h in json.load(open(HANDLES_PATH))['digests'].items() if k.startswith(lib + ' ')}
    got = handle_digests([lib])
    assert len(want) >= 5 and set(got) == set(want)
    bad = {k: (got.get(k), h) for k, h in want.items() if got.get(k) != h}
    assert not bad, 'outputs or workspaces moved against tests/golden/handle_digests.json: %s' % bad


REGRESSOR_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'regressor_form_digests.json')
REGRESSOR_FORMS = ['fp32', 'x3', 'x2', 'bf16', 'c3_default', 'c3_w1_0', 'c3_bf16']


@pytest.mark.parametrize('form', REGRESSOR_FORMS)
def test_regressor_form_digests_match_the_recorded_build(form):
    """Every form of the vertex regressor bit for bit against the build recorded before its operand slots, packers and epilogue were
    stated once in csrc/upsample_common.h: the stage entry with its pack kernels (fp32-input, three bf16 planes, two fp16 planes at
    B = 1, 33, 129, 257, fp32 also at its one-tile -> two-tile switch 224 / 225, bf16 at 1, 33, 65), the head-written operand in a whole
    forward, the joint epilogue with and without the vertex store, config 3's three regressors, weights times 2^12 (another pack-time
    shift), and one context through B = 33, 257, 1 (tools/ab_digest.py: regressor_digests)."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tools.ab_digest import REGRESSOR_FORMS as forms, regressor_digests
    assert sorted(forms) == sorted(REGRESSOR_FORMS)
    want = {k: h for k, h in json.load(open(REGRESSOR_PATH))['digests'].items() if k.startswith(form + ' ')}
    got = regressor_digests([form])
    assert len(want) >= 1 and set(got) == set(want)
    bad = {k: (got.get(k), h) for k, h in want.items() if got.get(k) != h}
    assert not bad, 'outputs moved bits against tests/golden/regressor_form_digests.json: %s' % bad


def test_byte_lo_weight_stream_equals_the_three_plane_stream_bit_for_bit(monkeypatch):
    """k_gat8 streams its weights with the lo plane as one byte per weight by default (gat8_forms.h: H3B); GATOR_GAT8_LOBYTE=0 keeps
    the three fp16 planes.  The switch is read per context, so both forms run in this process; the digests (which cover B = 5 / 256 / 700
    on k_gat8) must be equal.  (Which kernel ran is visible in profiles/r05_kernel_stats_*: k_gat8<true, 10, false, true>.)"""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tools.ab_digest import digests
    monkeypatch.setenv('GATOR_GAT8_TAIL', '0')      # (the fused tail exists on the byte-lo stream's kernel only: both forms keep the two tail launches)
    out = {}
    for lb in ('1', '0'):
        monkeypatch.setenv('GATOR_GAT8_LOBYTE', lb)
        out[lb] = digests()                          # fresh models: their contexts read the switches
        assert len(out[lb]) >= 8
    assert out['1'] == out['0']
