"""Parity hardening (round-1 verdict): a scale-free criterion at two output gains against goldens made by the REAL reference,
the per-block residual-stream taps, the Procrustes kernel against the reference's own rigid_align, the first bf16 call in
sub-batch mode, and config 3 (bf16 vertex regressor) at its full size B=2048, J=19."""
import numpy as np
import pytest
import torch

from gator_amd import eval as geval
from gator_amd import synthetic
from tests.helpers import build_model, load_golden, oracle_setup

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('fixture,gain', [('scale_gain02', 0.2), ('scale_gain10', 1.0)])
@pytest.mark.parametrize('x3', ['default', '1', '0'])
def test_scale_free_parity(fixture, gain, x3, monkeypatch):
    """max|ours - ref fp64| <= 1.5 x max|ref fp32 - ref fp64| on the same weights and inputs (B=64, fixed 512-vertex subset),
    at the human-scale gain 0.2 AND at gain 1.0 (5 m meshes, where an absolute 1e-3 mm bound is unmeetable by the reference
    itself): the error follows the reference's own fp32 noise, whatever the magnitude.  Shipped configuration, all-bf16x3, all-fp32-MFMA."""
    for k in ('GATOR_GAT_X3', 'GATOR_MDR_X3', 'GATOR_UPSAMPLE_X3'):      # 'default': the shipped configuration (no switch set)
        if x3 == 'default':
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, x3)
    if x3 == 'default':
        monkeypatch.delenv('GATOR_GAT8_H4', raising=False)
        monkeypatch.delenv('GATOR_GAT_TILED_H4', raising=False)
    else:
        monkeypatch.setenv('GATOR_GAT8_H4', '0')             # '1': no rounded operand anywhere
        monkeypatch.setenv('GATOR_GAT_TILED_H4', '0')
    z = load_golden(fixture)
    zz, m = build_model(str(z['variant']), 'fused', upsample_gain=gain)
    sub = torch.from_numpy(z['vertex_subset'].astype(np.int64)).cuda()
    verts, pose3d = m(torch.from_numpy(z['pose2d']).cuda())
    ours = np.abs(verts[:, sub].cpu().numpy().astype(np.float64) - z['verts_f64']) * 1e3
    ref = np.abs(z['ref32_minus_f64'].astype(np.float64)) * 1e3
    print('\n[%s x3=%s] ours vs ref-fp64: max %.3e rms %.3e mm ; ref-fp32 vs ref-fp64: max %.3e rms %.3e mm ; ratio %.2f'
          % (fixture, x3, ours.max(), np.sqrt((ours ** 2).mean()), ref.max(), np.sqrt((ref ** 2).mean()), ours.max() / ref.max()))
    assert ours.max() <= 1.5 * ref.max()
    assert np.sqrt((ours ** 2).mean()) <= 1.5 * np.sqrt((ref ** 2).mean())
    assert np.abs(pose3d.cpu().numpy() - z['pose3d_f64']).max() <= 1e-3
    if gain == 0.2:
        assert ours.max() <= 1e-3            # the north star's absolute bound at human scale


@pytest.mark.parametrize('name', ['h36m17_bn', 'coco19_alpha'])
def test_block_taps_match_reference(name):
    """Residual stream after GATBlock 0 and 5 (lib/models/GAT.py:145-147) against the reference's recorded activations."""
    z, m = build_model(name, 'fused')
    B, J = z['pose2d'].shape[:2]
    x = torch.from_numpy(z['pose2d']).cuda()
    v0, _ = m(x)
    m.enable_block_taps(True)
    v1, _ = m(x)
    assert torch.equal(v0, v1)                                        # the tap stores change nothing
    for blk in (0, 5):
        t = m.get_tap('gat_block%d' % blk, (B, J, 128)).cpu().numpy().astype(np.float64)
        ref = z['gat_block%d' % blk].astype(np.float64)
        err = np.abs(t - ref).max()
        print('[%s] gat_block%d max|d| %.2e (scale %.2f)' % (name, blk, err, np.abs(ref).max()))
        assert err <= 4e-6 * max(1.0, np.abs(ref).max())
    m.enable_block_taps(False)
    m(x)
    with pytest.raises(RuntimeError):
        m.get_tap('gat_block0', (B, J, 128))


def test_rigid_align_kernel_matches_reference_golden():
    """gator_rigid_align_f32 against lib/coord_utils.py:127-149 itself (tests/golden/rigid_align.npz: random, mirrored,
    near-coplanar, scaled); inputs are float32 on the device as in the eval loop."""
    z = load_golden('rigid_align')
    a, b = torch.from_numpy(z['A'].astype(np.float32)).cuda(), torch.from_numpy(z['B'].astype(np.float32)).cuda()
    out = geval.rigid_align(a, b).cpu().numpy().astype(np.float64)
    ref = z['aligned_from_f32']
    scale = np.abs(ref).max()
    print('\nrigid_align vs reference: max|d| %.3e mm (scale %.1f mm)' % (np.abs(out - ref).max(), scale))
    assert np.abs(out - ref).max() <= 2e-6 * scale                   # fp32 output rounding of an fp64 solve
    pa = float(geval.pa_mpjpe(a, b, eval_joints=list(range(14))))
    assert abs(pa - float(z['pa_mpjpe'])) <= 1e-4 * float(z['pa_mpjpe'])


def test_first_bf16_call_in_subbatch_mode_is_bitwise():
    """The FIRST gator_forward_bf16 on a fresh context in sub-batch-streams mode (the bf16 weight pack is lazy: the second
    half-batch runs on another stream and must not read the pack before it is complete)."""
    x = torch.from_numpy(synthetic.synthetic_pose2d(192, 19, seed=31)).cuda()
    z, ref_m = build_model('coco19_alpha', 'fused')
    ref_m.precision = 'bf16'
    want_v, want_p = ref_m(x)
    torch.cuda.synchronize()
    for trial in range(3):
        z, m = build_model('coco19_alpha', 'fused')
        m.precision = 'bf16'
        m.subbatch_streams = 2
        got_v, got_p = m(x)                                            # first call on a fresh ctx
        torch.cuda.synchronize()
        assert torch.equal(got_v, want_v) and torch.equal(got_p, want_p), 'trial %d' % trial


def test_bf16_config3_full_size():
    """BASELINE config 3 at its own size: B=2048 COCO 19-joint, 16-bit operand mode (MDR layers on one fp16 activation plane).  The
    fp32 path (parity-tested at this size in test_gpu_fullsize.py) is the anchor here, the oracle checks a 24-sample slice (all 2048
    samples against the oracle: tests/test_gpu_bf16.py); determinism is bitwise, a small batch of the same samples agrees to fp32
    noise on the fp32 path (it runs the other encoder kernel)."""
    from oracle import gator_oracle as go
    B, J = 2048, 19
    z, m = build_model('coco19_alpha', 'fused')
    x = torch.from_numpy(synthetic.synthetic_pose2d(B, J, seed=77)).cuda()
    m.precision = 'bf16'
    vb, pb = m(x)
    vb2, _ = m(x)
    assert torch.equal(vb, vb2)                                        # deterministic
    m.precision = 'f32'
    vf, pf = m(x)
    vs, _ = m(x[1000:1040])                                            # (another encoder kernel below 1024 samples: fp32 noise)
    assert float((vs - vf[1000:1040]).abs().max()) * 1e3 <= 1.5e-3
    assert float((pb - pf).abs().max()) <= 1.0                         # pose3d in mm: the 16-bit mode's encoder against the fp32 path's
    d = (vb - vf).abs() * 1e3
    rms = float(torch.sqrt((d.double() ** 2).mean()))
    print('\n[bf16 B=2048 J=19] vs fp32 path: max %.3f mm rms %.3f mm' % (float(d.max()), rms))
    assert float(d.max()) < 1.0 and rms < 0.2
    jr = synthetic.load_j_regressors()['h36m']
    reg = geval.JointRegressor(jr, 'cuda')
    jb, jf = reg(vb) * 1000.0, reg(vf) * 1000.0
    assert float((jb - jf).abs().max()) < 1.0
    gt = jf + torch.from_numpy(np.random.RandomState(0).randn(B, 17, 3).astype(np.float32) * 30.0).cuda()
    assert abs(float(geval.mpjpe(jb, gt)) - float(geval.mpjpe(jf, gt))) < 0.05
    zz, c, sd = oracle_setup('coco19_alpha')
    ref, _ = go.gator_forward(sd, c, x[500:524].cpu(), torch.float64)
    e = np.abs(vb[500:524].cpu().numpy().astype(np.float64) - ref.numpy()) * 1e3
    assert e.max() < 1.0 and np.sqrt((e ** 2).mean()) < 0.2


@pytest.mark.parametrize('key,gain', [('pose2mesh.encoder_1.norm2.weight', 3e4), ('pose_lifter.blocks.2.norm2.weight', 3e4),
                                       ('pose2mesh.bias_conv1d.weight', 1e6)])
def test_operand_range_violation_is_loud(key, gain):
    """The default arithmetic carries activations as fp16 planes of 16 x value: |value| must stay below 4 094 (include/gator_hip.h).
    Weights scaled so that an MLP's input and hidden (MDR or GAT encoder) resp. the coarse vertices leave that range: the forward must not
    return silently wrong numbers -- its vertices are NaN and the NEXT call on the ctx (or device_status) raises GATOR_EDEVICE;
    after the report the ctx keeps working.  (The MLP cases scale the norm in front of fc1 -- to the network that is fc1.weight x gain --
    because scaling fc1.weight itself spreads the three-plane weight set by 3e4: such a set is no longer packed, the ctx runs the exact
    form for it and the range is never tripped; tests/test_gpu_rescaled_weights.py::test_one_grid_scaled_up_is_demoted_and_right_at_once.)"""
    z, m = build_model('h36m17_bn', 'fused', device=None)
    sd = m.state_dict()
    good = sd[key].clone()
    sd[key] = good * gain
    m.load_state_dict(sd)
    m.on_device_status = 'raise'                            # the C ABI's behaviour (the module's default heals: next test)
    m = m.cuda()
    x = torch.from_numpy(synthetic.synthetic_pose2d(16, 17, seed=5)).cuda()
    v, p = m(x)
    torch.cuda.synchronize()
    assert not torch.isfinite(v).all()                     # loud in the data ...
    with pytest.raises(RuntimeError, match='non-finite|out-of-range'):
        m.device_status()                                   # ... and in the API
    m.device_status()                                       # reported once, then clear
    v2, _ = m(x)                                            # the ctx still accepts work
    torch.cuda.synchronize()
    from gator_amd._lib import DeferredDeviceStatus
    with pytest.raises(DeferredDeviceStatus) as ei:
        m(x)                                                # the forward after a bad one reports it without an explicit query ...
    assert ei.value.code == -8 and ei.value.reason == 2 and ei.value.outputs is not None      # ... as GATOR_EDEVICE_DEFERRED, its own outputs attached


@pytest.mark.parametrize('key,gain', [('pose2mesh.encoder_1.norm2.weight', 3e4), ('pose_lifter.blocks.2.norm2.weight', 3e4)])
def test_operand_range_violation_heals_by_itself(key, gain):
    """Round-5 review item 4: the reference's forward never raises (lib/models/GATOR.py:16-22), so a drop-in must not either.  The weights
    that break the default arithmetic's operand range, through the DEFAULT module: the first forward's vertices are NaN (nothing on the
    host can know in time), the second one notices the report, switches the module to the exact-split arithmetic, re-runs its batch
    there and returns the reference's numbers (criterion of test_exact_split_arithmetic_has_no_operand_range) -- with a warning, no
    exception, and for every later call."""
    import warnings
    from oracle import gator_oracle as go
    z, m = build_model('h36m17_bn', 'fused', device=None)
    zz, c, sd_o = oracle_setup('h36m17_bn')
    sd = m.state_dict()
    sd[key] = sd[key] * gain
    sd_o[key] = sd_o[key] * gain
    m.load_state_dict(sd)
    m = m.cuda()
    assert m.arithmetic == 'default' and m.on_device_status == 'heal'
    x = torch.from_numpy(synthetic.synthetic_pose2d(16, 17, seed=5))
    v0, _ = m(x.cuda())
    torch.cuda.synchronize()
    assert not torch.isfinite(v0).all()                    # the one forward the device could not warn about in time
    out = (torch.empty(16, 6890, 3, device='cuda'), torch.empty(16, 17, 3, device='cuda'))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        v, p = m(x.cuda(), out=out)                         # heals: same output tensors, exact arithmetic
        torch.cuda.synchronize()
    assert any('exact' in str(i.message) for i in w) and m.arithmetic == 'exact'
    assert v.data_ptr() == out[0].data_ptr() and torch.isfinite(v).all() and torch.isfinite(p).all()
    r64, _ = go.gator_forward(sd_o, c, x, torch.float64)
    r32, _ = go.gator_forward(sd_o, c, x, torch.float32)
    scale = float(r64.abs().max())
    ours = float(np.abs(v.cpu().numpy().astype(np.float64) - r64.numpy()).max()) / scale
    ref = float(np.abs(r32.numpy().astype(np.float64) - r64.numpy()).max()) / scale
    print('\n[%s x %g, healed] |ours - fp64| / max|v| = %.2e, reference arithmetic %.2e' % (key, gain, ours, ref))
    assert ours <= max(2e-6, 2.0 * ref)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        v3, _ = m(x.cuda())                                 # and stays healed, silently
        torch.cuda.synchronize()
    assert not w and torch.equal(v3, v)
    m.device_status()


@pytest.mark.parametrize('key,gain', [('pose2mesh.encoder_1.mlp.fc1.weight', 3e4), ('pose_lifter.blocks.2.mlp.fc1.weight', 3e4)])
def test_exact_split_arithmetic_has_no_operand_range(key, gain):
    """gator_config.arithmetic = GATOR_ARITH_EXACT_SPLIT (include/gator_hip.h; `model.arithmetic = 'exact'`): every product on the exact
    three-way bf16 split, so the weights that break the default's operand range above (an MLP hidden beyond 4 094) give finite
    vertices, a clean device status, and the reference's numbers -- compared with the fp64 oracle on the same scaled weights,
    relative to the reference arithmetic's own error (the oracle in fp32)."""
    from oracle import gator_oracle as go
    z, m = build_model('h36m17_bn', 'fused', device=None)
    zz, c, sd_o = oracle_setup('h36m17_bn')
    sd = m.state_dict()
    sd[key] = sd[key] * gain
    sd_o[key] = sd_o[key] * gain
    m.load_state_dict(sd)
    m.arithmetic = 'exact'
    m = m.cuda()
    x = torch.from_numpy(synthetic.synthetic_pose2d(16, 17, seed=5))
    v, p = m(x.cuda())
    torch.cuda.synchronize()
    assert torch.isfinite(v).all() and torch.isfinite(p).all()
    m.device_status()
    r64, _ = go.gator_forward(sd_o, c, x, torch.float64)
    r32, _ = go.gator_forward(sd_o, c, x, torch.float32)
    scale = float(r64.abs().max())
    ours = float(np.abs(v.cpu().numpy().astype(np.float64) - r64.numpy()).max()) / scale
    ref = float(np.abs(r32.numpy().astype(np.float64) - r64.numpy()).max()) / scale
    print('\n[%s x %g, exact split] |ours - fp64| / max|v| = %.2e, reference arithmetic %.2e' % (key, gain, ours, ref))
    assert ours <= max(2e-6, 2.0 * ref)


def test_device_status_is_clean_after_normal_forwards():
    z, m = build_model('coco19_alpha', 'fused')
    for B in (1, 33, 300):
        m(torch.from_numpy(synthetic.synthetic_pose2d(B, 19, seed=B)).cuda())
    m.device_status()


@pytest.mark.parametrize('gain', [3.0, 8.0])
def test_attention_rescale_paths_under_large_logits(gain):
    """The 431-key self-attention forms its probabilities against a running reference and rescales lazily; with the shipped synthetic
    weights the rescale branches (and, since round 4, the long way of a tile whose probabilities would leave the fp16 range) almost
    never run.  Here the q / k projections of all three layers are scaled so that the logits grow 9 x / 64 x: every tile sequence
    rescales, many tiles take the long way.  Criterion: the error against the fp64 oracle stays within twice the reference
    arithmetic's own error (the oracle in fp32) on the same weights, results are deterministic and batch independent."""
    from oracle import gator_oracle as go
    z, m = build_model('h36m17_bn', 'fused', device=None)
    zz, c, sd_o = oracle_setup('h36m17_bn')
    sd = m.state_dict()
    for sfx in ('', '_1', '_2'):
        for n in (0, 1):
            for leaf in ('weight', 'bias'):
                k = 'pose2mesh.selfatt%s.linears.%d.%s' % (sfx, n, leaf)
                sd[k] = sd[k] * gain
                sd_o[k] = sd_o[k] * gain
    m.load_state_dict(sd)
    m = m.cuda()
    x = torch.from_numpy(synthetic.synthetic_pose2d(24, 17, seed=9))
    v, p = m(x.cuda())
    torch.cuda.synchronize()
    m.device_status()
    r64, _ = go.gator_forward(sd_o, c, x, torch.float64)
    r32, _ = go.gator_forward(sd_o, c, x, torch.float32)
    ours = float(np.abs(v.cpu().numpy().astype(np.float64) - r64.numpy()).max() * 1e3)
    ref = float(np.abs(r32.numpy().astype(np.float64) - r64.numpy()).max() * 1e3)
    print('\n[logit gain %.0f^2] ours vs fp64 %.3e mm, reference arithmetic vs fp64 %.3e mm' % (gain, ours, ref))
    assert ours <= max(1.5e-3, 2.0 * ref)
    v2, _ = m(x.cuda())
    vs, _ = m(x[5:9].cuda())
    assert torch.equal(v, v2) and torch.equal(vs, v[5:9])


@pytest.mark.parametrize('level', [0.95, 1.05])
@pytest.mark.parametrize('form', ['default', 'upsample_x3', 'exact'])
def test_coarse_vertex_range_at_its_edge(form, level, monkeypatch):
    """The two-plane vertex regressor carries 16 x vert431 in fp16 planes: |vert431| < 4 094 (k_mdr_head / k_mdr_head_finish flag the rest).
    A constant added to every bias_conv1d row shifts every coarse vertex by that constant (the softmax mix of MDR.py:161-166 sums to 1),
    driving max|vert431| to 0.95 x and 1.05 x the limit.  Below it, and in the forms without the limit (GATOR_UPSAMPLE_X3=1, arithmetic =
    'exact') at both levels: no report, and the scale-free bar of test_scale_free_parity on the whole mesh.  Above it, the default form
    is loud (NaN, then reason 2) and heals to the same bar: there is no window where the answer is silently wrong."""
    import warnings
    from oracle import gator_oracle as go
    monkeypatch.delenv('GATOR_UPSAMPLE_X3', raising=False)
    if form == 'upsample_x3':
        monkeypatch.setenv('GATOR_UPSAMPLE_X3', '1')
    z, m = build_model('h36m17_bn', 'fused', device=None)
    zz, c, sd_o = oracle_setup('h36m17_bn')
    x = torch.from_numpy(synthetic.synthetic_pose2d(16, 17, seed=5))
    taps = {}
    go.gator_forward(sd_o, c, x, torch.float64, taps)
    vc = taps['vert431']
    key = 'pose2mesh.bias_conv1d.bias'
    shift = level * 4094.0 - float(vc.max())
    sd = m.state_dict()
    sd[key] = sd[key] + shift
    sd_o[key] = sd_o[key] + shift
    m.load_state_dict(sd)
    if form == 'exact':
        m.arithmetic = 'exact'
    m = m.cuda()
    taps = {}
    r64, _ = go.gator_forward(sd_o, c, x, torch.float64, taps)
    r32, _ = go.gator_forward(sd_o, c, x, torch.float32)
    top = float(taps['vert431'].abs().max())
    assert abs(top / 4094.0 - level) < 1e-3
    v, p = m(x.cuda())
    torch.cuda.synchronize()
    if form == 'default' and level > 1.0:
        assert not torch.isfinite(v).all()                  # loud in the data ...
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            v, p = m(x.cuda())                              # ... the next call carries reason 2 and heals
            torch.cuda.synchronize()
        assert m.arithmetic == 'exact' and any('exact' in str(i.message) for i in w)
    m.device_status()
    ours = np.abs(v.cpu().numpy().astype(np.float64) - r64.numpy())
    ref = np.abs(r32.numpy().astype(np.float64) - r64.numpy())
    print('\n[%s, max|vert431| = %.3f x 4094] ours vs fp64: max %.3e m rms %.3e m ; ref fp32 vs fp64: max %.3e m rms %.3e m'
          % (form, top / 4094.0, ours.max(), np.sqrt((ours ** 2).mean()), ref.max(), np.sqrt((ref ** 2).mean())))
    assert ours.max() <= 1.5 * ref.max()
