"""The vertex regressor's references (tests/upsample_refs.py) checked on the CPU: the GPU tests are only as good as these."""
import math

import numpy as np
import torch

from tests import upsample_refs as ur


def test_matmul_form_equals_conv1d():
    g = torch.Generator().manual_seed(1)
    vc = torch.randn(7, ur.V, 3, generator=g, dtype=torch.float64)
    w = torch.randn(97, ur.V, 3, generator=g, dtype=torch.float64)
    bias = torch.randn(97, generator=g, dtype=torch.float64)
    tpl = torch.randn(97, 3, generator=g, dtype=torch.float64)
    want = torch.nn.functional.conv1d(vc, w, bias, padding=1) + tpl[None]
    ref, s_aw, s = ur.reference(vc.numpy(), w.numpy(), bias.numpy(), tpl.numpy())
    scale = float(s.max())
    assert float((ref - want).abs().max()) <= 64 * np.finfo(np.float64).eps * scale
    # S_aw is the same sum over magnitudes, S adds |bias| + |tpl|
    want_aw = torch.nn.functional.conv1d(vc.abs(), w.abs(), None, padding=1)
    assert float((s_aw - want_aw).abs().max()) <= 64 * np.finfo(np.float64).eps * scale
    assert torch.equal(s, s_aw + bias.abs()[None, :, None] + tpl.abs()[None])
    assert bool((ref.abs() <= s * (1 + 1e-12)).all())
    # the float32 evaluation is the same function
    r32 = ur.reference32(vc.numpy(), w.numpy(), bias.numpy(), tpl.numpy())
    ref_r, _, s_r = ur.reference(vc.float().double().numpy(), w.float().double().numpy(), bias.float().double().numpy(), tpl.float().double().numpy())
    e32 = ur.measure_e32(r32, ref_r, s_r)
    assert 0 < e32 < 16 * ur.EPS32


def _bit_patterns(n, seed):
    """float32 values of every exponent, subnormals, zeros and infinities included; no NaN."""
    rs = np.random.RandomState(seed)
    x = rs.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    x = x[~np.isnan(x)]
    edge = np.array([0.0, -0.0, np.inf, -np.inf, 1.0, 1.00390625, 1.01171875, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 3.3895314e38, 1e-45, 1.1754944e-38],
                    np.float32)          # ties (both parities), the largest bf16 and a value that rounds up to infinity, subnormals
    return np.concatenate([x, edge, rs.randn(20000).astype(np.float32)])


def test_bf16_emulation_is_torch_bfloat16_bit_for_bit():
    x = _bit_patterns(100000, 3)
    assert x.size >= 100000
    got = ur.bf16_rne(x)
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).to(torch.float32).numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.isnan(ur.bf16_rne(np.array([np.nan], np.float32))[0])


def test_fp16_split_is_exact_and_22_bits():
    rs = np.random.RandomState(4)
    # every binade below 4094, down to where both planes are subnormal, and the coordinate-sized values the regressor sees
    x = np.concatenate([rs.randn(40000) * 0.3, rs.randn(20000) * 2.0 ** rs.randint(-30, 12, 20000), rs.uniform(-4094, 4094, 20000),
                        [4093.999, -4093.999, 0.0, 2.0 ** -28, 2.0 ** -29, 1.0, 255.9375]]).astype(np.float32)
    x = x[np.abs(x) < 4094]
    h, l = ur.f16_split(x, ur.ACT_SHIFT)
    assert np.isfinite(h).all() and np.isfinite(l).all()
    s32 = h + l                                          # float32 addition
    s64 = h.astype(np.float64) + l.astype(np.float64)
    assert np.array_equal(s32.astype(np.float64), s64)   # h + l is exact in float32
    sx = x.astype(np.float64) * 16.0
    assert (np.abs(sx - s64) <= 2.0 ** -23 * np.abs(sx) + 2.0 ** -25).all()
    assert np.array_equal(ur.f16_two_plane(x, ur.ACT_SHIFT), s64 / 16.0)
    # the subnormal term matters: at coordinate sizes a good share of the lo planes is subnormal, and some miss the relative term alone
    coord = (rs.randn(100000) * 0.3).astype(np.float32)
    hc, lc = ur.f16_split(coord, ur.ACT_SHIFT)
    sub = (np.abs(lc) < 2.0 ** -14) & (lc != 0)
    assert 0.1 < sub.mean() < 0.6
    # one plane: the hi plane alone, 11 bits
    w = (rs.randn(1000) * 0.005).astype(np.float32)
    sh = ur.weight_shift(np.abs(w).max())
    one = ur.f16_one_plane(w, sh)
    assert (np.abs(one - w.astype(np.float64)) <= 2.0 ** -11 * np.abs(w) + 2.0 ** -25 * 2.0 ** -sh).all()


def test_weight_shift_formula():
    want = {2.0 ** -40: 53, 2.0 ** -30: 43, 0.2: 16, 2.0 ** 13: 0, 2.0 ** 14: -1, 2.0 ** 31: -18, 0.0: 0, math.inf: 0, math.nan: 0,
            # the clamps: they only keep 2^shift and the epilogue's 2^-(shift + 4) normal floats
            2.0 ** -149: 118, 2.0 ** -110: 118, 2.0 ** -103: 116, float(np.finfo(np.float32).max): -114}
    for wmax, sh in want.items():
        assert ur.weight_shift(wmax) == sh, (wmax, sh)
    for wmax in (2.0 ** -40, 2.0 ** -30, 0.2, 2.0 ** 13, 2.0 ** 14, 2.0 ** 31, 0.029):
        scaled = wmax * 2.0 ** ur.weight_shift(wmax)
        assert 2.0 ** 13 <= scaled < 2.0 ** 14           # "wmax * 2^(14 - e) in [2^13, 2^14)"
    for sh in (ur.W_SHIFT_MIN, ur.W_SHIFT_MAX):
        for e in (sh, -(sh + ur.ACT_SHIFT)):
            assert -126 <= e <= 127


def test_round_operands_and_onehot_tables():
    rs = np.random.RandomState(6)
    vc = (rs.randn(2, ur.V, 3) * 0.3).astype(np.float32)
    w = (rs.randn(5, ur.V, 3) * 0.005).astype(np.float32)
    for form in ('fp32', 'basic', 'x3'):
        a, b = ur.round_operands(form, vc, w)
        assert np.array_equal(a, vc.astype(np.float64)) and np.array_equal(b, w.astype(np.float64))
    a, b = ur.round_operands('bf16', vc, w)
    assert (np.abs(a - vc) <= 2.0 ** -8 * np.abs(vc)).all() and (np.abs(b - w) <= 2.0 ** -8 * np.abs(w)).all()
    a2, b2 = ur.round_operands('x2', vc, w)
    a1, b1 = ur.round_operands('x2w1', vc, w)
    assert np.array_equal(a1, a2) and not np.array_equal(b1, b2)
    sh = ur.weight_shift(np.abs(w).max())
    assert (np.abs(b2 - w) <= 2.0 ** -23 * np.abs(w) + 2.0 ** -25 * 2.0 ** -sh).all()
    # the one-hot batch addresses every (coarse vertex, input position) once
    oh = ur.onehot_batch()
    assert oh.shape == (1294, ur.V, 3) and oh.sum() == 1293 and (oh.reshape(1294, -1).sum(1)[:-1] == 1).all() and oh[-1].sum() == 0
    wfull = (rs.randn(ur.NV, ur.V, 3) * 0.005).astype(np.float32)
    bias = rs.randn(ur.NV).astype(np.float32) * 0.02
    tpl = rs.randn(ur.NV, 3).astype(np.float32) * 0.3
    exp, wp, valid = ur.onehot_expected(wfull, bias, tpl)
    want = torch.nn.functional.conv1d(torch.from_numpy(oh[:60]).double(), torch.from_numpy(wfull).double(), None, padding=1).numpy()
    assert np.array_equal(wp[:60], want) and not wp[~np.broadcast_to(valid, wp.shape)].any()
    assert valid.sum() == 7 * ur.V                         # seven (position, output) pairs per coarse vertex; two fall on the padding
    assert np.array_equal(exp[:60], ((want.astype(np.float32) + bias[None, :, None]) + tpl[None]))


def test_joint_regressor_families():
    regs = ur.joint_regressors()
    assert set(regs) == {'vertex0', 'vertex6889', 'tail_block', 'crowded_block', 'empty_joint', 'one_joint', 'cancelling'}
    assert np.count_nonzero(regs['tail_block'][:, ur.NV - 10:]) == 30 and np.count_nonzero(regs['tail_block']) == 30
    assert np.count_nonzero(regs['crowded_block']) == 256
    assert not regs['empty_joint'][2].any() and regs['one_joint'].shape[0] == 1
    d = regs['cancelling']
    assert np.count_nonzero(d) == 3000 and (d > 0).sum() == 1500
    r, c, v, tot = ur.shuffled_with_duplicates(d)
    assert r.size == 3600 and len(set(zip(r.tolist(), c.tolist()))) == 3000
    assert (np.diff(r.astype(np.int64) * ur.NV + c) < 0).any()          # not sorted
    assert not np.array_equal(tot, d.astype(np.float64))                # the duplicates change the totals
    verts = torch.randn(2, ur.NV, 3, generator=torch.Generator().manual_seed(2))
    ref, mag = ur.joints_reference((r, c, v, d.shape[0]), verts)
    want = torch.einsum('jv,bvc->bjc', torch.from_numpy(tot), verts.double())
    assert float((ref - want).abs().max()) <= 1e-12 * float(mag.max())
