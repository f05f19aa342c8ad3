"""CPU-only: the rescaling families of tests/rescale_refs.py are exact symmetries of the reference (so the GPU tests that use them
need no tolerance of their own), and what the three-plane weight split does to a set whose grids differ in magnitude."""
import numpy as np
import pytest
import torch

from gator_amd import synthetic
from tests import rescale_refs as rr
from tests.helpers import oracle_setup

_ORACLE = {}


def _oracle(name):
    """(consts, state dict, pose2d, unscaled fp32 outputs) of a variant: computed once, never modified."""
    if name not in _ORACLE:
        from oracle import gator_oracle as go
        z, c, sd = oracle_setup(name)
        x = torch.from_numpy(synthetic.synthetic_pose2d(2, c.J, seed=4242))
        _ORACLE[name] = (c, sd, x, go.gator_forward(sd, c, x, torch.float32))
    return _ORACLE[name]


@pytest.mark.parametrize('k', [-12, 12])
@pytest.mark.parametrize('family', rr.GAT_EXACT + rr.MDR_EXACT + ('all',))
def test_exact_families_leave_the_fp32_oracle_bit_identical(family, k):
    from oracle import gator_oracle as go
    name = 'coco19_alpha' if family.startswith('mdr') else 'h36m17_bn'
    c, sd, x, (v0, p0) = _oracle(name)
    before = {key: t.clone() for key, t in sd.items()}
    sd2 = rr.rescale(sd, family, k)
    changed = [key for key in sd if not torch.equal(sd2[key], sd[key])]
    assert changed                                                         # the family names tensors that exist
    assert all(torch.equal(sd[key], before[key]) for key in sd)           # the input dict is left alone
    v, p = go.gator_forward(sd2, c, x, torch.float32)
    assert torch.equal(v, v0) and torch.equal(p, p0)


def test_near_families_scale_the_mlp_pair_and_nothing_else():
    c, sd, x, _ = _oracle('h36m17_bn')
    for family, keys in (('gat_mlp', 'pose_lifter.blocks.3.mlp.'), ('mdr_mlp', 'pose2mesh.encoder_1.mlp.')):
        sd2 = rr.rescale(sd, family, 8)
        assert torch.equal(sd2[keys + 'fc1.weight'], sd[keys + 'fc1.weight'] / 256) and torch.equal(sd2[keys + 'fc1.bias'], sd[keys + 'fc1.bias'] / 256)
        assert torch.equal(sd2[keys + 'fc2.weight'], sd[keys + 'fc2.weight'] * 256) and torch.equal(sd2[keys + 'fc2.bias'], sd[keys + 'fc2.bias'])
        assert sum(not torch.equal(sd2[key], sd[key]) for key in sd) == 3 * (6 if family == 'gat_mlp' else 3)


def test_all_alternates_the_sign_with_the_block_index():
    c, sd, x, _ = _oracle('h36m17_bn')
    sd2 = rr.rescale(sd, 'all', 4)
    for i in range(6):
        f = 16.0 if i % 2 == 0 else 1 / 16.0
        key = 'pose_lifter.blocks.%d.' % i
        assert torch.equal(sd2[key + 'gcn.W'], sd[key + 'gcn.W'] * f) and torch.equal(sd2[key + 'gcn.M'], sd[key + 'gcn.M'] / f)
        q = sd[key + 'attn.qkv.weight']
        assert torch.equal(sd2[key + 'attn.qkv.weight'], torch.cat([q[:128] * f, q[128:256] / f, q[256:] * f]))
    assert torch.equal(sd2['pose2mesh.encoder_1.attn.wq.weight'], sd['pose2mesh.encoder_1.attn.wq.weight'] / 16)


def _two_groups(k):
    rs = np.random.RandomState(7)
    big = (rs.randn(16, 1024) / np.sqrt(128.0)).astype(np.float32)
    small = ((rs.randn(16, 1024) / np.sqrt(128.0)) * 2.0 ** -k).astype(np.float32)
    return big, small


@pytest.mark.parametrize('k', [0, 4, 8, 12, 14, 16, 20, 24])
def test_h3_split_of_a_set_with_two_magnitudes(k):
    """One shift for two equal-sized groups of randn / sqrt(128) weights, the second scaled by 2^-k.  The quantity the create-time checks
    used to compare (the split's residual relative to the set's largest weight) never moves, while the small group's own precision
    passes fp32's 2^-24 between k = 12 and k = 14; the per-tile ratio that replaces it separates k <= 4 from k >= 14."""
    big, small = _two_groups(k)
    w = np.concatenate([big, small])
    shift = rr.h3_shift(np.abs(w).max())
    assert 2.0 ** 13 <= np.abs(w).max() * 2.0 ** shift < 2.0 ** 14
    h, m, lo, left = rr.h3_split(w, shift)
    residual = float(left.max()) / (float(np.abs(w).max()) * 2.0 ** shift)
    err = np.abs(rr.h3_value(h, m, lo, shift) - w.astype(np.float64))
    small_rel = float(err[16:].max() / np.sqrt((small.astype(np.float64) ** 2).mean()))
    ratio = rr.h3_min_tile_ratio(w)
    print('\nk=%2d shift=%d residual %.2e  small group: max error / rms %.2e  min tile ratio 2^%.1f' % (k, shift, residual, small_rel, np.log2(ratio)))
    assert residual < 2.0 ** -38                                          # the retired check (> 1e-7) could not fire
    assert float(err.max()) <= 2.0 ** -38 * float(np.abs(w).max())       # what the planes do hold: every weight to 2^-38 of the largest
    if k <= 12:
        assert small_rel < 2.0 ** -24
    if k >= 14:
        assert small_rel > 2.0 ** -24
    if k <= 4:
        assert ratio >= rr.H3_MIN_TILE_RATIO
    if k >= 14:
        assert ratio < rr.H3_MIN_TILE_RATIO


def test_the_restated_threshold_is_the_library_s():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'gator_amd', 'csrc', 'x3_common.h')).read()
    m = re.search(r'constexpr float kH3MinTileRatio = 0x1p(-\d+)f;', src)
    assert m and 2.0 ** int(m.group(1)) == rr.H3_MIN_TILE_RATIO
    assert 'left > 1e-7f' not in ''.join(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'gator_amd', 'csrc', f)).read()
                                         for f in ('fused_api.hip', 'gat_roles.hip', 'gat8_stream.hip'))      # the three checks that could not fire are gone


def test_x2_split_has_an_absolute_floor_below_two_to_the_minus_seven():
    """Activations travel as two fp16 planes of 16 x value: 22 bits while the low plane is a normal fp16 number, an absolute floor of
    2^-29 (half of fp16's smallest subnormal, over 16) once |value| falls below about 2^-7."""
    rs = np.random.RandomState(3)
    for e in (0, -4, -7, -10, -14, -18):
        v = (rs.uniform(1.0, 2.0, 4096) * 2.0 ** e).astype(np.float32)
        h, lo = rr.x2_split(v)
        err = np.abs(rr.x2_value(h, lo) - v.astype(np.float64))
        assert err.max() <= max(2.0 ** -29, 2.0 ** (e + 1 - 23))
        if e <= -10:
            assert err.max() > 2.0 ** -31                                 # the floor is really there
