"""Function-preserving power-of-two rescalings of a GATOR checkpoint, and numpy restatements of the two operand splits of the
default arithmetic (csrc/fused_pack.hip k_repack_h3, csrc/x3_common.h x2_split).

The network has exact symmetries: scaling one tensor group by 2^k and its partner by 2^-k changes no output of the reference, bit for
bit, in fp32 as well as fp64 (tests/test_host_rescale_refs.py proves that on the oracle).  They move the RATIO of magnitudes between
the weight grids of one checkpoint -- the one thing the seeded recipe (synthetic.seeded_state_dict) never moves, and the thing the
shared power-of-two scale of a three-plane weight set depends on.  Everything here works on a reference-layout state dict of torch
tensors (the oracle's `sd` and a module's state_dict() alike) and returns a new dict; the input is left as it was."""
import numpy as np

GAT = 'pose_lifter.blocks.%d.'
MDR_SFX = ('', '_1', '_2')

# family -> (index range, [(key template, row slice or None)] scaled by 2^k, [...] scaled by 2^-k)
_Q, _K, _V = slice(0, 128), slice(128, 256), slice(256, 384)


def _gat(keys):
    return [(GAT + k, r) for k, r in keys]


def _mdr(keys):
    return [('pose2mesh.' + k, r) for k, r in keys]


EXACT = {
    'gat_qk': (6, _gat([('attn.qkv.weight', _Q), ('attn.qkv.bias', _Q)]), _gat([('attn.qkv.weight', _K), ('attn.qkv.bias', _K)])),
    'gat_vproj': (6, _gat([('attn.qkv.weight', _V), ('attn.qkv.bias', _V)]), _gat([('attn.proj.weight', None)])),
    'gat_gcn': (6, _gat([('gcn.W', None)]), _gat([('gcn.M', None)])),
    'gat_xfeat': (6, _gat([('x_feat.linears.0.weight', None), ('x_feat.linears.0.bias', None), ('x_feat.linears.1.weight', None),
                           ('x_feat.linears.1.bias', None)]), _gat([('x_feat.linearback.weight', None)])),
    'mdr_qk': (3, _mdr([('encoder%s.attn.wq.weight', None)]), _mdr([('encoder%s.attn.wk.weight', None)])),
    'mdr_vproj': (3, _mdr([('encoder%s.attn.wv.weight', None)]), _mdr([('encoder%s.attn.proj.weight', None)])),
    'mdr_self_qk': (3, _mdr([('selfatt%s.linears.0.weight', None), ('selfatt%s.linears.0.bias', None)]),
                    _mdr([('selfatt%s.linears.1.weight', None), ('selfatt%s.linears.1.bias', None)])),
    'mdr_self_vo': (3, _mdr([('selfatt%s.linears.2.weight', None), ('selfatt%s.linears.2.bias', None)]),
                    _mdr([('selfatt%s.linears.3.weight', None)])),
}
# GELU sits between the two tensors: not a symmetry, the oracle is recomputed on the scaled weights.  (fc2 x 2^k, fc1 x 2^-k)
NEAR = {
    'gat_mlp': (6, _gat([('mlp.fc2.weight', None)]), _gat([('mlp.fc1.weight', None), ('mlp.fc1.bias', None)])),
    'mdr_mlp': (3, _mdr([('encoder%s.mlp.fc2.weight', None)]), _mdr([('encoder%s.mlp.fc1.weight', None), ('encoder%s.mlp.fc1.bias', None)])),
}
GAT_EXACT = ('gat_qk', 'gat_vproj', 'gat_gcn', 'gat_xfeat')
MDR_EXACT = ('mdr_qk', 'mdr_vproj', 'mdr_self_qk', 'mdr_self_vo')
FAMILIES = GAT_EXACT + MDR_EXACT + tuple(NEAR) + ('all',)


def _scale(out, sd, key, rows, k):
    t = out[key] if out[key] is not sd[key] else sd[key].clone()
    f = 2.0 ** k                                     # exact in every float format for |k| <= 126
    if rows is None:
        t.mul_(f)
    else:
        t[rows].mul_(f)
    out[key] = t


def _apply(out, sd, family, k, alternate):
    n, up, down = {**EXACT, **NEAR}[family]
    for i in range(n):
        ki = -k if (alternate and i % 2) else k
        idx = i if n == 6 else MDR_SFX[i]
        for group, sign in ((up, 1), (down, -1)):
            for tmpl, rows in group:
                _scale(out, sd, tmpl % idx, rows, sign * ki)


def rescale(sd, family, k):
    """-> a new state dict: `family` applied with exponent k to all six GAT blocks / all three MDR layers.  'all': every exact family
    at once, the sign of k alternating with the block / layer index."""
    out = dict(sd)
    if family == 'all':
        for fam in EXACT:
            _apply(out, sd, fam, k, True)
    else:
        _apply(out, sd, family, k, False)
    return out


def is_exact(family):
    return family == 'all' or family in EXACT


# ---- the operand formats of the default arithmetic, restated -------------------------------------------------------------------------

def h3_shift(wmax):
    """The one power-of-two exponent of a three-plane weight set (fused_repack_h3): 2^13 <= 2^shift wmax < 2^14, clamped to [-16, 24]."""
    wmax = float(wmax)
    if not (wmax > 0.0 and np.isfinite(wmax)):
        return 0
    return int(min(max(14 - np.frexp(np.float32(wmax))[1], -16), 24))


def h3_split(w, shift):
    """k_repack_h3: three fp16 planes of 2^shift w, every step in fp32 as on the device.  -> (hi, mid, lo, left) with
    left = |2^shift w - (hi + mid + lo)| per element (float32)."""
    x = (np.asarray(w, np.float32) * np.float32(2.0 ** shift)).astype(np.float32)
    h = x.astype(np.float16)
    r = (x - h.astype(np.float32)).astype(np.float32)
    m = r.astype(np.float16)
    r2 = (r - m.astype(np.float32)).astype(np.float32)
    lo = r2.astype(np.float16)
    return h, m, lo, np.abs(r2 - lo.astype(np.float32))


def h3_value(h, m, lo, shift):
    """What the three planes stand for, in float64."""
    return (h.astype(np.float64) + m.astype(np.float64) + lo.astype(np.float64)) * 2.0 ** -shift


def x2_split(v, scale=16.0):
    """x2_split_scaled: two fp16 planes of scale * v.  -> (hi, lo)."""
    x = (np.asarray(v, np.float32) * np.float32(scale)).astype(np.float32)
    h = x.astype(np.float16)
    return h, (x - h.astype(np.float32)).astype(np.float32).astype(np.float16)


def x2_value(h, lo, scale=16.0):
    return (h.astype(np.float64) + lo.astype(np.float64)) / scale


# The create-time criterion of the three-plane weight sets (csrc/fused_pack.hip, fused_repack_h3), restated: the smallest ratio of a
# 32 x 32 tile's own max|w| to the set's max|w|, over the tiles that hold a weight at all.  The planes hold every weight to 2^-38
# of the set's largest, so a tile at ratio r keeps its weights to 2^-38 / r of ITS largest; the set is accepted down to r = 2^-12
# (2^-26: a quarter of fp32's half-ulp at the tile's largest weight, which is what a weight of a quarter that size needs).
H3_MIN_TILE_RATIO = 2.0 ** -12


def h3_min_tile_ratio(tiles):
    """tiles: [ntiles, ...] -> min over the non-zero tiles of max|tile| / max|all|."""
    t = np.abs(np.asarray(tiles, np.float64)).reshape(len(tiles), -1).max(1)
    return float(t[t > 0].min() / t.max())
