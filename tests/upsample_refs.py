"""References and bounds for the vertex regressor's edge tests (tests/test_gpu_upsample_edges.py, tests/test_host_upsample_refs.py).

The operation (lib/models/MDR.py:122,167-168: Conv1d 431 -> 6890, kernel 3, padding 1 over the 3-long xyz axis, + bias + template):

    out[b, o, l] = bias[o] + tpl[o, l] + sum_{c, k} w[o, c, k] * vc[b, c, l + k - 1]        (zero where l + k - 1 is outside 0..2)

Nothing here calls the library: the product is nine-minus-two plain matmuls in torch, the operand roundings are restated in numpy from
the kernels' own headers (gator_amd/csrc/upsample_*.hip), and only constants are shared with gator_amd."""
import math

import numpy as np
import torch

V, NV = 431, 6890                 # coarse vertices, mesh vertices
K_TERMS = 3 * V                   # 1293 products per output at l = 1 (862 at l = 0 and 2)
EPS32 = float(np.finfo(np.float32).eps)

ACT_SHIFT = 4                     # upsample_x2.hip kActShift: activations x 2^4
W_SHIFT_MIN, W_SHIFT_MAX = -118, 118      # pack_upsample_x2's clamps (they only keep 2^shift and 2^-(shift + 4) normal floats)

# D_form: the share of every product a * w that a form does not compute, BY DESIGN, relative to |a| |w| of the operands it carries.
#   fp32 / basic : fp32 operands, every product formed (upsample_fused.hip, basic_kernels.hip)                               -> 0
#   bf16         : ONE bf16 plane per operand, one MFMA per product (upsample_bf16.hip)                                      -> 0
#   x2w1         : k_upsample_x2<false>: weights on one fp16 plane, activations on two; hi*hi and lo*hi are both formed      -> 0
#   x2           : k_upsample_x2<true>, "Three partial products per k-step (hi*hi | hi*lo, lo*hi)": lo*lo is dropped.  lo is the
#                  fp16 rounding of x - hi with hi = fp16(x), so |lo| <= 2^-11 |hi| on either side and |lo_a lo_w| <= 2^-22 |a| |w|
#   x3           : upsample_x3.hip forms six of the nine products of x = hi + mid + lo (bf16: 8 significand bits, unit roundoff 2^-8,
#                  so |mid| <= 2^-8 |x| and |lo| <= 2^-16 |x|); dropped: mid*lo and lo*mid (<= 2^-24 each) and lo*lo (<= 2^-32):
#                  2^-23 + 2^-32, the header's "below 2^-23 of the product" up to its last term
D_FORM = {'fp32': 0.0, 'basic': 0.0, 'bf16': 0.0, 'x2w1': 0.0, 'x2': 2.0 ** -22, 'x3': 2.0 ** -23 + 2.0 ** -32}
ORDER_FACTOR = 4.0                # admits another order of the same 1293 fp32 roundings (16-deep MFMA blocks, two-level totals), nothing else


# ---- operand roundings (numpy) ---------------------------------------------------------------------------------------------------
def bf16_rne(x):
    """float32 -> the nearest bf16 (ties to even), returned as float32.  Non-finite values pass through (NaN stays NaN)."""
    x = np.ascontiguousarray(x, np.float32)
    b = x.view(np.uint32).astype(np.uint64)
    r = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    out = r.astype(np.uint32).view(np.float32).copy()
    nan = np.isnan(x)
    out[nan] = x[nan]
    return out.reshape(x.shape)


def f16_split(x, shift):
    """The two fp16 planes of 2^shift * x (upsample_x2.hip split2): h = f16(s x), l = f16(s x - h), both as float32.  s x and
    s x - h are exact in float32 (a power-of-two scaling; h holds the leading 11 bits of s x)."""
    with np.errstate(over='ignore', invalid='ignore'):
        sx = np.asarray(x, np.float32) * np.float32(2.0 ** shift)
        h = sx.astype(np.float16).astype(np.float32)
        l = (sx - h).astype(np.float16).astype(np.float32)
    return h, l


def f16_two_plane(x, shift):
    """What the two-plane form carries of x: (h + l) / 2^shift, float64."""
    h, l = f16_split(x, shift)
    return (h.astype(np.float64) + l.astype(np.float64)) * 2.0 ** -shift


def f16_one_plane(x, shift):
    """k_upsample_x2<false>'s weights: f16(x 2^shift) / 2^shift, float64."""
    h, _ = f16_split(x, shift)
    return h.astype(np.float64) * 2.0 ** -shift


def weight_shift(wmax):
    """pack_upsample_x2: the largest power of two that keeps max|w| 2^shift below 2^14 ("wmax = m 2^e, m in [0.5, 1) -> wmax 2^(14 - e)
    in [2^13, 2^14)"), clamped; 0 when max|w| is zero, infinite or NaN ("a NaN weight wins: the scale falls back to 1")."""
    wmax = float(wmax)
    if not (wmax > 0.0 and math.isfinite(wmax)):
        return 0
    _, e = math.frexp(wmax)
    return max(W_SHIFT_MIN, min(W_SHIFT_MAX, 14 - e))


def round_operands(form, vc, w):
    """(vc, w) float32 numpy -> float64 numpy, rounded to exactly what `form` carries into its MFMAs."""
    vc, w = np.asarray(vc, np.float32), np.asarray(w, np.float32)
    if form in ('fp32', 'basic', 'x3'):          # x3: three bf16 planes hold all 24 significand bits ("nothing is lost")
        return vc.astype(np.float64), w.astype(np.float64)
    if form == 'bf16':
        return bf16_rne(vc).astype(np.float64), bf16_rne(w).astype(np.float64)
    sh = weight_shift(np.abs(w).max())
    if form == 'x2':
        return f16_two_plane(vc, ACT_SHIFT), f16_two_plane(w, sh)
    if form == 'x2w1':
        return f16_two_plane(vc, ACT_SHIFT), f16_one_plane(w, sh)
    raise ValueError(form)


# ---- the product -------------------------------------------------------------------------------------------------------------------
def conv_sum(vc, w):
    """sum_{c,k} w[o,c,k] vc[b,c,l+k-1] -> [B, 6890, 3] in the operands' dtype: one matmul per (l, k) pair whose input column l + k - 1
    exists (seven of the nine; the other two multiply the padding)."""
    B = vc.shape[0]
    out = torch.zeros((B, w.shape[0], 3), dtype=vc.dtype, device=vc.device)
    for l in range(3):
        for k in range(3):
            lp = l + k - 1
            if 0 <= lp <= 2:
                out[:, :, l] += vc[:, :, lp] @ w[:, :, k].T
    return out


def _t(a, dtype, device):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=device, dtype=dtype)


def reference(vc, w, bias, tpl, device='cpu'):
    """-> (ref, S_aw, S) float64 tensors [B, 6890, 3] on `device` for float64 numpy operands (already rounded as the form carries them)."""
    d = torch.float64
    vc_t, w_t, b_t, t_t = (_t(a, d, device) for a in (vc, w, bias, tpl))
    ref = conv_sum(vc_t, w_t) + b_t[None, :, None] + t_t[None]
    s_aw = conv_sum(vc_t.abs(), w_t.abs())
    s = s_aw + b_t.abs()[None, :, None] + t_t.abs()[None]
    return ref, s_aw, s


def reference32(vc, w, bias, tpl):
    """The same product evaluated plainly in float32 on the CPU (operands rounded to float32 where the form's sum of planes has more
    bits: at most one more rounding of 2^-24 per operand) -> float32 tensor."""
    f = torch.float32
    vc_t, w_t, b_t, t_t = (_t(np.asarray(a, np.float64).astype(np.float32), f, 'cpu') for a in (vc, w, bias, tpl))
    return (conv_sum(vc_t, w_t) + b_t[None, :, None]) + t_t[None]


def measure_e32(ref32, ref, s):
    """The float32 evaluation's largest error in units of S over the case."""
    r = (ref32.to(ref.device, torch.float64) - ref).abs() / s
    return float(r.max())


def bound(form, s_aw, s, e32):
    """|out - ref| <= D_form S_aw + 4 e32 S, per output element."""
    return D_FORM[form] * s_aw + ORDER_FACTOR * e32 * s


# ---- one-hot sweep (every coarse vertex x input position) ---------------------------------------------------------------------------
def onehot_batch():
    """vc [1294, 431, 3]: sample i = 3 c + lp has vc[i, c, lp] = 1; the last sample is zero."""
    vc = np.zeros((K_TERMS + 1, V, 3), np.float32)
    i = np.arange(K_TERMS)
    vc[i, i // 3, i % 3] = 1.0
    return vc


def onehot_expected(w_carried, bias, tpl):
    """-> (expected float32 [1293, 6890, 3], w' float64, valid bool [1293, 1, 3]): out[i,o,l] = fl32(fl32(w' + bias) + tpl) with
    w' = w[o, c, lp + 1 - l] as the form carries it; where lp + 1 - l is no tap, valid is False and the zero sample's value is expected."""
    w_carried = np.asarray(w_carried, np.float64)
    i = np.arange(K_TERMS)
    c, lp = i // 3, i % 3
    wp = np.zeros((K_TERMS, NV, 3), np.float64)
    valid = np.zeros((K_TERMS, 1, 3), bool)
    for l in range(3):
        k = lp + 1 - l
        ok = (k >= 0) & (k <= 2)
        wp[ok, :, l] = w_carried[:, c[ok], k[ok]].T
        valid[ok, 0, l] = True
    b32 = np.asarray(bias, np.float32)[None, :, None]
    t32 = np.asarray(tpl, np.float32)[None]
    exp = (wp.astype(np.float32) + b32) + t32          # w' has at most 24 significant bits in every form but x2 (22 + scale: also exact)
    return exp, wp, valid


# ---- joint regressors for the epilogue ---------------------------------------------------------------------------------------------
def joint_regressors(seed=11):
    """{name: dense float32 [nj, 6890]} -- the epilogue's table edges: first / last vertex, the 10-vertex tail block, a crowded
    32-vertex block, an empty joint, one joint, and 3000 entries whose signs cancel."""
    rs = np.random.RandomState(seed)
    out = {}
    d = np.zeros((2, NV), np.float32); d[0, 0] = 0.75; d[1, 0] = -1.25; out['vertex0'] = d
    d = np.zeros((2, NV), np.float32); d[1, NV - 1] = 1.5; d[0, NV - 1] = 0.3; out['vertex6889'] = d
    d = np.zeros((3, NV), np.float32); d[:, NV - 10:] = rs.randn(3, 10); out['tail_block'] = d
    d = np.zeros((8, NV), np.float32); d[:, 32 * 100:32 * 101] = rs.randn(8, 32); out['crowded_block'] = d
    d = np.zeros((4, NV), np.float32); d[0, 5] = 1.0; d[1, 3000:3010] = rs.rand(10); d[3, 6000] = 2.0; out['empty_joint'] = d      # joint 2 is empty
    d = np.zeros((1, NV), np.float32); d[0, rs.choice(NV, 40, replace=False)] = rs.rand(40) / 20; out['one_joint'] = d
    d = np.zeros((17, NV), np.float32)
    pos = rs.choice(17 * NV, 3000, replace=False)
    d.reshape(-1)[pos] = (rs.rand(3000) + 0.5) * np.where(np.arange(3000) % 2, -1.0, 1.0)
    out['cancelling'] = d
    return out


def shuffled_with_duplicates(dense, seed=12):
    """COO list (row, col, val int32/int32/float32) of `dense`, shuffled, with every fifth entry split into two entries of the same
    (joint, vertex) whose values add up to a different total -> (row, col, val, dense float64 of what the list sums to)."""
    rs = np.random.RandomState(seed)
    r, c = np.nonzero(dense)
    v = dense[r, c].astype(np.float32)
    extra = np.arange(0, r.size, 5)
    r2, c2 = np.concatenate([r, r[extra]]), np.concatenate([c, c[extra]])
    v2 = np.concatenate([v, (rs.rand(extra.size) - 0.5).astype(np.float32)])
    p = rs.permutation(r2.size)
    r2, c2, v2 = r2[p], c2[p], v2[p]
    tot = np.zeros(dense.shape, np.float64)
    np.add.at(tot, (r2, c2), v2.astype(np.float64))
    return r2.astype(np.int32), c2.astype(np.int32), v2.astype(np.float32), tot


def joints_reference(entries_dense_or_coo, verts):
    """float64 sum_e w_e verts[b, v_e] and sum_e |w_e| |verts| for COO (row, col, val, nj) over float32 verts (torch, any device)."""
    r, c, v, nj = entries_dense_or_coo
    dev = verts.device
    vd = verts.double()
    ci = torch.as_tensor(c.astype(np.int64), device=dev)
    ri = torch.as_tensor(r.astype(np.int64), device=dev)
    wv = torch.as_tensor(v.astype(np.float64), device=dev)
    prod = vd[:, ci, :] * wv[None, :, None]                      # [B, nnz, 3]
    B = vd.shape[0]
    ref = torch.zeros((B, nj, 3), dtype=torch.float64, device=dev).index_add_(1, ri, prod)
    mag = torch.zeros((B, nj, 3), dtype=torch.float64, device=dev).index_add_(1, ri, prod.abs())
    return ref, mag
