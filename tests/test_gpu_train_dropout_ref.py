"""Dropout ON against references that share nothing with the library: the masks of gator_t_dropout bit for bit against the numpy
Philox of tests/train_refs.py (itself pinned to the Random123 known answers in tests/test_host_train.py), and the fused attention /
small attention / drop_fused kernels against torch-CPU float64 autograd of the same formula with that mask.
tests/test_gpu_train_fused.py compares the same kernels with the library's own primitives drawing from the same generator, which a
shared indexing or scaling error passes."""
import numpy as np
import pytest
import torch

from gator_amd.train import ops
from tests.train_refs import attention_ref, attention_small_ref, check_close, drop_fused_ref, keep_factor, keep_mask

pytestmark = pytest.mark.gpu

SEEDS = (123, (1 << 32) + 0x9E3779B9 * 5 + 17)            # one below and one above 2^32: both key words are used
RATES = (0.1, 0.4, 0.999)
SIZES = (1, 3, 4, 5, 1023, 1025, (1 << 18) + 2)


def _gen(seed, offset):
    g = ops.Generator(seed)
    g.offset = offset - 1                                 # the next mask draws `offset`
    return g


@pytest.mark.parametrize('n', SIZES)
def test_dropout_masks_equal_the_host_philox(n):
    x = torch.ones(n, device='cuda', requires_grad=True)
    for seed in SEEDS:
        for offset in (1, 7):
            for rate in RATES:
                want = keep_mask(seed, offset, n, rate)
                y = ops.dropout(x, rate, _gen(seed, offset))
                saved = y.grad_fn.saved_tensors[0]
                assert saved.dtype == torch.uint8
                assert np.array_equal(saved.cpu().numpy(), want), ('saved mask', seed, offset, rate)
                assert np.array_equal((y.detach() != 0).cpu().numpy().astype(np.uint8), want), ('dropout', seed, offset, rate)
                kept = y.detach()[y.detach() != 0]
                assert kept.numel() == 0 or float((kept - 1.0 / (1.0 - np.float32(rate))).abs().max()) <= 1e-3 * (1.0 / (1.0 - rate))
                z = ops.drop_path(torch.ones(n, 1, 2, device='cuda'), rate, _gen(seed, offset))       # one decision per sample, n samples
                zm = (z != 0).cpu().numpy().astype(np.uint8)
                assert np.array_equal(zm[:, 0, 0], want) and np.array_equal(zm[:, 0, 1], want), ('drop_path', seed, offset, rate)


def test_device_step_counter_selects_the_high_word_of_the_offset():
    """Generator.device_steps: the counter starts at 0, gator_t_step_advance adds one per begin_step(), the masks are those of
    offset + 2^32 * step, and begin_step() restarts the site offsets at 1."""
    n, rate, seed = 1025, 0.4, SEEDS[1]
    x = torch.ones(n, device='cuda')
    g = ops.Generator(seed).device_steps('cuda')
    mask = lambda y: (y != 0).cpu().numpy().astype(np.uint8)
    steps = 0
    for target in (0, 1, 3):
        while steps < target:
            g.begin_step()
            steps += 1
        assert int(g.counter.item()) == target
        assert g.offset == 0 or target == 0
        g.offset = 0                                       # (target 0: no begin_step() has run yet)
        assert np.array_equal(mask(ops.dropout(x, rate, g)), keep_mask(seed, 1, n, rate, step=target)), target
        assert np.array_equal(mask(ops.dropout(x, rate, g)), keep_mask(seed, 2, n, rate, step=target)), target
        assert np.array_equal(mask(ops.drop_path(torch.ones(n, 3, device='cuda'), rate, g))[:, 0], keep_mask(seed, 3, n, rate, step=target)), target
        assert g.offset == 3
    g.begin_step()
    assert g.offset == 0 and int(g.counter.item()) == 4
    assert np.array_equal(mask(ops.dropout(x, rate, g)), keep_mask(seed, 1, n, rate, step=4))
    assert not np.array_equal(keep_mask(seed, 1, n, rate, step=4), keep_mask(seed, 1, n, rate, step=3))


def _attention_case(B, H, T, Tk, rate, seed, offset, peak=None):
    rs = np.random.RandomState(1000 * T + 10 * Tk + B)
    D = 32
    scale = 1.0 / np.sqrt(D)
    q, k, v = [torch.from_numpy(rs.randn(B, n, H * D)) for n in (T, Tk, Tk)]
    if peak is not None:                                   # scale q and k so that max |scale q k^T| is about `peak`
        qq, kk = [t.reshape(B, t.shape[1], H, D).transpose(1, 2) for t in (q, k)]
        f = np.sqrt(peak / float((scale * (qq @ kk.transpose(-2, -1))).abs().max()))
        q, k = q * f, k * f
    q, k, v = [t.float().double().requires_grad_(True) for t in (q, k, v)]          # values exactly representable in float32
    w = torch.from_numpy(rs.randn(B, T, H * D)).float().double()
    want = attention_ref(q, k, v, H, scale, keep_factor(seed, offset, (B, H, T, Tk), rate))
    gw = torch.autograd.grad(want, [q, k, v], grad_outputs=w)
    qd, kd, vd = [t.detach().float().cuda().requires_grad_(True) for t in (q, k, v)]
    got = ops.attention(qd, kd, vd, H, scale, rate, _gen(seed, offset), True)
    gg = torch.autograd.grad(got, [qd, kd, vd], grad_outputs=w.float().cuda())
    tag = 'attention B%d H%d T%d Tk%d rate %.1f%s' % (B, H, T, Tk, rate, '' if peak is None else ' peak %g' % peak)
    check_close(tag + ' o', got, want.detach())
    scales = {}
    if Tk == 1:
        # softmax over ONE key is the constant 1: dq and dk are exactly 0 in the reference, and max|ref| is no scale.  The kernels form
        # dS = p (dP keep - dO . O), the difference of two equal terms; the criterion there is 2e-5 of the size of those terms times
        # the k (resp. q) they multiply, taken from the float64 inputs.
        assert float(gw[0].abs().max()) == 0.0 and float(gw[1].abs().max()) == 0.0
        hd = lambda t: t.detach().reshape(B, t.shape[1], H, D).transpose(1, 2)
        term = scale * (hd(w) * hd(v)).sum(-1, keepdim=True) * keep_factor(seed, offset, (B, H, T, Tk), rate)      # [B, H, 1, 1]
        scales = {'dq': float((term * hd(k)).abs().max()), 'dk': float((term * hd(q)).abs().max())}
    for nm, a, b in zip(('dq', 'dk', 'dv'), gg, gw):
        check_close(tag + ' ' + nm, a, b, scale=scales.get(nm))


ATTN_SHAPES = [(2, 2, 431, 431), (1, 3, 77, 77), (3, 2, 33, 33), (2, 1, 1, 1), (2, 2, 431, 17), (2, 2, 431, 19), (1, 2, 100, 17), (1, 2, 140, 33),
               (2, 2, 64, 32)]


@pytest.mark.parametrize('B,H,T,Tk', ATTN_SHAPES)
def test_attention_with_dropout_against_float64(B, H, T, Tk):
    """softmax(scale q k^T) * keep_mask / (1 - rate) @ v in float64 with the host mask at the flat index of [B, H, T, Tk].  The shapes
    with Tk <= 128 and T >= 4 Tk take the qsplit path of _Attention.backward; (1, 2, 100, 17) has fewer query tiles than its cap."""
    _attention_case(B, H, T, Tk, 0.1, SEEDS[0], 1)
    _attention_case(B, H, T, Tk, 0.3, SEEDS[1], 7)


@pytest.mark.parametrize('B,H,T,Tk', [(2, 2, 431, 431), (2, 2, 431, 17)])
def test_attention_with_large_scores_against_float64(B, H, T, Tk):
    """rate 0, max |scale q k^T| about 80: the online softmax of the forward and the lse handed to the backward must hold"""
    _attention_case(B, H, T, Tk, 0.0, 0, 1, peak=80.0)


@pytest.mark.parametrize('B,H', [(7, 8), (3, 3)])
@pytest.mark.parametrize('J', [1, 2, 17, 19, 31, 32])
def test_small_attention_with_dropout_against_float64(J, B, H):
    """(3, 3): B * H is not a multiple of the four waves of a workgroup"""
    D, scale = 16, 0.25
    C = H * D
    for rate, seed, offset in ((0.0, 0, 1), (0.4, SEEDS[0], 1), (0.4, SEEDS[1], 7)):
        rs = np.random.RandomState(100 * J + B)
        qkv = torch.from_numpy(rs.randn(B, J, 3 * C)).float().double().requires_grad_(True)
        bias = torch.from_numpy(rs.randn(H, J, J)).float().double().requires_grad_(True)
        w = torch.from_numpy(rs.randn(B, J, C)).float().double()
        want = attention_small_ref(qkv, bias, H, scale, keep_factor(seed, offset, (B, H, J, J), rate))
        gw = torch.autograd.grad(want, [qkv, bias], grad_outputs=w)
        qd, bd = [t.detach().float().cuda().requires_grad_(True) for t in (qkv, bias)]
        got = ops.attention_small(qd, bd, H, scale, rate, _gen(seed, offset), True)
        gg = torch.autograd.grad(got, [qd, bd], grad_outputs=w.float().cuda())
        tag = 'attention_small J%d B%d H%d rate %.1f' % (J, B, H, rate)
        check_close(tag + ' o', got, want.detach())
        check_close(tag + ' dqkv', gg[0], gw[0])
        check_close(tag + ' dbias', gg[1], gw[1])


@pytest.mark.parametrize('shape', [(9, 19, 128), (5, 7, 3)])
@pytest.mark.parametrize('gelu,rate,path,with_res', [(True, 0.1, 0.0, False), (False, 0.2, 0.2, True), (False, 0.0, 0.3, True), (True, 0.0, 0.0, False)])
def test_drop_fused_against_float64(gelu, rate, path, with_res, shape):
    """res + path[b] * mask * gelu(x) / (1 - rate) with both masks from the host Philox; (5, 7, 3): 105 elements (not a multiple of 4)
    in samples of 21 (odd), so Philox quads straddle samples."""
    seed = SEEDS[1]
    rs = np.random.RandomState(8)
    x = torch.from_numpy(rs.randn(*shape)).float().double().requires_grad_(True)
    res = torch.from_numpy(rs.randn(*shape)).float().double().requires_grad_(True) if with_res else None
    w = torch.from_numpy(rs.randn(*shape)).float().double()
    first = 4                                              # offsets are drawn element mask first, DropPath second
    off = first if rate > 0 else None
    poff = (first + (1 if rate > 0 else 0)) if path > 0 else None
    ek = keep_factor(seed, off, shape, rate) if rate > 0 else None
    pk = keep_factor(seed, poff, (shape[0],), path) if path > 0 else None
    want = drop_fused_ref(x, res, gelu, ek, pk)
    ins = [x] + ([res] if with_res else [])
    gw = torch.autograd.grad(want, ins, grad_outputs=w)
    dev = [t.detach().float().cuda().requires_grad_(True) for t in ins]
    got = ops.drop_fused(dev[0], dev[1] if with_res else None, gelu, rate, path, _gen(seed, first), True)
    gg = torch.autograd.grad(got, dev, grad_outputs=w.float().cuda())
    tag = 'drop_fused %s gelu %d rate %.1f path %.1f res %d' % (shape, gelu, rate, path, with_res)
    check_close(tag + ' out', got, want.detach())
    for nm, a, b in zip(('dx', 'dres'), gg, gw):
        check_close(tag + ' ' + nm, a, b)
    if path > 0:                                           # the kept samples are those of the host mask, exactly
        kept = (got.detach().cpu().double() - (res.detach() if with_res else 0)).reshape(shape[0], -1).abs().sum(1) != 0
        assert np.array_equal(kept.numpy(), keep_mask(seed, poff, shape[0], path).astype(bool))
