"""The row kernels of the training step against float64 references that share nothing with the library: LayerNorm (both modes, the
skip-connection `add` input, dy_xhat, gradient slots), softmax, BatchNorm in training mode, the fused MGCN layer, gator_t_add_n and the
fork backward that drives it - value and every gradient, at the wave / workgroup / tile edges of each kernel.
tests/test_gpu_train_ops.py has one or two shapes of each and compares the MGCN layer only with the library's own primitives."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gator_amd import _lib
from gator_amd.train import ops
from tests.train_refs import check_close, close_bound, layernorm_ref, mgcn_ref

pytestmark = pytest.mark.gpu

PATTERN = 0xA5
LN_EPS = {0: 1e-5, 1: 1e-6}                                # nn.LayerNorm's default; vanilla_transformer_encoder.py:26


def _t(a):
    """float32 values held in float64"""
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).float().double()


def _dev(t):
    return None if t is None else t.detach().float().cuda().requires_grad_(t.requires_grad)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(nfloats, pad=256):
    """(whole uint8 buffer filled with the pattern, its float32 window of nfloats elements `pad` bytes in)"""
    whole = torch.full((2 * pad + 4 * nfloats,), PATTERN, dtype=torch.uint8, device='cuda')
    return whole, whole[pad:pad + 4 * nfloats].view(torch.float32)


def _guards_hold(whole, nfloats, pad=256):
    return bool((whole[:pad] == PATTERN).all()) and bool((whole[pad + 4 * nfloats:] == PATTERN).all())


def _slot(p):
    """gives the device leaf p a slice of a (here: private) flat gradient buffer, as optim.FlatParams.views does"""
    p._gslot = torch.full(p.shape, float('nan'), device='cuda')
    return p._gslot


# ---- LayerNorm -----------------------------------------------------------------------------------------------------------------
LN_ROWS = (1, 3, 4, 5, 9)                                  # a partial, a full and a just-over-full workgroup of four waves (one wave per row)
LN_NS = (1, 2, 3, 20, 63, 64, 65, 128, 272, 1000)


def _ln_inputs(rows, n, affine, seed, offset=0.0):
    rs = np.random.RandomState(seed)
    x = _t(rs.randn(rows, n) + offset).requires_grad_(True)
    w = _t(1.0 + 0.5 * rs.randn(n)).requires_grad_(True) if affine else None
    b = _t(rs.randn(n)).requires_grad_(True) if affine else None
    return x, w, b, _t(rs.randn(rows, n)), _t(rs.randn(rows, n))


def _ln_rinv(x, eps, mode):
    x = x.detach()
    return 1.0 / torch.sqrt(x.var(-1, keepdim=True, unbiased=False) + eps) if mode == 0 else 1.0 / (x.std(-1, keepdim=True) + eps)


def _ln_case(rows, n, mode, affine, skip, seed, offset=0.0, noise=False, slots=False):
    eps = LN_EPS[mode]
    x, w, b, gy, gs = _ln_inputs(rows, n, affine, seed, offset)
    names = ['dx'] + (['dw', 'db'] if affine else [])

    def ref(dtype):
        xx, ww, bb = [None if t is None else t.detach().to(dtype).requires_grad_(True) for t in (x, w, b)]
        y = layernorm_ref(xx, ww, bb, eps, mode)
        loss = (y * gy.to(dtype)).sum() + ((xx * gs.to(dtype)).sum() if skip else 0.0)        # LN(x) . W1 + x . W2: the skip connection
        return [y.detach()] + list(torch.autograd.grad(loss, [xx] + ([ww, bb] if affine else [])))

    want = ref(torch.float64)
    if n == 1:
        # one value per row: xhat is exactly 0, and so are the LayerNorm part of dx and dw = sum dy xhat; torch's own float64 rows leave a
        # rounding residue (1e-14) in both, which is no reference for an exact 0
        exact = [gs if skip else torch.zeros_like(gs)] + ([torch.zeros(1, dtype=torch.float64)] if affine else [])
        for i, e in enumerate(exact, 1):
            assert float((want[i] - e).abs().max()) < 1e-12
            want[i] = e
    noise32 = ref(torch.float32) if noise else [None] * len(want)
    xd, wd, bd = _dev(x), _dev(w), _dev(b)
    wslot, bslot = (_slot(wd), _slot(bd)) if slots else (None, None)
    if skip:
        y, res = ops.layernorm_skip(xd, wd, bd, eps, mode)
        assert torch.equal(res.detach(), xd.detach())
        got = torch.autograd.grad([y, res], [xd] + ([wd, bd] if affine else []), grad_outputs=[_dev(gy), _dev(gs)])
    else:
        y = ops.layernorm(xd, wd, bd, eps, mode)
        got = torch.autograd.grad(y, [xd] + ([wd, bd] if affine else []), grad_outputs=_dev(gy))
    if slots:
        # the weight / bias gradients were queued on Deferred, into the slots, and the slots themselves went to autograd
        assert got[1].data_ptr() == wslot.data_ptr() and got[2].data_ptr() == bslot.data_ptr()
        ops.Deferred.flush(xd.device)
        got = [got[0], wslot, bslot]
    tag = 'layernorm%s mode %d rows %d n %d%s%s%s' % (' skip' if skip else '', mode, rows, n, ' affine' if affine else '', ' slots' if slots else '',
                                                       ' mean %g' % offset if offset else '')
    scales = {}
    if n == 2:
        # Two values per row: xhat is +-1 up to eps, and dx = rinv (g - mean g - xhat mean(g xhat)) is the difference of terms that
        # cancel to a part in 1e5 or less (torch-CPU float32 is 9e-4 of max|dx| off in mode 0, 2e-2 in mode 1).  max|dx| is no scale for
        # a float32 result there; the size of the terms that cancel, max |rinv dy w| of the float64 reference, is.
        g = gy * (w.detach() if affine else 1.0)
        scales['dx'] = float((_ln_rinv(x, eps, mode) * g).abs().max())
    results = [('y', y.detach(), want[0], noise32[0])] + [(nm, a, r, q) for nm, a, r, q in zip(names, got, want[1:], noise32[1:])]
    for nm, a, r, q in results:
        if noise:
            # the noise term must not make the check vacuous: the whole bound stays at or below 1e-3 of the scale
            bound, scale = close_bound(r, noise32=q, scale=scales.get(nm))
            assert bound <= 1e-3 * scale, '%s %s: bound %.3e above 1e-3 of the scale %.3e' % (tag, nm, bound, scale)
        check_close('%s %s' % (tag, nm), a, r, noise32=q, scale=scales.get(nm))
    return y.detach(), got, want


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('n', LN_NS)
def test_layernorm_and_skip_against_float64(n, mode):
    """ops.layernorm and ops.layernorm_skip at every row count and width, with and without w, b.  n = 1 (mode 0 only; mode 1 has no
    unbiased std of one value): xhat is exactly 0, so y is b, d x is 0 and with the skip connection d x is the skip gradient, all bit for
    bit."""
    if n == 1 and mode == 1:
        x = torch.randn(3, 1, device='cuda', requires_grad=True)
        with pytest.raises(RuntimeError, match='gator_t_layernorm_fwd'):
            ops.layernorm(x, None, None, LN_EPS[1], 1)
        return
    for rows in LN_ROWS:
        for affine in (True, False):
            for skip in (False, True):
                seed = 7 * rows + 1000 * n + 2 * affine + skip
                y, got, want = _ln_case(rows, n, mode, affine, skip, seed)
                if n == 1:
                    x, w, b, gy, gs = _ln_inputs(rows, n, affine, seed)
                    assert torch.equal(y.cpu(), b.detach().float().expand(rows, 1) if affine else torch.zeros(rows, 1))
                    assert torch.equal(got[0].cpu(), gs.float() if skip else torch.zeros(rows, 1))


@pytest.mark.parametrize('mode', [0, 1])
def test_layernorm_skip_with_a_gradient_on_the_skip_output_only(mode):
    x, w, b, gy, gs = _ln_inputs(5, 65, True, 11)
    xd, wd, bd = _dev(x), _dev(w), _dev(b)
    y, res = ops.layernorm_skip(xd, wd, bd, LN_EPS[mode], mode)
    dx, dw, db = torch.autograd.grad([res], [xd, wd, bd], grad_outputs=[_dev(gs)], allow_unused=True)
    assert torch.equal(dx.cpu(), gs.float()) and dw is None and db is None
    check_close('layernorm skip-only y', y.detach(), layernorm_ref(x.detach(), w.detach(), b.detach(), LN_EPS[mode], mode))


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('rows,n', [(1, 20), (5, 65), (9, 1000)])
def test_layernorm_weight_gradients_land_in_their_slots(rows, n, mode):
    """w and b carry a gradient slot: the backward queues ones . (dy xhat) and ones . dy on Deferred into the slots and hands the slots
    themselves to autograd; after Deferred.flush they hold the float64 dw, db (checked in _ln_case)."""
    _ln_case(rows, n, mode, True, False, 13 + n, slots=True)
    _ln_case(rows, n, mode, True, True, 14 + n, slots=True)


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('n', [64, 65, 128, 1000])
def test_layernorm_with_a_mean_far_above_the_spread(n, mode):
    """x = 1e3 + randn: a one-pass (sum x^2 - n mean^2) or float-accumulated variance loses the spread here.  The same operation in
    torch-CPU float32 sets the noise, and the whole bound is capped at 1e-3 of the scale (about 1.7e-4 for these shapes).  Not used
    below n = 64: at n = 2 torch float32 itself is off by factors and the bound would mean nothing."""
    _ln_case(5, n, mode, True, False, 17 + n, offset=1e3, noise=True)
    _ln_case(5, n, mode, False, True, 18 + n, offset=1e3, noise=True)


@pytest.mark.parametrize('n', [2, 65])
def test_layernorm_mode_1_with_a_constant_row(n):
    """sigma = 0 in one row: torch's autograd gives NaN there; the kernel defines the d sigma term as 0.  That row's y is b bit for bit and
    its dx is finite; the other rows meet the criterion against a reference computed without the constant row, which contributes 0
    to dw (xhat = 0) and its dy to db."""
    rows, const, eps = 5, 2, LN_EPS[1]
    x, w, b, gy, _ = _ln_inputs(rows, n, True, 23 + n)
    x = x.detach()
    x[const] = 0.75
    keep = [r for r in range(rows) if r != const]
    xr, wr, br = x[keep].clone().requires_grad_(True), w.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
    yr = layernorm_ref(xr, wr, br, eps, 1)
    dxr, dwr, dbr = torch.autograd.grad((yr * gy[keep]).sum(), [xr, wr, br])
    xd, wd, bd = _dev(x.requires_grad_(True)), _dev(w), _dev(b)
    y = ops.layernorm(xd, wd, bd, eps, 1)
    dx, dw, db = torch.autograd.grad(y, [xd, wd, bd], grad_outputs=_dev(gy))
    assert torch.equal(y.detach()[const].cpu(), b.detach().float())
    assert bool(torch.isfinite(dx[const]).all())
    tag = 'layernorm mode 1 constant row n %d ' % n
    check_close(tag + 'y', y.detach()[keep], yr.detach())
    scale = float((_ln_rinv(x[keep], eps, 1) * gy[keep] * w.detach()).abs().max()) if n == 2 else None          # as in _ln_case
    check_close(tag + 'dx', dx[keep], dxr, scale=scale)
    check_close(tag + 'dw', dw, dwr)
    check_close(tag + 'db', db, dbr + gy[const])


def test_layernorm_c_abi_writes_inside_its_outputs_and_refuses_bad_widths():
    """One direct call of each direction at rows = 5, n = 65 with every output inside a larger buffer prefilled with 0xA5: y, mean, rinv,
    dx and dy_xhat (never read on its own by the wrappers: only its column sums are) are checked against float64, with the `add` input,
    and every byte outside them still holds the pattern.  The backward refuses the widths the forward refuses, before any launch."""
    lib = _lib.load()
    rows, n = 5, 65
    for mode in (0, 1):
        eps = LN_EPS[mode]
        x, w, b, gy, gs = _ln_inputs(rows, n, True, 29 + mode)
        xd, wd, bd, gyd, gsd = [_dev(t.detach()) for t in (x, w, b, gy, gs)]
        (Y, y), (MU, mu), (RI, ri), (DX, dx), (DYX, dyx) = [_guarded(k) for k in (rows * n, rows, rows, rows * n, rows * n)]
        assert lib.gator_t_layernorm_fwd(xd.data_ptr(), rows, n, wd.data_ptr(), bd.data_ptr(), eps, mode, y.data_ptr(), mu.data_ptr(), ri.data_ptr(),
                                         _stream()) == 0
        assert lib.gator_t_layernorm_bwd(gyd.data_ptr(), xd.data_ptr(), mu.data_ptr(), ri.data_ptr(), wd.data_ptr(), rows, n, eps, mode, dx.data_ptr(),
                                         dyx.data_ptr(), gsd.data_ptr(), _stream()) == 0
        torch.cuda.synchronize()
        for whole, k in ((Y, rows * n), (MU, rows), (RI, rows), (DX, rows * n), (DYX, rows * n)):
            assert _guards_hold(whole, k)
        xx = x.detach().clone().requires_grad_(True)
        yr = layernorm_ref(xx, w.detach(), b.detach(), eps, mode)
        dxr, = torch.autograd.grad((yr * gy).sum() + (xx * gs).sum(), [xx])
        rinv = _ln_rinv(x, eps, mode)
        tag = 'layernorm C ABI mode %d ' % mode
        check_close(tag + 'y', y.reshape(rows, n), yr.detach())
        check_close(tag + 'mean', mu, x.detach().mean(-1))
        check_close(tag + 'rinv', ri, rinv.reshape(-1))
        check_close(tag + 'dx', dx.reshape(rows, n), dxr)
        check_close(tag + 'dy_xhat', dyx.reshape(rows, n), gy * (x.detach() - x.detach().mean(-1, keepdim=True)) * rinv)
    # refusals: every pointer is valid, so it is the width that is refused; nothing is launched (dx keeps its pattern)
    DX, dx = _guarded(8)
    bwd = lambda n_, mode_: lib.gator_t_layernorm_bwd(gyd.data_ptr(), xd.data_ptr(), mu.data_ptr(), ri.data_ptr(), None, 1, n_, 1e-6, mode_, dx.data_ptr(),
                                                      None, None, _stream())
    assert bwd(0, 0) != 0 and bwd(-3, 0) != 0 and bwd(0, 1) != 0 and bwd(1, 1) != 0
    torch.cuda.synchronize()
    assert bool((DX == PATTERN).all())
    assert lib.gator_t_layernorm_fwd(xd.data_ptr(), 1, 1, None, None, 1e-6, 1, y.data_ptr(), mu.data_ptr(), ri.data_ptr(), _stream()) != 0
    assert bwd(1, 0) == 0 and bwd(2, 1) == 0                # the smallest widths each mode accepts
    torch.cuda.synchronize()


# ---- softmax -------------------------------------------------------------------------------------------------------------------
SM_NS = (1, 2, 20, 63, 64, 65, 431, 1000)


def _softmax_case(tag, x, seed, ref_x=None, noise=False):
    """ops.softmax of x (float64-held float32 values) and its dx against float64 softmax of ref_x (default: x)"""
    gy = _t(np.random.RandomState(seed).randn(*x.shape))
    xr = (x if ref_x is None else ref_x).detach().clone().requires_grad_(True)
    pr = xr.softmax(-1)
    auto, = torch.autograd.grad(pr, xr, grad_outputs=gy)
    # autograd's p (g - sum(p g)) cancels to about 1e-16 max|g| even in float64, which is the whole gradient of a row of wide logits
    # (one p nearly 1, max|dx| 1e-15).  The same derivative as dx_i = p_i sum_j p_j (g_i - g_j) has no such cancellation: that is the
    # reference, and autograd must agree with it to its own rounding.
    pp = pr.detach()
    dxr = (pp.unsqueeze(-1) * pp.unsqueeze(-2) * (gy.unsqueeze(-1) - gy.unsqueeze(-2))).sum(-1)
    assert float((auto - dxr).abs().max()) <= 1e-12 * float(gy.abs().max())
    assert bool(torch.isfinite(pr).all()) and bool(torch.isfinite(dxr).all())
    q = [None, None]
    if noise:
        x32 = x.detach().float().requires_grad_(True)
        p32 = x32.softmax(-1)
        q = [p32.detach(), torch.autograd.grad(p32, x32, grad_outputs=gy.float())[0]]
    xd = _dev(x.detach().requires_grad_(True))
    p = ops.softmax(xd)
    dx, = torch.autograd.grad(p, xd, grad_outputs=_dev(gy))
    check_close(tag + ' p', p.detach(), pr.detach(), noise32=q[0])
    check_close(tag + ' dx', dx, dxr, noise32=q[1])
    return p.detach(), dx


@pytest.mark.parametrize('rows', [1, 5])
@pytest.mark.parametrize('n', SM_NS)
def test_softmax_against_float64(n, rows):
    """standard-normal and wide (30 randn: many exponentials underflow) logits on both sides of a wave (63, 64, 65), the model's n = 20,
    and n = 1, where p is 1 and dx is 0 bit for bit"""
    rs = np.random.RandomState(100 * n + rows)
    for kind, amp in (('normal', 1.0), ('wide', 30.0)):
        p, dx = _softmax_case('softmax %s rows %d n %d' % (kind, rows, n), _t(amp * rs.randn(rows, n)), n + rows)
        if n == 1:
            assert torch.equal(p.cpu(), torch.ones(rows, 1)) and torch.equal(dx.cpu(), torch.zeros(rows, 1))


@pytest.mark.parametrize('rows', [1, 5])
@pytest.mark.parametrize('n', SM_NS)
def test_softmax_with_masked_entries(n, rows):
    """every 7th entry (i % 7 == 6) is -inf, the additive mask form: p is exactly 0 there and finite elsewhere, dx is finite, and both
    meet the criterion against float64 (whose own result is finite for this input: asserted in _softmax_case)"""
    x = _t(np.random.RandomState(200 * n + rows).randn(rows, n))
    masked = (torch.arange(n) % 7 == 6)
    x[:, masked] = float('-inf')
    assert bool(masked.any()) == (n >= 7)
    p, dx = _softmax_case('softmax -inf rows %d n %d' % (rows, n), x, n + rows)
    assert bool((p[:, masked.cuda()] == 0).all()) and bool(torch.isfinite(p).all()) and bool(torch.isfinite(dx).all())
    assert bool((p[:, ~masked.cuda()] > 0).all())


@pytest.mark.parametrize('rows', [1, 5])
@pytest.mark.parametrize('n', SM_NS)
def test_softmax_is_invariant_to_a_row_shift(n, rows):
    """x + 1e4 against x.  The logits are multiples of 1/64, so the shifted row is exact in float32 (1e4 + |x| < 2^14: spacing 2^-10) and
    the two inputs describe the same softmax; a kernel that does not subtract the row maximum overflows at exp(1e4).  Both results meet
    the criterion against each other and against the float64 softmax of the unshifted rows (noise: torch-CPU float32 on the shifted)."""
    x = _t(np.round(np.random.RandomState(300 * n + rows).randn(rows, n) * 64.0) / 64.0)
    shifted = x + 1e4
    assert torch.equal(shifted.float().double(), shifted)
    tag = 'softmax rows %d n %d ' % (rows, n)
    p0, dx0 = _softmax_case(tag + 'unshifted', x, n + rows, noise=True)
    p1, dx1 = _softmax_case(tag + 'shifted 1e4', shifted, n + rows, ref_x=x, noise=True)
    check_close(tag + 'shifted vs unshifted p', p1, p0.cpu().double())
    check_close(tag + 'shifted vs unshifted dx', dx1, dx0.cpu().double())


def test_softmax_c_abi_writes_inside_its_outputs():
    lib = _lib.load()
    rows, n = 5, 65
    rs = np.random.RandomState(31)
    x, gy = _t(rs.randn(rows, n)), _t(rs.randn(rows, n))
    (P, p), (DX, dx) = _guarded(rows * n), _guarded(rows * n)
    xd, gyd = _dev(x), _dev(gy)
    assert lib.gator_t_softmax_fwd(xd.data_ptr(), rows, n, p.data_ptr(), _stream()) == 0
    assert lib.gator_t_softmax_bwd(p.data_ptr(), gyd.data_ptr(), rows, n, dx.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert _guards_hold(P, rows * n) and _guards_hold(DX, rows * n)
    xr = x.clone().requires_grad_(True)
    pr = xr.softmax(-1)
    check_close('softmax C ABI p', p.reshape(rows, n), pr.detach())
    check_close('softmax C ABI dx', dx.reshape(rows, n), torch.autograd.grad(pr, xr, grad_outputs=gy)[0])


# ---- BatchNorm, training mode ---------------------------------------------------------------------------------------------------
def _bn_case(B, C, L, eps, momentum, seed, running=True, offset=0.0, noise=False, slots=False):
    rs = np.random.RandomState(seed)
    x = _t(rs.randn(B, C, L) + offset).requires_grad_(True)
    w, b = _t(1.0 + 0.5 * rs.randn(C)).requires_grad_(True), _t(rs.randn(C)).requires_grad_(True)
    rm, rv = (_t(rs.randn(C)), _t(0.5 + rs.rand(C))) if running else (None, None)
    gy = _t(rs.randn(B, C, L))

    def ref(dtype):
        xx, ww, bb = [t.detach().to(dtype).requires_grad_(True) for t in (x, w, b)]
        m, v = (rm.to(dtype).clone(), rv.to(dtype).clone()) if running else (None, None)
        y = F.batch_norm(xx, m, v, ww, bb, True, momentum, eps)
        return [y.detach()] + list(torch.autograd.grad(y, [xx, ww, bb], grad_outputs=gy.to(dtype))) + ([m, v] if running else [])

    want = ref(torch.float64)
    noise32 = ref(torch.float32) if noise else [None] * len(want)
    xd, wd, bd = _dev(x), _dev(w), _dev(b)
    md, vd = (rm.float().cuda(), rv.float().cuda()) if running else (None, None)
    wslot, bslot = (_slot(wd), _slot(bd)) if slots else (None, None)
    y = ops.batchnorm_train(xd, wd, bd, md, vd, eps, momentum)
    got = list(torch.autograd.grad(y, [xd, wd, bd], grad_outputs=_dev(gy)))
    if slots:
        assert got[1].data_ptr() == wslot.data_ptr() and got[2].data_ptr() == bslot.data_ptr()
        got[1], got[2] = wslot, bslot
    scales = {}
    if (B, C, L) == (2, 1, 1):
        # two values in the channel: the same cancellation as LayerNorm at n = 2 (torch-CPU float32 is 1.4e-4 of max|dx| off); the scale
        # is the size of the terms that cancel, max |w rinv dy| of the float64 reference
        xv = x.detach()
        rinv = 1.0 / torch.sqrt(xv.var((0, 2), unbiased=False, keepdim=True) + eps)
        scales['dx'] = float((w.detach().reshape(1, C, 1) * rinv * gy).abs().max())
    tag = 'batchnorm (%d,%d,%d) eps %g momentum %g%s%s ' % (B, C, L, eps, momentum, ' mean %g' % offset if offset else '', ' slots' if slots else '')
    names = ['y', 'dx', 'dw', 'db'] + (['run_mean', 'run_var'] if running else [])
    for nm, a, r, q in zip(names, [y.detach()] + got + ([md, vd] if running else []), want, noise32):
        if noise:
            bound, scale = close_bound(r, noise32=q, scale=scales.get(nm))
            assert bound <= 1e-3 * scale, '%s%s: bound %.3e above 1e-3 of the scale %.3e' % (tag, nm, bound, scale)
        check_close(tag + nm, a, r, noise32=q, scale=scales.get(nm))


@pytest.mark.parametrize('B,C,L,eps,momentum', [(2, 1, 1, 1e-3, 0.3), (1, 3, 2, 1e-3, 0.3), (100, 5, 3, 1e-5, 0.1), (256, 2, 1, 1e-3, 0.3),
                                                (257, 2, 1, 1e-5, 0.1), (3, 2, 100, 1e-3, 0.3), (9, 431, 3, 1e-5, 0.1)])
def test_batchnorm_train_against_float64(B, C, L, eps, momentum):
    """F.batch_norm(training=True) in float64: y, dx, dw, db and both running statistics.  B L = 2 (a factor of 2 between the unbiased
    and the biased running variance), exactly and just over one pass of the 256 threads, L below and above B, the model's (., 431, 3)."""
    _bn_case(B, C, L, eps, momentum, 37 + B)


def test_batchnorm_train_without_running_statistics_and_with_gradient_slots():
    _bn_case(100, 5, 3, 1e-3, 0.3, 41, running=False)
    _bn_case(3, 2, 100, 1e-5, 0.1, 42, slots=True)


def test_batchnorm_train_with_a_mean_far_above_the_spread():
    """x = 1e3 + randn at (100, 5, 3), noise from torch-CPU float32, the whole bound capped at 1e-3 of the scale"""
    _bn_case(100, 5, 3, 1e-5, 0.1, 43, offset=1e3, noise=True)


def test_batchnorm_train_refuses_one_value_per_channel():
    """B L = 1: no variance to normalise by and no unbiased one for run_var.  torch raises; so does the library, before it writes."""
    x = torch.randn(1, 3, 1, device='cuda', requires_grad=True)
    w, b = torch.ones(3, device='cuda', requires_grad=True), torch.zeros(3, device='cuda', requires_grad=True)
    rm, rv = torch.randn(3, device='cuda'), torch.rand(3, device='cuda') + 0.5
    rm0, rv0 = rm.clone(), rv.clone()
    with pytest.raises(ValueError):
        F.batch_norm(x.detach().cpu(), rm0.cpu(), rv0.cpu(), None, None, True)
    with pytest.raises(RuntimeError, match='gator_t_batchnorm_fwd'):
        ops.batchnorm_train(x, w, b, rm, rv)
    torch.cuda.synchronize()
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)


# ---- MGCN ----------------------------------------------------------------------------------------------------------------------
def _mgcn_case(B, J, C, seed, slots=False):
    rs = np.random.RandomState(seed)
    ins = [_t(rs.randn(*s)).requires_grad_(True) for s in ((B, J, C), (B, J, C), (J, J), (J, C), (C,))]         # h0, h1, adj (not symmetric), M, bias
    gy = _t(rs.randn(B, J, C))
    want = mgcn_ref(*ins)
    gw = torch.autograd.grad(want, ins, grad_outputs=gy)
    dev = [_dev(t) for t in ins]
    mslot, bslot = (_slot(dev[3]), _slot(dev[4])) if slots else (None, None)
    out = ops.mgcn(*dev)
    got = list(torch.autograd.grad(out, dev, grad_outputs=_dev(gy)))
    if slots:
        assert got[3].data_ptr() == mslot.data_ptr() and got[4].data_ptr() == bslot.data_ptr()
        ops.Deferred.flush(out.device)
        got[3], got[4] = mslot, bslot
    tag = 'mgcn (%d,%d,%d)%s ' % (B, J, C, ' slots' if slots else '')
    check_close(tag + 'out', out.detach(), want.detach())
    for nm, a, r in zip(('dh0', 'dh1', 'dadj', 'dM', 'dbias'), got, gw):
        check_close(tag + nm, a, r)
    if J == 1:
        assert float(gw[1].abs().max()) == 0.0 and torch.equal(got[1].cpu(), torch.zeros(B, 1, C))         # no off-diagonal entry: dh1 is exactly 0


@pytest.mark.parametrize('B,J,C', [(1, 1, 1), (2, 2, 3), (3, 17, 128), (2, 19, 65), (2, 32, 64), (5, 3, 300)])
def test_mgcn_against_float64(B, J, C):
    """out and all five gradients against the formula of include/gator_train.h in float64 with a non-symmetric adj (a transposed read
    shows).  d adj runs one wave per entry over c += 64: C = 1, 3 (most lanes idle), 64, 65, 128, 300; J C above and below one workgroup."""
    _mgcn_case(B, J, C, 47 + J)


def test_mgcn_weight_gradients_land_in_their_slots():
    _mgcn_case(2, 19, 65, 53, slots=True)


# ---- gator_t_add_n and the fork backward ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 3, 1025, 16384 * 256 + 5])
def test_add_n_equals_the_left_to_right_float32_sum_bit_for_bit(n):
    """2, 3 and 4 operands; the last size is past the 16384-workgroup grid (the grid-stride loop).  The build contracts nothing and has no
    fast-math, so ((a + b) + c) + d in numpy float32 is the exact answer.  The output's tail keeps its pattern."""
    lib = _lib.load()
    rs = np.random.RandomState(n % 1000)
    host = [(rs.randn(n) * 10.0 ** k).astype(np.float32) for k in (0, 1, -1, 2)]
    dev = [torch.from_numpy(h).cuda() for h in host]
    for k in (2, 3, 4):
        whole, out = _guarded(n)
        ptr = [d.data_ptr() for d in dev[:k]] + [None] * (4 - k)
        assert lib.gator_t_add_n(ptr[0], ptr[1], ptr[2], ptr[3], out.data_ptr(), n, _stream()) == 0
        torch.cuda.synchronize()
        want = host[0] + host[1]
        for h in host[2:k]:
            want = want + h
        assert want.dtype == np.float32 and np.array_equal(out.cpu().numpy(), want), k
        assert _guards_hold(whole, n)
    assert lib.gator_t_add_n(dev[0].data_ptr(), dev[1].data_ptr(), None, dev[3].data_ptr(), out.data_ptr(), n, _stream()) != 0     # d without c


@pytest.mark.parametrize('k,unused', [(2, None), (3, None), (4, None), (5, None), (6, None), (4, 2)])
def test_fork_sums_the_gradients_of_its_aliases(k, unused):
    """each alias of x is multiplied by its own tensor; dx = sum_i r_i g_i in float64.  k = 5 fills one four-operand launch, k = 6 needs a
    second; an alias that is never used contributes nothing (and no zero-filled gradient is made for it)."""
    rs = np.random.RandomState(60 + k)
    shape = (3, 5, 71)
    x = _dev(_t(rs.randn(*shape)).requires_grad_(True))
    r, g = [_t(rs.randn(*shape)) for _ in range(k)], [_t(rs.randn(*shape)) for _ in range(k)]
    used = [i for i in range(k) if i != unused]
    aliases = ops.fork(x, k)
    assert all(torch.equal(a.detach(), x.detach()) for a in aliases)
    outs = [ops.mul(aliases[i], _dev(r[i])) for i in used]
    dx, = torch.autograd.grad(outs, [x], grad_outputs=[_dev(g[i]) for i in used])
    check_close('fork k %d%s dx' % (k, '' if unused is None else ' (alias %d unused)' % unused), dx, sum(r[i] * g[i] for i in used))
