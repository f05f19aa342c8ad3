"""k_t_gemm at its edges against float64: every M, N on and around the 64-wide tile edge times every K on and around the 32-deep
step, both load layouts per operand, bias / alpha / accumulate, the a_rowsum side output with several column tiles, stride-0 batches,
K = 0, explicit split-K (with slices that have nothing to do) through the raw entry point, the grouped form with split and unsplit
problems mixed, and the argument checks the host code makes before any launch.

Reference: alpha * (A.double() @ B.double()) + bias (+ the prior C).  Criterion: 2e-5 * max|ref| for K <= 512 (the suite's float32
criterion); for longer K the same product in torch-CPU float32 sets the noise: |ours - ref64| <= 4 |torch32 - ref64| + 2e-5 max|ref|."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from gator_amd import _lib
from gator_amd.train import ops
from tests.train_refs import check_close

pytestmark = pytest.mark.gpu

_I64x2 = ctypes.c_int64 * 2
LONG_K = 512


def _rand(rs, *shape):
    return torch.from_numpy(rs.randn(*shape).astype(np.float32))


def _operand(rs, rows, cols, transposed):
    """float32 CPU [rows, cols]: dense, or the transposed view of a dense [cols, rows]"""
    return _rand(rs, cols, rows).t() if transposed else _rand(rs, rows, cols)


def _dev(t):
    """the same values AND strides on the device"""
    base = torch.empty(t.untyped_storage().size() // 4 if t.numel() else 1, dtype=torch.float32, device='cuda')
    d = torch.as_strided(base, t.shape, t.stride())
    d.copy_(t)
    return d


def _ref(A, B, bias, alpha, prior, dtype=torch.float64):
    r = alpha * (A.to(dtype) @ B.to(dtype))
    if bias is not None:
        r = r + bias.to(dtype)
    if prior is not None:
        r = r + prior.to(dtype)
    return r


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _raw_gemm(A, B, C, M, N, K, sa, sb, bias=None, alpha=1.0, accumulate=0, ksplit=1, ws=None, rowsum=None, nb=(1, 1), ba=(0, 0), bb=(0, 0), bc=(0, 0)):
    """gator_t_gemm with explicit sizes; every pointer is a live device tensor.  Returns the return code."""
    lib = _lib.load()
    ptr = lambda t: t.data_ptr() if t is not None else None
    return lib.gator_t_gemm(ptr(A), ptr(B), ptr(C), M, N, K, _I64x2(*sa), _I64x2(*sb), _I64x2(C.stride(-2), C.stride(-1)), nb[0], nb[1], _I64x2(*ba), _I64x2(*bb),
                            _I64x2(*bc), ptr(bias), float(alpha), int(accumulate), int(ksplit), ptr(ws), ptr(rowsum), _stream())


@pytest.mark.parametrize('M', [1, 63, 64, 65])
@pytest.mark.parametrize('N', [1, 63, 64, 65])
def test_gemm_tile_edges_all_layouts(M, N):
    rs = np.random.RandomState(1000 * M + N)
    worst = 0.0
    for K in (1, 31, 32, 33, 64, 97):
        for ta, tb in itertools.product((False, True), repeat=2):
            A, B = _operand(rs, M, K, ta), _operand(rs, K, N, tb)
            Ad, Bd = _dev(A), _dev(B)
            assert Ad.stride() == A.stride() and Bd.stride() == B.stride()
            for with_bias, acc in itertools.product((False, True), repeat=2):
                bias = _rand(rs, N) if with_bias else None
                prior = _rand(rs, M, N)
                out = prior.cuda().reshape(1, 1, M, N)
                got = ops.raw_gemm(Ad[None, None], Bd[None, None], out=out, bias=bias.cuda() if with_bias else None, alpha=-0.5, accumulate=acc)
                assert got.data_ptr() == out.data_ptr()
                want = _ref(A, B, bias, -0.5, prior if acc else None)
                worst = max(worst, check_close('gemm %dx%dx%d ta%d tb%d bias%d acc%d' % (M, N, K, ta, tb, with_bias, acc), got[0, 0], want, verbose=False))
    print('gemm M=%d N=%d: worst |ours - ref64| %.3e over K, layouts, bias, accumulate' % (M, N, worst))


@pytest.mark.parametrize('N', [65, 130])
def test_gemm_rowsum_with_several_column_tiles(N):
    """only the first column tile may write a_rowsum[m] = alpha * sum_k A[m][k]; the buffer is overwritten, not accumulated"""
    rs = np.random.RandomState(N)
    for M, K, ta in itertools.product((1, 63, 64, 65, 130), (1, 33, 97), (False, True)):
        A, B = _operand(rs, M, K, ta), _operand(rs, K, N, False)
        rowsum = torch.full((M,), 7.0, device='cuda')
        got = ops.raw_gemm(_dev(A)[None, None], _dev(B)[None, None], alpha=-0.5, a_rowsum=rowsum)
        tag = 'rowsum %dx%dx%d ta%d' % (M, N, K, ta)
        check_close(tag + ' C', got[0, 0], _ref(A, B, None, -0.5, None), verbose=False)
        check_close(tag + ' a_rowsum', rowsum, -0.5 * A.double().sum(1), verbose=False)


def test_gemm_batched_with_stride_zero_operands():
    rs = np.random.RandomState(3)
    M, N, K = 65, 63, 33
    for which in ('A', 'B'):
        A = _rand(rs, 1 if which == 'A' else 3, 2, M, K)
        B = _rand(rs, 3, 2 if which == 'A' else 1, K, N)
        Ae, Be = A.cuda().expand(3, 2, M, K), B.cuda().expand(3, 2, K, N)
        assert (Ae.stride(0) == 0) == (which == 'A') and (Be.stride(1) == 0) == (which == 'B')
        bias = _rand(rs, N)
        prior = _rand(rs, 3, 2, M, N)
        got = ops.raw_gemm(Ae, Be, out=prior.cuda(), bias=bias.cuda(), alpha=-0.5, accumulate=True)
        check_close('batched 3x2, stride 0 on ' + which, got, _ref(A.expand(3, 2, M, K), B.expand(3, 2, K, N), bias, -0.5, prior))


@pytest.mark.parametrize('acc', [0, 1])
def test_gemm_with_k_zero_gives_the_bias(acc):
    """the header allows K >= 0: C = bias (+ C).  A and B point at real allocations (torch reports a null data_ptr() for an empty
    tensor, and the entry point rejects null)."""
    rs = np.random.RandomState(9)
    M, N = 65, 33
    A, B = torch.ones(M, 1, device='cuda'), torch.ones(1, N, device='cuda')
    bias, prior = _rand(rs, N), _rand(rs, M, N)
    C = prior.cuda()
    rowsum = torch.full((M,), 7.0, device='cuda')
    assert _raw_gemm(A, B, C, M, N, 0, (1, 1), (N, 1), bias=bias.cuda(), alpha=-0.5, accumulate=acc, rowsum=rowsum) == 0
    torch.cuda.synchronize()
    want = bias.double().expand(M, N) + (prior.double() if acc else 0)
    assert torch.equal(C.cpu().double(), want.float().double())
    assert float(rowsum.abs().max()) == 0.0
    C2 = prior.cuda()
    assert _raw_gemm(A, B, C2, M, N, 0, (1, 1), (N, 1), accumulate=acc) == 0          # no bias: zeros, or C unchanged
    assert torch.equal(C2.cpu(), prior if acc else torch.zeros(M, N))


SPLIT_CASES = [(48, 64, 6000, 46), (70, 33, 1000, 2), (5, 5, 40, 4), (64, 64, 4096, 64), (65, 130, 777, 5), (48, 64, 6000, 1), (64, 64, 4096, 1)]


@pytest.mark.parametrize('M,N,K,ksplit', SPLIT_CASES)
def test_gemm_explicit_split_k(M, N, K, ksplit):
    """ksplit chosen by the caller, workspace ksplit * (M N + M) floats as the header states.  kper is rounded up to 32, so
    (5, 5, 40, 4) leaves two slices with nothing to do; the long K also run unsplit (ksplit = 1)."""
    rs = np.random.RandomState(K + ksplit)
    for transposed, with_rowsum in itertools.product((False, True), repeat=2):
        A, B = _operand(rs, M, K, transposed), _operand(rs, K, N, transposed)
        bias, prior = _rand(rs, N), _rand(rs, M, N)
        Ad, Bd, C = _dev(A), _dev(B), prior.cuda()
        ws = torch.full((ksplit * (M * N + M),), float('nan'), device='cuda') if ksplit > 1 else None
        rowsum = torch.full((M,), 7.0, device='cuda') if with_rowsum else None
        rc = _raw_gemm(Ad, Bd, C, M, N, K, A.stride(), B.stride(), bias=bias.cuda(), alpha=-0.5, accumulate=1, ksplit=ksplit, ws=ws, rowsum=rowsum)
        assert rc == 0, _lib.load().gator_last_error()
        torch.cuda.synchronize()
        long_k = K > LONG_K
        tag = 'split-K %dx%dx%d / %d transposed %d rowsum %d' % (M, N, K, ksplit, transposed, with_rowsum)
        check_close(tag + ' C', C, _ref(A, B, bias, -0.5, prior), noise32=_ref(A, B, bias, -0.5, prior, torch.float32) if long_k else None)
        if with_rowsum:
            check_close(tag + ' a_rowsum', rowsum, -0.5 * A.double().sum(1), noise32=-0.5 * A.contiguous().sum(1) if long_k else None)


def _problem(p, A, B, C, rowsum, bias, ksplit, alpha, accumulate):
    p.A, p.B, p.C = A.data_ptr(), B.data_ptr(), C.data_ptr()
    p.a_rowsum = rowsum.data_ptr() if rowsum is not None else None
    p.bias = bias.data_ptr() if bias is not None else None
    p.M, p.K, p.N, p.ksplit = A.shape[0], A.shape[1], B.shape[1], ksplit
    p.stride_a[0], p.stride_a[1] = A.stride()
    p.stride_b[0], p.stride_b[1] = B.stride()
    p.stride_c[0], p.stride_c[1] = C.stride()
    p.alpha, p.accumulate = alpha, accumulate


def test_grouped_gemm_mixes_split_and_unsplit_problems():
    lib = _lib.load()
    assert lib.gator_t_struct_size(0) == ctypes.sizeof(_lib.GemmProblem)
    rs = np.random.RandomState(21)
    #        M    N    K    ksplit rowsum bias  acc alpha  ta     tb
    spec = [(70, 33, 1000, 4, True, True, 0, 1.0, True, False),
            (1, 1, 1, 1, False, False, 0, 1.0, False, False),
            (65, 130, 97, 1, True, False, 1, -0.5, False, False),
            (48, 64, 6000, 46, False, True, 1, 0.5, True, False),
            (5, 5, 40, 4, True, False, 0, 1.0, False, True),
            (64, 64, 32, 1, False, True, 0, 2.0, False, True)]
    n = len(spec)
    arr = (_lib.GemmProblem * n)()
    host, dev = [], []
    for p, (M, N, K, ks, rsum, wb, acc, alpha, ta, tb) in zip(arr, spec):
        A, B = _operand(rs, M, K, ta), _operand(rs, K, N, tb)
        bias, prior = (_rand(rs, N) if wb else None), _rand(rs, M, N)
        d = (_dev(A), _dev(B), prior.cuda(), torch.full((M,), 7.0, device='cuda') if rsum else None, bias.cuda() if wb else None)
        _problem(p, d[0], d[1], d[2], d[3], d[4], ks, alpha, acc)
        host.append((A, B, bias, prior))
        dev.append(d)
    ws_floats = int(lib.gator_t_gemm_grouped_prepare(arr, n))
    assert ws_floats == sum(ks * (M * N + M) for (M, N, K, ks, *_) in spec if ks > 1)
    assert arr[0].total_wgs == sum(((M + 63) // 64) * ((N + 63) // 64) * ks for (M, N, K, ks, *_) in spec)
    ws = torch.full((ws_floats,), float('nan'), device='cuda')
    table = torch.empty(n * ctypes.sizeof(_lib.GemmProblem), device='cuda', dtype=torch.uint8)
    _lib.check(lib.gator_t_gemm_grouped(arr, n, table.data_ptr(), ws.data_ptr(), _stream()), 'gator_t_gemm_grouped')
    torch.cuda.synchronize()                                   # `arr` (the host table) is alive until here, as the header requires
    for i, ((M, N, K, ks, rsum, wb, acc, alpha, ta, tb), (A, B, bias, prior), d) in enumerate(zip(spec, host, dev)):
        long_k = K > LONG_K
        tag = 'grouped #%d %dx%dx%d / %d' % (i, M, N, K, ks)
        check_close(tag + ' C', d[2], _ref(A, B, bias, alpha, prior if acc else None),
                    noise32=_ref(A, B, bias, alpha, prior if acc else None, torch.float32) if long_k else None)
        if rsum:
            check_close(tag + ' a_rowsum', d[3], alpha * A.double().sum(1), noise32=alpha * A.contiguous().sum(1) if long_k else None)
    del arr


def test_gemm_argument_checks_return_before_any_launch():
    """Each of these returns non-zero from the host checks at the top of gator_t_gemm / gator_t_gemm_grouped(_prepare), before
    hipLaunchKernelGGL, with a message in gator_last_error().  Every pointer is a real allocation that would cover the call."""
    lib = _lib.load()
    M = N = K = 4
    A, B, C = torch.ones(2, 2, M, K, device='cuda'), torch.ones(2, 2, K, N, device='cuda'), torch.zeros(2, 2, M, N, device='cuda')
    ws, rowsum = torch.zeros(4 * (M * N + M), device='cuda'), torch.zeros(M, device='cuda')
    sa, sb = (K, 1), (N, 1)
    bstr = dict(ba=(2 * M * K, M * K), bb=(2 * K * N, K * N), bc=(2 * M * N, M * N))

    def rejected(rc, word):
        msg = lib.gator_last_error().decode()
        assert rc != 0 and word in msg, (rc, msg)

    rejected(_raw_gemm(A, B, C, M, N, K, sa, sb, rowsum=rowsum, nb=(2, 2), **bstr), 'a_rowsum')
    rejected(_raw_gemm(A, B, C, M, N, K, sa, sb, ksplit=2, ws=None), 'split-K')
    rejected(_raw_gemm(A, B, C, M, N, K, sa, sb, ksplit=2, ws=ws, nb=(2, 2), **bstr), 'split-K')
    rejected(_raw_gemm(A, B, C, 1, 1, 1, (1, 1), (1, 1), nb=(256, 256)), '65535')              # batch strides 0: one product's memory covers it
    rejected(_raw_gemm(A, B, C, 0, N, K, sa, sb), 'bad argument')
    arr = (_lib.GemmProblem * 1)()
    _problem(arr[0], A[0, 0], B[0, 0], C[0, 0], None, None, 1, 1.0, 0)
    table = torch.empty(ctypes.sizeof(_lib.GemmProblem), device='cuda', dtype=torch.uint8)
    rejected(lib.gator_t_gemm_grouped(arr, 1, table.data_ptr(), ws.data_ptr(), _stream()), 'prepare')       # never prepared: total_wgs == 0
    arr[0].ksplit = 0
    assert lib.gator_t_gemm_grouped_prepare(arr, 1) == -1
    torch.cuda.synchronize()
    assert float(C.abs().max()) == 0.0                         # nothing ran
    assert _raw_gemm(A, B, C, M, N, K, sa, sb) == 0            # and the entry point still works afterwards
    torch.cuda.synchronize()
    assert torch.equal(C[0, 0].cpu(), torch.full((M, N), float(K))) and float(C[1].abs().max()) == 0.0
