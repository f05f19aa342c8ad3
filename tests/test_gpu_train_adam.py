"""gator_t_adam on plain device buffers, through the C ABI, against torch.optim.Adam and the one-step rule of tests/train_refs.py in
float64.  Every run starts from p = 0, so max|p| is the size of the movement and 2e-5 of it is a bound on the update rule itself
(the trainer test of tests/test_gpu_train_step.py moves weights of size 1 by 6e-6 and allows 2.4e-7: a few percent of the step)."""
import ctypes

import numpy as np
import pytest
import torch

from gator_amd import _lib
from tests.train_refs import adam_step_ref, check_close

pytestmark = pytest.mark.gpu

GRID_LIMIT = 16384 * 256                                   # elements one pass of the largest grid covers: beyond it the grid-stride loop runs
MAGNITUDES = (1.0, 0.0, 1e-6, 1e-3, 1e3)                   # of element i % 5: gradients of every size in one buffer, and none at all


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).float().double()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _adam(p, g, m, v, lr, b1, b2, eps, step, counter=None):
    return _lib.load().gator_t_adam(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, b1, b2, eps, step,
                                    counter.data_ptr() if counter is not None else None, _stream())


def _state(n, seed):
    """a random optimiser state (p = 0, m, v > 0) and one gradient, float32 values in float64"""
    rs = np.random.RandomState(seed)
    return torch.zeros(n, dtype=torch.float64), _t(rs.randn(n)), _t(0.1 * rs.randn(n)), _t(0.01 + 0.1 * rs.rand(n))


@pytest.mark.parametrize('n', [1, 3, 5, 1023, 1025])
def test_twenty_steps_follow_torch_adam(n):
    """lr 1e-3, default betas, gradients redrawn every step with a fixed per-element magnitude in {1, 0, 1e-6, 1e-3, 1e3}; the same run
    of torch.optim.Adam in float32 on the CPU is the noise.  An element that never sees a gradient stays exactly 0."""
    rs = np.random.RandomState(70 + n)
    mag = np.array(MAGNITUDES)[np.arange(n) % 5]
    grads = [_t(mag * rs.randn(n)) for _ in range(20)]
    runs = {}
    for dtype in (torch.float64, torch.float32):
        p = torch.zeros(n, dtype=dtype, requires_grad=True)
        opt = torch.optim.Adam([p], lr=1e-3)
        for g in grads:
            p.grad = g.to(dtype)
            opt.step()
        runs[dtype] = (p.detach(), opt.state[p]['exp_avg'], opt.state[p]['exp_avg_sq'])
    pd, md, vd = [torch.zeros(n, device='cuda') for _ in range(3)]
    for t, g in enumerate(grads, 1):
        assert _adam(pd, g.float().cuda(), md, vd, 1e-3, 0.9, 0.999, 1e-8, t) == 0
    for nm, a, r, q in zip(('p', 'exp_avg', 'exp_avg_sq'), (pd, md, vd), runs[torch.float64], runs[torch.float32]):
        check_close('adam 20 steps n %d %s' % (n, nm), a, r, noise32=q)
    still = torch.from_numpy(mag == 0.0)
    for a in (pd, md, vd):
        assert bool((a.cpu()[still] == 0).all())
    assert n == 1 or bool(still.any())


@pytest.mark.parametrize('counter', [False, True], ids=['host step', 'device counter'])
@pytest.mark.parametrize('step', [1, 2, 10, 1000, 100000])
def test_single_step_from_a_random_state(step, counter):
    """One step at `step` against adam_step_ref.  With a device counter the host passes step = 1 and the kernel forms the bias
    corrections of the counter's value itself; the counter is only read."""
    n = 1025
    p, g, m, v = _state(n, 80 + step)
    want = adam_step_ref(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, step)
    pd, gd, md, vd = [t.float().cuda() for t in (p, g, m, v)]
    cnt = torch.tensor([step], dtype=torch.int64, device='cuda') if counter else None      # the bits of a uint64
    assert _adam(pd, gd, md, vd, 1e-3, 0.9, 0.999, 1e-8, 1 if counter else step, cnt) == 0
    for nm, a, r in zip(('p', 'exp_avg', 'exp_avg_sq'), (pd, md, vd), want):
        check_close('adam step %d%s %s' % (step, ' (device counter)' if counter else '', nm), a, r)
    assert cnt is None or int(cnt.item()) == step


@pytest.mark.parametrize('counter', [False, True], ids=['host step', 'device counter'])
def test_single_step_with_other_hyperparameters(counter):
    n, step, lr, b1, b2, eps = 1025, 7, 3e-2, 0.8, 0.99, 1e-6
    p, g, m, v = _state(n, 90)
    mag = torch.from_numpy(np.array(MAGNITUDES)[np.arange(n) % 5])
    g, m, v = [(t * mag ** k).float().double() for t, k in ((g, 1), (m, 1), (v, 2))]        # eps = 1e-6 decides the step where |g| is 1e-6
    want = adam_step_ref(p, g, m, v, lr, b1, b2, eps, step)
    pd, gd, md, vd = [t.float().cuda() for t in (p, g, m, v)]
    cnt = torch.tensor([step], dtype=torch.int64, device='cuda') if counter else None
    assert _adam(pd, gd, md, vd, lr, b1, b2, eps, 1 if counter else step, cnt) == 0
    for nm, a, r in zip(('p', 'exp_avg', 'exp_avg_sq'), (pd, md, vd), want):
        check_close('adam lr %g betas (%g, %g) eps %g%s %s' % (lr, b1, b2, eps, ' (device counter)' if counter else '', nm), a, r)
    assert cnt is None or int(cnt.item()) == step


def test_single_step_past_the_largest_grid():
    """n = 16384 * 256 + 5: the last five elements belong to the second trip of the grid-stride loop.  They, and the first of them alone,
    are checked on their own scale as well as within the whole buffer."""
    n = GRID_LIMIT + 5
    p, g, m, v = _state(n, 95)
    want = adam_step_ref(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 3)
    pd, gd, md, vd = [t.float().cuda() for t in (p, g, m, v)]
    assert _adam(pd, gd, md, vd, 1e-3, 0.9, 0.999, 1e-8, 3) == 0
    for nm, a, r in zip(('p', 'exp_avg', 'exp_avg_sq'), (pd, md, vd), want):
        check_close('adam grid-stride %s' % nm, a, r)
        check_close('adam grid-stride %s tail' % nm, a[GRID_LIMIT:], r[GRID_LIMIT:])
        check_close('adam grid-stride %s element 16384 * 256' % nm, a[GRID_LIMIT:GRID_LIMIT + 1], r[GRID_LIMIT:GRID_LIMIT + 1])
        check_close('adam grid-stride %s last of the first trip' % nm, a[GRID_LIMIT - 1:GRID_LIMIT], r[GRID_LIMIT - 1:GRID_LIMIT])


def test_bad_arguments_are_refused_before_any_launch():
    p, g, m, v = [t.float().cuda() for t in _state(5, 99)]
    keep = [t.clone() for t in (p, m, v)]
    lib = _lib.load()
    args = (5, 1e-3, 0.9, 0.999, 1e-8)
    assert lib.gator_t_adam(None, g.data_ptr(), m.data_ptr(), v.data_ptr(), *args, 1, None, _stream()) != 0
    assert lib.gator_t_adam(p.data_ptr(), None, m.data_ptr(), v.data_ptr(), *args, 1, None, _stream()) != 0
    assert lib.gator_t_adam(p.data_ptr(), g.data_ptr(), None, v.data_ptr(), *args, 1, None, _stream()) != 0
    assert lib.gator_t_adam(p.data_ptr(), g.data_ptr(), m.data_ptr(), None, *args, 1, None, _stream()) != 0
    assert _adam(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 0) != 0                   # step 0 has no bias correction (1 - beta^0 = 0) ...
    assert _adam(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, -2) != 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((p, m, v), keep))
    assert _adam(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 1) == 0                   # ... and the same buffers at step 1 are accepted
    torch.cuda.synchronize()
    assert not torch.equal(p, keep[0])
