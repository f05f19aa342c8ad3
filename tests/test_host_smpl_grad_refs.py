"""The references of the SMPL backward tests without a GPU: the torch float64 restatement (tests/smpl_grad_refs.py) against the numpy
one, its VJP against central differences, the golden file (tests/golden/smpl_layer_grad.npz, the real layer's fp32 autograd) against
the VJP, and the host-side argument checks of gator_smpl_backward_f32."""
import ctypes
import json

import numpy as np
import pytest
import torch

from gator_amd import _lib
from tests import smpl_grad_refs as gr
from tests import smpl_refs as sr
from tests.helpers import load_golden

EPS = 2.0 ** -52


@pytest.mark.parametrize('name', ['nv65', 'families', 'no_betas_no_trans', 'center0', 'center23', 'scale1000', 'dense', 'nb0'])
def test_the_torch_restatement_is_the_numpy_one(name):
    """Both are float64 and sum in different orders: the longest sums have 207 + 10 (blend shapes) and 24 (skinning) terms of the
    outputs' magnitude, so 1000 roundings of the largest output bound the difference with room to spare."""
    o = gr.case_options(name)
    m = sr.synthetic_model(*sr.CASES[name][0])
    args = tuple(None if a is None else a[:16] for a in gr.case_arguments(name))
    v, j = sr.lbs_forward(m, *args, o['center_idx'], o['out_scale'])
    with torch.no_grad():
        tv, tj = gr.lbs_forward64(m, *(None if a is None else torch.from_numpy(a.astype(np.float64)) for a in args), o['center_idx'], o['out_scale'])
    tol = 1000 * EPS * max(np.abs(v).max(), np.abs(j).max())
    assert np.abs(tv.numpy() - v).max() <= tol and np.abs(tj.numpy() - j).max() <= tol


def _objective(m, o, args, gV, gJ):
    """Per sample: sum(verts * gV) + sum(joints * gJ), and the sum of the terms' magnitudes."""
    with torch.no_grad():
        v, j = gr.lbs_forward64(m, *(None if a is None else torch.from_numpy(a) for a in args), o['center_idx'], o['out_scale'])
    tv, tj = v.numpy() * gV, j.numpy() * gJ
    return tv.sum((1, 2)) + tj.sum((1, 2)), np.abs(tv).sum((1, 2)) + np.abs(tj).sum((1, 2))


@pytest.mark.parametrize('name,B', [('nv65', 8), ('families', len(sr.FAMILIES)), ('center23', 4)])
def test_vjp_against_central_differences(name, B):
    """Along random unit directions d of a sample's whole input, (f(x + h d) - f(x - h d)) / 2h against <vjp, d>, per sample.
    f = sum of the outputs times the upstream gradients; S = the sum of its terms' magnitudes.  With h = 1e-5:
      rounding    each f carries at most ~1000 eps S (the sums above), so the quotient 1000 eps S / h = 2.2e-8 S;
      truncation  h^2 / 6 |f'''|; f is a trigonometric polynomial in the pose along a chain of up to 9 joints plus the pose blend
                  shapes, so |f'''| <= 10^3 S along a unit direction: 1.7e-8 S.
    The directional derivative itself is of the order S, so this pins the VJP to ~4e-8 relative.  The 'families' samples put the
    zero pose (finite only through the `+ 1e-8`), exact pi and 5 rad under the same bound."""
    h = 1e-5
    o = gr.case_options(name)
    m = sr.synthetic_model(*sr.CASES[name][0])
    args = tuple(None if a is None else a[:B].astype(np.float64) for a in gr.case_arguments(name))
    gV, gJ = (g[:B].astype(np.float64) for g in gr.upstream(name))
    g = gr.vjp64(m, args, o, gV, gJ)
    rs = np.random.RandomState(5)
    for _ in range(3):
        d = [None if a is None else rs.randn(*a.shape) for a in args]
        norm = np.sqrt(sum((x ** 2).sum(1) for x in d if x is not None))
        d = [None if x is None else x / norm[:, None] for x in d]
        fp, S = _objective(m, o, tuple(None if a is None else a + h * x for a, x in zip(args, d)), gV, gJ)
        fm, _ = _objective(m, o, tuple(None if a is None else a - h * x for a, x in zip(args, d)), gV, gJ)
        numeric = (fp - fm) / (2 * h)
        analytic = sum((g[k] * x).sum(1) for k, x in zip(gr.OUTPUTS, d) if x is not None)
        tol = (1000 * EPS / h + h * h / 6 * 1e3) * S
        print('central differences %-10s max |numeric - analytic| / S %.2e (bound %.2e), |analytic| / S %.2e'
              % (name, (np.abs(numeric - analytic) / S).max(), (tol / S).max(), (np.abs(analytic) / S).min()))
        assert np.isfinite(analytic).all()
        assert (np.abs(numeric - analytic) <= tol).all()


@pytest.mark.parametrize('name', sorted(sr.CASES))
def test_golden_rows_lie_within_their_spreads(name):
    """The stored fp32 gradients of the real layer against the float64 VJP on the same samples, within the spread recorded over all 65;
    the spreads are a few roundings of the largest gradient, as an fp32 autograd's error should be."""
    z = load_golden('smpl_layer_grad')
    meta = json.loads(str(z['meta']))
    assert sorted(meta) == sorted(sr.CASES)
    o = gr.case_options(name)
    assert meta[name]['model'] == list(sr.CASES[name][0]) and meta[name]['stored'] == min(4, o['keep'])
    k = meta[name]['stored']
    m = sr.synthetic_model(*sr.CASES[name][0])
    args = tuple(None if a is None else a[:k] for a in gr.case_arguments(name))
    gV, gJ = (g[:k] for g in gr.upstream(name))
    g = gr.vjp64(m, args, o, gV, gJ)
    spread = z[name + '.spread.full']
    for i, key in enumerate(gr.OUTPUTS):
        if g[key] is None:
            assert spread[i] == 0 and '%s.g_%s32' % (name, key) not in z.files
            continue
        stored = z['%s.g_%s32' % (name, key)]
        assert stored.dtype == np.float32 and stored.shape == g[key].shape
        assert np.abs(stored - g[key]).max() <= spread[i] * (1 + 1e-6)
        if name != 'nv1':                      # one vertex: sums of one term, and joints that do not move with the pose
            assert 2e-8 * np.abs(g[key]).max() < spread[i] < 2e-6 * np.abs(g[key]).max()
    for which in ('verts', 'joints'):
        assert z['%s.spread.%s' % (name, which)].shape == (3,)


def test_backward_is_declared_and_refuses_on_the_host():
    lib = _lib.load()
    assert len(_lib.SIGNATURES['gator_smpl_backward_f32'][1]) == 13 and _lib.ABI_VERSION == 2
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.gator_smpl_backward_f32(None, p, None, None, 1, -1, 1.0, p, None, p, None, None, None) == -1
    assert b'gator_smpl_backward_f32' in lib.gator_last_error() and b'null ctx' in lib.gator_last_error()
    assert lib.gator_smpl_backward_f32(None, p, None, p, 1, 0, 1.0, p, None, p, None, None, None) == -1
    assert b'center_idx goes with trans = NULL' in lib.gator_last_error()
    assert lib.gator_abi_version() == 2
