"""Every form of the vertex regressor (upsample_conv + bias + template: 431 coarse vertices x 3 taps -> 6890 vertices) at its tile and
plane edges, against the float64 product of exactly the operands the form carries (tests/upsample_refs.py).

Forms: 'fp32' = k_upsample<1>/<2> (GATOR_UPSAMPLE_X3=0), 'x3' = k_upsample_x3 (=1), 'x2' = k_upsample_x2<true> (=2, the default),
'x2w1' = k_upsample_x2<false> (inside gator_forward_bf16 only), 'bf16' = k_upsample_bf16, 'basic' = the bring-up path.  The switches are
read when a context is created, so every model here is built and first used under its own environment and cached for the module.

The bound, per output element: |out - ref| <= D_form S_aw + 4 e32 S (upsample_refs.bound), e32 measured per case from a plain float32
evaluation of the same product.  Lines starting with '[upsample-edges]' are the figures profiles/upsample_edge_tests.txt records
(run with -s)."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from gator_amd import _lib, synthetic
from tests import upsample_refs as ur
from tests.helpers import build_model

pytestmark = pytest.mark.gpu

NAME = 'h36m17_bn'
EINVAL, EUNSUPPORTED = -1, -6
X3_OF = {'fp32': '0', 'x3': '1', 'x2': '2'}
BATCHES = (1, 31, 32, 33, 64, 65, 96, 97, 127, 128, 129, 224, 225, 255, 256, 257, 288, 289, 513)
ROUNDING_OF = {'fp32': 'fp32', 'basic': 'fp32', 'x3': 'fp32', 'x2': 'x2', 'x2w1': 'x2w1', 'bf16': 'bf16'}      # forms that carry the same operands share a reference


def _say(fmt, *a):
    print('\n[upsample-edges] ' + fmt % a, end='')


@contextlib.contextmanager
def _env(**kw):
    with pytest.MonkeyPatch.context() as mp:
        for k, v in kw.items():
            mp.setenv(k, v)
        yield


_MODELS, _ROW0 = {}, {}


def _env_of(key):
    """key -> environment of the contexts of that model.  'x2:...' keys are further models of the default form."""
    form = key.split(':')[0]
    env = {'GATOR_UPSAMPLE_X3': X3_OF.get(form, '2')}
    if key == 'x2:c3_w1_0':
        env['GATOR_C3_UPSAMPLE_W1'] = '0'
    if key == 'x2:c3_bf16':
        env['GATOR_C3_UPSAMPLE_BF16'] = '1'
    return env


def _model(key):
    """The cached GATOR module of `key`; calls on it belong inside `with _env(**_env_of(key))` (a context is created on first use)."""
    if key not in _MODELS:
        _, m = build_model(NAME, 'fused')
        if key == 'basic':
            m.impl = m.pose2mesh.impl = 'basic'
        _MODELS[key] = m
    return _MODELS[key]


def _stage(key, vc, precision='f32'):
    with _env(**_env_of(key)):
        out = _model(key).pose2mesh.upsample(vc, precision=precision)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope='module', autouse=True)
def _drop_models():
    yield
    _MODELS.clear()
    _ROW0.clear()


@pytest.fixture(scope='module')
def params():
    """The regressor's parameters as every model of this module holds them (numpy float32)."""
    sd = _model('x2').state_dict()
    return {'w': sd['pose2mesh.upsample_conv.weight'].cpu().numpy(), 'bias': sd['pose2mesh.upsample_conv.bias'].cpu().numpy(),
            'tpl': sd['pose2mesh.init_vertices_6890'].cpu().numpy()}


def _case(form, vc, p, device='cuda'):
    """-> (ref, S_aw, S, e32) for float32 numpy activations under the form's operand rounding."""
    a, w = ur.round_operands(form, vc, p['w'])
    ref, s_aw, s = ur.reference(a, w, p['bias'], p['tpl'], device)
    e32 = ur.measure_e32(ur.reference32(a, w, p['bias'], p['tpl']), ref, s)
    return ref, s_aw, s, e32


def _hold(form, out, ref, s_aw, s, e32, what, where=None):
    """Bound (3) on every element (of the mask `where`); -> the worst |out - ref| / (e32 S)."""
    if where is not None:
        out, ref, s_aw, s = out[where], ref[where], s_aw[where], s[where]
    assert bool(torch.isfinite(out).all()), what
    err = (out.double() - ref).abs()
    bnd = ur.bound(form, s_aw, s, e32)
    ratio = float((err / (e32 * s)).max())
    worst = float((err / bnd).max())
    _say('%-34s form %-5s e32 %.3e   max|out-ref|/(e32 S) %.3f   max err/bound %.3f', what, form, e32, ratio, worst)
    assert bool((err <= bnd).all()), (what, form, ratio, worst)
    return ratio


# ---- (a) batch edges, every form, through the stage entry -------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def draw513(params):
    vc = (torch.randn(513, ur.V, 3, generator=torch.Generator().manual_seed(20261)) * 0.3).float()
    return vc.cuda(), {r: _case(r, vc.numpy(), params) for r in ('fp32', 'x2', 'bf16')}


@pytest.mark.parametrize('form,B', [(f, B) for f in ('fp32', 'x3', 'x2', 'bf16') for B in BATCHES] + [('basic', 1), ('basic', 33)])
def test_batch_edges(draw513, form, B):
    """B crosses every sample-tile and workgroup boundary of every form: 32-sample tiles, 128 samples (x2), 256 (x3, bf16), the fp32
    form's one-tile -> two-tile switch at 225 and its ragged pair at 257.  Rows are independent, so one 513-row reference serves all."""
    vc, cases = draw513
    ref, s_aw, s, e32 = cases[ROUNDING_OF[form]]
    key = {'bf16': 'x2'}.get(form, form)
    out = _stage(key, vc[:B].contiguous(), 'bf16' if form == 'bf16' else 'f32')
    assert out.shape == (B, ur.NV, 3)
    _hold(form, out, ref[:B], s_aw[:B], s[:B], e32, 'stage B=%d' % B)
    first = _ROW0.setdefault(form, out[0].clone())
    assert torch.equal(out[0], first), 'sample 0 depends on the batch it was computed in'


# ---- (b) every (coarse vertex, tap), every form ------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def onehot(params):
    vc = torch.from_numpy(ur.onehot_batch()).cuda()
    tables = {}

    def get(rounding):
        if rounding not in tables:
            _, w = ur.round_operands(rounding, np.zeros((1, ur.V, 3), np.float32), params['w'])
            exp, wp, valid = ur.onehot_expected(w, params['bias'], params['tpl'])
            tables[rounding] = (torch.from_numpy(exp).cuda(), torch.from_numpy(np.abs(wp)).cuda(), torch.from_numpy(valid).cuda())
        return tables[rounding]
    return vc, get


@pytest.mark.parametrize('form', ('fp32', 'x3', 'x2', 'bf16', 'basic'))
def test_every_coarse_vertex_and_tap(onehot, params, form):
    """1293 one-hot samples address every (coarse vertex, input position): sample i returns single weights (+ bias + template), and
    exactly the zero sample's value where the tap falls on the padding.  A misplaced `c < kV`, a swapped tap or a padded k-step that
    is not zero shows here and nowhere else."""
    vc, get = onehot
    exp, wabs, valid = get(ROUNDING_OF[form])
    key = {'bf16': 'x2'}.get(form, form)
    out = _stage(key, vc, 'bf16' if form == 'bf16' else 'f32')
    bias = torch.from_numpy(params['bias']).cuda()
    tpl = torch.from_numpy(params['tpl']).cuda()
    zero = out[-1]
    assert torch.equal(zero, bias[:, None] + tpl), 'the zero sample is fl32(bias + template)'
    got = out[:-1]
    pad = ~valid.expand_as(got)
    assert torch.equal(got[pad], zero[None].expand_as(got)[pad]), 'a padding tap contributed'
    tol = 2 * ur.EPS32 * (wabs + bias.abs().double()[None, :, None] + tpl.abs().double()[None])
    if form == 'x2':
        tol = tol + 2.0 ** -25 * 2.0 ** -ur.weight_shift(np.abs(params['w']).max())
    err = (got.double() - exp.double()).abs()
    exact = bool(torch.equal(got, exp))
    _say('one-hot sweep (1293 positions)      form %-5s bit-exact: %s   max err / allowed %.3f', form, exact, float((err / tol).max()))
    assert bool((err <= tol).all()), form


# ---- (c) magnitude families, x2 and x3, B = 33 -------------------------------------------------------------------------------------------
def _scaled(key, p, wscale, zero_offsets=False):
    """The model of `key` with the regressor's weights times `wscale` (and, optionally, no bias and no template) -> parameters."""
    m = _model(key)
    q = {'w': (p['w'] * np.float32(wscale)).astype(np.float32), 'bias': p['bias'] * (0 if zero_offsets else 1),
         'tpl': p['tpl'] * (0 if zero_offsets else 1)}
    assert np.isfinite(q['w']).all()
    with torch.no_grad():
        m.pose2mesh.upsample_conv.weight.copy_(torch.from_numpy(q['w']))
        m.pose2mesh.upsample_conv.bias.copy_(torch.from_numpy(q['bias']))
        m.pose2mesh.init_vertices_6890.copy_(torch.from_numpy(q['tpl']))
    m.pose2mesh.invalidate()
    return q


@pytest.mark.parametrize('mexp', (-10, -6, 0, 6, 10))
@pytest.mark.parametrize('form', ('x2', 'x3'))
def test_activation_magnitudes(params, form, mexp):
    """randn * 2^mexp: at 2^-6 and below every lo plane of the two-plane form is fp16-subnormal (a flushed denormal in a convert or an
    MFMA input would show as a miss of the bound, not be absorbed by it).  At 2^10 a few of the 42 669 draws pass 4094, the two-plane
    form's documented operand range (16 x value overflows its fp16 hi plane, in the reference's rounding as in the kernel's): the
    outputs such a coordinate feeds must be non-finite, every other element holds the bound -- never finite and wrong."""
    vc = (torch.randn(33, ur.V, 3, generator=torch.Generator().manual_seed(300 + mexp)) * 2.0 ** mexp).float()
    ref, s_aw, s, _ = _case(form, vc.numpy(), params)
    out = _stage(form, vc.cuda())
    fin = torch.isfinite(ref)
    n_over = int((vc.abs() >= 4094).sum())
    if form == 'x3' or mexp < 10:
        assert bool(fin.all()) and (form == 'x3' or n_over == 0)
    else:
        assert 0 < n_over < 20 and not bool(fin.all())
        assert not bool(torch.isfinite(out[~fin]).any()), 'finite output from an operand outside the fp16 range'
        _say('activations randn * 2^10: %d coordinates >= 4094, %d of %d outputs non-finite in reference and kernel alike', n_over, int((~fin).sum()), fin.numel())
    # e32 over the in-range rows only (a non-finite row has no float32 evaluation either)
    rows = fin.reshape(33, -1).all(1)
    assert int(rows.sum()) >= 20
    keep = rows.cpu().numpy()
    e32 = _case(form, vc.numpy()[keep], params)[3]
    _hold(form, out, ref, s_aw, s, e32, 'activations randn * 2^%d' % mexp, where=fin)


@pytest.mark.parametrize('wexp', (-12, 12))
@pytest.mark.parametrize('form', ('x2', 'x3'))
def test_weight_magnitudes(params, form, wexp):
    """Weights times 2^-12 and 2^12: the pack-time scale follows them, bound (3) holds unchanged."""
    vc = (torch.randn(33, ur.V, 3, generator=torch.Generator().manual_seed(77)) * 0.3).float()
    key = form + ':scaled'
    q = _scaled(key, params, 2.0 ** wexp)
    ref, s_aw, s, e32 = _case(form, vc.numpy(), q)
    out = _stage(key, vc.cuda())
    _hold(form, out, ref, s_aw, s, e32, 'weights * 2^%d' % wexp)


@pytest.mark.parametrize('zero_offsets', (False, True), ids=('golden-offsets', 'no-offsets'))
@pytest.mark.parametrize('wexp', (-36, 34, -60, 60))
def test_weight_scale_extremes_are_right_or_loud(params, wexp, zero_offsets):
    """Weights times 2^-36 and 2^34 (where pack_upsample_x2 used to clamp its scale at 2^24 / 2^-16), and 2^-60 / 2^60, against the EXACT
    float64 product of the unrounded operands: the result is within bound (3) of it, or loud (non-finite outputs and a device status
    reason) -- never finite and wrong.  With the golden bias and template S is dominated by them at 2^-36 and the check cannot fail;
    without them S = S_aw, the bound is relative to the product itself, and a scale that leaves the weights fp16-subnormal misses it
    by orders of magnitude (profiles/upsample_edge_tests.txt has the parent's figures)."""
    vc = (torch.randn(33, ur.V, 3, generator=torch.Generator().manual_seed(78)) * 0.3).float()
    q = _scaled('x2:scaled', params, 2.0 ** wexp, zero_offsets)
    ref, s_aw, s, e32 = _case('fp32', vc.numpy(), q)            # no operand rounding: the exact product
    out = _stage('x2:scaled', vc.cuda())
    what = 'weights * 2^%d %s' % (wexp, 'no bias/template' if zero_offsets else 'golden bias/template')
    if bool(torch.isfinite(out).all()):
        _hold('x2', out, ref, s_aw, s, e32, what + ' vs exact')
        _say('%-34s outcome: finite and within the bound', what)
    else:
        with pytest.raises(_lib.DeviceStatusError):
            _model('x2:scaled').pose2mesh.device_status()
        _say('%-34s outcome: loud (non-finite, device status)', what)


# ---- (d) the forward's own packer ---------------------------------------------------------------------------------------------------------
def _pose(B, seed=41):
    return torch.from_numpy(synthetic.synthetic_pose2d(B, 17, seed=seed)).cuda()


def _forward(key, x, precision='f32'):
    m = _model(key)
    with _env(**_env_of(key)):
        m.precision = precision
        try:
            verts, pose3d = m(x)
            tap = m.get_tap('vert431', (x.shape[0], ur.V, 3)).clone()
        finally:
            m.precision = 'f32'
    torch.cuda.synchronize()
    return verts, pose3d, tap


@pytest.mark.parametrize('B', (1, 33, 129, 257))
@pytest.mark.parametrize('form', ('fp32', 'x3', 'x2'))
def test_forward_packer(params, form, B):
    """In a full forward the MDR head writes the packed operand itself (mdr_head.hip head_store); behind it runs the same kernel as
    behind k_pack_vc*.  The head's packed values are the stage packers' by construction (same scale, same splits), so the vertices are
    bit-equal to the stage entry on the tapped coarse vertices, and hold bound (3) against their product."""
    verts, _, tap = _forward(form, _pose(B))
    ref, s_aw, s, e32 = _case(form, tap.cpu().numpy(), params)
    _hold(form, verts, ref, s_aw, s, e32, 'forward B=%d (head packer)' % B)
    same = torch.equal(verts, _stage(form, tap))
    _say('forward B=%-4d vs stage entry on its tap      form %-5s bit-equal: %s', B, form, same)
    assert same


@pytest.mark.parametrize('form', ('fp32', 'x3', 'x2'))
def test_one_context_over_a_batch_sequence(form):
    """B = 33, 257, 1, 129 on ONE context, stage and forward: the workspace regrows at 257, the x3 planes are strided by its capacity,
    and tiles past the batch keep what an earlier, larger batch left there.  Every result is bit-equal to a fresh context's."""
    def renew():
        torch.cuda.synchronize()
        m.invalidate(); m.pose2mesh.invalidate()
    m = _model(form)
    seq = (33, 257, 1, 129)
    xs = {B: _pose(B, seed=50 + B) for B in seq}
    g = torch.Generator().manual_seed(9)
    vcs = {B: (torch.randn(B, ur.V, 3, generator=g) * 0.3).float().cuda() for B in seq}
    with _env(**_env_of(form)):
        fresh = {}
        for B in seq:
            renew()
            fresh[B] = (m(xs[B])[0].clone(), m.pose2mesh.upsample(vcs[B]).clone())
        renew()
        for B in seq:
            v = m(xs[B])[0]
            u = m.pose2mesh.upsample(vcs[B])
            assert torch.equal(v, fresh[B][0]), ('forward', B)
            assert torch.equal(u, fresh[B][1]), ('stage', B)
        # and once more with forward and stage sharing one context's workspace history the other way round
        for B in seq[::-1]:
            assert torch.equal(m.pose2mesh.upsample(vcs[B]), fresh[B][1]), ('stage, descending', B)
            assert torch.equal(m(xs[B])[0], fresh[B][0]), ('forward, descending', B)


# ---- (e) config 3's regressors --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', (1, 33, 129, 257))
@pytest.mark.parametrize('setting,form', (('x2', 'x2w1'), ('x2:c3_w1_0', 'x2'), ('x2:c3_bf16', 'bf16')),
                         ids=('default-x2w1', 'W1=0-x2', 'BF16=1-bf16'))
def test_config3_regressors(params, setting, form, B):
    """gator_forward_bf16's three regressors against the product of their own tapped coarse vertices: k_upsample_x2<false> (weights on
    one fp16 plane, the default), k_upsample_x2<true> (GATOR_C3_UPSAMPLE_W1=0) and k_upsample_bf16 (GATOR_C3_UPSAMPLE_BF16=1)."""
    verts, _, tap = _forward(setting, _pose(B, seed=43), precision='bf16')
    ref, s_aw, s, e32 = _case(form, tap.cpu().numpy(), params)
    _hold(form, verts, ref, s_aw, s, e32, 'config 3 forward B=%d' % B)


# ---- (f) the joint epilogue -------------------------------------------------------------------------------------------------------------------
_REGS = ur.joint_regressors()


def _coo(dense):
    r, c = np.nonzero(dense)
    return r.astype(np.int32), c.astype(np.int32), dense[r, c].astype(np.float32), int(dense.shape[0])


def _check_joints(m, x, coo, what):
    j1, p1 = m.forward_joints(x)
    j2, p2, v2 = m.forward_joints(x, with_verts=True)
    v0, p0 = m(x)
    torch.cuda.synchronize()
    assert torch.equal(j1, j2), 'joints depend on whether the vertices are stored'
    assert torch.equal(v2, v0) and torch.equal(p1, p0) and torch.equal(p2, p0)
    ref, mag = ur.joints_reference(coo, v2)
    err = (j2.double() - ref).abs()
    bnd = 2.0 ** -23 * mag
    worst = float((err / bnd.clamp_min(1e-300)).max())
    _say('%-40s max err / (2^-23 sum|w||v|) %.3f', what, worst)
    assert bool((err <= bnd).all()), what
    return j2


@pytest.mark.parametrize('reg', sorted(_REGS))
@pytest.mark.parametrize('form', ('x3', 'x2'))
def test_joint_epilogue_tables(form, reg):
    """The epilogue's block / entry tables at their edges: an entry at vertex 0 and at 6889, the 10-vertex tail block filled, 256
    entries in one 32-vertex block, a joint without entries (exactly 0), one joint, 3000 entries with cancelling signs."""
    m = _model(form)
    dense = _REGS[reg]
    with _env(**_env_of(form)):
        m.set_joint_regressor(dense)
        for B in (1, 33, 129):
            j = _check_joints(m, _pose(B, seed=60), _coo(dense), 'epilogue %s %s B=%d' % (form, reg, B))
            assert j.shape == (B, dense.shape[0], 3)
            if reg == 'empty_joint':
                assert not bool(j[:, 2].any()), 'a joint without entries is exactly 0'


def _raw_set(m, r, c, v, nnz, nj):
    return _lib.load().gator_set_joint_regressor(m._ctx, r.ctypes.data, c.ctypes.data, v.ctypes.data, int(nnz), int(nj))


@pytest.mark.parametrize('form', ('x3', 'x2'))
def test_joint_epilogue_unsorted_duplicated_list_and_argument_checks(form):
    """Through the C ABI: the cancelling list shuffled, with duplicated (joint, vertex) entries -- the duplicates add (the
    reference sums every entry of the list).  Then the
    argument checks: each returns its code and leaves the registered regressor as it was."""
    m = _model(form)
    dense = _REGS['cancelling']
    r, c, v, tot = ur.shuffled_with_duplicates(dense)
    nj = dense.shape[0]
    x = _pose(33, seed=61)
    with _env(**_env_of(form)):
        m(x)                                                   # the context exists
        assert _raw_set(m, r, c, v, r.size, nj) == 0
        m._jreg, m._jreg_ctx = (r, c, v, nj), m._ctx.value     # forward_joints() keeps what is registered on this context
        for B in (1, 33, 129):
            _check_joints(m, _pose(B, seed=60), (r, c, v, nj), 'epilogue %s shuffled+duplicates B=%d' % (form, B))
        j_before, _ = m.forward_joints(x)
        bad = lambda a, i, val: np.concatenate([a[:i], np.array([val], a.dtype), a[i + 1:]])
        for what, args in (('row = nj', (bad(r, 5, nj), c, v, r.size, nj)), ('row = -1', (bad(r, r.size - 1, -1), c, v, r.size, nj)),
                           ('col = 6890', (r, bad(c, 0, ur.NV), v, r.size, nj)), ('col = -1', (r, bad(c, 7, -1), v, r.size, nj)),
                           ('nnz = 0', (r, c, v, 0, nj)), ('nnz = -1', (r, c, v, -1, nj)), ('nj = 0', (r, c, v, r.size, 0))):
            assert _raw_set(m, *args) == EINVAL, what
        j_after, _ = m.forward_joints(x)
        assert torch.equal(j_before, j_after), 'a refused regressor changed the registered one'
        m._jreg = m._jreg_ctx = None


def test_joint_epilogue_refuses_the_fp32_form_before_any_launch():
    """GATOR_UPSAMPLE_X3=0 has no epilogue: gator_forward_joints_f32 returns GATOR_EUNSUPPORTED and has queued nothing -- no output
    buffer is touched, pose3d (which the encoder would write first) included."""
    m = _model('fp32')
    x = _pose(33, seed=62)
    r, c, v, nj = _coo(_REGS['vertex0'])
    with _env(**_env_of('fp32')):
        m(x)
        assert _raw_set(m, r, c, v, r.size, nj) == 0
        joints = torch.full((33, nj, 3), 12345.0, device='cuda')
        pose3d = torch.full((33, 17, 3), 12345.0, device='cuda')
        verts = torch.full((33, ur.NV, 3), 12345.0, device='cuda')
        torch.cuda.synchronize()
        rc = _lib.load().gator_forward_joints_f32(m._ctx, x.data_ptr(), 33, joints.data_ptr(), pose3d.data_ptr(), verts.data_ptr(),
                                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == EUNSUPPORTED
        for t in (joints, pose3d, verts):
            assert bool((t == 12345.0).all()), 'a refused call wrote to its outputs'
        v2, _ = m(x)                                            # and the context goes on working
        assert bool(torch.isfinite(v2).all())
