"""The forward under the input poses a caller can hand it: tests/input_refs.py's `contract` batch (inside the input contract, far from a
Gaussian draw: one-joint outliers, coincident and collinear joints, heavy tails, exact ties) and `units` batch (outside it, and still a
finite mesh in the reference: zero padding, -0.0, denormals, y == 0, gains 2^-100 .. 2^40, raw pixels, an offset of 1e6), in every kernel
form that reads the pose -- the embedding (gat_roles.hip, gat_fused.hip, gat_tiled.hip), the five pose columns of the MDR joint tokens
(gat8_tail.h, gat_tail.hip, k_mdr_joint) and the norm statistics behind both.  tests/test_host_input_refs.py proves on the oracle that
the reference maps every row to a mesh within the floors of the bars below.

The forms are those of tests/test_gpu_softmax_edges.py (ENC_FORMS, MDR_FORMS, HEAD_FORMS: a fresh module per form, switches read when
its context is created) plus impl = 'basic', precision = 'bf16' (config 3) and subbatch_streams = 2.  Every test runs one B = 16 batch
twice and prints one line per row; the sub-batch form runs the 16 rows eight times over (B = 128, from where the library splits a batch
into two halves on two streams: the odd rows sit in both halves) and asserts that the forward was split.

Bar, per row (the suite's figures, tests/test_gpu_softmax_edges.py): vertices <= max(1.5e-3 mm, 2 x ref_v), pose3d <= max(1e-3 mm,
2 x ref_p) against the fp64 oracle, ref = the fp32 oracle's error on the same row.  Config 3: its mode's 1 mm max / 0.2 mm rms on the
vertices and 1 mm on pose3d (tests/test_gpu_bf16.py).

STRICT (the `contract` batch on every form; the zero / -0.0 / denormal / y == 0 rows of `units` on every form; all of `units` on the forms
without an operand range: 'exact', 'basic', the fp32-input forms): the first forward meets the bar, no warning, m.arithmetic unchanged,
device_status() clean, a second run and rows run alone are bit-equal.
RIGHT OR LOUD (the gain, pixel and offset rows of `units` on the default arithmetic's forms; the contract of
tests/test_gpu_rescaled_weights.py::test_default_arithmetic_is_right_or_loud): the second forward meets the bar on every row; a row whose
first forward does not must be non-finite in it and reported with reason 2 (the module heals to arithmetic = 'exact'; a warning of any
other reason fails: the inputs are finite).  A finite first-forward row outside the bar is the failure this file exists to catch.
Measured figures: profiles/input_family_tests.txt."""
import warnings

import numpy as np
import pytest
import torch

from gator_amd import _lib
from tests import input_refs as ir
from tests.helpers import oracle_setup
from tests.test_gpu_softmax_edges import C, ENC_FORMS, H, HEAD_FORMS, MDR_FORMS, _module

pytestmark = pytest.mark.gpu

# every distinct form of the three tables (the encoder's and the MDR table's 'exact' are one form)
FORMS = {}
for _table in (ENC_FORMS, MDR_FORMS, HEAD_FORMS):
    for _k, _v in _table.items():
        if _v not in FORMS.values():
            FORMS[_k] = _v
NO_OPERAND_RANGE = ('exact', 'basic', 'gat_fp32', 'mdr_fp32')
EXTRA = {'basic': ({}, 'default'), 'bf16': ({}, 'default'), 'subbatch2': ({}, 'default')}
ALL_FORMS = dict(FORMS, **EXTRA)
SPLIT_COPIES = 8        # 'subbatch2': fused_forward splits a batch over its two streams from B = 128 on, so that form gets the 16 rows 8 times over


def _cases():
    """Both batches on every form; gat8 on both variants, the other forms on one, alternating."""
    out, n = [], 0
    for batch in ('contract', 'units'):
        for form in ALL_FORMS:
            if form == 'gat8':
                names = (H, C)
            else:
                names = ((H, C)[n % 2],)
                n += 1
            out += [pytest.param(name, form, batch, id='%s-%s-%s' % (batch, form, name)) for name in names]
    return out


def _fresh(monkeypatch, name, form):
    m = _module(monkeypatch, name, ALL_FORMS, form, oracle_setup(name)[2], precision='bf16' if form == 'bf16' else 'f32')
    if form == 'basic':
        m.impl = 'basic'
    if form == 'subbatch2':
        m.subbatch_streams = 2
    return m


def _copies(r, k):
    """The batch of r, k times over (B = 16 k): the same cached oracle answers, row i + 16 j = row i."""
    t = ir.Run()
    t.x, t.names = r.x.repeat(k, 1, 1), r.names * k
    t.v64, t.p64 = np.tile(r.v64, (k, 1, 1)), np.tile(r.p64, (k, 1, 1))
    t.ref_v, t.ref_p = np.tile(r.ref_v, k), np.tile(r.ref_p, k)
    return t


def _assert_split(m, r):
    """The last forward of m, on r.x, ran as two halves on two streams: the library keeps the 'feat' tap of a whole-batch forward and
    clears it after a split one (fused_api.hip: fused_forward).  The small forwards of the same tests read the tap back, so this
    cannot pass on a module that never records it."""
    with pytest.raises(RuntimeError, match='no tap named'):
        m.get_tap('feat', (r.x.shape[0], r.x.shape[1], 128))


def _rows(out, r):
    """-> per row: vertex error (mm), pose3d error (mm), finite."""
    v, p = out
    vn, pn = v.cpu().numpy().astype(np.float64), p.cpu().numpy().astype(np.float64)
    n = vn.shape[0]
    fin = np.isfinite(vn).reshape(n, -1).all(1) & np.isfinite(pn).reshape(n, -1).all(1)
    with np.errstate(invalid='ignore'):
        return np.abs(vn - r.v64).reshape(n, -1).max(1) * 1e3, np.abs(pn - r.p64).reshape(n, -1).max(1), fin


def _bars(r, form):
    bv, bp = ir.bars(r.ref_v, r.ref_p)
    if form == 'bf16':
        bv = np.full(len(bv), 1.0)             # config 3: 1 mm max (and 0.2 mm rms, _rms_ok) on the vertices, 1 mm on pose3d -- the encoder's
        bp = np.full(len(bp), 1.0)             # linears run on one activation plane too (tests/test_gpu_bf16.py)
    return bv, bp


def _rms_ok(out, r, form, rows):
    if form != 'bf16' or not len(rows):
        return True
    e = (out[0].cpu().numpy().astype(np.float64)[rows] - r.v64[rows]) * 1e3
    rms = float(np.sqrt((e ** 2).mean()))
    print('  config 3 rms over rows %s: %.4f mm' % ([int(i) for i in rows], rms))
    return rms < 0.2


def _table(tag, name, form, r, e1, e2, bv, bp, state):
    n = len(e1[0])
    print('\n[input-family] %s %s %s%s' % (tag, name, form, '' if n == ir.B else ' (B = %d: each line the worst of the row\'s %d copies)' % (n, n // ir.B)))
    if n != ir.B:       # NaN, if any, wins the maximum
        worst = lambda e: None if e is None else tuple(np.asarray(a).reshape(-1, ir.B).max(0) for a in e[:2])
        e1, e2 = worst(e1), worst(e2)
        state = ['right' if all(s == 'right' for s in state[i::ir.B]) else next(s for s in state[i::ir.B] if s != 'right') for i in range(ir.B)]
    for i in range(ir.B):
        second = '' if e2 is None else ' second %.3e' % e2[0][i]
        print('  %2d %-16s verts first %.3e%s ref %.3e bar %.1e mm | pose3d first %.3e ref %.3e mm | %s'
              % (i, r.names[i], e1[0][i], second, r.ref_v[i], bv[i], e1[1][i], r.ref_p[i], state[i]))


def _clone(out):
    return tuple(t.clone() for t in out)


def _strict(m, r, form, arith, tag, name):
    """The whole batch strictly: right at once, silent, clean, deterministic, batch independent."""
    x = r.x.cuda()
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)                      # a heal (RuntimeWarning) would swap the form under test
        first = _clone(m(x))
        torch.cuda.synchronize()
        m.device_status()
        if form == 'subbatch2':
            _assert_split(m, r)
        second = _clone(m(x))
        alone = _clone(m(x[3:6].contiguous()))
        torch.cuda.synchronize()
        m.device_status()
        if form == 'subbatch2':
            m.get_tap('feat', (3, x.shape[1], 128))                        # three rows run whole, and a whole-batch forward keeps its tap
    assert m.arithmetic == arith
    bv, bp = _bars(r, form)
    e1 = _rows(first, r)
    ok = (e1[0] <= bv) & (e1[1] <= bp) & e1[2]
    _table(tag, name, form, r, e1, None, bv, bp, ['right' if o else 'WRONG' for o in ok])
    assert ok.all(), 'rows %s outside the bar on the first forward' % np.nonzero(~ok)[0].tolist()
    assert _rms_ok(first, r, form, np.arange(len(ok)))
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    for a, b in zip(first, alone):
        assert torch.equal(a[3:6], b)


def _right_or_loud(m, r, form, tag, name):
    """`units` on a form of the default arithmetic: rows 0..6 strictly, the rest right or loud."""
    x = r.x.cuda()
    strict = np.array([i for i in range(x.shape[0]) if i % ir.B in ir.STRICT_ROWS['units']])
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        pad = _clone(m(x[3:7].contiguous()))                               # zero, -0.0, denormal, y == 0 alone: padding costs a module nothing
        torch.cuda.synchronize()
        m.device_status()
        if form == 'subbatch2':
            m.get_tap('feat', (4, x.shape[1], 128))                        # four rows run whole, and a whole-batch forward keeps its tap
    assert m.arithmetic == 'default' and m.on_device_status == 'heal'
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        first = _clone(m(x))
        torch.cuda.synchronize()
        if form == 'subbatch2':
            _assert_split(m, r)
        second = _clone(m(x))                                               # carries the first one's report, if any, and heals
        torch.cuda.synchronize()
    msgs = [str(i.message) for i in w if issubclass(i.category, RuntimeWarning)]
    healed = m.arithmetic == 'exact'                                        # HipModule._run switches the module for reason 2 alone; every other
    other = msgs[1:] if healed else msgs                                    # reason is a warning that switches nothing
    m.device_status()                                                       # the second forward left nothing
    bv, bp = _bars(r, form)
    e1, e2 = _rows(first, r), _rows(second, r)
    ok1 = (e1[0] <= bv) & (e1[1] <= bp) & e1[2]
    ok2 = (e2[0] <= bv) & (e2[1] <= bp) & e2[2]
    state = ['right' if ok1[i] else ('non-finite, reported (reason 2), healed' if (not e1[2][i] and healed) else 'WRONG: finite and outside the bar'
                                     if e1[2][i] else 'WRONG: non-finite and not reported') for i in range(len(ok1))]
    _table(tag, name, form, r, e1, e2, bv, bp, state)
    print('  first forward reported: %s%s' % ('reason 2 -> arithmetic = %r' % m.arithmetic if healed else 'nothing', ''.join('\n  ' + s for s in other)))
    assert not other, 'a report other than reason 2 on finite inputs'
    assert len(msgs) == int(healed)
    assert ok2.all(), 'rows %s outside the bar on the second forward' % np.nonzero(~ok2)[0].tolist()
    assert ok1[strict].all(), 'strict rows %s outside the bar on the first forward' % strict[~ok1[strict]].tolist()
    bad = np.nonzero(~ok1)[0]
    assert not e1[2][bad].any(), 'rows %s are finite and outside the bar on the first forward' % bad[e1[2][bad]].tolist()
    assert healed or not len(bad), 'rows %s are non-finite on the first forward and nothing was reported' % bad.tolist()
    assert _rms_ok(first, r, form, np.nonzero(ok1)[0]) and _rms_ok(second, r, form, np.arange(len(ok2)))
    for a, b in zip(first, pad):
        assert torch.equal(a[3:7], b)
    if not healed:
        for a, b in zip(first, second):
            assert torch.equal(a, b)


@pytest.mark.parametrize('name,form,batch', _cases())
def test_input_families(monkeypatch, name, form, batch):
    r = ir.run(name, batch)
    if form == 'subbatch2':
        r = _copies(r, SPLIT_COPIES)                                        # B = 128: halves of 64, every odd row in both
    m = _fresh(monkeypatch, name, form)
    arith = ALL_FORMS[form][1]
    if batch == 'contract' or form in NO_OPERAND_RANGE:
        _strict(m, r, form, arith, batch, name)
    else:
        _right_or_loud(m, r, form, batch, name)


@pytest.mark.parametrize('name,encoder', [(H, 'sample'), (C, 'tiled'), (H, 'tiled'), (C, 'sample')])
def test_odd_rows_change_no_ordinary_row(monkeypatch, name, encoder):
    """Rows 0..2 are the same three poses in all three batches: through ONE module (default arithmetic, on_device_status = 'raise', any
    report read before the next forward) they come out bit-equal whatever rows 3..15 hold.  On the pinned sample-tiled encoder rows 0..6
    (J = 17) resp. 0..5 (J = 19) share a workgroup's token tiles, so each odd row sits beside ordinary ones."""
    m = _fresh(monkeypatch, name, 'gat8' if encoder == 'sample' else 'tiled_h4')     # GATOR_GAT_TILED=1: the tiled encoder at every batch size
    m.on_device_status = 'raise'
    if encoder == 'sample':
        m.set_encoder('sample')
    o = ir.run(name, 'ordinary')
    clean = _clone(m(o.x.cuda()))
    torch.cuda.synchronize()
    m.device_status()
    assert m.encoder_for_batch(ir.B) == encoder
    for batch in ('contract', 'units'):
        r = ir.run(name, batch)
        out = _clone(m(r.x.cuda()))
        torch.cuda.synchronize()
        reason = 0
        try:
            m.device_status()
        except _lib.DeviceStatusError:
            reason = _lib.load().gator_status_reason(m._ctx)
        m.device_status()
        e = _rows(out, r)
        print('\n[input-family] isolation %s %s %s: reported reason %d; non-finite rows %s' % (name, encoder, batch, reason, np.nonzero(~e[2])[0].tolist()))
        assert reason in ((0,) if batch == 'contract' else (0, _lib.REASON_NONFINITE))
        for a, b in zip(clean, out):
            assert torch.equal(a[0:3], b[0:3]), '%s: an ordinary row changed' % batch
        bv, bp = ir.bars(r.ref_v, r.ref_p)
        ok = (e[0] <= bv) & (e[1] <= bp) & e[2]
        assert (ok | ~e[2]).all() and (reason or ok.all())                  # right, or non-finite and reported
        assert ok[list(ir.STRICT_ROWS[batch])].all()
    again = m(o.x.cuda())
    torch.cuda.synchronize()
    m.device_status()
    for a, b in zip(clean, again):
        assert torch.equal(a, b)


@pytest.mark.parametrize('name,form', [(H, 'x2'), (C, 'x3'), (H, 'mdr_fp32'), (C, 'exact')])
def test_mdr_stage_entry_under_unit_poses(monkeypatch, name, form):
    """m.pose2mesh on the fp64 oracle's pose_combine of the `units` batch (rounded to fp32) against the oracle's mdr_forward on the same
    tensor: k_mdr_joint's five pose columns, LN1 and K / V tiles without the encoder in front.  Same bar, same rule."""
    r = ir.run(name, 'units')
    v64, ref = ir.mdr_run(name)
    m = _fresh(monkeypatch, name, form)
    mm = m.pose2mesh
    mm.arithmetic = MDR_FORMS[form][1]
    pc = r.pc.cuda()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        first = mm(pc).clone()
        torch.cuda.synchronize()
        second = mm(pc).clone()
        torch.cuda.synchronize()
    mm.device_status()
    msgs = [str(i.message) for i in w if issubclass(i.category, RuntimeWarning)]
    healed = MDR_FORMS[form][1] == 'default' and mm.arithmetic == 'exact'   # HipModule._run switches the module for reason 2 alone
    bv = ir.bars(ref)

    def rows(v):
        vn = v.cpu().numpy().astype(np.float64)
        with np.errstate(invalid='ignore'):
            return np.abs(vn - v64).reshape(ir.B, -1).max(1) * 1e3, np.isfinite(vn).reshape(ir.B, -1).all(1)
    (e1, f1), (e2, f2) = rows(first), rows(second)
    ok1, ok2 = (e1 <= bv) & f1, (e2 <= bv) & f2
    print('\n[input-family] mdr stage %s %s: reported %s' % (name, form, 'reason 2, healed' if healed else 'nothing'))
    for i in range(ir.B):
        print('  %2d %-16s verts first %.3e second %.3e ref %.3e bar %.1e mm | %s' % (
            i, r.names[i], e1[i], e2[i], ref[i], bv[i], 'right' if ok1[i] else 'non-finite, reported' if (not f1[i] and healed) else 'WRONG'))
    assert len(msgs) == int(healed), msgs
    assert ok2.all()
    if form in NO_OPERAND_RANGE:
        assert not msgs and ok1.all() and mm.arithmetic == MDR_FORMS[form][1]
    strict = list(ir.STRICT_ROWS['units'])
    assert ok1[strict].all()
    assert not f1[~ok1].any(), 'a finite row outside the bar on the first forward'
    assert healed or ok1.all()
    if not healed:
        assert torch.equal(first, second)
