"""Input poses between "a standardised Gaussian" and "not finite", and the oracle's answers to them.

Every other accuracy test of the forward feeds synthetic.synthetic_pose2d (i.i.d. Gaussian, standardised per sample, |x| <~ 3) or a
NaN / inf pose (tests/test_gpu_poisoned_samples.py).  The batches here hold what lies between: poses inside the input contract
(synthetic.py: per-sample, per-axis zero mean / unit population std) that no Gaussian draw reaches, and poses outside it that the
reference still maps to a finite mesh -- zero padding, raw pixels, an offset, a gain.  The pose enters the forward at two sites: the
embedding (GraphLinear 2 -> 64 in front of a GroupNorm, which takes a gain out again) and the five pose columns of the MDR joint tokens
(get_joint_feature in front of LN1, which does the same): `mdr_jf` grows linearly with the input, the outputs barely move.

Three batches of B = 16 per golden variant, rows 0..2 the same three synthetic_pose2d poses in each:

    contract   3, 4  an exact one-joint outlier (joint 0 / joint J-1 at sqrt(J-1), the others coincident at -1/sqrt(J-1))
               5     the same at a middle joint, with 1e-3 jitter          6     two clusters of alternating joints
               7, 8  collinear: y = x, y = -x                              9     joints 1..5 placed on joint 0, re-standardised
               10    Student-t (df = 2), standardised                      11    a lattice: every coordinate one of two values
               12..15 ordinary poses
    units      3, 4, 5  all zero, all -0.0, +-1e-40 (denormal)             6     y == 0
               7..13 ONE standardised pose x 2^-100, 2^-20, 2^-8, 2^3, 2^10, 2^15, 2^40
               14    1080p pixels: pose * (60, 140) + (960, 540)           15    pose * 1e-2 + 1e6
    ordinary   sixteen Gaussian rows: the clean batch of the isolation checks

The builders are deterministic numpy; run(name, batch) evaluates the fp64 and the fp32 oracle once per (variant, batch) and is never
modified afterwards.  tests/test_host_input_refs.py proves on the oracle that the batches are what this text says."""
import numpy as np
import torch

B = 16
BATCHES = ('contract', 'units', 'ordinary')
SHARED_SEED, ORDINARY_SEED, FAMILY_SEED = 7, 8, 20240921
GAINS = (-100, -20, -8, 3, 10, 15, 40)                  # units rows 7..13: the pose x 2^k
GAIN_ROWS = tuple(range(7, 7 + len(GAINS)))
PIXEL_ROW, OFFSET_ROW = 14, 15
STRICT_ROWS = {'contract': tuple(range(B)), 'ordinary': tuple(range(B)), 'units': tuple(range(7))}   # rows no form may report on
ROW_NAMES = {
    'contract': ('gauss0', 'gauss1', 'gauss2', 'outlier@0', 'outlier@J-1', 'outlier@mid+jit', 'two-clusters', 'y=x', 'y=-x', 'coincident1..5',
                 'student-t2', 'lattice', 'gauss', 'gauss', 'gauss', 'gauss'),
    'units': ('gauss0', 'gauss1', 'gauss2', 'zero', '-0.0', 'denormal', 'y==0') + tuple('x2^%d' % k for k in GAINS) + ('pixels', '1e6+1e-2x'),
    'ordinary': ('gauss0', 'gauss1', 'gauss2') + ('gauss',) * 13,
}


def standardise(x):
    """[..., J, 2] float64 -> per-axis zero mean / unit population std over the joints (the input contract)."""
    x = np.asarray(x, np.float64)
    return (x - x.mean(-2, keepdims=True)) / x.std(-2, keepdims=True)


def _gauss(n, J, seed):
    from gator_amd import synthetic
    return synthetic.synthetic_pose2d(n, J, seed=seed).astype(np.float64)


def _outlier(J, k, sign_y):
    x = np.full((J, 2), -1.0 / np.sqrt(J - 1.0))
    x[k] = np.sqrt(J - 1.0)
    x[:, 1] *= sign_y
    return x


def contract(J):
    rs = np.random.RandomState(FAMILY_SEED + J)
    x = np.empty((B, J, 2))
    x[0:3] = _gauss(3, J, SHARED_SEED)
    x[3] = _outlier(J, 0, 1.0)
    x[4] = _outlier(J, J - 1, -1.0)
    x[5] = standardise(_outlier(J, J // 2, 1.0) + 1e-3 * rs.randn(J, 2))
    alt = np.where(np.arange(J) % 2 == 0, 1.0, -1.0)
    x[6] = standardise(np.stack([alt, -alt], 1))
    line = standardise(rs.randn(J, 1))
    x[7] = np.concatenate([line, line], 1)
    x[8] = np.concatenate([line, -line], 1)
    co = rs.randn(J, 2)
    co[1:6] = co[0]
    x[9] = standardise(co)
    x[10] = standardise(rs.standard_t(2, (J, 2)))
    lat = np.where(rs.rand(J, 2) < 0.5, -1.0, 1.0)
    lat[0], lat[1] = (-1.0, 1.0), (1.0, -1.0)           # both values on both axes, whatever the draw
    x[11] = standardise(lat)
    x[12:16] = _gauss(4, J, ORDINARY_SEED)
    return x.astype(np.float32)


def units(J):
    rs = np.random.RandomState(FAMILY_SEED + 100 + J)
    x = np.empty((B, J, 2), np.float32)
    x[0:3] = _gauss(3, J, SHARED_SEED)
    x[3] = 0.0
    x[4] = -0.0
    x[5] = np.where(rs.rand(J, 2) < 0.5, -1.0, 1.0).astype(np.float32) * np.float32(1e-40)
    y0 = standardise(rs.randn(J, 2))
    y0[:, 1] = 0.0
    x[6] = y0
    pose = standardise(rs.randn(J, 2)).astype(np.float32)                  # one pose under every gain: the rows differ by the gain alone
    for row, k in zip(GAIN_ROWS, GAINS):
        x[row] = np.ldexp(pose, k)                                          # exact in fp32 for every k here
    x[PIXEL_ROW] = standardise(rs.randn(J, 2)) * (60.0, 140.0) + (960.0, 540.0)
    x[OFFSET_ROW] = standardise(rs.randn(J, 2)) * 1e-2 + 1e6
    return x


def ordinary(J):
    x = np.empty((B, J, 2))
    x[0:3] = _gauss(3, J, SHARED_SEED)
    x[3:16] = _gauss(13, J, ORDINARY_SEED + 1)
    return x.astype(np.float32)


BUILDERS = {'contract': contract, 'units': units, 'ordinary': ordinary}


class Run:
    """One (variant, batch): x [B,J,2] fp32 tensor; v64 / p64 the fp64 oracle (numpy; metres / mm); per row (numpy [B]): ref_v / ref_p =
    the fp32 oracle's error against fp64 (mm), finite32, embed = max|gat_embed|, jf = max|mdr_jf|, enc_absmax / enc_spread and
    cross_absmax / cross_spread of the logits in front of the encoder's and the cross-attention's softmax; pc = the fp64 oracle's
    pose_combine rounded to fp32 [B,J,133]."""


_RUNS, _MDR = {}, {}


def _rowmax(t):
    return t.abs().reshape(t.shape[0], -1).max(1).values.numpy()


def _row_ranges(ts):
    absmax = np.max([_rowmax(t) for t in ts], 0)
    spread = np.max([(t.max(-1).values - t.min(-1).values).reshape(t.shape[0], -1).max(1).values.numpy() for t in ts], 0)
    return absmax, spread


def run(name, batch):
    key = (name, batch)
    if key not in _RUNS:
        from oracle import gator_oracle as go
        from tests.helpers import oracle_setup
        z, c, sd = oracle_setup(name)
        r = Run()
        r.c, r.sd, r.names = c, sd, ROW_NAMES[batch]
        r.x = torch.from_numpy(BUILDERS[batch](c.J))
        taps = {}
        v, p = go.gator_forward(sd, c, r.x, torch.float64, taps)
        v32, p32 = go.gator_forward(sd, c, r.x, torch.float32)
        r.v64, r.p64 = v.numpy(), p.numpy()
        r.finite32 = (torch.isfinite(v32).reshape(B, -1).all(1) & torch.isfinite(p32).reshape(B, -1).all(1)).numpy()
        r.ref_v = np.abs(v32.numpy().astype(np.float64) - r.v64).reshape(B, -1).max(1) * 1e3
        r.ref_p = np.abs(p32.numpy().astype(np.float64) - r.p64).reshape(B, -1).max(1)
        r.embed, r.jf = _rowmax(taps['gat_embed']), _rowmax(taps['mdr_jf'])
        r.enc_absmax, r.enc_spread = _row_ranges([taps['enc_logits%d' % i] for i in range(6)])
        r.cross_absmax, r.cross_spread = _row_ranges([taps['cross_logits%d' % i] for i in range(3)])
        r.pc = torch.cat((r.x.double(), taps['pose3d'] / 1000, taps['feat']), dim=2).float()
        _RUNS[key] = r
    return _RUNS[key]


def mdr_run(name, batch='units'):
    """The MDR stage alone on run(name, batch).pc: -> (v64 [B,6890,3] numpy, ref_v [B] mm) of the oracle's mdr_forward in fp64 / fp32."""
    key = (name, batch)
    if key not in _MDR:
        from oracle import gator_oracle as go
        r = run(name, batch)
        with torch.no_grad():
            v = go.mdr_forward(r.sd, r.c, r.pc, torch.float64).numpy()
            v32 = go.mdr_forward(r.sd, r.c, r.pc, torch.float32).numpy().astype(np.float64)
        _MDR[key] = (v, np.abs(v32 - v).reshape(B, -1).max(1) * 1e3)
    return _MDR[key]


def bars(ref_v, ref_p=None):
    """The suite's bars (tests/test_gpu_softmax_edges.py), per row: vertices <= max(1.5e-3 mm, 2 x ref_v), pose3d <= max(1e-3 mm, 2 x ref_p)."""
    bv = np.maximum(1.5e-3, 2.0 * np.asarray(ref_v))
    return bv if ref_p is None else (bv, np.maximum(1e-3, 2.0 * np.asarray(ref_p)))


def fmt_row(r, i):
    return '%2d %-16s fp32 oracle verts %.2e mm pose3d %.2e mm | |embed|<=%.2f |jf|<=%.3g | enc |l|<=%.1f spread %.1f | cross |l|<=%.1f spread %.1f' % (
        i, r.names[i], r.ref_v[i], r.ref_p[i], r.embed[i], r.jf[i], r.enc_absmax[i], r.enc_spread[i], r.cross_absmax[i], r.cross_spread[i])
