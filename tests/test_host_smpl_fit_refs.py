"""The float64 restatement of the SMPL fit (tests/smpl_fit_refs.py) checked on the CPU: its Jacobian against central differences of
smpl_refs.lbs_forward, its convergence on the case table, the stationarity on a noisy target, the float32 floor the device bounds are
taken from (measured and printed; profiles/smpl_fit.txt holds the table), and the declarations of the new entry points."""
import os
import re

import numpy as np

from tests import smpl_fit_refs as fr
from tests import smpl_refs as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND_M = 1e-9          # the issue's 1e-6 mm; the synthetic models are in metres


def test_jacobian_columns_match_central_differences():
    """beta = 0 on a model with zeroed posedirs: the regime where the stated Jacobian is exact.  Rotation column 3 k + a is the derivative
    along R_k <- exp(Rg_parent^T h e_a) R_k, translation column a along trans += h e_a.
    Tolerance.  A vertex moves on a circle of radius rho <= 2 L about the joint (L: the largest coordinate magnitude of the sample), so
    the central difference (f(h) - f(-h)) / 2h of its position differs from the derivative by h^2 / 6 rho + O(h^4) <= h^2 L / 3; each of
    the two forwards carries fp64 rounding of a few eps L (a chain of <= 24 joints: bounded by 64 eps L), divided by 2h.  With
    h = 1e-4: 3.3e-9 L + 7e-11 L; the bound below is h^2 L / 3 + 64 eps L / h.  Translation is linear: the rounding term alone."""
    m = fr.model('nv65')
    m['posedirs'] = np.zeros_like(m['posedirs'])
    nj = 24
    truth = fr.case_truth('nv65', 1.2)
    pose, betas, trans = truth[0][0].astype(np.float64), np.zeros(10), truth[2][0].astype(np.float64)
    tgt = np.zeros((65, 3))
    J, L = fr.jacobian(m, pose, betas, trans, tgt)
    R, Rg, _, _, _ = fr.parts(m, pose, betas)
    h, eps = 1e-4, 2.0 ** -53
    tol_rot, tol_tr = h * h * L / 3 + 64 * eps * L / h, 64 * eps * L / h

    def verts(p, t):
        return sr.lbs_forward(m, p[None], betas[None], t[None])[0][0].reshape(-1)

    worst = 0.0
    for k in range(nj):
        Rp = np.eye(3) if k == 0 else Rg[int(m['parents'][k])]
        for a in range(3):
            side = []
            for s in (1.0, -1.0):
                p = pose.copy().reshape(nj, 3)
                p[k] = fr.layer_axisang(fr.so3_log(fr.so3_exp(Rp.T @ (s * h * np.eye(3)[a])) @ R[k]))
                side.append(verts(p.reshape(-1), trans))
            err = np.abs((side[0] - side[1]) / (2 * h) - J[:, 3 * k + a]).max()
            worst = max(worst, err)
            assert err <= tol_rot, (k, a, err, tol_rot)
    for a in range(3):
        e = np.eye(3)[a] * h
        err = np.abs((verts(pose, trans + e) - verts(pose, trans - e)) / (2 * h) - J[:, 3 * nj + 10 + a]).max()
        assert err <= tol_tr, (a, err, tol_tr)
    print('smpl fit jacobian: worst rotation column error %.3e (bound %.3e)' % (worst, tol_rot))
    assert np.abs(J[:, 3 * nj:3 * nj + 10]).max() > 0            # the shape block is there (not exact: the joints move with beta)


def test_fp64_fit_converges_on_the_case_table():
    """At most 1e-6 mm within 20 iterations, on the float64 target itself (the device tests round the same target through float32,
    which alone moves it by ~3e-5 mm).  All five sizes of the table converged as drawn, NV = 64 included: no case was changed."""
    for label, name, truth, _, init in fr.table():
        m = fr.model(name)
        tgt, _ = sr.lbs_forward(m, *truth)
        for i in range(len(tgt)):
            st, rms = fr.fit(m, tgt[i], None if init is None else tuple(a[i] for a in init), fr.ITERS)
            ev = fr.rms_of(m, st, tgt[i])
            print('smpl fit fp64 %-12s sample %d: rms %.3e m (evaluated by lbs_forward %.3e m)' % (label, i, rms, ev))
            assert ev <= BOUND_M and rms <= BOUND_M, (label, i, ev, rms)


def test_noisy_target_is_stationary():
    name, tgt = fr.noisy_target()
    h = []
    fr.fit(fr.model(name), tgt[0], None, fr.ITERS, history=h)
    last = np.array(h[-10:])
    print('smpl fit noisy: rms over the last 10 evaluations %.15e .. %.15e' % (last.min(), last.max()))
    assert 0.5 * fr.NOISE_SIGMA * np.sqrt(3) < h[-1] < 1.5 * fr.NOISE_SIGMA * np.sqrt(3)      # the noise's own rms distance, about sigma sqrt(3)
    assert last.max() - last.min() <= 1e-12 * last.min()


def test_float32_floor_measured():
    """Measured and printed (the record is profiles/smpl_fit.txt, written by tools/smpl_fit_bench.py from the same function).  The one
    check: the constants the device bounds use still cover what this machine measures."""
    rows, ratio, excess = fr.float32_floor()
    for label, e32, rms in rows:
        print('smpl fit f32 floor %-14s e32 %.3e m  emulated fit, fp64-evaluated rms %.6e m' % (label, e32, rms))
    print('smpl fit f32 floor: ratio %.4f (recorded %.4f, K = %.4f)  noisy excess %.3e (recorded %.3e, eps = %.3e)'
          % (ratio, fr.F32_RATIO, fr.K_FLOOR, excess, fr.F32_NOISY_EXCESS, fr.EPS_NOISY))
    assert ratio <= fr.K_FLOOR and abs(excess) <= fr.EPS_NOISY


def test_header_and_binding_declare_the_fit():
    from gator_amd import _lib, build, kernel_resources
    header = open(os.path.join(ROOT, 'include', 'gator_hip.h')).read()
    for n in ('gator_smpl_fit_f32', 'gator_smpl_fit_normal_f32', 'gator_smpl_fit_width'):
        mt = re.search(r'\bint %s\(([^;]*)\);' % n, header)
        assert mt, n
        assert n in _lib.SIGNATURES, n
        assert len(_lib.SIGNATURES[n][1]) == mt.group(1).count(',') + 1, n
    for k in ('k_smpl_fit_normal<', 'k_smpl_fit_solve'):
        assert k in kernel_resources.HOT
    assert 'smpl_fit.hip' in build.SOURCES
    src = open(os.path.join(ROOT, 'gator_amd', 'csrc', 'smpl_fit.hip')).read()
    assert '__builtin_amdgcn_mfma_f32_32x32x2f32' in src
