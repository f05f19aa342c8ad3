"""fp64 numpy restatements for the temporal evaluation tests (tests/test_host_temporal_refs.py, tests/test_gpu_temporal.py): the
one-euro filter of lib/smooth_utils.py as smooth_pose drives it, and the three per-frame error columns of gator_sequence_errors
(lib/coord_utils.compute_error_accel, data/PW3D/dataset.py:398-403).  Everything here is numpy on the host and shares nothing with
the kernels; the Procrustes step is oracle.gator_oracle.rigid_align."""
import math
import warnings

import numpy as np

from oracle import gator_oracle as go

LENGTHS = (1, 2, 3, 5, 64, 65, 130)                   # the videos of tests/golden/temporal.npz
PARAMS = ((0.004, 0.005), (0.004, 0.7), (1.0, 0.0))   # its (min_cutoff, beta) sets at dt = 1


def one_euro(x, min_cutoff=0.004, beta=0.7, d_cutoff=1.0, dt=1.0, t=None):
    """One video x [T, ...] -> float64 [T, ...].  Whole frames at a time, every operation a numpy float64 ufunc: the rounding of each
    product, sum and quotient is IEEE's, in the reference's order.  t_e = dt at every step, or t[i] - t[i-1] when timestamps are given
    (the reference called with t = idx * dt sees differences that are not exactly dt)."""
    x = np.asarray(x, np.float64)
    out = np.empty_like(x)
    out[0] = x[0]
    x_prev, dx_prev = x[0], np.zeros_like(x[0])
    for i in range(1, len(x)):
        t_e = np.float64(dt) if t is None else np.float64(t[i]) - np.float64(t[i - 1])
        r = 2 * math.pi * d_cutoff * t_e
        a_d = r / (r + 1)
        dx = (x[i] - x_prev) / t_e
        dx_hat = a_d * dx + (1 - a_d) * dx_prev
        cutoff = min_cutoff + beta * np.abs(dx_hat)
        r = 2 * math.pi * cutoff * t_e
        a = r / (r + 1)
        x_hat = a * x[i] + (1 - a) * x_prev
        out[i] = x_hat
        x_prev, dx_prev = x_hat, dx_hat
    return out


def seg_starts(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def one_euro_videos(x, lengths, **kw):
    with np.errstate(all='ignore'):
        s = seg_starts(lengths)
        return np.concatenate([one_euro(x[a:b], **kw) for a, b in zip(s[:-1], s[1:])])


def accel_rows(pred, gt, lengths, valid=None):
    """[F] float64: entry i = the acceleration error of frames (i, i+1, i+2); NaN for the last two frames of a video and for a triple
    with an invalid frame."""
    pred, gt = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    out = np.full(len(pred), np.nan)
    s = seg_starts(lengths)
    for a, b in zip(s[:-1], s[1:]):
        for i in range(a, b - 2):
            if valid is not None and not (valid[i] and valid[i + 1] and valid[i + 2]):
                continue
            ap = pred[i] - 2 * pred[i + 1] + pred[i + 2]
            ag = gt[i] - 2 * gt[i + 1] + gt[i + 2]
            out[i] = np.linalg.norm(ap - ag, axis=1).mean()
    return out


def error_rows(pred, gt, lengths, valid=None):
    """[F,3] float64: the columns of gator_sequence_errors."""
    pred, gt = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    rows = np.empty((len(pred), 3))
    rows[:, 0] = accel_rows(pred, gt, lengths, valid)
    rows[:, 1] = np.sqrt(((pred - gt) ** 2).sum(2)).mean(1)
    rows[:, 2] = [np.sqrt(((go.rigid_align(p, g) - g) ** 2).sum(1)).mean() for p, g in zip(pred, gt)]
    return rows


def video_sums(rows, lengths):
    """[V,6]: what k_seq_reduce writes, from the rows."""
    s = seg_starts(lengths)
    out = np.zeros((len(lengths), 6))
    for v, (a, b) in enumerate(zip(s[:-1], s[1:])):
        r0 = rows[a:b, 0]
        ok = ~np.isnan(r0)
        out[v] = [r0[ok].sum(), rows[a:b, 1].sum(), rows[a:b, 2].sum(), ok.sum(), b - a, 0.0]
    return out


def summary(rows, lengths):
    """The reference's three averages (data/PW3D/dataset.py:391-413) from the rows, as it forms them: np.mean per video (NaN with a
    warning for a video without a triple), np.mean over the videos, np.mean over all frames for PA-MPJPE."""
    s = seg_starts(lengths)
    acc, mp = [], []
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore')                   # "Mean of empty slice"
        for a, b in zip(s[:-1], s[1:]):
            r0 = rows[a:b, 0]
            acc.append(np.mean(r0[~np.isnan(r0)]))
            mp.append(np.mean(rows[a:b, 1]))
        return {'accel': float(np.mean(acc)), 'MPJPE': float(np.mean(mp)), 'PA-MPJPE': float(np.mean(rows[:, 2]))}


def walk(rs, lengths, ne=14, step=8.0, jitter=3.0, spread=300.0):
    """Random-walk joints in millimetres with per-frame jitter, float32 [F,ne,3]: every video starts afresh."""
    out = []
    for T in lengths:
        base = rs.randn(1, ne, 3) * spread
        out.append(base + np.cumsum(rs.randn(T, ne, 3) * step, 0) + rs.randn(T, ne, 3) * jitter)
    return np.concatenate(out).astype(np.float32)
