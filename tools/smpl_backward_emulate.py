#!/usr/bin/env python3
"""A numpy emulation, on the host, of the accumulation order of the device SMPL backward (gator_amd/csrc/smpl_backward.hip), to tell
before a device run whether that order meets the tests' bound: every gradient element within 3x the reference layer's own fp32
error (the spreads of tests/golden/smpl_layer_grad.npz) of the float64 VJP.

What is emulated in float32, in the kernel's order: the coefficient rows and skinning transforms rounded once from fp64; the blend
product as one fmaf chain over k; v_posed; T^R as a chain over the vertex's influences; gx = s gV; gp; per 128-vertex tile the gA sums
as a chain over the tile's vertices of w * round(gx_r * p_c) and the g_coef sums as a chain over (coordinate, vertex); the tile's g_off
share in fp64, even vertices then odd ones.  Then, in fp64 as on the device: the sum over the tiles in order and the whole chain stage.
An fmaf is emulated as a float64 multiply-add rounded to float32 (the product of two float32 is exact in float64).

With --exact the hot part runs in float64 with plain sums instead: the formulas alone, against the autograd reference.

Usage:  python tools/smpl_backward_emulate.py [--exact] [case ...]      default: every golden case, on all 65 samples (nv6890: the 3 stored ones)"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests import smpl_grad_refs as gr  # noqa: E402
from tests import smpl_refs as sr  # noqa: E402

TV = 128
f32 = np.float32


def fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def rodrigues_vjp(a, g):
    """a [..., 3], g [..., 9] -> [..., 3]: the derivative stated in smpl_backward.hip."""
    e = a + 1e-8
    angle = np.sqrt((e * e).sum(-1))
    half = angle * 0.5
    sn, cs = np.sin(half), np.cos(half)
    u = sn / angle
    q = np.concatenate([cs[..., None], u[..., None] * a], -1)
    qn = np.sqrt((q * q).sum(-1))
    w, x, y, z = (q[..., i] / qn for i in range(4))
    G = [g[..., i] for i in range(9)]
    hw = 2 * (w * (G[0] + G[4] + G[8]) - z * G[1] + y * G[2] + z * G[3] - x * G[5] - y * G[6] + x * G[7])
    hx = 2 * (x * (G[0] - G[4] - G[8]) + y * G[1] + z * G[2] + y * G[3] - w * G[5] + z * G[6] + w * G[7])
    hy = 2 * (y * (G[4] - G[0] - G[8]) + x * G[1] + w * G[2] + x * G[3] + z * G[5] - w * G[6] + z * G[7])
    hz = 2 * (z * (G[8] - G[0] - G[4]) - w * G[1] + x * G[2] + w * G[3] + y * G[5] + x * G[6] + y * G[7])
    dot = w * hw + x * hx + y * hy + z * hz
    k = np.stack([(hw - w * dot) / qn, (hx - x * dot) / qn, (hy - y * dot) / qn, (hz - z * dot) / qn], -1)
    gu = (a * k[..., 1:]).sum(-1)
    gh = -sn * k[..., 0] + cs / angle * gu
    gangle = 0.5 * gh - u / angle * gu
    return u[..., None] * k[..., 1:] + (gangle / angle)[..., None] * e


def emulate(m, pose, betas, trans, center_idx, out_scale, gV, gJ, exact=False):
    """-> {'pose', 'betas', 'trans'} float32 arrays (None for an absent input), as the device computes them."""
    nv, nj = m['weights'].shape
    nb = m['shapedirs'].shape[2]
    parents = [int(p) for p in m['parents']]
    B = pose.shape[0]
    p64 = pose.astype(np.float64).reshape(B, nj, 3)
    b64 = None if betas is None else betas.astype(np.float64)
    R = sr.rodrigues(p64)
    # the pose stage, fp64
    jr = m['J_regressor'].astype(np.float64)
    J0 = jr @ m['v_template'].astype(np.float64)
    Js = np.einsum('jv,vck->jck', jr, m['shapedirs'].astype(np.float64))
    J = np.broadcast_to(J0, (B, nj, 3)).copy()
    if b64 is not None and nb:
        J = J + np.einsum('jck,bk->bjc', Js, b64)
    GR, Gt = np.zeros((B, nj, 3, 3)), np.zeros((B, nj, 3))
    GR[:, 0], Gt[:, 0] = R[:, 0], J[:, 0]
    for j in range(1, nj):
        p = parents[j]
        GR[:, j] = GR[:, p] @ R[:, j]
        Gt[:, j] = np.einsum('brc,bc->br', GR[:, p], J[:, j] - J[:, p]) + Gt[:, p]
    coef = np.concatenate([np.zeros((B, nb)) if b64 is None else b64, (R[:, 1:] - np.eye(3)).reshape(B, -1)], 1)
    basis = np.concatenate([m['shapedirs'], m['posedirs']], 2)          # [NV,3,K] float32
    W = m['weights']
    s = out_scale
    ntile = (nv + TV - 1) // TV
    K = coef.shape[1]
    if exact:
        pv = m['v_template'].astype(np.float64) + np.einsum('vck,bk->bvc', basis.astype(np.float64), coef)
        TR = np.einsum('vj,bjrc->bvrc', W.astype(np.float64), GR)
        gx = np.zeros((B, nv, 3)) if gV is None else gV.astype(np.float64) * s
        gp = np.einsum('bvrc,bvr->bvc', TR, gx)
        gAR = np.einsum('vj,bvr,bvc->bjrc', W.astype(np.float64), gx, pv)
        gAt = np.einsum('vj,bvr->bjr', W.astype(np.float64), gx)
        gcoef = np.einsum('vck,bvc->bk', basis.astype(np.float64), gp)
        goffv = gx.sum(1)
    elif gV is None:
        gAR, gAt, gcoef, goffv = np.zeros((B, nj, 3, 3)), np.zeros((B, nj, 3)), np.zeros((B, K)), np.zeros((B, 3))
    else:
        c32, A32 = coef.astype(f32), GR.astype(f32)
        a = np.zeros((B, nv, 3), f32)
        for k in range(K):
            a = fma(c32[:, None, k:k + 1], basis[None, :, :, k], a)
        pv = m['v_template'][None] + a
        TR = np.zeros((B, nv, 3, 3), f32)
        order = np.argsort(W == 0, 1, kind='stable')                  # a vertex's influences in joint order, as the packed lists hold them
        for slot in range(int((W != 0).sum(1).max())):
            j = order[:, slot]
            wj = W[np.arange(nv), j]
            TR = fma(wj[None, :, None, None], A32[:, j], TR)
        gx = gV.astype(f32) * f32(s)
        gp = np.zeros((B, nv, 3), f32)
        for c in range(3):
            gp[:, :, c] = fma(TR[:, :, 0, c], gx[:, :, 0], fma(TR[:, :, 1, c], gx[:, :, 1], TR[:, :, 2, c] * gx[:, :, 2]))
        gAR, gAt, gcoef, goffv = np.zeros((B, nj, 3, 3)), np.zeros((B, nj, 3)), np.zeros((B, K)), np.zeros((B, 3))
        for t in range(ntile):
            v0, v1 = t * TV, min(nv, (t + 1) * TV)
            accR, acct, accc = np.zeros((B, nj, 3, 3), f32), np.zeros((B, nj, 3), f32), np.zeros((B, K), f32)
            for v in range(v0, v1):
                y = gx[:, v, :, None] * pv[:, v, None, :]               # round(gx_r * p_c)
                accR = fma(W[v][None, :, None, None], y[:, None], accR)
                acct = fma(W[v][None, :, None], gx[:, v][:, None, :], acct)
            for c in range(3):
                for v in range(v0, v1):
                    accc = fma(basis[v, c][None, :], gp[:, v, c:c + 1], accc)
            even = gx[:, v0:v1:2].astype(np.float64)
            odd = gx[:, v0 + 1:v1:2].astype(np.float64)
            se, so = np.zeros((B, 3)), np.zeros((B, 3))
            for i in range(even.shape[1]):
                se += even[:, i]
            for i in range(odd.shape[1]):
                so += odd[:, i]
            gAR += accR
            gAt += acct
            gcoef += accc
            goffv += se + so
    # the chain stage, fp64
    gq = np.zeros((B, nj, 3)) if gJ is None else gJ.astype(np.float64) * s
    goff = goffv + gq.sum(1)
    gGR = gAR - gAt[..., :, None] * J[..., None, :]
    gGt = gAt + gq
    gJt = -np.einsum('bjrc,bjr->bjc', GR, gAt)
    gR = np.zeros((B, nj, 3, 3))
    gR[:, 1:] = gcoef[:, nb:].reshape(B, nj - 1, 3, 3)
    if trans is None and center_idx is not None:
        gGt[:, center_idx] -= goff
    for j in range(nj - 1, 0, -1):
        p = parents[j]
        gR[:, j] += np.einsum('bkr,bkc->brc', GR[:, p], gGR[:, j])
        gGR[:, p] += gGR[:, j] @ R[:, j].transpose(0, 2, 1) + gGt[:, j][:, :, None] * (J[:, j] - J[:, p])[:, None, :]
        gd = np.einsum('bkc,bk->bc', GR[:, p], gGt[:, j])
        gJt[:, j] += gd
        gJt[:, p] -= gd
        gGt[:, p] += gGt[:, j]
    gR[:, 0] += gGR[:, 0]
    gJt[:, 0] += gGt[:, 0]
    gb = None
    if betas is not None:
        gb = (gcoef[:, :nb] + np.einsum('jck,bjc->bk', Js, gJt)).astype(f32)
    gpose = rodrigues_vjp(p64, gR.reshape(B, nj, 9)).reshape(B, nj * 3).astype(f32)
    return {'pose': gpose, 'betas': gb, 'trans': None if trans is None else goff.astype(f32)}


def run_case(name, exact, B):
    o = gr.case_options(name)
    m = sr.synthetic_model(*sr.CASES[name][0])
    args = tuple(None if a is None else a[:B] for a in gr.case_arguments(name))
    gV, gJ = (g[:B] for g in gr.upstream(name))
    spreads = None
    path = os.path.join(REPO, 'tests', 'golden', 'smpl_layer_grad.npz')
    if os.path.exists(path):
        z = np.load(path)
        spreads = {w: z['%s.spread.%s' % (name, w)] for w in gr.UPSTREAMS}
    for which in gr.UPSTREAMS:
        v, j = gr.select_upstream(which, gV, gJ)
        ref = gr.vjp64(m, args, o, v, j)
        got = emulate(m, *args, o['center_idx'], o['out_scale'], v, j, exact=exact)
        for i, k in enumerate(gr.OUTPUTS):
            if ref[k] is None:
                continue
            err = np.abs(got[k].astype(np.float64) - ref[k]).max()
            scale = np.abs(ref[k]).max()
            if spreads is None:
                print('emulation %-18s B %2d %-6s g_%-5s err %.3e  max|g| %.3e  err/max|g| %.2e' % (name, B, which, k, err, scale, err / max(scale, 1e-300)))
            else:
                sp = float(spreads[which][i])
                print('emulation %-18s B %2d %-6s g_%-5s err %.3e  spread %.3e  ratio %.2f (bound 3)' % (name, B, which, k, err, sp, err / sp))


def main():
    argv = [a for a in sys.argv[1:] if a != '--exact']
    exact = '--exact' in sys.argv
    for name in argv or tuple(sr.CASES):
        run_case(name, exact, 3 if name == 'nv6890' else sr.N_SAMPLES)      # what tests/test_gpu_smpl_backward.py runs on the device


if __name__ == '__main__':
    main()
