"""References of the SMPL fit tests (gator_smpl_fit_f32, csrc/smpl_fit.hip): a float64 numpy restatement of the damped Gauss-Newton
iteration, built on smpl_refs.lbs_forward / smpl_refs.synthetic_model.  Nothing here is shared with the kernels.

The iteration.  Unknowns P = 3 NJ + NB + 3: a world-frame rotation increment per joint, the betas, the translation.
  residual      r_v = verts_v + trans - target_v
  rotation      d verts_v / d delta_k = -[c_vk]x,  c_vk = sum_{j in subtree(k)} w_vj (x_vj - p_k),  x_vj = A_j [v_posed_v ; 1]
  shape         d verts_v / d beta_b  = (sum_j w_vj Rg_j) S_v[:, b]
  translation   identity
  M = [J | r]^T [J | r], padded to N = 32 ceil((P + 1) / 32):  H = M[:P,:P], g = M[:P,P], err = M[P,P].
  A step: evaluate M at the candidate; accept iff err < the current err (the initial state is the first candidate and is accepted when
  its err is finite, without a change of lambda); accept: lambda = max(lambda / 4, 1e-9); reject: lambda = min(8 lambda, 1e6) and the
  current M stays; solve (H + lambda diag H + 1e-12 I) d = -g by Cholesky; a non-positive pivot is one more rejection (lambda again
  times 8, d = 0); R_k <- exp(Rg_parent(k)^T d_k) R_k, pose_k = layer_axisang(log R_k) (below), betas += d, trans += d.  lambda_0 = 1e-2.  fit(iters) takes
  `iters` steps and evaluates iters + 1 candidates; the answer is the current state after the last evaluation.

Bounds of the stage test (u = 2^-24), for one element M[a][b] = sum over the 3 NV rows of J_a J_b:
  D.  The device forms each product exactly (fp32-input MFMA) and adds it into an fp32 accumulator: one rounding per row.  A wave owns
  48 of a 64-vertex tile's 192 rows and walks the 8 tiles of a 512-vertex chunk: a chain of 384 additions; the four waves' sums are
  added in order (3 more), then the ceil(NV / 512) chunks (S - 1 more).  Any product passes through at most 384 + 3 + S - 1 roundings,
  so the sum is within D u sum|J_a J_b| of the exact sum of the device's own entries, D(NV) = 386 + ceil(NV / 512), to first order
  (the second-order term is D u times that, 2.4e-5 of it).
  floor.  The device's entries are float32 evaluations.  With L = the largest coordinate magnitude among images, joints, target and
  translation of the sample: an image x_vj = A_j [v_posed ; 1] carries the roundings of A (4 entries, u / 2 each on magnitudes <= 1 and
  <= L), of v_posed (template + a blend sum whose terms are <= 1e-2 of it: 2 u) and a chain of three fmaf: <= 8 u L.  c_vk sums at most
  four w (x - p): p rounded (u / 2 L), the difference (u 2L), product and add (2 u) each: <= 16 u L per entry with sum w <= 1.  The
  residual blends four images (8 u L + 4 u L), adds trans and subtracts the target (2 u 2L): <= 16 u L.  The shape entries are 1e-2 of
  that.  So every entry of [J | r] is within e = E_ENTRY u L, E_ENTRY = 16, of its fp64 value, and
      |M_dev - M_ref| <= D u sum|J_a J_b| + e sum_rows (|J_a| + |J_b|) + 3 NV e^2.
  The float32 emulation below (fit(..., f32=True) and jacobian(..., f32=True)) measures the same e on the host: profiles/smpl_fit.txt."""
import numpy as np

from tests import smpl_refs as sr

U32 = 2.0 ** -24
E_ENTRY = 16.0
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX, RIDGE = 1e-2, 1e-9, 1e6, 1e-12
CHUNK = 512

# name -> (NV, model seed): the case table of both test modules
CASES = {'nv63': (63, 12), 'nv64': (64, 13), 'nv65': (65, 18), 'nv129': (129, 23), 'nv257': (257, 15)}
ZERO_INIT_MAX, NEAR_INIT_MAX = 0.8, 1.2
PERTURB = (0.15, 0.3, 0.02)          # rad per joint, betas, metres


def D_of(nv):
    return 386.0 + -(-nv // CHUNK)


def widths(m):
    nj, nb = m['weights'].shape[1], m['shapedirs'].shape[2]
    P = 3 * nj + nb + 3
    return P, 32 * -(-(P + 1) // 32)


def model(name):
    nv, seed = CASES[name]
    return sr.synthetic_model(nv, 24, 10, seed)


def case_truth(name, max_angle, n=2):
    """n true states of the case: axis-angles of uniform magnitude in [0, max_angle] per joint, betas ~ N(0,1), trans ~ N(0,1) m."""
    nv, seed = CASES[name]
    rs = np.random.RandomState(5000 + seed + int(max_angle * 10))
    ax = rs.randn(n, 24, 3)
    ax /= np.linalg.norm(ax, axis=-1, keepdims=True)
    pose = (ax * rs.uniform(0, max_angle, (n, 24, 1))).reshape(n, 72)
    return pose.astype(np.float32), rs.randn(n, 10).astype(np.float32), rs.randn(n, 3).astype(np.float32)


def perturbed(name, truth):
    """The table's near initialisation: the truth moved by up to 0.15 rad per joint entry, 0.3 per beta, 2 cm."""
    nv, seed = CASES[name]
    rs = np.random.RandomState(7000 + seed)
    pose, betas, trans = truth
    return ((pose + rs.uniform(-1, 1, pose.shape) * PERTURB[0] / np.sqrt(3)).astype(np.float32),
            (betas + rs.uniform(-1, 1, betas.shape) * PERTURB[1]).astype(np.float32),
            (trans + rs.uniform(-1, 1, trans.shape) * PERTURB[2]).astype(np.float32))


def ancestors(parents):
    """D[k, j] = 1 when k is j or an ancestor of j."""
    nj = len(parents)
    D = np.zeros((nj, nj))
    for j in range(nj):
        k = j
        while True:
            D[k, j] = 1.0
            if k == 0:
                break
            k = int(parents[k])
    return D


def cross_matrix(c):
    """[..., 3] -> [..., 3, 3], [c]x."""
    z = np.zeros_like(c[..., 0])
    return np.stack([np.stack([z, -c[..., 2], c[..., 1]], -1), np.stack([c[..., 2], z, -c[..., 0]], -1),
                     np.stack([-c[..., 1], c[..., 0], z], -1)], -2)


def so3_exp(r):
    a = np.sqrt((r * r).sum())
    if a == 0.0:
        return np.eye(3)
    K = cross_matrix(r / a)
    return np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)


def so3_log(M):
    """Rotation vector with the angle in [0, pi], through the quaternion (largest pivot): accurate at 0 and at pi."""
    t = np.trace(M)
    c = [t, M[0, 0], M[1, 1], M[2, 2]]
    i = int(np.argmax(c))
    if i == 0:
        q = np.array([1 + t, M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
    elif i == 1:
        q = np.array([M[2, 1] - M[1, 2], 1 + M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[0, 2] + M[2, 0]])
    elif i == 2:
        q = np.array([M[0, 2] - M[2, 0], M[0, 1] + M[1, 0], 1 + M[1, 1] - M[0, 0] - M[2, 2], M[1, 2] + M[2, 1]])
    else:
        q = np.array([M[1, 0] - M[0, 1], M[0, 2] + M[2, 0], M[1, 2] + M[2, 1], 1 + M[2, 2] - M[0, 0] - M[1, 1]])
    if q[0] < 0:
        q = -q
    n = np.sqrt((q[1:] ** 2).sum())
    if n == 0.0:
        return np.zeros(3)
    return q[1:] * (2.0 * np.arctan2(n, q[0]) / n)


def layer_axisang(rho):
    """The axis-angle a whose LAYER rotation is exp(rho).  The layer's Rodrigues takes the angle as |a + 1e-8| and normalises the
    quaternion (cos(h), sin(h) a / |a + 1e-8|), h = |a + 1e-8| / 2, so its rotation of a has a's axis and the angle
    theta(a) = 2 atan2(sin(h) |a| / |a + 1e-8|, cos(h)), off |a| by up to ~1e-8.  One fixed-point step a = rho (2 |rho| - theta(rho)) / |rho|
    leaves an error of the order 1e-16; without it every step of the fit would carry a 1e-8 rad error into the next evaluation."""
    n = np.sqrt((rho * rho).sum())
    if n == 0.0:
        return np.zeros(3)
    al = np.sqrt(((rho + 1e-8) ** 2).sum())
    theta = 2.0 * np.arctan2(np.sin(al * 0.5) * n / al, np.cos(al * 0.5))
    return rho * ((2.0 * n - theta) / n)


def parts(m, pose, betas, f32=False):
    """One sample's forward pieces: local rotations R [NJ,3,3], global rotations Rg, posed joints p [NJ,3], skinning transforms
    A [NJ,3,4], v_posed [NV,3].  f32: the pose stage in float64 with A, p and the blend coefficients rounded to float32 (what the
    layer's pose kernel hands on), everything per vertex in float32."""
    f = {k: np.asarray(m[k], np.float64) for k in ('v_template', 'shapedirs', 'posedirs', 'weights', 'J_regressor')}
    nj = f['weights'].shape[1]
    pose, betas = np.asarray(pose, np.float64), np.asarray(betas, np.float64)
    R = sr.rodrigues(pose.reshape(nj, 3))
    pose_map = (R[1:] - np.eye(3)).reshape(-1)
    Jr = f['J_regressor'] @ (f['v_template'] + f['shapedirs'] @ betas)
    Rg, p = np.zeros((nj, 3, 3)), np.zeros((nj, 3))
    for j in range(nj):
        if j == 0:
            Rg[0], p[0] = R[0], Jr[0]
        else:
            q = int(m['parents'][j])
            Rg[j] = Rg[q] @ R[j]
            p[j] = Rg[q] @ (Jr[j] - Jr[q]) + p[q]
    A = np.concatenate([Rg, (p - np.einsum('jrc,jc->jr', Rg, Jr))[:, :, None]], 2)
    if f32:
        t = np.float32
        vp = m['v_template'].astype(t) + (m['shapedirs'].astype(t) @ betas.astype(t) + m['posedirs'].astype(t) @ pose_map.astype(t))
        return R, Rg.astype(t), p.astype(t), A.astype(t), vp
    return R, Rg, p, A, f['v_template'] + f['shapedirs'] @ betas + f['posedirs'] @ pose_map


def jacobian(m, pose, betas, trans, target, f32=False):
    """One sample -> ([J | r] of shape [3 NV, P + 1], rows 3 v + c, and the images' largest magnitude L).  float64 unless f32."""
    t = np.float32 if f32 else np.float64
    R, Rg, p, A, vp = parts(m, pose, betas, f32)
    w, S = m['weights'].astype(t), m['shapedirs'].astype(t)
    nv, nj = w.shape
    x = np.einsum('jrc,vc->vjr', A[:, :, :3], vp) + A[None, :, :, 3]                      # [NV, NJ, 3]
    verts = np.einsum('vj,vjr->vr', w, x)
    D = ancestors(m['parents']).astype(t)
    c = np.einsum('kj,vj,vjr->vkr', D, w, x) - np.einsum('kj,vj->vk', D, w)[:, :, None] * p[None]
    Jrot = -cross_matrix(c)                                                                 # [NV, NJ, 3, 3]
    Jrot = np.transpose(Jrot, (0, 2, 1, 3)).reshape(nv, 3, nj * 3)
    Jshape = np.einsum('vj,jrc,vcb->vrb', w, Rg, S)
    Jtr = np.broadcast_to(np.eye(3, dtype=t), (nv, 3, 3))
    r = verts + np.asarray(trans, t) - np.asarray(target, t)
    out = np.concatenate([Jrot, Jshape, Jtr, r[:, :, None]], 2).reshape(nv * 3, -1)
    L = max(np.abs(x[w != 0]).max(), np.abs(p).max(), np.abs(target).max(), np.abs(trans).max())
    return out.astype(np.float64), float(L)


def normal_matrix(m, pose, betas, trans, target, f32=False):
    """Batched: -> M [B, N, N] float64 (the full symmetric matrix; rows and columns past P are zero)."""
    P, N = widths(m)
    B = len(pose)
    M = np.zeros((B, N, N))
    for b in range(B):
        Jr, _ = jacobian(m, pose[b], betas[b], trans[b], target[b], f32)
        M[b, :P + 1, :P + 1] = Jr.T @ Jr
    return M


def stage_bound(m, pose, betas, trans, target):
    """[N, N]: the bound of the module docstring for one sample."""
    P, N = widths(m)
    Jr, L = jacobian(m, pose, betas, trans, target)
    a = np.abs(Jr)
    nv = m['weights'].shape[0]
    e = E_ENTRY * U32 * L
    col = a.sum(0)
    out = np.zeros((N, N))
    out[:P + 1, :P + 1] = D_of(nv) * U32 * (a.T @ a) + e * (col[:, None] + col[None, :]) + 3 * nv * e * e
    return out


def rms_of(m, state, target):
    """float64 rms vertex distance of a state (one sample), through lbs_forward."""
    pose, betas, trans = (np.asarray(a, np.float64)[None] for a in state)
    v, _ = sr.lbs_forward(m, pose, betas, trans)
    return float(np.sqrt(((v[0] - target) ** 2).sum(-1).mean()))


def default_init(m, target):
    nj, nb = m['weights'].shape[1], m['shapedirs'].shape[2]
    return np.zeros(nj * 3), np.zeros(nb), target.mean(0) - m['v_template'].astype(np.float64).mean(0)


def fit(m, target, init=None, iters=20, f32=False, history=None):
    """One sample.  -> ((pose, betas, trans), rms).  f32: the state is rounded to float32 after every update and every forward
    quantity goes through float32 (the emulation of the device); the solve stays float64 either way.  history: a list that receives
    the current rms after every evaluation."""
    t = np.float32 if f32 else np.float64
    nv, nj = m['weights'].shape
    nb = m['shapedirs'].shape[2]
    P = 3 * nj + nb + 3
    target = np.asarray(target, np.float64)
    cand = tuple(np.asarray(a, t) for a in (default_init(m, target) if init is None else init))
    cur, Mcur, err, lam = None, None, np.inf, LAMBDA0
    for it in range(iters + 1):
        Jr, _ = jacobian(m, cand[0], cand[1], cand[2], target.astype(t) if f32 else target, f32)
        M = Jr.T @ Jr
        e = M[P, P]
        if it == 0:
            if not np.isfinite(e):
                nan = np.full(1, np.nan)
                return (nan.repeat(nj * 3), nan.repeat(nb), nan.repeat(3)), float('nan')
            cur, Mcur, err = cand, M, e
        elif e < err:
            cur, Mcur, err, lam = cand, M, e, max(lam / 4, LAMBDA_MIN)
        else:
            lam = min(8 * lam, LAMBDA_MAX)
        if history is not None:
            history.append(np.sqrt(err / nv))
        if it == iters:
            break
        H, g = Mcur[:P, :P], Mcur[:P, P]
        try:
            Lc = np.linalg.cholesky(H + lam * np.diag(np.diag(H)) + RIDGE * np.eye(P))
            d = -np.linalg.solve(Lc.T, np.linalg.solve(Lc, g))
        except np.linalg.LinAlgError:
            lam, d = min(8 * lam, LAMBDA_MAX), np.zeros(P)
        R, Rg, _, _, _ = parts(m, cur[0], cur[1])
        pose = np.zeros((nj, 3))
        for k in range(nj):
            Rp = np.eye(3) if k == 0 else Rg[int(m['parents'][k])]
            pose[k] = layer_axisang(so3_log(so3_exp(Rp.T @ d[3 * k:3 * k + 3]) @ R[k]))
        cand = (pose.reshape(-1).astype(t), (cur[1].astype(np.float64) + d[3 * nj:3 * nj + nb]).astype(t),
                (cur[2].astype(np.float64) + d[3 * nj + nb:]).astype(t))
    return tuple(np.asarray(a, np.float64) for a in cur), float(np.sqrt(err / nv))


# --- the targets of both test modules and the reference-side figures the device bounds take their margins from ---
NOISE_SIGMA = 0.005                   # 5 mm on a model in metres
ITERS, WARM_ITERS = 20, 8


def targets(name, max_angle):
    """(truth (pose, betas, trans) float32 [n, .], target [n, NV, 3] float64 = lbs_forward at the truth, rounded through float32 as the
    device receives it)."""
    truth = case_truth(name, max_angle)
    tgt, _ = sr.lbs_forward(model(name), *truth)
    return truth, tgt.astype(np.float32).astype(np.float64)


def table():
    """The case table as (label, case name, truth, target, init or None): zero initialisation up to 0.8 rad, the perturbed
    initialisation up to 1.2 rad."""
    for name in CASES:
        truth, tgt = targets(name, ZERO_INIT_MAX)
        yield name + '/zero', name, truth, tgt, None
        truth, tgt = targets(name, NEAR_INIT_MAX)
        yield name + '/near', name, truth, tgt, perturbed(name, truth)


def noisy_target():
    """nv257, sample 0 of the 0.8 rad draw, 5 mm Gaussian noise on every coordinate -> (case name, target [1, NV, 3] float64)."""
    truth, tgt = targets('nv257', ZERO_INIT_MAX)
    rs = np.random.RandomState(99)
    return 'nv257', (tgt[:1] + rs.randn(*tgt[:1].shape) * NOISE_SIGMA).astype(np.float32).astype(np.float64)


def e32_of(m, state, target):
    """rms over the vertices of (float32 forward - float64 forward) at a state: the float32 floor of one sample."""
    a, _ = jacobian(m, state[0], state[1], state[2], target, f32=True)
    b, _ = jacobian(m, state[0], state[1], state[2], target)
    d = (a[:, -1] - b[:, -1]).reshape(-1, 3)
    return float(np.sqrt((d * d).sum(-1).mean()))


def float32_floor():
    """Host test 4: the float32-emulated fit on the case table and on the noisy target.  -> (rows, ratio, excess): rows of
    (label, e32 at the truth, fp64-evaluated final rms of the emulated fit), the largest rms / e32, and the noisy case's
    rms32 / rms64 - 1 against the float64 fit's minimum."""
    rows, ratio = [], 0.0
    for label, name, truth, tgt, init in table():
        m = model(name)
        for i in range(len(tgt)):
            e32 = e32_of(m, tuple(a[i] for a in truth), tgt[i])
            st, _ = fit(m, tgt[i], None if init is None else tuple(a[i] for a in init), ITERS, f32=True)
            rms = rms_of(m, st, tgt[i])
            rows.append(('%s/%d' % (label, i), e32, rms))
            ratio = max(ratio, rms / e32)
    name, tgt = noisy_target()
    m = model(name)
    st64, _ = fit(m, tgt[0], None, ITERS)
    st32, _ = fit(m, tgt[0], None, ITERS, f32=True)
    r64, r32 = rms_of(m, st64, tgt[0]), rms_of(m, st32, tgt[0])
    rows.append(('noisy/fp64', float('nan'), r64))
    rows.append(('noisy/f32', float('nan'), r32))
    return rows, ratio, r32 / r64 - 1.0


# The figures float32_floor() gave when the bounds were set (profiles/smpl_fit.txt holds the whole table); the device tests use these,
# never the device's own output.  tests/test_host_smpl_fit_refs.py re-measures them and checks that they still cover this machine.
F32_RATIO = 1.0714474              # the emulated fit's largest fp64-evaluated rms / e32 over the case table
K_FLOOR = 2.0 * F32_RATIO          # device bound 2: rms <= K_FLOOR e32; the factor 2 covers the MFMA's different summation order
F32_NOISY_EXCESS = 2.74e-9         # |rms32 / rms64 - 1| on the noisy target.  The emulated fit ended BELOW the float64 fit there: with a
                                   # non-zero residual the iteration's fixed point (J^T r = 0 with the stated, truncated J) is not the exact
                                   # minimiser, and points around it differ in cost by this much either way.
EPS_NOISY = 10.0 * F32_NOISY_EXCESS
