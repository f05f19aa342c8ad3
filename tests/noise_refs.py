"""The detector noise restated in numpy (gator_amd/csrc/detector_noise.hip, include/gator_hip.h: gator_preprocess_noise_f32): the
reference's lib/noise_utils.synthesize_pose and generate_syn_error / replace_joint_img (data/Human36M/dataset.py:143-155, 421-453) with
numpy's generators replaced by the Philox4x32 stream of tests/train_refs.py.  Everything is evaluated -- every candidate of every
set -- and every decision is returned, so that the device can be compared decision for decision and the restatement's distribution
against recorded runs of the real functions (tests/golden/detector_noise.npz, tools/gen_golden_noise.py).

The crop chain in front of the noise is restated rounding for rounding as csrc/joints2d.h has it (crop_chain), because the candidates'
centres are its float32 results: the oracle's chain (oracle.gator_oracle.preprocess_pose2d) agrees with it to the chain's 2e-5, not
to the bit."""
import numpy as np

from tests.train_refs import DEVICE_ROUNDS, philox4x32

F32, F64 = np.float32, np.float64
NJ = 17
SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
SYMMETRY = ((1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16))
KS = (0.10, 0.50, 0.85)
N = 500                                         # jitter and inversion; miss 4 N per centre, good N // 4
SET_JITTER, SET_MISS0, SET_MISS1, SET_INV, SET_GOOD, SET_PICKS, SET_RESAMPLE, SET_STATS = range(8)
CASE_JITTER, CASE_MISS, CASE_INV, CASE_SWAP, CASE_GOOD = range(5)
UNDECIDED = 2.0 ** -40                          # a candidate whose distance is within this (relative) of its threshold is undecided
_M32 = 0xFFFFFFFF

COCO_FLIP_PAIRS = ((1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16))
H36M_FLIP_PAIRS = ((1, 4), (2, 5), (3, 6), (14, 11), (15, 12), (16, 13))


def partner_of(j):
    for q, w in SYMMETRY:
        if j == q:
            return w
        if j == w:
            return q
    return -1


def jitter_prob(j, n_valid):
    g = 0 if j == 0 or 13 <= j <= 16 else 1 if 1 <= j <= 10 else 2
    return ((0.15, 0.20, 0.25) if n_valid <= 10 else (0.10, 0.15, 0.20))[g]


def miss_prob(j, n_valid):
    g = 0 if 0 <= j <= 4 else 1 if j in (5, 6, 15, 16) else 2
    return ((0.15, 0.20, 0.25) if n_valid <= 5 else (0.10, 0.13, 0.15) if n_valid <= 10 else (0.02, 0.05, 0.10))[g]


def inv_prob(j):
    return 0.01 if j <= 4 else 0.03 if j <= 10 else 0.06


# ---- the stream -----------------------------------------------------------------------------------------------------------------
def words(seed, step, sample, set_, joint, index):
    """[n,4] uint32: the blocks of draw sites (set_, joint, index[i]) of one sample (include/gator_hip.h has the counter's packing)."""
    index = np.atleast_1d(np.asarray(index, np.uint64))
    ctr = np.empty((len(index), 4), np.uint64)
    ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = index, int(joint) | int(set_) << 8, int(sample) & _M32, int(step) & _M32
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox4x32(ctr, [[seed & _M32, seed >> 32]], DEVICE_ROUNDS)


def uniform(w):
    return (np.asarray(w).astype(F64) + 0.5) * 2.0 ** -32


def index_of(w, n):
    return (int(w) * int(n)) >> 32


# ---- the crop chain, csrc/joints2d.h rounding for rounding ------------------------------------------------------------------------
def crop_chain(joints, rot_deg, res):
    """joints [J,2|3] float32, image pixels -> (ok, T [2,3] fp64, tight box float32 (x, y, w, h)); ok False where process_bbox rejects."""
    x, y = joints[:, 0].astype(F64), joints[:, 1].astype(F64)
    xmin, xmax, ymin, ymax = x.min(), x.max(), y.min(), y.max()
    xc, bw0, yc, bh0 = (xmin + xmax) / 2., xmax - xmin, (ymin + ymax) / 2., ymax - ymin
    bxmin, bxmax, bymin, bymax = xc - 0.5 * bw0, xc + 0.5 * bw0, yc - 0.5 * bh0, yc + 0.5 * bh0
    box = np.array([bxmin, bymin, bxmax - bxmin, bymax - bymin]).astype(F32)
    bx, by, bw, bh = box
    one, two, half = F32(1), F32(2), F32(0.5)
    x2, y2 = bx + (bw - one), by + (bh - one)
    if not (bw * bh > 0 and x2 >= bx and y2 >= by):
        return False, None, box
    w, h = x2 - bx, y2 - by
    cx, cy = bx + w / two, by + h / two
    ar = F64(res[0]) / F64(res[1])
    if F64(w) > ar * F64(h):
        h = F32(F64(w) / ar)
    elif F64(w) < ar * F64(h):
        w = F32(F64(h) * ar)
    fx, fy = cx - w / two, cy - h / two
    cen0, cen1 = fx + w * half, fy + h * half
    rr = np.pi * F64(F32(rot_deg)) / 180.0
    sn, cs = np.sin(rr), np.cos(rr)
    p1 = F64(w * F32(-0.5))
    sd0, sd1 = 0.0 * cs - p1 * sn, 0.0 * sn + p1 * cs
    W, H = res
    src = np.zeros((3, 2), F32)
    dst = np.zeros((3, 2), F32)
    src[0] = cen0, cen1
    src[1] = F32(F64(cen0) + sd0), F32(F64(cen1) + sd1)
    dst[0] = F32(W) * half, F32(H) * half
    dst[1] = F32(W * 0.5 + 0.0), F32(H * 0.5 + F64(F32(W) * F32(-0.5)))
    for m in (src, dst):
        d0, d1 = m[0, 0] - m[1, 0], m[0, 1] - m[1, 1]
        m[2] = m[1, 0] + (-d1), m[1, 1] + d0
    (a0, b0), (a1, b1), (a2, b2) = src.astype(F64)
    det = a0 * (b1 - b2) - b0 * (a1 - a2) + (a1 * b2 - a2 * b1)
    T = np.zeros((2, 3))
    for r in range(2):
        d0, d1, d2 = dst[:, r].astype(F64)
        T[r, 0] = (d0 * (b1 - b2) - b0 * (d1 - d2) + (d1 * b2 - d2 * b1)) / det
        T[r, 1] = (a0 * (d1 - d2) - d0 * (a1 - a2) + (a1 * d2 - a2 * d1)) / det
        T[r, 2] = (a0 * (b1 * d2 - b2 * d1) - b0 * (a1 * d2 - a2 * d1) + d0 * (a1 * b2 - a2 * b1)) / det
    return True, T, box


def affine(T, x, y):
    x, y = np.asarray(x, F64), np.asarray(y, F64)
    return np.stack([T[0, 0] * x + T[0, 1] * y + T[0, 2], T[1, 0] * x + T[1, 1] * y + T[1, 2]], -1)


def box_area(T, box):
    """replace_joint_img's `area` (dataset.py:425-430): three corners of the tight float32 box through the affine."""
    xmin, ymin, xmax, ymax = box[0], box[1], box[0] + box[2], box[1] + box[3]                 # float32 sums
    p1, p2, p3 = affine(T, xmin, ymin), affine(T, xmax, ymin), affine(T, xmax, ymax)
    return np.sqrt((p2[0] - p1[0]) ** 2 + (p2[1] - p1[1]) ** 2) * np.sqrt((p3[0] - p2[0]) ** 2 + (p3[1] - p2[1]) ** 2)


def finish(crop, flip, pairs, res):
    """flip_2d_joint on the float32 crop joints, /[W,H] in float32, the standardisation with fp64 sums -> float32 [J,2]."""
    kp = crop.astype(F32).copy()
    if flip:
        kp[:, 0] = (F32(res[0]) - kp[:, 0]) - F32(1)
        for a, b in pairs:
            if a < len(kp) and b < len(kp):
                kp[a], kp[b] = kp[b].copy(), kp[a].copy()
    kp = kp / np.array([res[0], res[1]], F32)
    k64 = kp.astype(F64)
    J = len(kp)
    mean = np.array([sum(k64[:, 0].tolist()), sum(k64[:, 1].tolist())]) / J                   # sequential sums, as the kernel's
    d = k64 - mean
    std = np.sqrt(np.array([sum((d[:, 0] * d[:, 0]).tolist()), sum((d[:, 1] * d[:, 1]).tolist())]) / J)
    with np.errstate(all='ignore'):
        return (d / std).astype(F32)


# ---- synthesize_pose ----------------------------------------------------------------------------------------------------------------
def _candidates(stream, set_, j, n, centre, other, lo, hi, thr):
    """One candidate set: -> (x, y of the accepted candidates in candidate order, number of undecided candidates).  thr None: the
    candidate's own r."""
    w = words(*stream, set_, j, np.arange(n))
    angle = (2 * np.pi) * uniform(w[:, 0])
    r = lo + (hi - lo) * uniform(w[:, 1])
    x, y = centre[0] + r * np.cos(angle), centre[1] + r * np.sin(angle)
    if other is None:
        return x, y, 0
    t = r if thr is None else np.full(n, thr)
    dist = np.sqrt((other[0] - x) ** 2 + (other[1] - y) ** 2)
    mask = dist > t
    return x[mask], y[mask], int((np.abs(dist - t) <= UNDECIDED * t).sum())


def synthesize_joint(stream, j, n_valid, area, centre, other):
    """One joint of synthesize_pose.  centre, other: float32-valued (x, y), other None when the partner does not count.
    -> dict(counts [5], case, pick, sub, xy float32 [2], undecided)."""
    var = (SIGMAS * 2) ** 2
    d10, d50, d85 = (np.sqrt(-2 * area * var * np.log(ks))[j] for ks in KS)
    c = (F64(centre[0]), F64(centre[1]))
    o = None if other is None else (F64(other[0]), F64(other[1]))
    sets = {SET_JITTER: _candidates(stream, SET_JITTER, j, N, c, o, d85, d50, None),
            SET_MISS0: _candidates(stream, SET_MISS0, j, 4 * N, c, o, d50, d10, d50),
            SET_GOOD: _candidates(stream, SET_GOOD, j, N // 4, c, o, 0.0, d85, None)}
    empty = (np.zeros(0), np.zeros(0), 0)
    sets[SET_MISS1] = _candidates(stream, SET_MISS1, j, 4 * N, o, c, d50, d10, d50) if o is not None else empty
    sets[SET_INV] = _candidates(stream, SET_INV, j, N, o, c, 0.0, d50, None) if o is not None else empty
    counts = [len(sets[s][0]) for s in (SET_JITTER, SET_MISS0, SET_MISS1, SET_INV, SET_GOOD)]
    nj, nm0, nm1, ni, ng = counts
    nmiss = nm0 + nm1 // 4
    jp, mp, ip, sp = jitter_prob(j, n_valid), miss_prob(j, n_valid), inv_prob(j), 0
    gp = 1 - (jp + mp + ip + sp)
    assert gp >= 0
    if nj == 0:
        jp = 0
    if ni == 0:
        ip = 0
    if nmiss == 0:
        mp = 0
    if ng == 0:
        gp = 0
    out = dict(counts=counts, case=-1, pick=-1, sub=-1, xy=np.zeros(2, F32), undecided=sum(v[2] for v in sets.values()))
    normalizer = jp + mp + ip + sp + gp
    if normalizer == 0:
        return out
    p = np.array([jp / normalizer, mp / normalizer, ip / normalizer, sp / normalizer, gp / normalizer], F64)
    cdf = p.cumsum()
    cdf /= cdf[-1]
    picks, choice = words(*stream, SET_PICKS, j, [0, 1])
    case = int(cdf.searchsorted(uniform(choice[0]), side='right'))
    if case == CASE_JITTER:
        pick = index_of(picks[0], nj)
        xy = sets[SET_JITTER][0][pick], sets[SET_JITTER][1][pick]
    elif case == CASE_MISS:
        pick = index_of(picks[1], nmiss)
        if pick < nm0:
            xy = sets[SET_MISS0][0][pick], sets[SET_MISS0][1][pick]
        else:
            out['sub'] = sub = index_of(words(*stream, SET_RESAMPLE, j, [pick - nm0])[0, 0], nm1)
            xy = sets[SET_MISS1][0][sub], sets[SET_MISS1][1][sub]
    elif case == CASE_INV:
        pick = index_of(picks[2], ni)
        xy = sets[SET_INV][0][pick], sets[SET_INV][1][pick]
    else:
        assert case == CASE_GOOD
        pick = index_of(picks[3], ng)
        xy = sets[SET_GOOD][0][pick], sets[SET_GOOD][1][pick]
    out.update(case=case, pick=pick, xy=np.array(xy).astype(F32))
    return out


def synthesize_pose(crop, joint_valid, area, stream):
    """lib/noise_utils.synthesize_pose on float32 crop joints [17,2] with validity [17], joints in order: a joint reads its partner's
    CURRENT position (perturbed when the partner comes first) and ORIGINAL validity.  -> (synth float32 [17,2], list of 17 decisions)."""
    synth = crop.astype(F32).copy()
    n_valid = int((np.asarray(joint_valid) > 0).sum())
    decisions = []
    for j in range(NJ):
        q = partner_of(j)
        other = synth[q] if q >= 0 and joint_valid[q] > 0 else None
        d = synthesize_joint(stream, j, n_valid, area, synth[j], other)
        synth[j] = d['xy']
        decisions.append(d)
    return synth, decisions


# ---- generate_syn_error -------------------------------------------------------------------------------------------------------------
def syn_error(table, stream):
    """table [J,5] fp64 (mean xy, std xy, weight) -> noise float32 [J,2], applied [J] bool: generate_syn_error with Box-Muller normals."""
    J = len(table)
    noise, applied = np.zeros((J, 2), F32), np.zeros(J, bool)
    for j in range(J):
        w = words(*stream, SET_STATS, j, [0])[0]
        rad, ang = np.sqrt(-2.0 * np.log(uniform(w[0]))), (2 * np.pi) * uniform(w[1])
        noise[j] = table[j, 0] + table[j, 2] * (rad * np.cos(ang)), table[j, 1] + table[j, 3] * (rad * np.sin(ang))
        applied[j] = F64(F32(table[j, 4])) > uniform(w[2])
    return noise * applied[:, None].astype(F32), applied


# ---- the whole call -------------------------------------------------------------------------------------------------------------------
def noisy_input(joints, mode, *, seed=0, step=0, sample_offset=0, joint_valid=None, rot_deg=None, flip=None, flip_pairs=(), res=(288, 384),
                table=None, detections=None):
    """gator_preprocess_noise_f32 for a batch [B,J,2|3] float32.  mode 'coco' | 'stats' | 'detections' | 'clean' (no noise at all).
    -> dict(pose2d [B,J,2] f32, valid [B], crop [B,J,2] f32 (noisy), clean [B,J,2] f32, area [B], decisions: per sample a list of 17
    dicts or None, undecided: total)."""
    joints = np.asarray(joints, F32)
    B, J = joints.shape[:2]
    out = dict(pose2d=np.zeros((B, J, 2), F32), valid=np.zeros(B, np.int32), crop=np.zeros((B, J, 2), F32), clean=np.zeros((B, J, 2), F32),
               area=np.zeros(B), decisions=[None] * B, undecided=0)
    for b in range(B):
        rot = 0.0 if rot_deg is None else rot_deg[b]
        ok, T, box = crop_chain(joints[b], rot, res)
        if not ok:
            continue
        out['valid'][b] = 1
        src = detections[b] if mode == 'detections' else joints[b]
        crop = affine(T, src[:, 0], src[:, 1]).astype(F32)
        out['clean'][b] = affine(T, joints[b, :, 0], joints[b, :, 1]).astype(F32)
        out['area'][b] = box_area(T, box)
        stream = (seed, step, sample_offset + b)
        if mode == 'coco':
            jv = np.ones(J, F32) if joint_valid is None else np.asarray(joint_valid[b], F32).reshape(-1)
            crop[:NJ], dec = synthesize_pose(crop[:NJ], jv[:NJ], out['area'][b], stream)
            out['decisions'][b] = dec
            out['undecided'] += sum(d['undecided'] for d in dec)
        elif mode == 'stats':
            noise, _ = syn_error(np.asarray(table, F64), stream)
            crop = crop + noise / F32(256) * np.array([res[0], res[1]], F32)
        out['crop'][b] = crop
        out['pose2d'][b] = finish(crop, bool(flip[b]) if flip is not None else False, flip_pairs, res)
    return out


def decisions_array(decisions):
    """The device's [B,17,8] int32 layout of noisy_input's decisions (-1 rows where the box was rejected)."""
    out = np.full((len(decisions), NJ, 8), -1, np.int32)
    for b, dec in enumerate(decisions):
        if dec is not None:
            for j, d in enumerate(dec):
                out[b, j] = d['counts'] + [d['case'], d['pick'], d['sub']]
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
COCO_T_POSE = np.array([[0, -62], [4, -66], [-4, -66], [9, -63], [-9, -63], [19, -40], [-19, -40], [30, -12], [-30, -12], [34, 14], [-34, 14],
                        [12, 10], [-12, 10], [13, 50], [-13, 50], [14, 88], [-14, 88]], F64)


def coco_pose(rs, scale=4.0, centre=(500.0, 400.0), spread=0.08, pelvis_neck=False):
    """A standing COCO pose of about 150 * scale pixels with every joint moved by spread * its distance scale: partners stay distinct."""
    p = COCO_T_POSE * (1.0 + rs.uniform(-spread, spread, COCO_T_POSE.shape)) + rs.uniform(-3, 3, COCO_T_POSE.shape)
    a = rs.uniform(-0.4, 0.4)
    p = p @ np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]).T * scale + np.asarray(centre)
    if pelvis_neck:
        p = np.concatenate([p, (p[11:12] + p[12:13]) * 0.5, (p[5:6] + p[6:7]) * 0.5])
    return p.astype(F32)


def histogram(xy, ref, area, j):
    """The fixture's bins for one joint's outputs xy [n,2] against the point ref: [0, ks85), [ks85, ks50), [ks50, ks10), >= ks10, zeroed."""
    var = (SIGMAS * 2) ** 2
    edges = [np.sqrt(-2 * area * var[j] * np.log(ks)) for ks in (0.85, 0.50, 0.10)]
    zero = (xy == 0).all(1)
    d = np.sqrt(((xy.astype(F64) - np.asarray(ref, F64)) ** 2).sum(1))[~zero]
    return np.array([(d < edges[0]).sum(), ((d >= edges[0]) & (d < edges[1])).sum(), ((d >= edges[1]) & (d < edges[2])).sum(),
                     (d >= edges[2]).sum(), zero.sum()], np.int64)


# ---- the cases the GPU tests restate (tests/test_gpu_noise.py), checked on the host for undecided candidates first --------------------
_CASES = {}


def gpu_case(name):
    """Inputs of one restated GPU case, at most 16 samples: dict(joints, mode, kw) with kw for noisy_input here and on the device."""
    if name in _CASES:
        return _CASES[name]
    rs = np.random.RandomState({'coco19': 11, 'stats17': 12, 'detections19': 13}[name])
    if name == 'coco19':                        # J = 19, rotation and flip on, the three validity tiers, a rejected box
        B = 12
        joints = np.stack([coco_pose(rs, scale=rs.uniform(1.0, 5.0), centre=rs.uniform(200, 800, 2), pelvis_neck=True) for _ in range(B)])
        joints[7, :, 0] = joints[7, 0, 0]                                      # no width: process_bbox rejects it
        valid = np.ones((B, 19), F32)
        valid[3:6, [0, 3, 4, 6, 9, 13, 16]] = 0                                # 10 valid
        valid[8:11] = 0
        valid[8:11, [1, 2, 5, 11, 14]] = 1                                     # 5 valid
        valid[11, 17:] = 0                                                     # rows beyond the 17 do not count
        kw = dict(seed=0x9E3779B97F4A7C15, step=3, sample_offset=1000, joint_valid=valid, flip_pairs=COCO_FLIP_PAIRS + ((17, 18),))
    elif name == 'stats17':                     # J = 17, a rejected box
        B = 12
        joints = (rs.rand(B, 17, 3) * np.array([300.0, 500.0, 1.0]) + np.array([100.0, 80.0, 0.0])).astype(F32)
        joints[5, :, 1] = joints[5, 0, 1]
        kw = dict(seed=77, step=2 ** 31 + 5, sample_offset=2 ** 32 - B, flip_pairs=H36M_FLIP_PAIRS)
    else:                                       # the test split: detections through the clean joints' crop
        B = 5
        joints = np.stack([coco_pose(rs, scale=rs.uniform(1.0, 5.0), centre=rs.uniform(200, 800, 2), pelvis_neck=True) for _ in range(B)])
        joints[2, :, 0] = joints[2, 0, 0]
        kw = dict(seed=1, detections=(joints + rs.randn(B, 19, 2) * 6.0).astype(F32), flip_pairs=COCO_FLIP_PAIRS)
    rots = np.array([0.0, 30.0, -30.0, 12.5, -47.0, 60.0], F32)
    kw.update(rot_deg=rots[np.arange(B) % len(rots)], flip=((np.arange(B) // 2) % 2).astype(np.int32), res=(288, 384))
    _CASES[name] = dict(joints=joints, mode=name.rstrip('0123456789'), kw=kw)
    return _CASES[name]


_RESTATED = {}


def restated(name, table=None):
    """noisy_input of gpu_case(name), computed once and shared; table: the [17,5] error table for 'stats17'."""
    if name not in _RESTATED:
        c = gpu_case(name)
        _RESTATED[name] = noisy_input(c['joints'], c['mode'], table=table, **c['kw'])
    return _RESTATED[name]
