"""gator_preprocess_noise_f32 / gator_amd.noise on the device.

Against tests/noise_refs.py, which evaluates every candidate in numpy from the same Philox stream: the accepted counts, the chosen case
and the chosen index are equal EXACTLY (tests/test_host_noise_refs.py checks on the CPU that none of these inputs has a candidate within
a relative 2^-40 of its threshold); the noisy crop joints agree within one float32 rounding, |d| <= 2^-23 |value| (the device and
numpy may round an fp64 value that differs in its last bits to neighbouring float32 values); pose2d is held to the chain's own
criterion, 2e-5 (tests/test_gpu_eval_edges.py: _check_chain).  Everything else -- batch and shard invariance, determinism, graph replay,
zero noise, camera_frame_batch -- is bit for bit.

The kernels' boundaries: k_noise_crop and k_noise_finish take one lane per sample in 64-lane blocks (batches 63, 64, 65, 130);
k_noise_candidates takes one wave per (sample, joint) and has no batch boundary of its own."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from gator_amd import _lib, batch, noise, preprocess
from tests import noise_refs as nr
from tests.helpers import load_golden

pytestmark = pytest.mark.gpu

EINVAL = -1
F32_ROUNDING = 2.0 ** -23
CHAIN_TOL = 2e-5


def dev(x, dtype=torch.float32):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to('cuda', dtype)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def stats_table():
    return load_golden('detector_noise')['stats_table']


@functools.lru_cache(maxsize=None)
def stats_model():
    t = stats_table()
    return noise.ErrorStatsNoise(t[:, :2], t[:, 2:4], t[:, 4])


def device_kwargs(kw):
    """noise_refs' keyword arguments as noisy_input takes them."""
    out = {k: v for k, v in kw.items() if k not in ('joint_valid', 'rot_deg', 'flip', 'detections')}
    out['rot_deg'], out['flip'] = dev(kw['rot_deg']), dev(kw['flip'], torch.int32)
    if kw.get('joint_valid') is not None:
        out['joint_valid'] = dev(kw['joint_valid'])
    if kw.get('detections') is not None:
        out['detections'] = dev(kw['detections'])
    return out


def run_case(name, **extra):
    c = nr.gpu_case(name)
    model = {'coco': noise.CocoDetectorNoise(), 'stats': stats_model(), 'detections': None}[c['mode']]
    return noise.noisy_input(dev(c['joints']), model, **{**device_kwargs(c['kw']), **extra})


def check_against_restatement(name, got, ref):
    pose2d, valid, crop = (t.cpu().numpy() for t in got[:3])
    assert np.array_equal(valid, ref['valid']) and (valid == 0).sum() == 1
    assert not pose2d[valid == 0].any() and not crop[valid == 0].any()
    err = np.abs(crop.astype(np.float64) - ref['crop'])
    bound = F32_ROUNDING * np.abs(ref['crop'].astype(np.float64))
    print('\n%s: noisy crop worst |device - restatement| %.3e (bound %.3e there), differing values %d of %d' %
          (name, err.max(), bound.reshape(-1)[err.argmax()], int((err > 0).sum()), err.size))
    assert (err <= bound).all()
    perr = np.abs(pose2d.astype(np.float64) - ref['pose2d']).max()
    print('%s: pose2d worst |device - restatement| %.3e (criterion %.0e)' % (name, perr, CHAIN_TOL))
    assert perr <= CHAIN_TOL and np.isfinite(pose2d).all()
    return pose2d, valid, crop


def test_coco_noise_equals_the_restatement_decision_for_decision():
    """J = 19 with rows 17 and 18 clean, rotation and flip on, the three validity tiers, a rejected box."""
    ref = nr.restated('coco19')
    assert ref['undecided'] == 0
    got = run_case('coco19', return_decisions=True)
    pose2d, valid, crop = check_against_restatement('coco19', got, ref)
    want = nr.decisions_array(ref['decisions'])
    dec = got[3].cpu().numpy()
    assert np.array_equal(dec, want), np.argwhere(dec != want)[:8]
    assert np.array_equal(crop[:, 17:], ref['clean'][:, 17:])                              # pelvis and neck keep the clean crop joints
    moved = np.abs(crop[valid == 1][:, :17] - ref['clean'][valid == 1][:, :17]).max(2)
    assert (moved > 0).all()                                                               # every one of the 17 was perturbed
    cases = dec[valid == 1][:, :, 5]
    print('coco19: cases taken %s' % {noise.CASES[c]: int((cases == c).sum()) for c in np.unique(cases)})


def test_stats_noise_equals_the_restatement():
    """J = 17, the Human3.6M table, rotation and flip on, a rejected box, sample indices up to 2^32 - 1 and a step above 2^31."""
    ref = nr.restated('stats17', table=stats_table())
    pose2d, valid, crop = check_against_restatement('stats17', run_case('stats17'), ref)
    applied = (crop != ref['clean'])[valid == 1].any(2)
    want = np.stack([nr.syn_error(stats_table(), (77, 2 ** 31 + 5, 2 ** 32 - 12 + b))[1] for b in range(12)])[valid == 1]
    assert np.array_equal(applied, want)


def test_detections_mode_equals_the_restatement():
    ref = nr.restated('detections19')
    pose2d, valid, crop = check_against_restatement('detections19', run_case('detections19'), ref)
    assert (np.abs(crop - ref['clean'])[valid == 1].max((1, 2)) > 0.1).all()                # the detections, not the clean joints


@functools.lru_cache(maxsize=None)
def big_batch(mode):
    rs = np.random.RandomState(5 if mode == 'coco' else 6)
    B = 130
    if mode == 'coco':
        joints = np.stack([nr.coco_pose(rs, scale=rs.uniform(1.0, 5.0), centre=rs.uniform(200, 800, 2), pelvis_neck=True) for _ in range(B)])
        valid = (rs.rand(B, 19) < 0.7).astype(np.float32)
        valid[::3] = 1
    else:
        joints = (rs.rand(B, 17, 2) * np.array([300.0, 500.0]) + 100.0).astype(np.float32)
        valid = None
    joints[64, :, 0] = joints[64, 0, 0]                                                     # a rejected box at a block's first lane
    rot = (rs.rand(B) * 120 - 60).astype(np.float32)
    flip = (rs.rand(B) < 0.5).astype(np.int32)
    return joints, valid, rot, flip


def call(mode, joints, valid, rot, flip, sl=slice(None), **kw):
    model = noise.CocoDetectorNoise() if mode == 'coco' else stats_model()
    pairs = nr.COCO_FLIP_PAIRS if mode == 'coco' else nr.H36M_FLIP_PAIRS
    args = dict(seed=2025, step=4, joint_valid=None if valid is None else dev(valid[sl]), rot_deg=dev(rot[sl]), flip=dev(flip[sl], torch.int32),
                flip_pairs=pairs, return_decisions=mode == 'coco')
    args.update(kw)
    return noise.noisy_input(dev(joints[sl]), model, **args)


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


@pytest.mark.parametrize('mode', ['coco', 'stats'])
def test_batch_and_shard_invariance_bitwise(mode):
    """Batches of 1, 63, 64, 65 and 130 (either side of the 64-lane blocks); a row is the single-sample call at its sample_offset; two
    halves are the whole; an offset batch is the tail of the whole."""
    joints, valid, rot, flip = big_batch(mode)
    whole = call(mode, joints, valid, rot, flip)
    assert int(whole[1].sum()) == 129 and not whole[0][64].any()
    for B in (1, 63, 64, 65):
        part = call(mode, joints, valid, rot, flip, slice(0, B))
        assert same(part, [t[:B] for t in whole]), B
    for b in (0, 63, 64, 65, 129):
        one = call(mode, joints, valid, rot, flip, slice(b, b + 1), sample_offset=b)
        assert same(one, [t[b:b + 1] for t in whole]), b
    lo = call(mode, joints, valid, rot, flip, slice(0, 65))
    hi = call(mode, joints, valid, rot, flip, slice(65, 130), sample_offset=65)
    assert same([torch.cat([x, y]) for x, y in zip(lo, hi)], whole)
    other = call(mode, joints, valid, rot, flip, slice(0, 8), sample_offset=1)               # another sample index: other noise
    assert not torch.equal(other[2], whole[2][:8])


@pytest.mark.parametrize('mode', ['coco', 'stats'])
def test_determinism_steps_and_graph_replay(mode):
    """The same seed and step twice: the same bits.  Another step or seed: other noise.  A device step word gives the host step's bits,
    and a captured graph replayed after the word is advanced equals the eager calls of those steps."""
    joints, valid, rot, flip = big_batch(mode)
    sl = slice(0, 65)
    a, b = call(mode, joints, valid, rot, flip, sl), call(mode, joints, valid, rot, flip, sl)
    assert same(a, b)
    for kw in (dict(step=5), dict(seed=2026)):
        c = call(mode, joints, valid, rot, flip, sl, **kw)
        assert not torch.equal(c[2], a[2]) and torch.equal(c[1], a[1])
    word = torch.tensor([4], dtype=torch.int64, device='cuda')
    assert same(call(mode, joints, valid, rot, flip, sl, step=word), a)
    eager = {s: call(mode, joints, valid, rot, flip, sl, step=s) for s in (4, 5, 6)}
    model = noise.CocoDetectorNoise() if mode == 'coco' else stats_model()
    x, r, f = dev(joints[sl]), dev(rot[sl]), dev(flip[sl], torch.int32)
    v = None if valid is None else dev(valid[sl])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = noise.noisy_input(x, model, seed=2025, step=word, joint_valid=v, rot_deg=r, flip=f)
    for s in (4, 5, 6):
        word.fill_(s)
        g.replay()
        torch.cuda.synchronize()
        # the captured call has no flip pairs (their table would be copied from the host inside the capture): compare with its eager twin
        want = noise.noisy_input(x, model, seed=2025, step=s, joint_valid=v, rot_deg=r, flip=f)
        assert same(out, want), s
        assert torch.equal(out[2], eager[s][2])                                             # the noisy crop joints do not depend on the pairs


def test_zero_noise_is_the_existing_chain():
    """A table of zero weights: valid and -- for every sample that is not flipped -- pose2d of preprocess_chain, bit for bit, with
    rotation on.  A flipped sample is held to the chain's 2e-5: the training datasets flip the float32 joints AFTER the noise step
    (data/Human36M/dataset.py:369-373), preprocess_chain flips in fp64 before the float32 cast as j2d_processing(f=1) does
    (lib/aug_utils.py:61-63), and W - float32(x) - 1 in float32 is not always float32(W - x - 1).  Measured on one MI355X: 0 for
    the 130 samples without a flip, at most 3.6e-7 with 55 of them flipped."""
    joints, _, rot, flip = big_batch('stats')
    t = stats_table()
    zero = noise.ErrorStatsNoise(t[:, :2], t[:, 2:4], np.zeros(17))
    x = dev(joints)
    for fl in (np.zeros_like(flip), flip):
        pose2d, valid, crop = noise.noisy_input(x, zero, seed=1, rot_deg=dev(rot), flip=dev(fl, torch.int32), flip_pairs=nr.H36M_FLIP_PAIRS)
        want, ok = preprocess.preprocess_chain(x, dev(rot), dev(fl, torch.int32), nr.H36M_FLIP_PAIRS)
        assert torch.equal(valid, ok)
        keep = torch.from_numpy(fl == 0).cuda()
        assert torch.equal(pose2d[keep], want[keep])
        err = (pose2d - want).abs().max().item()
        print('\nzero noise, %d flipped samples: worst |noisy_input - preprocess_chain| %.3e' % (int(fl.sum()), err))
        assert err <= CHAIN_TOL
    assert flip.sum() > 30 and (flip == 0).sum() > 30


@pytest.mark.parametrize('lift_set', ['human36', 'coco'])
def test_camera_frame_batch_with_and_without_noise(lift_set):
    from tests.test_gpu_batch import e2e_setup
    from gator_amd import eval as gator_eval
    c, layer, pose, betas, trans, R, cam_t, focal, princpt, h, k = e2e_setup()
    pairs = nr.COCO_FLIP_PAIRS if lift_set == 'coco' else nr.H36M_FLIP_PAIRS
    rot, flip = dev(np.float32([0.0, 30.0, -90.0])), dev(np.int32([1, 0, 1]), torch.int32)
    regs = [gator_eval._Coo(*x[:3], 17, 6890, 'cuda', 'test') for x in (h, k)]
    kw = dict(trans=dev(trans), cam_R=dev(R), cam_t=dev(cam_t), compensate_root=True, focal=dev(focal), princpt=dev(princpt), regressor_h36m=regs[0],
              regressor_coco=regs[1], input_joint_name=lift_set, rot_deg=rot, flip=flip, flip_pairs=pairs)
    model = noise.CocoDetectorNoise() if lift_set == 'coco' else stats_model()
    plain = batch.camera_frame_batch(layer, dev(pose), dev(betas), **kw)
    clean = [{k_: v.clone() for k_, v in d.items()} for d in plain]
    noisy = batch.camera_frame_batch(layer, dev(pose), dev(betas), noise=model, noise_seed=9, noise_step=2, **kw)
    # noise=None: what the function did before -- preprocess_chain on its own joint_img -- and no new key
    p2d, ok = preprocess.preprocess_chain(clean[2]['joint_img'], rot, flip, pairs, res=(288, 384))
    assert torch.equal(clean[0]['pose2d'], p2d) and torch.equal(clean[2]['input_valid'], ok) and 'joint_crop_noisy' not in clean[2]
    # noise=: noisy_input on its own meta['joint_img']; everything else untouched
    want = noise.noisy_input(noisy[2]['joint_img'], model, seed=9, step=2, rot_deg=rot, flip=flip, flip_pairs=pairs)
    assert torch.equal(noisy[0]['pose2d'], want[0]) and torch.equal(noisy[2]['input_valid'], want[1]) and torch.equal(noisy[2]['joint_crop_noisy'], want[2])
    assert not torch.equal(noisy[0]['pose2d'], clean[0]['pose2d']) and torch.isfinite(noisy[0]['pose2d']).all()
    for k_ in clean[1]:
        assert torch.equal(noisy[1][k_], clean[1][k_]), k_
    for k_ in clean[2]:
        assert torch.equal(noisy[2][k_], clean[2][k_], ) or k_ == 'fit_error' and torch.isnan(clean[2][k_]).all(), k_
    with pytest.raises(ValueError):
        batch.camera_frame_batch(layer, dev(pose), dev(betas), noise='coco', **kw)


def _args(B=3, J=19, mode=_lib.NOISE_COCO):
    """A complete, valid argument struct and the tensors it points to (outputs filled with a sentinel)."""
    rs = np.random.RandomState(1)
    t = dict(joints=dev(np.stack([nr.coco_pose(rs, pelvis_neck=True) for _ in range(B)])[:, :J]),
             stats=dev(np.ones((J, 5)), torch.float64), detections=dev(rs.rand(B, J, 2) * 100),
             pose2d=torch.full((B, J, 2), 7.0, device='cuda'), noisy_crop=torch.full((B, J, 2), 7.0, device='cuda'),
             valid=torch.full((B,), 7, device='cuda', dtype=torch.int32), area=torch.full((B,), 7.0, device='cuda', dtype=torch.float64))
    a = _lib.PreprocessNoiseArgs()
    a.struct_size = ctypes.sizeof(_lib.PreprocessNoiseArgs)
    a.batch, a.n_joints, a.comps, a.mode, a.n_pairs, a.res_w, a.res_h = B, J, 2, mode, 0, 288, 384
    a.seed, a.step, a.sample_offset = 1, 0, 0
    for name in ('joints', 'stats', 'detections', 'pose2d', 'noisy_crop', 'valid', 'area'):
        setattr(a, name, t[name].data_ptr())
    model = noise.CocoDetectorNoise().struct()
    a.coco = ctypes.pointer(model)
    t['model'] = model
    return a, t


def test_c_abi_edges():
    """Every refusal returns GATOR_EINVAL with the function's name in gator_last_error(), before any launch: the outputs keep their
    sentinel.  The valid struct runs (so that each refusal below is due to its one change)."""
    lib = _lib.load()
    fn = lib.gator_preprocess_noise_f32
    a, t = _args()
    assert fn(ctypes.byref(a), stream()) == 0
    torch.cuda.synchronize()
    assert (t['valid'] == 1).all() and (t['pose2d'] != 7.0).all()

    def refused(change, J=19, mode=_lib.NOISE_COCO):
        a, t = _args(J=J, mode=mode)
        change(a)
        assert fn(ctypes.byref(a), stream()) == EINVAL
        assert b'gator_preprocess_noise_f32' in lib.gator_last_error()
        torch.cuda.synchronize()
        for name in ('pose2d', 'noisy_crop', 'valid', 'area'):
            assert (t[name] == 7).all(), name

    assert fn(None, stream()) == EINVAL and b'gator_preprocess_noise_f32' in lib.gator_last_error()
    for name in ('joints', 'pose2d', 'valid', 'noisy_crop'):
        refused(lambda a, n=name: setattr(a, n, None))
    refused(lambda a: setattr(a, 'struct_size', a.struct_size - 8))
    refused(lambda a: setattr(a, 'struct_size', a.struct_size + 8))
    refused(lambda a: setattr(a, 'n_joints', 33))
    refused(lambda a: setattr(a, 'n_joints', 0))
    refused(lambda a: None, J=16)                                                           # coco with fewer than 17 joints
    refused(lambda a: setattr(a, 'coco', None))
    refused(lambda a: setattr(a, 'area', None))
    refused(lambda a: setattr(a, 'stats', None), J=17, mode=_lib.NOISE_STATS)
    refused(lambda a: setattr(a, 'detections', None), mode=_lib.NOISE_DETECTIONS)
    refused(lambda a: setattr(a, 'mode', 3))
    refused(lambda a: setattr(a, 'comps', 1))
    refused(lambda a: setattr(a, 'res_w', 0))
    refused(lambda a: setattr(a, 'n_pairs', 2))                                             # pairs without a table
    refused(lambda a: setattr(a, 'batch', -1))
    refused(lambda a: setattr(a, 'sample_offset', -1))
    refused(lambda a: setattr(a, 'sample_offset', 2 ** 32 - 2))

    def broken_model(a):
        m = noise.CocoDetectorNoise().struct()
        m.partner[3] = 5                                                                    # 3 -> 5 but 5 -> 6: no pairing
        a.coco = ctypes.pointer(m)
    refused(broken_model)

    def no_candidates(a):
        m = noise.CocoDetectorNoise().struct()
        m.n_miss = 0
        a.coco = ctypes.pointer(m)
    refused(no_candidates)
    a, t = _args()
    a.batch = 0
    assert fn(ctypes.byref(a), stream()) == 0                                               # an empty batch is no error and launches nothing
