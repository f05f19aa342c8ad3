"""Digest of the forward's outputs for a few (variant, batch, encoder pin) cases.
  * A/B of two builds: run it under each (GATOR_AMD_LIB=...) and compare the lines -- equal digests = bitwise equal results.
  * `--write tests/golden/fp32_digests.json` records the digests of the CURRENT library (on a GPU box); tests/test_gpu_digest.py then
    holds every later build to them, so that a change that is meant to be a schedule only (round 4: dead token rows, C-layout GELU,
    zero operands on dead lanes) is checked bit for bit by the suite instead of by hand.  Re-record only with a change that is MEANT to
    move bits, together with the error budget (tests/error_budget.py).
  * `--forms --write tests/golden/mdr_form_digests.json` does the same for form_digests(): the MDR kernels' non-default arithmetic forms
    and whole-head kernels at B = 11, which the fp32 digests above never reach.
python tools/ab_digest.py [tag] [--forms] [--write path [--commit hash-of-the-recorded-build]]"""
import contextlib, hashlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gator_amd import synthetic
from tests.helpers import build_model

VARIANTS = (('h36m17_bn', 17), ('coco19_alpha', 19))
CASES = [(name, J, B, pin) for name, J in VARIANTS for B, pin in ((5, 'auto'), (256, 'auto'), (700, 'auto'), (700, 'tiled'))]


def digests():
    out = {}
    models = {}
    for name, J, B, pin in CASES:
        if name not in models:
            models[name] = build_model(name, 'fused')[1]
        m = models[name]
        m.set_encoder(pin)
        x = torch.from_numpy(synthetic.synthetic_pose2d(B, J, seed=B)).cuda()
        v, p = m(x)
        torch.cuda.synchronize()
        m.set_encoder('auto')
        assert bool(torch.isfinite(v).all())
        out['%s B=%d %s' % (name, B, pin)] = hashlib.sha256(v.cpu().numpy().tobytes() + p.cpu().numpy().tobytes()).hexdigest()[:32]
    return out


# The MDR kernels' forms (mdr_fused.hip / mdr_head.hip): operand arithmetic XA = 2 (default), 1 (exact split), 0 (fp32-input MFMA), 3 (config 3:
# precision 'bf16'), and the whole-head kernels instead of the tiles' partial sums + k_mdr_head_finish.
FORMS = {'default': ({}, 'f32'), 'x3_1': ({'GATOR_MDR_X3': '1'}, 'f32'), 'x3_0': ({'GATOR_MDR_X3': '0'}, 'f32'), 'bf16': ({}, 'bf16'),
         'head_partials0': ({'GATOR_MDR_HEAD_PARTIALS': '0'}, 'f32')}
FORM_SWITCHES = ('GATOR_MDR_X3', 'GATOR_MDR_HEAD_PARTIALS', 'GATOR_MDR_PERSIST')
FORM_B = 11     # XCD queues 0-2 hold two samples and 3-7 one (a last ticket with two dead waves), the four-launch grid of 39 workgroups ends half empty, token tile 13 lacks 17 keys
FORM_B_ROLLED = 513     # k_mdr_head<512, false> (the rolled whole head) is planned only above 2 x 256 CUs' worth of samples


@contextlib.contextmanager
def _switches(env):
    old = {k: os.environ.get(k) for k in FORM_SWITCHES}
    try:
        for k in FORM_SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _sha(*tensors):
    return hashlib.sha256(b''.join(t.cpu().numpy().tobytes() for t in tensors)).hexdigest()[:32]


def form_digests(forms=None):
    """{'<form> persist=<0|1> <variant> B=<B> <forward|pose2mesh>': digest}.  'forward' is the whole forward (vertices + pose3d);
    'pose2mesh' is the MDR entry point on a seeded randn pose_combine (k_mdr_joint and the pc branch of tile mode 0, both JointArgs::x2).
    The switches are read when a context is created, so every case drops the models' contexts first."""
    out = {}
    models = {name: build_model(name, 'fused')[1] for name, _ in VARIANTS}
    for form in (forms or FORMS):
        env, precision = FORMS[form]
        for persist in ('0', '1'):
            for name, J in VARIANTS:
                batches = (FORM_B, FORM_B_ROLLED) if form == 'head_partials0' and name == 'h36m17_bn' else (FORM_B,)
                for B in batches:
                    m = models[name]
                    with _switches(dict(env, GATOR_MDR_PERSIST=persist)):
                        m.invalidate()
                        m.pose2mesh.invalidate()
                        m.precision = precision
                        x = torch.from_numpy(synthetic.synthetic_pose2d(B, J, seed=B)).cuda()
                        v, p = m(x)
                        pc = torch.randn((B, J, 133), generator=torch.Generator().manual_seed(B)).cuda()
                        w = m.pose2mesh(pc)
                        torch.cuda.synchronize()
                        m.precision = 'f32'
                        m.invalidate()
                        m.pose2mesh.invalidate()
                    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(w).all())
                    key = '%s persist=%s %s B=%d ' % (form, persist, name, B)
                    out[key + 'forward'], out[key + 'pose2mesh'] = _sha(v, p), _sha(w)
    return out


def main():
    if '--forms' in sys.argv:
        return main_forms()
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    write = sys.argv[sys.argv.index('--write') + 1] if '--write' in sys.argv else None
    if write in args:
        args.remove(write)
    tag = args[0] if args else os.path.basename(os.environ.get('GATOR_AMD_LIB', 'default'))
    d = digests()
    for k, h in d.items():
        print('%-24s %-32s %s' % (tag, k, h), flush=True)
    if write:
        with open(write, 'w') as f:
            json.dump({'what': 'sha256[:32] of (vertices, pose3d) bytes of gator_forward_f32, default arithmetic, gfx950; inputs synthetic_pose2d(B, J, seed=B), golden weights',
                       'digests': d}, f, indent=1)


def main_forms():
    write = sys.argv[sys.argv.index('--write') + 1] if '--write' in sys.argv else None
    d = form_digests()
    for k, h in d.items():
        print('%-56s %s' % (k, h), flush=True)
    if write:
        commit = sys.argv[sys.argv.index('--commit') + 1] if '--commit' in sys.argv else 'unknown'
        what = ('sha256[:32] per MDR form (tools/ab_digest.py: form_digests), gfx950, golden weights: forward = (vertices, pose3d) bytes on '
                'synthetic_pose2d(B, J, seed=B); pose2mesh = vertices of the MDR entry point on randn(B, J, 133) seeded with B.  Recorded with '
                'the library of commit %s' % commit)
        with open(write, 'w') as f:
            json.dump({'what': what, 'digests': d}, f, indent=1)


if __name__ == '__main__':
    main()
