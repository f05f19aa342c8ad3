"""gator_smpl_backward_f32 and the autograd of gator_amd.smpl.SMPLLayer on the device, against the float64 VJP of the restated layer
(tests/smpl_grad_refs.py) on the golden cases with their seeded upstream gradients.

Bounds.  tests/golden/smpl_layer_grad.npz records, per case and upstream (full, verts only, joints only), max |reference fp32 autograd
- float64 VJP| over the 65 samples for g_pose, g_betas and g_trans: the real layer's own fp32 error, 0.7e-7 .. 6.5e-7 of the largest
gradient.  The device is held to 3x that figure against the VJP, element by element -- the project's convention for an fp32 reference,
tests/test_gpu_smpl.py -- and to 4x against the stored fp32 rows.  A run on the first B samples is held to the case's figure.  Every
parity test prints its measured errors before it asserts (profiles/smpl_backward_tests.txt).

Sizes.  The hot kernel's tile is 32 samples x 128 vertices and its vertex sums are cut per 128-vertex tile whatever the batch, so B
takes 1 / 2 / 31 / 32 / 33 / 65 and NV takes 127 / 128 / 129 beside 1 / 63 / 64 / 65 / 257 and 6890 (54 tiles: the cross-tile sum); the
chunking adds no batch edge of its own."""
import functools

import numpy as np
import pytest
import torch

from gator_amd import _lib, smpl
from tests import smpl_grad_refs as gr
from tests import smpl_refs as sr
from tests.helpers import load_golden

pytestmark = pytest.mark.gpu

PARITY_CASES = ('nv1', 'nv63', 'nv64', 'nv65', 'nv127', 'nv128', 'nv129', 'nv257', 'families')
OPTION_CASES = ('no_betas_no_trans', 'center0', 'center23', 'scale1000', 'dense', 'nb0')
BATCHES = (1, 2, 31, 32, 33, 65)


class Case:
    """A golden case on the device: model, layer, inputs and upstream gradients (numpy and device), the spreads and the stored rows."""

    def __init__(self, name):
        z = load_golden('smpl_layer_grad')
        self.name, self.o = name, gr.case_options(name)
        self.m = sr.synthetic_model(*sr.CASES[name][0])
        self.layer = smpl.SMPLLayer.from_arrays(self.m['v_template'], self.m['shapedirs'], self.m['posedirs'], self.m['weights'],
                                                self.m['J_regressor'], self.m['parents'], center_idx=self.o['center_idx'],
                                                out_scale=self.o['out_scale'])
        self.np_in = gr.case_arguments(name)
        self.np_up = gr.upstream(name)
        self.dev_in = tuple(None if a is None else torch.from_numpy(a).cuda() for a in self.np_in)
        self.dev_up = tuple(torch.from_numpy(a).cuda() for a in self.np_up)
        self.spread = {w: z['%s.spread.%s' % (name, w)] for w in gr.UPSTREAMS}
        self.gold = {k: z['%s.g_%s32' % (name, k)] for k in gr.OUTPUTS if '%s.g_%s32' % (name, k) in z.files}
        self.center = -1 if (self.o['center_idx'] is None or self.np_in[2] is not None) else int(self.o['center_idx'])

    @functools.lru_cache(maxsize=None)
    def ref(self, which, B):
        """The float64 VJP of the first B samples."""
        gV, gJ = gr.select_upstream(which, *(g[:B] for g in self.np_up))
        return gr.vjp64(self.m, tuple(None if a is None else a[:B] for a in self.np_in), self.o, gV, gJ)

    def run(self, B=sr.N_SAMPLES, first=0, which='full', needs=(True, True, True), inputs=None, upstream=None):
        """gator_smpl_backward_f32 on samples first .. first + B: {'pose', 'betas', 'trans'} -> tensor, or None where not computed."""
        sl = slice(first, first + B)
        ins = [None if a is None else a[sl].contiguous() for a in (inputs or self.dev_in)]
        gV, gJ = gr.select_upstream(which, *(g[sl].contiguous() for g in (upstream or self.dev_up)))
        outs = [torch.full_like(a, 7.0) if (a is not None and n) else None for a, n in zip(ins, needs)]
        ptr = _lib.ptr
        _lib.check(_lib.load().gator_smpl_backward_f32(self.layer._ctx, ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), B, self.center, self.o['out_scale'],
                                                       ptr(gV), ptr(gJ), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]),
                                                       _lib.stream_ptr(self.layer.device)), 'gator_smpl_backward_f32')
        return dict(zip(gr.OUTPUTS, outs))


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def check_parity(c, B, which):
    got = c.run(B, which=which)
    ref = c.ref(which, B if c.name == 'nv6890' else sr.N_SAMPLES)
    for i, k in enumerate(gr.OUTPUTS):
        if ref[k] is None:
            assert got[k] is None
            continue
        g = got[k].cpu().numpy().astype(np.float64)
        assert g.shape == ref[k][:B].shape
        err, sp = np.abs(g - ref[k][:B]).max(), float(c.spread[which][i])
        line = 'smpl backward parity %-18s B %2d %-6s g_%-5s device %.3e reference %.3e ratio %.2f' % (c.name, B, which, k, err, sp, err / sp if sp else 0.0)
        gerr = None
        if which == 'full':
            n = min(B, c.gold[k].shape[0])
            gerr = np.abs(g[:n] - c.gold[k][:n]).max()
            line += '  (vs golden fp32 %.3e)' % gerr
        print(line)
        assert err <= 3 * sp
        assert gerr is None or gerr <= 4 * sp


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('name', PARITY_CASES)
def test_parity_with_the_fp64_vjp(name, B):
    c = case(name)
    for which in gr.UPSTREAMS:
        check_parity(c, B, which)


def test_parity_nv6890_across_54_vertex_tiles():
    c = case('nv6890')
    for which in gr.UPSTREAMS:
        check_parity(c, c.gold['pose'].shape[0], which)


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('name', OPTION_CASES)
def test_options_and_models(name, B):
    """betas = None and trans = None, centring on joints 0 and 23 (the offset's gradient goes back into the chain), out_scale 1000,
    24 influences per vertex, a model without betas."""
    c = case(name)
    if name == 'dense':
        assert (c.m['weights'] != 0).sum(1).min() == 24
    for which in gr.UPSTREAMS:
        check_parity(c, B, which)


def test_largest_model_and_a_smaller_ctx_beside_it():
    """NJ = 32, NB = 16, the handle's limits: K = 295, ten 32-coefficient passes of step 4, 155 136 bytes of LDS.  The reference layer
    cannot run it (its pose map is hard-wired to 23 joints), so there is no golden: each output is held to 3x the nv257 case's spread
    taken relative to that case's largest gradient -- the reference's own fp32 error on the same input distribution and vertex count,
    as a fraction of the gradient's size.  A ctx with fewer joints made afterwards must not lower the LDS limit of the kernels both use."""
    m = sr.synthetic_model(257, 32, 16, 41)
    make = lambda mm: smpl.SMPLLayer.from_arrays(mm['v_template'], mm['shapedirs'], mm['posedirs'], mm['weights'], mm['J_regressor'], mm['parents'])  # noqa: E731
    layer = make(m)
    rs = np.random.RandomState(42)
    B = 33
    pose = (rs.randn(B, 96) * 0.4).astype(np.float32)
    betas = rs.uniform(-2.5, 2.5, (B, 16)).astype(np.float32)
    trans = (rs.randn(B, 3) * 1.2).astype(np.float32)
    gV, gJ = rs.randn(B, 257, 3).astype(np.float32), rs.randn(B, 32, 3).astype(np.float32)
    ref = gr.vjp64(m, (pose, betas, trans), {'center_idx': None, 'out_scale': 1.0}, gV, gJ)
    c = case('nv257')
    r257 = c.ref('full', sr.N_SAMPLES)

    def run():
        leaves = [torch.from_numpy(a).cuda().requires_grad_(True) for a in (pose, betas, trans)]
        v, j = layer(*leaves)
        return torch.autograd.grad([v, j], leaves, [torch.from_numpy(gV).cuda(), torch.from_numpy(gJ).cuda()])

    first = run()
    for i, (g, k) in enumerate(zip(first, gr.OUTPUTS)):
        bound = 3 * float(c.spread['full'][i]) / np.abs(r257[k]).max() * np.abs(ref[k]).max()
        err = np.abs(g.cpu().numpy() - ref[k]).max()
        print('smpl backward NJ 32 NB 16 g_%-5s device %.3e bound %.3e' % (k, err, bound))
        assert err <= bound
    c.run(2)                                   # a 24-joint ctx is live and has run
    small = make(sr.synthetic_model(65, 24, 10, 14))
    second = run()
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    del small


def same(a, b):
    return all((a[k] is None and b[k] is None) or torch.equal(a[k], b[k]) for k in gr.OUTPUTS)


@pytest.mark.parametrize('name', ['nv129', 'dense', 'center23'])
def test_subsets_are_the_full_call_bit_for_bit(name):
    """An absent upstream gradient is a zero one; an output that is not asked for changes no other output."""
    c = case(name)
    B = 33
    full = c.run(B)
    zero_v, zero_j = torch.zeros_like(c.dev_up[0]), torch.zeros_like(c.dev_up[1])
    assert same(c.run(B, which='verts'), c.run(B, upstream=(c.dev_up[0], zero_j)))
    assert same(c.run(B, which='joints'), c.run(B, upstream=(zero_v, c.dev_up[1])))
    for which in gr.UPSTREAMS:
        whole = c.run(B, which=which)
        for i, k in enumerate(gr.OUTPUTS):
            if full[k] is None:
                continue
            one = c.run(B, which=which, needs=tuple(j == i for j in range(3)))
            assert torch.equal(one[k], whole[k]), (which, k)
            assert all(one[o] is None for o in gr.OUTPUTS if o != k)
            two = c.run(B, which=which, needs=tuple(j != i for j in range(3)))
            assert all(two[o] is None or torch.equal(two[o], whole[o]) for o in gr.OUTPUTS)


@pytest.mark.parametrize('name', ['nv129', 'nv6890'])
def test_a_row_does_not_depend_on_its_batch(name):
    c = case(name)
    whole = c.run(65)
    again = c.run(65)
    assert same(whole, again)
    for i in (range(65) if name == 'nv129' else (0, 31, 32, 64)):
        one = c.run(1, first=i)
        for k in gr.OUTPUTS:
            assert torch.equal(one[k][0], whole[k][i]), (k, i)
    part = c.run(33, first=20)                 # another tiling of the same samples
    for k in gr.OUTPUTS:
        assert torch.equal(part[k], whole[k][20:53]), k
    for which in ('verts', 'joints'):
        w = c.run(65, which=which)
        one = c.run(1, first=40, which=which)
        for k in gr.OUTPUTS:
            assert torch.equal(one[k][0], w[k][40]), (which, k)


def test_poison_stays_in_its_sample():
    c = case('nv129')
    clean = c.run(65)
    nan, inf = float('nan'), float('inf')

    def expect(bad_rows, inputs=None, upstream=None, which='full'):
        got = c.run(65, inputs=inputs, upstream=upstream, which=which)
        base = clean if which == 'full' else c.run(65, which=which)
        bad = torch.zeros(65, dtype=torch.bool, device='cuda')
        bad[bad_rows] = True
        for k in gr.OUTPUTS:
            assert torch.isnan(got[k][bad]).all(), k
            assert torch.equal(got[k][~bad], base[k][~bad]), k

    pose, betas, trans = (a.clone() for a in c.dev_in)
    pose[7, 20 * 3] = nan                      # an elbow
    betas[40, 3] = inf
    trans[41, 1] = nan
    expect([7, 40, 41], inputs=(pose, betas, trans))
    gV, gJ = (g.clone() for g in c.dev_up)
    gV[12, 128, 2] = nan                       # the one vertex of the second tile
    gV[33, 5, 0] = -inf
    gJ[50, 23, 1] = nan
    expect([12, 33, 50], upstream=(gV, gJ))
    expect([12, 33], upstream=(gV, gJ), which='verts')
    expect([50], upstream=(gV, gJ), which='joints')
    pose2 = c.dev_in[0].clone()
    pose2[3, 0] = inf                          # the root
    expect([3], inputs=(pose2, c.dev_in[1], c.dev_in[2]), which='joints')


def test_arguments_are_checked_on_a_live_ctx():
    c = case('nv65')
    lib = _lib.load()
    p, b, t = (a[:2].contiguous() for a in c.dev_in)
    gv, gj = (g[:2].contiguous() for g in c.dev_up)
    out = torch.zeros(2, 72, device='cuda')
    ctx = c.layer._ctx
    assert lib.gator_smpl_backward_f32(ctx, p.data_ptr(), b.data_ptr(), t.data_ptr(), 2, -1, 1.0, None, None, out.data_ptr(), None, None, None) == -1
    assert b'nothing to propagate' in lib.gator_last_error()
    assert lib.gator_smpl_backward_f32(ctx, p.data_ptr(), b.data_ptr(), t.data_ptr(), 2, 0, 1.0, gv.data_ptr(), None, out.data_ptr(), None, None, None) == -1
    assert b'center_idx' in lib.gator_last_error()
    assert lib.gator_smpl_backward_f32(ctx, p.data_ptr(), b.data_ptr(), None, 2, 24, 1.0, gv.data_ptr(), None, out.data_ptr(), None, None, None) == -1
    assert lib.gator_smpl_backward_f32(ctx, p.data_ptr(), b.data_ptr(), None, -1, -1, 1.0, gv.data_ptr(), None, out.data_ptr(), None, None, None) == -1
    assert lib.gator_smpl_backward_f32(ctx, None, b.data_ptr(), None, 2, -1, 1.0, gv.data_ptr(), None, out.data_ptr(), None, None, None) == -1
    assert lib.gator_smpl_backward_f32(ctx, p.data_ptr(), b.data_ptr(), None, 0, -1, 1.0, gv.data_ptr(), None, out.data_ptr(), None, None, None) == 0
    assert lib.gator_smpl_backward_f32(ctx, p.data_ptr(), b.data_ptr(), None, 2, 23, 1.0, None, gj.data_ptr(), out.data_ptr(), None, None, None) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and out.abs().max() > 0


def leaves(c, B, first=0):
    return [None if a is None else a[first:first + B].clone().requires_grad_(True) for a in c.dev_in]


def test_loss_backward_fills_the_leaves():
    """Fails without the feature: the layer's outputs carried no grad_fn."""
    c = case('nv257')
    B = 33
    pose, betas, trans = leaves(c, B)
    verts, joints = c.layer(pose, betas, trans)
    assert verts.grad_fn is not None and joints.grad_fn is not None
    pv, pj = c.layer(*(a[:B] for a in c.dev_in))
    assert pv.grad_fn is None and torch.equal(verts.detach(), pv) and torch.equal(joints.detach(), pj)
    gV, gJ = (g[:B] for g in c.dev_up)
    ((verts * gV).sum() + (joints * gJ).sum()).backward()
    direct = c.run(B)
    for leaf, k in zip((pose, betas, trans), gr.OUTPUTS):
        assert leaf.grad is not None and torch.equal(leaf.grad, direct[k]), k
    ref = c.ref('full', sr.N_SAMPLES)
    for i, (leaf, k) in enumerate(zip((pose, betas, trans), gr.OUTPUTS)):
        assert np.abs(leaf.grad.cpu().numpy() - ref[k][:B]).max() <= 3 * c.spread['full'][i]


def test_autograd_subsets_and_plain_paths():
    c = case('nv65')
    B = 8
    gV, gJ = (g[:B] for g in c.dev_up)
    # only the pose requires grad; only the joints are asked for
    pose = c.dev_in[0][:B].clone().requires_grad_(True)
    none, joints = c.layer(pose, c.dev_in[1][:B], c.dev_in[2][:B], want_verts=False)
    assert none is None and joints.grad_fn is not None
    (joints * gJ).sum().backward()
    assert torch.equal(pose.grad, c.run(B, which='joints', needs=(True, False, False))['pose'])
    # both outputs made, the loss uses the vertices alone: the unused output's gradient arrives as None
    pose, betas, trans = leaves(c, B)
    verts, joints = c.layer(pose, betas, trans)
    (verts * gV).sum().backward()
    want = c.run(B, which='verts')
    assert all(torch.equal(leaf.grad, want[k]) for leaf, k in zip((pose, betas, trans), gr.OUTPUTS))
    # betas alone, through want_joints=False
    betas = c.dev_in[1][:B].clone().requires_grad_(True)
    verts, none = c.layer(c.dev_in[0][:B], betas, c.dev_in[2][:B], want_joints=False)
    (verts * gV).sum().backward()
    assert none is None and torch.equal(betas.grad, want['betas'])
    # no graph where none is wanted
    pose, betas, trans = leaves(c, B)
    with torch.no_grad():
        v, j = c.layer(pose, betas, trans)
    assert v.grad_fn is None and j.grad_fn is None and not v.requires_grad
    v2, j2 = c.layer(pose.detach(), betas.detach(), trans.detach())
    assert v2.grad_fn is None and not j2.requires_grad and torch.equal(v, v2) and torch.equal(j, j2)
    # first derivatives only
    pose, betas, trans = leaves(c, B)
    verts, _ = c.layer(pose, betas, trans)
    g, = torch.autograd.grad((verts * gV).sum(), pose, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


def test_the_call_s_own_options_are_used_in_backward():
    """get_smpl_coord sets out_scale for the length of its call; backward, later, must use that call's value."""
    c = case('nv6890')                         # the wrapper reads the face key points at their SMPL vertex numbers
    B = 2
    layer = smpl.SMPLLayer.from_arrays(c.m['v_template'], c.m['shapedirs'], c.m['posedirs'], c.m['weights'], c.m['J_regressor'], c.m['parents'])
    pose, betas, trans = leaves(c, B)
    mesh, joints = smpl.get_smpl_coord(layer, pose, betas, trans)
    assert layer.out_scale == 1.0
    (mesh * c.dev_up[0][:B]).sum().backward()
    pose1, betas1, trans1 = leaves(c, B)
    v1, _ = layer(pose1, betas1, trans1)
    (v1 * c.dev_up[0][:B]).sum().backward()
    # mm against m: every gradient is 1000 times larger, up to the rounding of gx = 1000 gV (half an ulp of each term)
    assert torch.allclose(pose.grad, 1000 * pose1.grad, rtol=1e-4, atol=1e-4 * float(pose.grad.abs().max()))
    assert torch.allclose(trans.grad, 1000 * trans1.grad, rtol=1e-4, atol=1e-4 * float(trans.grad.abs().max()))


def test_ten_adam_steps_lower_the_loss():
    c = case('nv257')
    B = 8
    with torch.no_grad():
        target, _ = c.layer(*(a[:B] for a in c.dev_in))
    rs = np.random.RandomState(3)
    pose = (c.dev_in[0][:B] + torch.from_numpy((rs.randn(B, 72) * 0.1).astype(np.float32)).cuda()).requires_grad_(True)
    betas = (c.dev_in[1][:B] + 0.3).requires_grad_(True)
    trans = (c.dev_in[2][:B] + 0.05).requires_grad_(True)
    opt = torch.optim.Adam([pose, betas, trans], lr=0.02)
    losses = []
    for _ in range(10):
        opt.zero_grad()
        verts, _ = c.layer(pose, betas, trans)
        loss = ((verts - target) ** 2).sum() + 1e-3 * (pose ** 2).sum()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print('smpl backward adam: loss %.4e -> %.4e' % (losses[0], losses[-1]))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_capture_and_replay_give_the_eager_bits():
    c = case('nv257')
    B = 33
    eager = c.run(B, first=32)
    eager_v, eager_j = c.layer(*(a[32:65] for a in c.dev_in))
    args = [a[:B].clone().requires_grad_(True) for a in c.dev_in]
    ups = [g[:B].clone() for g in c.dev_up]

    def step():
        v, j = c.layer(*args)
        return (v, j) + torch.autograd.grad([v, j], args, ups)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                               # every workspace exists before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    base = c.layer.workspace(), c.layer.workspace_bytes()        # the forward's block, and every grown block's bytes and growths
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = step()
    with torch.no_grad():                                    # new contents in the captured buffers: the replay computes them
        for a, src in zip(args, c.dev_in):
            a.copy_(src[32:65])
        for a, src in zip(ups, c.dev_up):
            a.copy_(src[32:65])
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(outs[0], eager_v) and torch.equal(outs[1], eager_j)
    for got, k in zip(outs[2:], gr.OUTPUTS):
        assert torch.equal(got, eager[k]), k
    assert (c.layer.workspace(), c.layer.workspace_bytes()) == base
    for _ in range(3):                                       # repeated calls at one batch grow nothing
        c.run(B)
        step()
    assert (c.layer.workspace(), c.layer.workspace_bytes()) == base
    fresh = smpl.SMPLLayer.from_arrays(c.m['v_template'], c.m['shapedirs'], c.m['posedirs'], c.m['weights'], c.m['J_regressor'], c.m['parents'])
    assert fresh.workspace_bytes() == (0, 0)                 # a layer that never differentiates holds no transposed basis
    fresh(*(a[:4] for a in c.dev_in))
    forward_only = fresh.workspace_bytes()
    lib, ptr = _lib.load(), _lib.ptr
    p, b, t = (a[:4].contiguous() for a in c.dev_in)
    gj, out = c.dev_up[1][:4].contiguous(), torch.empty(4, 72, device='cuda')
    _lib.check(lib.gator_smpl_backward_f32(fresh._ctx, ptr(p), ptr(b), ptr(t), 4, -1, 1.0, None, ptr(gj), ptr(out), None, None,
                                           _lib.stream_ptr(fresh.device)), 'gator_smpl_backward_f32')
    assert fresh.workspace_bytes() == forward_only           # nor does a joints-only backward grow anything
