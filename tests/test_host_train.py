"""Host-side pieces of the training row that need no GPU: the ctypes mirrors of the C structs, the vertex incidence lists that
order the face-loss gradient gathers, the learning-rate schedule, the parameter / buffer split of a reference state_dict."""
import ctypes

import numpy as np

from gator_amd import _lib, synthetic
from gator_amd.train import losses, model as M
from gator_amd.train.optim import Adam
from tests.helpers import golden_shapes, load_golden


def test_ctypes_structs_mirror_the_c_abi():
    lib = _lib.load()
    assert ctypes.sizeof(_lib.GemmProblem) == lib.gator_t_struct_size(0)
    assert lib.gator_t_struct_size(7) == -1


def test_vertex_incidence_lists():
    faces = synthetic.synthetic_faces(3, num_faces=500, num_verts=120)
    ptr, idx = losses.vertex_incidence(faces, 120)
    assert ptr[0] == 0 and ptr[-1] == 1500 and len(idx) == 1500
    flat = faces.reshape(-1)
    for v in (0, 7, 59, 119):
        mine = idx[ptr[v]:ptr[v + 1]]
        assert np.array_equal(np.sort(mine), np.nonzero(flat == v)[0]) and np.all(np.diff(mine) > 0)     # every (face, corner), ascending
    assert (np.diff(ptr) >= 1).all()                      # synthetic_faces uses every vertex
    f = synthetic.synthetic_faces(0)
    assert f.shape == (13776, 3) and (f[:, 0] != f[:, 1]).all() and (f[:, 0] != f[:, 2]).all() and (f[:, 1] != f[:, 2]).all()


def test_multistep_lr_follows_the_reference_loop():
    a = Adam.__new__(Adam)
    a.base_lr, a.gamma, a.milestones = 1e-3, 0.1, (30,)
    lrs = {}
    for e in (1, 2, 30, 31, 40):
        a.epoch = e
        lrs[e] = a.lr
    assert lrs[1] == lrs[30] == 1e-3 and abs(lrs[31] - 1e-4) < 1e-12 and abs(lrs[40] - 1e-4) < 1e-12     # main/train.py:36-39, config.py:76-77


def test_parameter_buffer_split_and_rates():
    z = load_golden('h36m17_bn')
    keys = list(golden_shapes(z))
    bufs = [k for k in keys if M.is_buffer(k)]
    assert sorted(b.rsplit('.', 1)[-1] for b in bufs) == sorted(['graph_adj', 'init_vertices', 'init_vertices', 'init_vertices_6890', 'running_mean',
                                                                  'running_var', 'num_batches_tracked'])
    names = [str(k) for k in load_golden('train_h36m17_bn')['param_names']]
    assert sorted(k for k in keys if not M.is_buffer(k)) == names          # exactly the reference's named_parameters()
    r = M.Rates()
    assert r.gat_path[0] == 0.0 and abs(r.gat_path[-1] - 0.2) < 1e-12 and r.gat_attn == 0.4 and r.mdr_self == 0.1
    assert M.Rates(0.0).gat_attn == 0.0


def test_philox_reference_reproduces_the_random123_known_answers():
    """The numpy Philox4x32 of tests/train_refs.py at 10 rounds against the known-answer vectors published with Random123
    (kat_vectors, philox4x32 10): the mask reference of the GPU dropout tests is independent of the code under test."""
    from tests.train_refs import philox4x32
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(int(w) for w in philox4x32([ctr], [key], 10)[0]) == want
    got = philox4x32([k[0] for k in kat], [k[1] for k in kat], 10)         # rows are independent blocks
    assert [tuple(int(w) for w in r) for r in got] == [k[2] for k in kat]
    assert not np.array_equal(philox4x32([kat[2][0]], [kat[2][1]], 7), got[2:])


def test_keep_mask_reference_statistics_at_the_device_round_count():
    from tests.train_refs import DEVICE_ROUNDS, keep_mask, keep_threshold
    assert DEVICE_ROUNDS == 7
    n = 1 << 18
    masks = {}
    for rate in (0.1, 0.4):
        m = masks[rate] = keep_mask(123, 1, n, rate)
        assert m.dtype == np.uint8 and m.shape == (n,) and set(np.unique(m)) <= {0, 1}
        assert abs(float(m.mean()) - (1.0 - rate)) < 0.01
    a, b = masks[0.4].astype(np.float64), keep_mask(123, 2, n, 0.4).astype(np.float64)
    assert abs(float(np.corrcoef(a, b)[0, 1])) < 0.01
    # the counter layout: a prefix of a longer mask, the step in the high word of the offset, the saturated threshold
    assert np.array_equal(keep_mask(123, 1, 5, 0.4), masks[0.4][:5])
    assert np.array_equal(keep_mask(123, 1, 64, 0.4, step=3), keep_mask(123, 1 + (3 << 32), 64, 0.4))
    assert not np.array_equal(keep_mask(123, 1, 64, 0.4, step=3), masks[0.4][:64])
    assert keep_threshold(0.0) == 0 and keep_threshold(0.5) == 1 << 31 and keep_threshold(0.99999999999) == 0xffffffff


def test_mgcn_reference_equals_the_explicit_triple_loop():
    import torch
    from tests.train_refs import mgcn_ref
    rs = np.random.RandomState(40)
    B, J, C = 2, 3, 4
    h0, h1, adj, Mw, bias = rs.randn(B, J, C), rs.randn(B, J, C), rs.randn(J, J), rs.randn(J, C), rs.randn(C)
    want = np.zeros((B, J, C))
    for b in range(B):
        for i in range(J):
            for c in range(C):
                acc = adj[i, i] * Mw[i, c] * h0[b, i, c] + bias[c]
                for j in range(J):
                    if j != i:
                        acc += adj[i, j] * Mw[j, c] * h1[b, j, c]
                want[b, i, c] = acc
    got = mgcn_ref(*[torch.from_numpy(a) for a in (h0, h1, adj, Mw, bias)]).numpy()
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-14 * np.abs(want).max()
    assert np.abs(adj - adj.T).max() > 0.1                 # a transposed adjacency would not pass


def test_adam_reference_follows_torch_adam_for_five_steps():
    import torch
    from tests.train_refs import adam_step_ref
    rs = np.random.RandomState(41)
    for lr, betas, eps in ((1e-3, (0.9, 0.999), 1e-8), (3e-2, (0.8, 0.99), 1e-6)):
        p = torch.from_numpy(rs.randn(33))
        tp = p.clone().requires_grad_(True)
        opt = torch.optim.Adam([tp], lr=lr, betas=betas, eps=eps)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        for t in range(1, 6):
            g = torch.from_numpy(rs.randn(33) * 10.0 ** rs.randint(-3, 3, 33))
            tp.grad = g.clone()
            opt.step()
            p, m, v = adam_step_ref(p, g, m, v, lr, betas[0], betas[1], eps, t)
            st = opt.state[tp]
            for ours, theirs in ((p, tp.detach()), (m, st['exp_avg']), (v, st['exp_avg_sq'])):
                assert float((ours - theirs).abs().max()) <= 1e-13 * float(theirs.abs().max()), t


def test_layernorm_reference_mode_1_equals_the_oracle():
    import torch
    from oracle.gator_oracle import _custom_ln
    from tests.train_refs import layernorm_ref
    rs = np.random.RandomState(42)
    for n in (2, 20, 65):
        x, w, b = [torch.from_numpy(rs.randn(*s)) for s in ((5, n), (n,), (n,))]
        want = _custom_ln(x, w, b, 1e-6)
        assert float((layernorm_ref(x, w, b, 1e-6, 1) - want).abs().max()) <= 1e-14 * float(want.abs().max())
        assert float((layernorm_ref(x, None, None, 1e-6, 1) - _custom_ln(x, 1.0, 0.0, 1e-6)).abs().max()) <= 1e-14 * float(want.abs().max())
    x = torch.from_numpy(rs.randn(3, 7))
    assert torch.equal(layernorm_ref(x, None, None, 1e-5, 0), torch.nn.functional.layer_norm(x, (7,), None, None, 1e-5))
