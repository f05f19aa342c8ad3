"""Who frees what: a context that allocated everything it can gives all of it back at gator_destroy, and a gator_create that fails
half way leaves nothing behind.  Device memory is read with torch.cuda.mem_get_info() (the driver's figure, after torch's own cache
is emptied); the bound is one context's weight arena: a workspace, a packed weight image or an arena that is not freed is far above
it, the allocator's granularity far below."""
import gc

import pytest
import torch

from gator_amd import synthetic
from tests.helpers import build_model

pytestmark = pytest.mark.gpu

VARIANTS = (('h36m17_bn', 17), ('coco19_alpha', 19))


def _x(B, J, seed):
    return torch.from_numpy(synthetic.synthetic_pose2d(B, J, seed=seed)).cuda()


def _arena_bytes(m):
    """The weight arena of a context holds a device copy of every tensor of the state dict (plus small constants)."""
    return sum(t.numel() * t.element_size() for t in m.state_dict().values())


def _free_bytes():
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return torch.cuda.mem_get_info()[0]


def _cycle():
    """Both golden variants, every lazily allocated buffer of a context -> (outputs on the host, largest arena in bytes)."""
    outs, arena = [], 0

    def keep(*ts):
        outs.extend(t.cpu() for t in ts)

    for name, J in VARIANTS:
        z, m = build_model(name, 'fused')
        arena = max(arena, _arena_bytes(m))
        small, big = _x(8, J, 1), _x(160, J, 2)
        keep(*m(small))
        keep(*m(big))                                      # the workspace grows
        m.precision = 'bf16'                               # the bf16 weight image and its operand buffer, grown once
        keep(*m(small))
        keep(*m(big))
        m.precision = 'f32'
        m.enable_block_taps(True)                          # the block-tap buffer, grown once
        keep(*m(small))
        keep(*m(big))
        keep(m.get_tap('gat_block5', (160, J, 128)))
        m.enable_block_taps(False)
        m.set_joint_regressor(synthetic.model_j_regressor(J))
        keep(*m.forward_joints(small, with_verts=True))
        keep(*m.forward_joints(big, with_verts=True))      # the partial-product buffer grows
        m.set_graph_replay(True)
        out = (torch.empty(160, 6890, 3, device='cuda'), torch.empty(160, J, 3, device='cuda'))
        for it in range(4):                                # direct, capture + launch, replay, replay
            m(big, out=out)
        assert m.graph_launches() == 3
        keep(*out)
        m.subbatch_streams = 2                             # another context key: the module drops its context and creates the next
        keep(*m(big))                                      # B >= 128: two halves, two workspace sets, the second stream and its events
        m.precision = 'bf16'
        keep(*m(big))
        m.invalidate()
        torch.cuda.synchronize()
        del m, small, big, out
    return outs, arena


@pytest.mark.timeout(900)
def test_four_create_destroy_cycles_give_all_device_memory_back():
    free, first, last, arena = {}, None, None, 0
    for cyc in range(1, 5):
        outs, arena = _cycle()
        if cyc == 1:
            first = outs
        last = outs
        del outs
        if cyc >= 2:                                       # the first two cycles warm the runtime's own pools
            free[cyc] = _free_bytes()
    print('\n[ctx lifetime] free device memory after cycles 2, 3, 4: %d %d %d bytes; lost from 2 to 4: %d; bound (one weight arena): %d'
          % (free[2], free[3], free[4], free[2] - free[4], arena))
    assert free[2] - free[4] <= arena
    assert len(first) == len(last)
    for i, (a, b) in enumerate(zip(first, last)):
        assert torch.equal(a, b), i


@pytest.mark.timeout(600)
def test_a_failed_create_leaves_nothing_behind_and_the_module_recovers(monkeypatch):
    """GATOR_UPSAMPLE_X3=5 is an argument error of gator_create (read_fused_options: GATOR_EINVAL), found after the arena, the folded
    constants and the status word exist: the create unwinds."""
    z, m = build_model('h36m17_bn', 'fused')
    arena = _arena_bytes(m)
    x = _x(16, 17, 3)
    free0 = _free_bytes()
    monkeypatch.setenv('GATOR_UPSAMPLE_X3', '5')
    for it in range(10):
        with pytest.raises(RuntimeError, match='GATOR_UPSAMPLE_X3'):
            m(x)
    free1 = _free_bytes()
    monkeypatch.delenv('GATOR_UPSAMPLE_X3')
    print('\n[ctx lifetime] free device memory before / after ten failed creates: %d %d bytes; moved: %d; bound (one weight arena): %d'
          % (free0, free1, free0 - free1, arena))
    assert abs(free0 - free1) < arena
    got = m(x)
    z, fresh = build_model('h36m17_bn', 'fused')
    want = fresh(x)
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    m.device_status()
