"""The automatic boundaries of the launch policy (gator_amd/csrc/forward_plan.h), observed on the device with default switches: the MDR
layers turn from four launches to the persistent form between B = 219 and B = 220 on a 256-CU device, k_gat8 runs its own tail below the
sample-tiled threshold, and the library's answer about the encoder of a batch does not follow a pin."""
import pytest
import torch

from gator_amd import synthetic
from tests.helpers import build_model

pytestmark = pytest.mark.gpu

SWITCHES = ('GATOR_MDR_PERSIST', 'GATOR_MDR_PERSIST_CHUNK', 'GATOR_MDR_PERSIST_GRID', 'GATOR_GAT8', 'GATOR_GAT8_TAIL', 'GATOR_GAT8_LOBYTE', 'GATOR_GAT8_H4',
            'GATOR_GAT_X3', 'GATOR_GAT_TILED', 'GATOR_GAT_TILED_MIN_BATCH', 'GATOR_MDR_X3', 'GATOR_SUBBATCH_STREAMS', 'GATOR_GRAPH')


def test_automatic_boundaries(monkeypatch):
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    if n_cu != 256:
        pytest.skip('the automatic policy is pinned for a 256-CU device; this one reports %d' % n_cu)
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    z, m = build_model('h36m17_bn', 'fused')
    x = torch.from_numpy(synthetic.synthetic_pose2d(220, 17, seed=220)).cuda()
    m(x)                                           # creates the context, sizes the workspace for both batches
    m.profile(1)
    stages = {}
    for B in (219, 220):
        m(x[:B])
        torch.cuda.synchronize()
        m.device_status()
        stages[B] = {k: n for k, (ms, n) in m.profile_read().items()}
    m.profile(0)
    print('\n', stages)
    four, one = stages[219], stages[220]
    assert (four.get('mdr_layer0'), four.get('mdr_layer'), four.get('mdr_attn_head')) == (1, 2, 1) and 'mdr_layers' not in four, four
    assert one.get('mdr_layers') == 1 and not {'mdr_layer0', 'mdr_layer', 'mdr_attn_head'} & set(one), one
    for s in (four, one):
        assert 'gat' in s and 'gat_tail' not in s, s
    assert m.encoder_for_batch(1024) == 'sample' and m.encoder_for_batch(1025) == 'tiled'
    m.set_encoder('tiled')
    try:
        assert m.encoder_for_batch(5) == 'sample'          # what AUTO would do, whatever is pinned
    finally:
        m.set_encoder('auto')
