"""The launch policy of the fused path (gator_amd/csrc/forward_plan.h) as a pure function, on the CPU.  tests/host_forward_plan.cpp
includes that header alone and is built as plain C++17 (no offload flags: the header must not need HIP); it prints the plan of every
case.  The expectations below were worked out by hand from the rules the launchers applied before the plan existed -- not from the
planner's output: nwg = (14 B + 3) / 4 MDR workgroups, persistent iff nwg / 256 >= 3 on a 256-CU device, B / 256 chunks (ceil(B / 384) on
one plane) capped at 64; the sample-tiled encoder from 1024 samples in full rounds of n_cu * (128 / J), the remainder too if it is more
than 4 n_cu."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# What read_fused_options derives from a switch that others need (forward_plan.h): a case names the derived values as well
GAT8_OFF = 'gat8=0,gat8_lobyte=0,gat8_tail=0,c3_encoder=0'
GAT_X3_OFF = 'gat_x3=0,' + GAT8_OFF


@pytest.fixture(scope='module')
def planner(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('forward_plan') / 'host_forward_plan')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    subprocess.check_call([hipcc, '-std=c++17', '-x', 'c++', '-Wall', '-Werror', '-I' + os.path.join(ROOT, 'gator_amd', 'csrc'),
                           os.path.join(HERE, 'host_forward_plan.cpp'), '-o', exe])

    def plan(*cases):
        out = subprocess.run([exe] + list(cases), check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(out) == len(cases)
        return [dict(kv.split('=', 1) for kv in (line.split(' ') if not line.startswith('error=') else [line])) for line in out]
    return plan


def _check(planner, table):
    got = planner(*[case for case, _ in table])
    for (case, want), plan in zip(table, got):
        for k, v in want.items():
            assert plan.get(k) == str(v), '%s: %s is %s, expected %s (%s)' % (case, k, plan.get(k), v, plan)


def test_mdr_form_and_chunks_by_batch(planner):
    _check(planner, [
        ('B=219', dict(persist=0, xa=2, head='finish')),                  # nwg = 767 < 768: four launches
        ('B=220', dict(persist=1, nch=1, base=220, rem=0, grid=512)),     # nwg = 770
        ('B=511', dict(persist=1, nch=1, base=511, rem=0)),
        ('B=512', dict(persist=1, nch=2, base=256, rem=0)),
        ('B=700', dict(persist=1, nch=2, base=350, rem=0)),
        ('B=2048', dict(persist=1, nch=8, base=256, rem=0)),
        ('B=20000', dict(persist=1, nch=64, base=312, rem=32)),           # 78 chunks capped at 64: 32 of 313, 32 of 312
        ('B=250,mdr_persist_chunk=100', dict(persist=1, nch=3, base=83, rem=1)),
        ('B=256,mdr_persist_grid=13', dict(persist=1, grid=13)),
    ])


def test_encoder_split_by_batch(planner):
    _check(planner, [
        ('J=17,B=1023', dict(n_tiled=0, sample='k_gat8')),
        ('J=17,B=1024', dict(n_tiled=0, sample='k_gat8')),                # remainder 1024 is not > 4 * 256
        ('J=17,B=1025', dict(n_tiled=1025, sample='none', n_tail=1025, fused_tail=0, ctr_zero='k_gat_joint')),
        ('J=17,B=2048', dict(n_tiled=1792, sample='k_gat8', k_gat8='1,10,0,1,1', k_gat_tiled='17,1,0', fused_tail=1, n_tail=1792, ctr_zero='k_gat8', enc16=0)),
        ('J=17,B=3000', dict(n_tiled=3000, sample='none')),               # remainder 1208 > 1024
        ('J=19,B=2048', dict(n_tiled=1536, sample='k_gat8', k_gat8='1,12,0,1,1', k_gat_tiled='19,1,0', n_tail=1536)),
        ('J=17,B=256', dict(n_tiled=0, k_gat8='1,10,0,1,1', fused_tail=1, n_tail=0, ctr_zero='k_gat8', up='x2', w1=0, joints=0)),
    ])


def test_config3(planner):
    _check(planner, [
        ('bf16=1,B=384', dict(xa=3, persist=1, nch=1, enc16=1, k_gat8='1,10,1,0,1', fused_tail=1, up='x2', w1=1)),
        ('bf16=1,B=385', dict(xa=3, nch=2, base=192, rem=1)),
        ('bf16=1,B=2048', dict(xa=3, nch=6, base=341, rem=2, n_tiled=1792, k_gat_tiled='17,1,1', k_gat8='1,10,1,0,1')),
        ('bf16=1,J=19,B=2048', dict(n_tiled=1536, k_gat_tiled='19,1,1', k_gat8='1,12,1,0,1')),
        ('bf16=1,B=256,c3_up_bf16=1', dict(up='bf16', w1=0)),
        ('bf16=1,B=256,c3_up_w1=0', dict(up='x2', w1=0)),
        ('bf16=1,B=256,c3_mdr=0,c3_encoder=0', dict(xa=2, enc16=0, k_gat8='1,10,0,1,1', nch=1)),      # what the guard leaves
        ('bf16=1,B=256,gat8_lobyte=0', dict(fused_tail=1, k_gat8='1,10,1,0,1')),      # the one-plane form keeps its fused tail
    ])


def test_switches(planner):
    _check(planner, [
        ('B=256,gat8_lobyte=0', dict(fused_tail=0, n_tail=256, ctr_zero='k_gat_joint', sample='k_gat8', k_gat8='1,10,0,0,0')),
        ('B=256,gat8_tail=0', dict(fused_tail=0, n_tail=256, ctr_zero='k_gat_joint', k_gat8='1,10,0,1,0')),
        ('B=256,gat8_h4=0,gat8_lobyte=0,gat8_tail=0,c3_encoder=0', dict(k_gat8='0,16,0,0,0', n_tail=256)),
        ('B=256,' + GAT8_OFF, dict(sample='k_gat', k_gat='1,0', fused_tail=0, n_tail=256, ctr_zero='k_gat_joint')),
        ('B=256,' + GAT_X3_OFF, dict(sample='k_gat', k_gat='0,0', n_tail=256)),
        ('B=256,gat8=0', dict(sample='k_gat', fused_tail=0, n_tail=256, ctr_zero='k_gat_joint')),      # only k_gat8 has a fused tail, whatever gat8_tail says
        ('B=3000,' + GAT_X3_OFF, dict(n_tiled=0, sample='k_gat')),        # never tiled without the split-precision weights
        ('B=2048,gat_tiled_h4=0', dict(n_tiled=1792, k_gat_tiled='17,0,0')),
        ('B=2048,mdr_persist=0', dict(persist=0, ctr_zero='nobody', nch=1, base=2048)),
        ('B=5,mdr_persist=1,n_cu=64', dict(persist=1, grid=128, ctr_zero='k_gat8')),      # only the automatic policy looks at the CU count
        ('B=1000,n_cu=64', dict(persist=0, ctr_zero='k_gat8')),           # (the joint-token launch zeroes whenever the ctx MAY run persistent launches)
        ('B=512,mdr_head_partials=0', dict(head='head<512,true>')),
        ('B=513,mdr_head_partials=0', dict(head='head<512,false>')),
        ('B=256,up_x3=1,c3_up_bf16=1', dict(up='x3')),
        ('B=256,up_x3=0,c3_up_bf16=1', dict(up='fp32')),
        ('B=256,mdr_x3=1,gat8_tail=0,c3_mdr=0', dict(xa=1, fused_tail=0)),
        ('B=1,pin=1', dict(n_tiled=1, sample='none', n_tail=1, ctr_zero='k_gat_joint')),      # pinned to the tiled encoder: every batch
        ('B=3000,pin=0', dict(n_tiled=0, sample='k_gat8')),
        ('B=1500,gat_tiled_min_batch=2000', dict(n_tiled=0)),
        ('B=1792,n_cu=64', dict(n_tiled=1792, sample='none')),            # four full rounds of 64 * 7
    ])


def test_entry_points_and_refusals(planner):
    _check(planner, [
        ('entry=1,B=33', dict(sample='k_gat', k_gat='1,1', n_tiled=0, n_tail=0, ctr_zero='nobody', xa=-1, up='none')),
        ('entry=1,B=33,' + GAT_X3_OFF, dict(sample='k_gat', k_gat='0,1', xa=-1, up='none')),
        ('entry=1,B=3000', dict(sample='k_gat', n_tiled=0)),
        ('entry=2,B=300', dict(sample='none', n_tiled=0, n_tail=0, ctr_zero='k_mdr_joint', persist=1, xa=2, up='x2')),
        ('entry=2,B=300,mdr_persist=0', dict(ctr_zero='nobody', persist=0)),
        ('joints=1,B=33', dict(up='x2', joints=1, w1=0)),
        ('joints=1,B=33,up_x3=1,c3_up_bf16=1', dict(up='x3', joints=1)),
    ])
    # (the last: switches as read_fused_options never leaves them -- the byte-lo stream and the tail without the four-product form -- are refused)
    for case, why in (('joints=1,B=33,up_x3=0,c3_up_bf16=1', 'split-precision vertex regressor'), ('joints=1,B=33,bf16=1', 'split-precision vertex regressor'),
                      ('bf16=1,B=33,c3_mdr=1,mdr_x3=1,gat8_tail=0', '16-bit MDR layers need'), ('bf16=1,B=2048,gat_tiled_h4=0', 'four-product weight image'),
                      ('bf16=1,B=33,gat8_h4=0,gat8_lobyte=0,gat8_tail=0', 'four-product weight stream'),
                      ('B=33,gat8_h4=0', 'no fused tail on the three-plane')):
        (plan,) = planner(case)
        assert why in plan.get('error', ''), (case, plan)
