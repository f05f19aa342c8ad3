"""The operand slots of the vertex regressor (gator_amd/csrc/regressor_slots.h) as pure functions, on the CPU.
tests/host_regressor_slots.cpp includes that header alone and is built as plain C++17 (no offload flags: the header must not need HIP).
It walks every packed buffer in the order of the layout comments in csrc/fused_state.h -- which is the order in which the kernels form
their fragment indices (tile, k-step, position | tap, plane, lane, j) -- and holds the slot function to it at every padded coordinate:
the same element, inside the buffer, none named twice, none left out.  The sizes below are written from those comments (dimensions
multiplied out by hand), not taken from the program's output."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

TILE = 3 * 28 * 64 * 8            # one 32-sample tile of a 16-bit plane: [3][28][64][8] = 43 008 elements (an fp32 tile set [3][14][4][64][4] has as many)
GROUP = 28 * 4 * 3 * 2 * 64 * 8   # one 128-sample group of the two-plane form: [28][4][3][plane 2][64][8] = 344 064
TILES = {1: 1, 33: 2, 129: 5}     # 32-sample tiles of a batch
GROUPS = {1: 1, 33: 1, 129: 2}    # 128-sample groups


def _line(name, B, cap, elems, walked):
    return '%s B=%d cap=%d elems=%d walked=%d differ=0 outside=0 repeated=0 unnamed=0' % (name, B, cap, elems, walked)


def _expected():
    out = []
    for B in (1, 33, 129):
        out.append(_line('act_f32', B, B, TILES[B] * TILE, TILES[B] * TILE))
        out.append(_line('act_x2', B, B, GROUPS[B] * GROUP, GROUPS[B] * GROUP))
        if B <= 33:
            out.append(_line('act_x3', B, 33, 3 * 2 * TILE, 3 * TILES[B] * TILE))         # planes strided by the capacity's two tiles
        out.append(_line('act_x3', B, 257, 3 * 9 * TILE, 3 * TILES[B] * TILE))            # ... by its nine tiles
        out.append(_line('act_bf16', B, B, TILES[B] * TILE, TILES[B] * TILE))
    w_plane = 3 * 216 * 28 * 64 * 8                                                       # [tap 3][ob 216][28][64][8]
    out.append(_line('w_x3', 0, 0, 3 * w_plane, 3 * w_plane))
    out.append(_line('w_bf16', 0, 0, w_plane, w_plane))
    out.append(_line('w_x2', 0, 0, 108 * 28 * 2 * 3 * 2 * 64 * 8, 108 * 28 * 2 * 3 * 2 * 64 * 8))   # [ob/2 108][28][2][tap 3][plane 2][64][8]
    out.append('taps n=7 ok')
    return out


@pytest.fixture(scope='module')
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('regressor_slots') / 'host_regressor_slots')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    subprocess.check_call([hipcc, '-std=c++17', '-O1', '-x', 'c++', '-Wall', '-Werror', '-I' + os.path.join(ROOT, 'gator_amd', 'csrc'),
                           os.path.join(HERE, 'host_regressor_slots.cpp'), '-o', exe])
    return subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()


def test_the_sizes_are_the_layout_comments_dimensions():
    assert (TILE, GROUP) == (43008, 344064)


@pytest.mark.parametrize('i,want', list(enumerate(_expected())), ids=[w.split(' elems')[0].replace(' ', '-') for w in _expected()])
def test_every_slot_is_the_element_the_kernel_reads(lines, i, want):
    assert len(lines) == len(_expected())
    assert lines[i] == want
