"""The grouping rule of the renderer's and the 2D overlay's image tables (gator_amd/csrc/image_groups.h) as a pure function, on the CPU.
tests/host_image_groups.cpp includes that header alone and is built as plain C++17 (no offload flags: the header must not need HIP); it
prints the tables of every case.  The expectations below were written by hand from the rule -- img_off: prefix counts of the members per
image; member_of: the members of image n in member order at img_off[n]..; slot: a member's rank within its image -- not taken from the
function's output."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope='module')
def groups(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('image_groups') / 'host_image_groups')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    subprocess.check_call([hipcc, '-std=c++17', '-x', 'c++', '-Wall', '-Werror', '-I' + os.path.join(ROOT, 'gator_amd', 'csrc'),
                           os.path.join(HERE, 'host_image_groups.cpp'), '-o', exe])

    def run(*cases):
        out = subprocess.run([exe] + list(cases), check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(out) == len(cases)
        return out
    return run


def _line(most, img_off, member_of, slot=None):
    lists = [('img_off', img_off), ('member_of', member_of)] + ([('slot', slot)] if slot is not None else [])
    return 'most=%d ' % most + ' '.join('%s=%s' % (k, ','.join(str(x) for x in v)) for k, v in lists) + ' guards=ok'


TABLES = [
    ('1/0', _line(1, [0, 1], [0], [0])),                                                  # M = 1, N = 1
    ('1/0,0,0,0', _line(4, [0, 4], [0, 1, 2, 3], [0, 1, 2, 3])),                          # all members in one image
    ('3/1,1,1', _line(3, [0, 0, 3, 3], [0, 1, 2], [0, 1, 2])),                            # ... the middle one of three
    ('2/1,0,1', _line(2, [0, 1, 3], [1, 0, 2], [0, 0, 1])),
    ('4/3,2,1,0', _line(1, [0, 1, 2, 3, 4], [3, 2, 1, 0], [0, 0, 0, 0])),                 # reverse order
    ('3/1,2,2,1', _line(2, [0, 0, 2, 4], [0, 3, 1, 2], [0, 0, 1, 1])),                    # the first image has no member
    ('3/2,0,0,2,2', _line(3, [0, 2, 2, 5], [1, 2, 0, 3, 4], [0, 0, 1, 1, 2])),            # the middle one
    ('3/0,1,0', _line(2, [0, 2, 3, 3], [0, 2, 1], [0, 0, 1])),                            # the last one
    ('5/4,1', _line(1, [0, 0, 1, 1, 1, 2], [1, 0], [0, 0])),                              # N > M
    ('2/1,0,1/noslot', _line(2, [0, 1, 3], [1, 0, 2])),                                   # the overlay's call: no slots
]


@pytest.mark.parametrize('case,want', TABLES, ids=[c for c, _ in TABLES])
def test_tables(groups, case, want):
    assert groups(case) == [want]


def test_an_index_outside_the_images_is_reported_with_its_position(groups):
    assert groups('2/0,-1,1', '2/0,1,2', '1/1', '3/0,5,-1') == [
        'error=outside at=1 value=-1 guards=ok', 'error=outside at=2 value=2 guards=ok', 'error=outside at=0 value=1 guards=ok',
        'error=outside at=1 value=5 guards=ok']                                           # the first offender; nothing was written


def test_without_an_index_every_member_has_its_own_image(groups):
    assert groups('1/null/1', '3/null/3', '4/null/2', '1/null/2', '3/null/4') == [
        'most=1 guards=ok', 'most=1 guards=ok', 'most=1 guards=ok', 'error=null_too_many guards=ok', 'error=null_too_many guards=ok']
