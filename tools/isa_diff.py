"""Per-kernel comparison of the device assembly of two source trees (build machine only: it compiles, it runs nothing).
    python tools/isa_diff.py <parent-tree> <new-tree> [sources...]
Each source (a name under gator_amd/csrc/, default: every .hip of either tree's build.SOURCES) is compiled in both trees with that tree's
own build.FLAGS as `hipcc $FLAGS -x hip --cuda-device-only -S`.  The listings are split at `.type <symbol>,@function` ...
`.end_amdhsa_kernel` and compared by symbol over ALL the given sources, so a kernel that moved to another file is matched with itself.
Masked: the per-function number in local labels and in the comments that quote them (.LBB<n>_, BB<n>_, .Lfunc_end<n>: a kernel's position
in its file) and runs of blanks (the label column shifts with that number's width).  Nothing else.
Prints `identical` / `DIFFERS` with the instruction counts per kernel, then the kernels only one tree has; exit status 1 if any differs."""
import concurrent.futures
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile

LABEL = re.compile(r'(\.LBB|BB|\.Lfunc_end|\.Lfunc_begin)\d+')
BLANKS = re.compile(r'[ \t]+')
TYPE = re.compile(r'^\s*\.type\s+(\S+),@function\s*$', re.M)


def tree_build(tree):
    spec = importlib.util.spec_from_file_location('isa_diff_build_%d' % abs(hash(tree)), os.path.join(tree, 'gator_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assemble(build, source, out):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    cmd = [hipcc] + build.FLAGS + ['-x', 'hip', '--cuda-device-only', '-S', os.path.join(build.CSRC, source), '-o', out]
    subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
    return open(out).read()


def kernels(text):
    """{symbol: (masked lines, instruction count)} of the kernels (not the plain device functions) of one listing."""
    out = {}
    marks = list(TYPE.finditer(text))
    for m, nxt in zip(marks, marks[1:] + [None]):
        body = text[m.start():nxt.start() if nxt else len(text)]
        end = body.find('.end_amdhsa_kernel')
        if end < 0:
            continue
        lines = [BLANKS.sub(' ', LABEL.sub(r'\1#', ln)).strip() for ln in body[:end].splitlines() if '__hip_cuid_' not in ln]
        code = lines[:next((i for i, ln in enumerate(lines) if ln.startswith('.section')), len(lines))]
        n = sum(1 for ln in code if ln and ln[0] not in '.;' and not ln.split(';')[0].strip().endswith(':'))
        out[m.group(1)] = (lines, n)
    return out


def demangle(names):
    tool = shutil.which('llvm-cxxfilt') or shutil.which('c++filt')
    if not tool or not names:
        return {n: n for n in names}
    r = subprocess.run([tool] + list(names), capture_output=True, text=True, check=True)
    return dict(zip(names, r.stdout.splitlines()))


def main():
    parent, new, sources = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2]), sys.argv[3:]
    builds = [tree_build(parent), tree_build(new)]
    found = [{}, {}]
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(8) as pool:
        jobs = []
        for side, b in enumerate(builds):
            for s in (sources or [s for s in b.SOURCES if s.endswith('.hip')]):
                if os.path.exists(os.path.join(b.CSRC, s)):
                    jobs.append((side, s, pool.submit(assemble, b, s, os.path.join(tmp, '%d_%s.s' % (side, s)))))
        for side, s, job in jobs:
            for sym, (lines, n) in kernels(job.result()).items():
                found[side][sym] = (s, lines, n)
    names = demangle(sorted(set(found[0]) | set(found[1])))
    differs = 0
    for sym in sorted(set(found[0]) & set(found[1]), key=names.get):
        (s0, l0, n0), (s1, l1, n1) = found[0][sym], found[1][sym]
        same = l0 == l1
        differs += not same
        where = s0 if s0 == s1 else '%s -> %s' % (s0, s1)
        print('%-10s %6d -> %6d  %-28s %s' % ('identical' if same else 'DIFFERS', n0, n1, where, names[sym]))
    for side, what in ((0, 'only in parent'), (1, 'only in new')):
        for sym in sorted(set(found[side]) - set(found[1 - side]), key=names.get):
            print('%-17s %6d  %-28s %s' % (what, found[side][sym][2], found[side][sym][0], names[sym]))
    return 1 if differs else 0


if __name__ == '__main__':
    sys.exit(main())
