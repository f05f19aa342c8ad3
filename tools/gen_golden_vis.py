#!/usr/bin/env python3
"""Record matplotlib's 'rainbow' colours as lib/vis.py's vis_2d_keypoints forms them (the map sampled at np.linspace(0, 1, L), reversed
to BGR, times 255) for the two skeletons of demo/run.py (L = 16: human36, L = 19: coco) and for L = 1, 2, into
tests/golden/vis_colors.npz.  gator_amd.vis.rainbow_colors must reproduce them exactly without matplotlib
(tests/test_host_draw_refs.py); only this tool needs matplotlib (recorded with 3.10).

    python tools/gen_golden_vis.py [--out tests/golden/vis_colors.npz]"""
import argparse
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMBS = (1, 2, 16, 19)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'vis_colors.npz'))
    a = ap.parse_args()
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    cmap = plt.get_cmap('rainbow')
    rec = {}
    for L in LIMBS:
        rgba = [cmap(i) for i in np.linspace(0, 1, L)]
        rec['L%d' % L] = np.array([(c[2] * 255, c[1] * 255, c[0] * 255) for c in rgba], np.float64)
    np.savez(a.out, matplotlib_version=np.array(matplotlib.__version__), **rec)
    print('%s: %d bytes, matplotlib %s' % (a.out, os.path.getsize(a.out), matplotlib.__version__))


if __name__ == '__main__':
    main()
