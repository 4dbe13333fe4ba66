#!/usr/bin/env python3
"""How often can sd_tile_fast (csrc/retrack_det.hip) leave a side box unread?  CPU only: oracle warp, NumPy float64 integral image, the
screen's model (tests/det_screen_model.py) on every position and on the kernel's waves (2 rows x 64 columns; lit steps of the fast
path only - dark steps read nothing anyway, the row-clipped first and last steps read everything).  Per scan and box size:

    dxy needed      dxx * dyy > thr                                              (the kernel's rare second half)
    dyy -> xx-side  the bound from an exact dyy fails to rule out the xx-side box (the order the kernel uses)
    dxx -> yy-side  the bound from an exact dxx fails to rule out the yy-side box (the other order)

as a share of the positions and of the waves; a wave reads the box when any of its 128 positions needs it.  The gain of the screen
is the share of waves that do NOT read: it depends on the scene, and shrinks with the share of the image that holds strong returns.

python profiles/det_screen_rate.py [bench] [steady] [real]     (default: all three)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import oracle
import det_candidate_cases as dc
import det_screen_model as m

THR = dc.THRESHOLD


def scans(which):
    from radarslampy_amd import synth
    if which == "real":
        pay = np.load(os.path.join(ROOT, "tests", "golden", "tiny_track.npz"))["payload"]
        for t in (0, len(pay) // 2, len(pay) - 1):
            yield "real scan %d (tests/golden/tiny_track.npz)" % t, pay[t].astype(np.float32) / np.float32(255.)
        return
    if which == "bench":
        import bench
        work = bench.WORK_RETRACK
    else:
        work = dict(n_static=460, n_movers=24)                               # what profiles/time_doh.py renders by default
    recs = synth.make_sequence(5, 2, distortion=True, **work)[0]
    yield "%s workload, seed 5 frame 1 %s" % (which, work), oracle.extractDataFromRadarImage(recs[1])[0]


def table(name, polar):
    cart = oracle.convertPolarImageToCartesian(polar)
    S = dc.integral(cart)
    lit = ~dc.dark_steps(polar.shape[1], polar.shape[0])                     # (strips, steps)
    print("%s: image %d x %d, %.1f %% of the strip-steps lit" % (name, cart.shape[0], cart.shape[1], 100.0 * lit.mean()))
    print("  %-28s %21s   %21s" % ("quantity (size 15 / size 30)", "positions", "waves"))
    rows = {"dxy needed": [], "dyy -> xx-side not ruled out": [], "dxx -> yy-side not ruled out": []}
    for size in m.SIZES:
        for key, exact in (("dyy -> xx-side not ruled out", "dyy"), ("dxx -> yy-side not ruled out", "dxx")):
            need, passing, fast = m.waves(S, size, THR, exact)
            sel = lit[:, :, None] & fast[None, :, None] & np.ones(8, bool)   # (strips, steps, 8): the waves of the fast path
            assert not (passing & ~need).any(), "a passing product was ruled out"
            rows[key].append((need[sel].mean(), need.any(axis=-1)[sel].mean()))
        rows["dxy needed"].append((passing[sel].mean(), passing.any(axis=-1)[sel].mean()))
    for key, ((p15, w15), (p30, w30)) in rows.items():
        print("  %-28s %8.2f %% / %6.2f %%   %8.1f %% / %6.1f %%" % (key, 100 * p15, 100 * p30, 100 * w15, 100 * w30))


if __name__ == "__main__":
    for which in (sys.argv[1:] or ["bench", "steady", "real"]):
        for name, polar in scans(which):
            table(name, polar)
