#!/usr/bin/env python3
"""peaks_cond.npz: the reference's getPointCloudPolarInd(polarImage, peakDistance, peakProminence) (getPointCloud.py:11-54).
RUNS ONLY IN THE BUILD CONTAINER, like make_goldens.py (same import stubs).

The reference is called as it is, with numpy.argsort rebound to NumPy 1.22.3's introsort (oracle.argsort_numpy122, the
reference's pin) for the duration of each call: find_peaks' distance condition walks the peaks in np.argsort order of their
heights, and equal heights are everywhere in rows of u8 codes.  Inputs: the two real scans of peaks.npz (named by key, not
copied), seeded synthetic scans (named by seed and row count, checked by hash), the hand-made rows of peaks_cond_cases.py.
Stored: arrays only, each output as int16 (2, K) = the transposed (K, 2) point cloud."""
import hashlib
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path.insert(0, OUT)
sys.path.insert(0, ROOT)
from make_goldens import REF, _install_stubs, quiet            # noqa: E402
from gen_inputs import synthetic_polar_u8                       # noqa: E402
import peaks_cond_cases as pc                                   # noqa: E402


def attained_prominence(img):
    """a prominence value that real candidates have exactly (the pmin <= prominence test at equality)"""
    from scipy.signal import find_peaks, peak_prominences
    vals = np.concatenate([peak_prominences(r.astype(np.float64), find_peaks(r)[0])[0] for r in img])
    u = np.unique(vals)
    return float(u[len(u) // 2])


def main():
    import oracle
    oracle.build()
    _install_stubs()
    sys.path.insert(0, REF)
    cwd = os.getcwd()
    os.chdir(REF)
    with quiet():
        import getPointCloud as r_pc
    os.chdir(cwd)

    base = np.load(os.path.join(OUT, "peaks.npz"))
    z = {}
    inputs = {}
    for k in ("real0_u8", "real1_u8"):
        inputs[k] = pc.decode(base[k])
    for seed in (5, 6):
        name = f"synth{seed}x32"
        u8 = synthetic_polar_u8(seed, rows=32)
        z["sha_" + name] = np.array(hashlib.sha256(u8.tobytes()).hexdigest())
        inputs[name] = pc.decode(u8)
    for name, u8 in (("hand_u8", pc.hand_u8()), ("alt4096_u8", pc.alt4096_u8())):
        z[name] = u8
        inputs[name] = pc.decode(u8)
    z["hand_f32"] = pc.hand_f32()
    inputs["hand_f32"] = z["hand_f32"]

    att = attained_prominence(inputs["real0_u8"])
    prom = [att if p == "attained" else p for p in pc.PROMINENCES]
    scan_grid = ([(d, None) for d in pc.DISTANCES[1:]] + [(None, p) for p in prom[1:]] +
                 [(3, 0.03), (5, (0.02, 0.2)), (10.5, 0.01), (1.7, 0), (20, att), (4096, 0.1), (3, (None, 0.05))])
    full_grid = [(d, p) for d in pc.DISTANCES for p in prom if not (d is None and p is None)]
    grids = {"real0_u8": scan_grid, "real1_u8": scan_grid, "synth5x32": scan_grid, "synth6x32": full_grid,
             "hand_u8": full_grid, "hand_f32": full_grid,
             "alt4096_u8": [(d, None) for d in pc.DISTANCES[1:]] + [(None, 0), (3, 0), (5, (None, 0.005)), (20, 0.001)]}
    z["inputs"] = np.array(list(grids))
    n = 0
    for name, grid in grids.items():
        for d, p in grid:
            with pc.numpy122_argsort(), quiet():
                got = r_pc.getPointCloudPolarInd(inputs[name], peakDistance=d, peakProminence=p)
            got = np.asarray(got).reshape(-1, 2)
            assert got.max(initial=0) < 2 ** 15
            z[f"c{n}_input"] = np.array(name)
            z[f"c{n}_dist"] = np.array([] if d is None else [d], np.float64)
            z[f"c{n}_prom"] = np.array([] if p is None else ([p] if np.isscalar(p) else [np.nan if v is None else v for v in p]),
                                       np.float64)
            z[f"c{n}_out"] = np.ascontiguousarray(got.T).astype(np.int16)      # [azimuths; ranges]: compresses better
            n += 1
    z["n_cases"] = np.array(n)
    path = os.path.join(OUT, "peaks_cond.npz")
    np.savez_compressed(path, **z)
    print(path, n, "cases", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
