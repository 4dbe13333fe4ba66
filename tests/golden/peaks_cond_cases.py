"""Inputs and truth of the find_peaks(distance=, prominence=) fixtures (peaks_cond.npz, written by make_peaks_cond.py).

The truth is live scipy.signal.find_peaks with numpy.argsort rebound to NumPy 1.22.3's introsort (oracle.argsort_numpy122) -
scipy's _select_by_peak_distance looks np.argsort up at call time, and the reference pins numpy 1.22.3, whose unstable sort
decides between equal peak heights - followed by the reference's own mean + std threshold (getPointCloud.py:37-45)."""
import contextlib
import warnings

import numpy as np

DISTANCES = [None, 1.7, 3, 5, 10.5, 20, 4096]
PROMINENCES = [None, 0, 0.01, 0.03, 0.1, 0.3, "attained", (None, 0.05), (0.02, 0.2)]


@contextlib.contextmanager
def numpy122_argsort():
    """np.argsort of a 1-D array as NumPy 1.22.3 orders it, for the duration of the block"""
    import oracle
    orig = np.argsort

    def argsort(a, axis=-1, kind=None, order=None, **kw):
        if kind is None and order is None and not kw and axis in (-1, 0) and np.ndim(a) == 1:
            return oracle.argsort_numpy122(a)
        return orig(a, axis=axis, kind=kind, order=order, **kw)
    np.argsort = argsort
    try:
        yield
    finally:
        np.argsort = orig


def decode(u8):
    """the u8 power codes as the reference's float32 polar image (parseData.py:49-51)"""
    return np.asarray(u8).astype(np.float32) / 255.


def threshold_rows(img, find):
    """getPointCloud.py:26-54 with find(row) -> peak indices standing in for its find_peaks call"""
    out = []
    for az, row in enumerate(np.asarray(img, np.float32)):
        ind = find(row)
        h = row[ind]
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            thr = np.mean(h) + np.std(h)
        keep = ind[h >= thr]
        out.append(np.stack([np.full_like(keep, az), keep], 1))
    return np.concatenate(out).astype(np.int64) if out else np.empty((0, 2), np.int64)


def truth(img, distance=None, prominence=None, numpy122=True):
    """the point cloud the reference computes under its pinned NumPy (numpy122=False: this NumPy's own argsort)"""
    from scipy.signal import find_peaks

    def find(row):
        return find_peaks(row, distance=distance, prominence=prominence)[0]
    with (numpy122_argsort() if numpy122 else contextlib.nullcontext()), warnings.catch_warnings():
        warnings.simplefilter("ignore")                 # PeakPropertyWarning on prominence-0 peaks
        return threshold_rows(img, find)


def hand_u8():
    """16 x 257 u8 rows for the corners: heavy ties, long plateaus, no candidate at all, one or two peaks, a spike among bumps"""
    rng = np.random.default_rng(4242)
    c = 257
    rows = [rng.integers(0, 4, c), rng.integers(0, 2, c),
            np.repeat(rng.integers(0, 6, c), rng.integers(1, 21, c))[:c],
            np.full(c, 7), np.arange(c) % 256, np.r_[np.zeros(100), 9, np.zeros(c - 101)]]
    two = np.zeros(c)
    two[[50, 53, 56]] = 9                                # equal peaks closer than most distances: tie order decides
    rows += [two, np.r_[200, np.zeros(c - 2), 200], rng.integers(0, 256, c)]
    spike = rng.integers(0, 3, c)
    spike[128] = 180
    rows.append(spike)
    rows += [rng.integers(0, 3, c) for _ in range(4)]
    plateau = np.repeat(rng.integers(0, 4, 20), 13)[:c]
    rows.append(np.pad(plateau, (0, c - len(plateau))))
    return np.stack(rows).astype(np.uint8)


def alt4096_u8():
    """4096-column rows with a candidate at every odd position: 2047 of them, the most a row of ROAM_MAX_COLS can have"""
    rng = np.random.default_rng(4096)
    a = np.zeros((2, 4096), np.uint8)
    a[0, 1::2] = 1
    a[1, 1::2] = rng.integers(1, 5, 2048)
    return a


def hand_f32():
    """generic float32 rows (not k / 255): ties, plateaus and noise"""
    rng = np.random.default_rng(3232)
    a = (rng.integers(0, 5, (8, 300)) / 7).astype(np.float32)
    a[4:] = (rng.random((4, 300), dtype=np.float32) ** 2).astype(np.float32)
    a[6, 100:140] = 0.75
    return a


def prominence_arg(p):
    """fixture encoding of a prominence argument: [] = None, [v] = v, [a, b] = (a, b) with NaN = None"""
    p = np.asarray(p, np.float64)
    if p.size == 0:
        return None
    if p.size == 1:
        return float(p[0])
    return tuple(None if np.isnan(v) else float(v) for v in p)


def distance_arg(d):
    d = np.asarray(d, np.float64)
    return None if d.size == 0 else float(d[0])


def load_cases(z, golden_dir):
    """[(name, input image as the u8 codes or None, f32 image, distance, prominence, expected (K, 2) int64)] of peaks_cond.npz"""
    import os
    import hashlib
    from gen_inputs import synthetic_polar_u8
    base = np.load(os.path.join(golden_dir, "peaks.npz"))
    srcs = {}
    for name in z["inputs"]:
        name = str(name)
        if name in ("real0_u8", "real1_u8"):
            u8 = base[name]
        elif name.startswith("synth"):
            seed, rows = (int(v) for v in name[5:].split("x"))
            u8 = synthetic_polar_u8(seed, rows=rows)
            assert hashlib.sha256(u8.tobytes()).hexdigest() == str(z["sha_" + name])
        elif name == "hand_f32":
            srcs[name] = (None, z[name])
            continue
        else:
            u8 = z[name]
        srcs[name] = (u8, decode(u8))
    cases = []
    for i in range(int(z["n_cases"])):
        name = str(z[f"c{i}_input"])
        u8, f32 = srcs[name]
        cases.append((name, u8, f32, distance_arg(z[f"c{i}_dist"]), prominence_arg(z[f"c{i}_prom"]),
                      z[f"c{i}_out"].astype(np.int64).reshape(2, -1).T))
    return cases
