"""Shared, seeded inputs of the scan-context tests (test_scan_context_cpu.py, test_gpu_scan_context.py).  The model's results are
computed once per case and cached; nothing here touches a device."""
import functools
import os

import numpy as np

import scan_context_model as model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# ---------------------------------------------------------------------------------------------------------------- describe
# name -> (S, R, clip_px); the images come from describe_images(name): (n, rows, cols) float32, possibly a strided view
DESCRIBE_CASES = {
    "real_60x20": (60, 20, 2025),
    "rand_16x8": (16, 8, None),
    "rand_64x128_one_pixel_bins": (64, 128, None),
    "rand_7x3": (7, 3, None),
    "strided_399x497_clip400": (60, 20, 400),
    "batch65_16x8": (16, 8, 100),
    "batch3_7x3": (7, 3, None),
}
FLOORS = (0.0, 30.0 / 255.0)


@functools.lru_cache(maxsize=None)
def real_codes():
    """the two real scans of golden/peaks.npz: (2, 400, 2025) uint8"""
    g = np.load(os.path.join(GOLDEN, "peaks.npz"))
    return np.stack([g["real0_u8"], g["real1_u8"]])


@functools.lru_cache(maxsize=None)
def describe_images(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "real_60x20":
        return real_codes().astype(np.float32) / np.float32(255.0)
    if name == "strided_399x497_clip400":
        return rng.random((2, 399, 504), dtype=np.float32)[:, :, 5:502]
    n = {"batch65_16x8": 65, "batch3_7x3": 3}.get(name, 1)
    return rng.random((n, 64, 128), dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------- distances
# name -> (S, R, entries, queries, content).  queries: None = every entry; "regular" = every entry but the all-zero and the
# sector-constant one; a number = that many, those two left out.  Every shift of a pair with one of those two ties (exactly, or within
# rounding), so its best shift is not compared: as queries they would take 4 / entries of the pairs out of the comparison, and they are
# queries only where that stays under the 5 % the CPU test allows - in the two cases of 200 entries that are cheap in the model
DISTANCE_CASES = {
    "60x20_n1": (60, 20, 1, None, "uniform"),
    "60x20_n63": (60, 20, 63, "regular", "uniform"),
    "60x20_n64": (60, 20, 64, "regular", "uniform"),
    "60x20_n65": (60, 20, 65, "regular", "uniform"),
    "60x20_n200": (60, 20, 200, 40, "uniform"),
    "60x20_n1000": (60, 20, 1000, 12, "uniform"),
    "7x3_n200": (7, 3, 200, None, "uniform"),
    "64x32_n200": (64, 32, 200, 20, "uniform"),
    "256x128_n65": (256, 128, 65, 5, "uniform"),
    "2x1_n200": (2, 1, 200, None, "one_sector"),
}
# the special entries of a database of at least 8: (index or None when the database is smaller)
ZERO_SECTORS, ALL_ZERO, SECTOR_CONSTANT, TRIPLE_FIRST = 1, 2, 3, 5


def triple(n):
    """the three indices that hold one descriptor"""
    return (TRIPLE_FIRST, n // 2, n - 1)


@functools.lru_cache(maxsize=None)
def distance_case(name):
    """-> (desc (n, S, R) float32, query indices (m,) int32)"""
    S, R, n, nq, content = DISTANCE_CASES[name]
    rng = np.random.default_rng(1000 + sum(map(ord, name)))
    D = rng.random((n, S, R), dtype=np.float32)
    if content == "one_sector":             # S = 2, R = 1: every shift of two full columns ties, so each entry has one empty sector
        D[np.arange(n), rng.integers(0, S, n)] = 0
    if n >= 8:
        D[ZERO_SECTORS, rng.permutation(S)[:S // 2]] = 0
        for j in range(8, n, 7):                                  # more entries with a few empty sectors
            if content == "uniform":
                D[j, rng.permutation(S)[:int(rng.integers(1, 4))]] = 0
        D[ALL_ZERO] = 0
        D[SECTOR_CONSTANT] = D[SECTOR_CONSTANT, 0]
        a, b, c = triple(n)
        D[b] = D[a]
        D[c] = D[a]
    if nq is None:
        q = np.arange(n)
    elif nq == "regular":
        q = np.array([j for j in range(n) if j not in (ALL_ZERO, SECTOR_CONSTANT)])
    else:                                                         # the ends, two special entries and a seeded choice of the rest
        fixed = [0, ZERO_SECTORS, TRIPLE_FIRST, n - 1]
        rest = [j for j in rng.permutation(n) if j not in fixed + [ALL_ZERO, SECTOR_CONSTANT]][:nq - len(fixed)]
        q = np.array(fixed + rest)
    return D, q.astype(np.int32)


@functools.lru_cache(maxsize=None)
def distance_model(name):
    """-> (dist (m, n), shift (m, n), second-best d_k (m, n)) of the model for the case's queries against its whole database"""
    D, q = distance_case(name)
    return model.distances(D[q], D)


@functools.lru_cache(maxsize=None)
def tolerance_measured():
    """name -> the largest |d_k in the model's order - d_k in the kernel's order| (both float64, scan_context_model) over every
    shift of every pair of the case"""
    out = {}
    for name in DISTANCE_CASES:
        D, q = distance_case(name)
        prep = model.prepare(D)
        out[name] = max(float(np.abs(model.shift_distances(D[i], D, prep) - model.shift_distances_kernel_order(D[i], D, prep)).max())
                        for i in q)
    return out


def tolerance():
    """the bound on |device distance - model distance|: ten times the largest difference between the two summation orders"""
    return 10.0 * max(tolerance_measured().values())


def decided(name):
    """(m, n) bool: the pairs of a distance case whose best and second-best d_k differ by more than twice the tolerance in the
    model - the only ones on which the best shift is compared"""
    dist, _, second = distance_model(name)
    return second - dist > 2.0 * tolerance()


# ---------------------------------------------------------------------------------------------------------------- top-k
TOPK_S, TOPK_R, TOPK_ENTRIES, TOPK_QUERIES, TOPK_PLANTED = 60, 20, 160, 3, 8
TOPK_MAX_DISTANCE = 0.2


@functools.lru_cache(maxsize=None)
def topk_case():
    """-> (desc (n, S, R), query indices (3,), planted (3, 8) indices by rising noise, planted shifts (3, 8)).  Per query eight rolled
    copies with uniform noise in [-a, a], a = 0.05 ... 0.75, clipped at zero, sit among random entries; the queries are the last three entries"""
    rng = np.random.default_rng(77)
    n, S, R = TOPK_ENTRIES, TOPK_S, TOPK_R
    D = rng.random((n, S, R), dtype=np.float32)
    q = np.arange(n - TOPK_QUERIES, n)
    slots = rng.permutation(n - TOPK_QUERIES)[:TOPK_QUERIES * TOPK_PLANTED].reshape(TOPK_QUERIES, TOPK_PLANTED)
    shifts = rng.integers(0, S, size=slots.shape)
    amps = np.linspace(0.05, 0.75, TOPK_PLANTED)
    for i in range(TOPK_QUERIES):
        for p in range(TOPK_PLANTED):
            noise = np.float32(amps[p]) * (2 * rng.random((S, R), dtype=np.float32) - 1)
            D[slots[i, p]] = np.maximum(np.roll(D[q[i]], shifts[i, p], axis=0) + noise, 0)
    return D, q.astype(np.int32), slots, shifts


@functools.lru_cache(maxsize=None)
def topk_model():
    D, q, _, _ = topk_case()
    return model.distances(D[q], D)


def topk_queries():
    """(tag, max_index (3,), k, max_distance) of every top-k query on topk_case()"""
    D, q, slots, _ = topk_case()
    base = np.full(TOPK_QUERIES, len(D) - TOPK_QUERIES, np.int32)
    cut = np.sort(slots, axis=1)[:, 4].astype(np.int32)           # the four lowest planted indices of each query stay
    out = [(f"k{k}", base, k, TOPK_MAX_DISTANCE) for k in (1, 3, 8, 32)]
    out.append(("max_index_0", np.zeros(TOPK_QUERIES, np.int32), 8, TOPK_MAX_DISTANCE))
    out.append(("max_index_cuts_the_planted", cut, 8, TOPK_MAX_DISTANCE))
    out.append(("no_threshold_k32", base, 32, np.inf))
    return out


@functools.lru_cache(maxsize=None)
def small_db_case():
    """k larger than the database: five entries at (7, 3)"""
    return np.random.default_rng(5).random((5, 7, 3), dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------- revisits
REVISIT_S, REVISIT_R, REVISIT_CLIP = 60, 20, 2025
PLACES = [(0, 0), (300, 0), (0, 400), (-500, 250), (800, 800), (150, -700), (60, 0), (0, -90)]
REVISITS = [(0, (1.0, -0.5, np.pi / 2)), (3, (-499.2, 250.6, -1.1)), (4, (800.5, 799.3, 4.2))]      # (place, pose), t_index 20, 21, 22
REVISIT_FLOOR_CODES = (0, 30)


def place_pose(i):
    return (float(PLACES[i][0]), float(PLACES[i][1]), 0.3 * i)


@functools.lru_cache(maxsize=None)
def revisit_records():
    """eleven Oxford records (400 x 3779 uint8): the eight places, then the three revisits"""
    from radarslampy_amd import synth
    w = synth.StreamWorld(5, per_tile=40)
    recs = [synth.render_stream_record(w, place_pose(i), t_index=i) for i in range(len(PLACES))]
    recs += [synth.render_stream_record(w, pose, t_index=20 + t) for t, (_, pose) in enumerate(REVISITS)]
    return recs


@functools.lru_cache(maxsize=None)
def next_record_after_place_0():
    """the scan one frame after place 0 (0.9 m on): something for an engine's lane to step to"""
    from radarslampy_amd import synth
    return synth.render_stream_record(synth.StreamWorld(5, per_tile=40), (0.9, 0.02, 0.01), t_index=1)


@functools.lru_cache(maxsize=None)
def revisit_descriptors(floor_code):
    from radarslampy_amd import synth
    return np.stack([model.describe_u8(r[:, synth.META:synth.META + REVISIT_CLIP], REVISIT_S, REVISIT_R, REVISIT_CLIP, floor_code)
                     for r in revisit_records()])


def revisit_true_shift(t):
    """the yaw of revisit t minus the yaw of its place, in sectors, in [0, S)"""
    place, pose = REVISITS[t]
    return ((pose[2] - place_pose(place)[2]) % (2 * np.pi)) * REVISIT_S / (2 * np.pi)
