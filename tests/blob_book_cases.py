"""Crafted candidate lists for the device blob bookkeeping (csrc/retrack_blobs.hip, K4-K6): every case is a seeded generator that
returns what the determinant kernel would have left - rc = row << 16 | col << 2 | layer (uint32, shuffled), val (float64) - and the
side of the square it lives in, and names the switch of the kernel it is there to cross.  tests/test_blob_book_cpu.py asserts each
case's properties (tree nodes, pairs, overlapping pairs, order sensitivity, the introselect fallback, the slid split) with live
scipy / CPython and the oracle alone, so that a case cannot silently stop reaching its branch; tests/test_gpu_blob_book.py runs them
through roam_engine_debug_blobs.

Everything the device does is integer or exactly rounded float64, so the truth (truth()) is compared without any tolerance."""
import ctypes as C
import math
from collections import namedtuple

import numpy as np

import oracle

SIG = (None, 5.005, 10.0)                        # sigma of layer 1 | 2: the engine's (np.linspace(0.01, 10, 3)[1:])
MAX_PTS, MAX_PAIRS, MAX_TASKS = 2048, 32767, 8192
SMALL_PTS, SMALL_PAIRS, NPL, LDS_PAIRS, NCL, WAVE_MIN = 1024, 1228, 3328, 4914, 4096, 100
F_CAND, F_TREE, F_PAIR = 1, 2, 4
SMALL_SIDE = 130                                 # cases within this square also fit the small batch engine (W = 132)

# name, rc, val, side, cand_n (None = the rows given), why (the switch), want: properties the CPU test asserts -
#   pairs / pairs_min / pairs_max, nodes_min, overlaps_min, sensitive, fallback (root introselect takes the heap select), slid (the
#   oracle's tree has a slid split), flip (scipy's float64 bound and the integer bound disagree at a node pair), flags, tasks_min
Case = namedtuple("Case", "name rc val side cand_n why want")


def radius(layers):
    return 2 * (SIG[2] if np.any(np.asarray(layers) == 2) else SIG[1]) * math.sqrt(2)


def pack(rows, cols, layers):
    return (np.asarray(rows, np.uint32) << 16) | (np.asarray(cols, np.uint32) << 2) | np.asarray(layers, np.uint32)


def unpack(rc):
    rc = np.asarray(rc, np.uint32)
    return (rc >> 16).astype(np.int64), ((rc >> 2) & 0x3fff).astype(np.int64), (rc & 3).astype(np.int64)


def blobs_of(rc, val):
    """the blobs in peak_local_max order: C (row, col, layer) order, then a stable sort by falling response"""
    rc, val = np.asarray(rc, np.uint32), np.asarray(val, np.float64)
    o = np.argsort(rc, kind="stable")
    rc, val = rc[o], val[o]
    o = np.argsort(-val, kind="stable")
    r, c, l = unpack(rc[o])
    return np.column_stack([r, c, np.where(l == 2, SIG[2], SIG[1])]).astype(np.float64)


def ssc_indices(kp, W):
    kp = np.ascontiguousarray(kp, np.float64)
    sel = np.empty(max(len(kp), 1), np.int32)
    n = oracle.lib().oracle_ssc(kp.ctypes.data_as(C.POINTER(C.c_double)), len(kp), 200, C.c_double(0.1), int(W), int(W),
                                sel.ctypes.data_as(C.POINTER(C.c_int32)))
    return sel[:n].copy()


def truth(rc, val, W):
    """-> kp (m, 3), sel (indices into kp): sort by key, stable argsort of -val, oracle.prune_blobs, oracle.argsort_numpy122 of the
    sigmas, oracle.ssc(kp, 200, 0.1, W, W)"""
    b = blobs_of(rc, val)
    if len(b) == 0:
        return np.empty((0, 3)), np.empty(0, np.int32)
    kept = oracle.prune_blobs(b)
    kp = kept[oracle.argsort_numpy122(kept[:, 2])]
    sel = ssc_indices(kp, W)
    assert np.array_equal(kp[sel], oracle.ssc(kp, 200, 0.1, W, W))
    return kp, sel


# ------------------------------------------------------------------------------------------------ generators
def _finish(rng, rows, cols, layers, val=None):
    rows, cols, layers = np.asarray(rows), np.asarray(cols), np.asarray(layers)
    rc = pack(rows, cols, layers)
    assert len(np.unique(rc)) == len(rc)
    if val is None:
        val = rng.permutation(len(rc)).astype(np.float64) * 1e-4 + 5e-4      # distinct responses
    p = rng.permutation(len(rc))
    return rc[p], np.asarray(val, np.float64)[p]


def _uniform_px(rng, n, side, lo=0):
    """n distinct pixels of [lo, lo + side)^2"""
    px = rng.choice(side * side, size=n, replace=False)
    return lo + px // side, lo + px % side


def uniform(seed, n, side, layer=None):
    rng = np.random.default_rng(seed)
    r, c = _uniform_px(rng, n, side)
    lay = rng.integers(1, 3, n) if layer is None else np.full(n, layer)
    return _finish(rng, r, c, lay)


def n_pairs(rows, cols, layers):
    from scipy.spatial import cKDTree
    if len(rows) < 2:
        return 0
    return len(cKDTree(np.column_stack([rows, cols]).astype(float)).query_pairs(radius(layers)))


def uniform_with_pairs(seed, n, side, target):
    """uniform distinct pixels moved one at a time until query_pairs returns exactly `target` pairs (n and the side stay)"""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(seed)
    r, c = _uniform_px(rng, n, side)
    lay = rng.integers(1, 3, n)
    lay[:2] = (1, 2)
    rad = radius(lay)
    pts = np.column_stack([r, c]).astype(float)
    for _ in range(20000):
        tree = cKDTree(pts)
        cur = len(tree.query_pairs(rad))
        if cur == target:
            break
        deg = np.array([len(x) - 1 for x in tree.query_ball_point(pts, rad)])
        i = int(rng.integers(n))
        q = rng.integers(0, side, 2).astype(float)
        if (pts == q).all(axis=1).any():
            continue
        gain = len(tree.query_ball_point(q, rad)) - (1 if np.hypot(*(pts[i] - q)) <= rad else 0) - deg[i]
        if abs(cur + gain - target) < abs(cur - target):
            pts[i] = q
    else:
        raise AssertionError("no layout with %d pairs" % target)
    return _finish(rng, pts[:, 0].astype(int), pts[:, 1].astype(int), lay)


def cluster(seed, n, rad, centre, layer=2):
    """n candidates on the pixels of one disc (both layers unless `layer`)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[-rad:rad + 1, -rad:rad + 1]
    m = yy * yy + xx * xx <= rad * rad
    slots = [(centre + y, centre + x, l) for y, x in zip(yy[m], xx[m]) for l in ((1, 2) if layer is None else (layer,))]
    pick = rng.choice(len(slots), size=n, replace=False)
    r, c, l = np.array([slots[k] for k in pick]).T
    return _finish(rng, r, c, l)


def at_extreme(seed, a, b, side, at_max=False, embed=0, gap=40):
    """a candidates on ONE row (the node's minimum - or maximum - along its widest dimension: the columns stay within side / 2), b
    elsewhere, at least `gap` rows away and one of them on the far row; embed: plus that many uniform candidates of a 1000-pixel
    square below (the layout is then a subtree, not the root)"""
    rng = np.random.default_rng(seed)
    wc = side // 2
    slots = rng.permutation(2 * wc)[:a]                                        # (col, layer) on the row
    r = [side - 1 if at_max else 0] * a
    c, l = list(slots % wc), list(slots // wc + 1)
    px = rng.choice((side - gap) * wc, size=b, replace=False)
    br = px // wc + (0 if at_max else gap)
    br[0] = 0 if at_max else side - 1
    r += list(br); c += list(px % wc); l += list(rng.integers(1, 3, b))
    if embed:
        er, ec = _uniform_px(rng, embed, 1000)
        r += list(er + side + 40); c += list(ec); l += list(rng.integers(1, 3, embed))
    return _finish(rng, r, c, l)


def three_rows(seed, counts=(3, 12, 5), rows=(0, 500, 900)):
    """the 20-point node of keys 0 x 3, 500 x 12, 900 x 5: its 17-point child has its median at its minimum"""
    rng = np.random.default_rng(seed)
    r = np.repeat(rows, counts)
    c = rng.permutation(400)[:len(r)]
    return _finish(rng, r, c, rng.integers(1, 3, len(r)))


def slid_flip(seed, n_s=80, n_b=38):
    """three clusters in columns 0 .. 20: S (rows 480 .. 499, 80 points), A (row 500: every column in both layers, 42 points) and B
    (rows 501 .. 540, 38 points).  The root's median row is 500; its greater child A + B has its median at its minimum, so the split
    slides and A's tracker box ends at nextafter(500).  Against the halves of S (rows from 480, columns spanning 20) the box distance
    is (20 + 2^-44)^2 + 20^2 > 800.0000000000001 = (2 * 10 * sqrt 2)^2 in float64, while 20^2 + 20^2 = 800 is below it: scipy walks
    these node pairs with the distance test (both nodes split at once), the integer bound would not (the first node down to its
    leaves, then the second).  The halves of S have inner children (40 -> 20 + 20 points), so the two descents meet the leaf blocks in
    another order: a traversal that ignores the slid bit emits the same pairs in another order (asserted on the CPU; the GPU test
    compares the device's pair list with the emission order)"""
    rng = np.random.default_rng(seed)
    while True:
        px = rng.choice(20 * 21, size=n_s, replace=False)
        sr, sc = 480 + px // 21, px % 21
        if sr.min() == 480 and sc.min() == 0 and sc.max() == 20:
            break
    ar, ac, al = [500] * 42, list(range(21)) * 2, [1] * 21 + [2] * 21
    px = rng.choice(40 * 21, size=n_b, replace=False)
    br, bc = 501 + px // 21, px % 21
    br[0] = 540
    lay = list(rng.integers(1, 3, n_s)) + al + list(rng.integers(1, 3, n_b))
    return _finish(rng, list(sr) + ar + list(br), list(sc) + ac + list(bc), lay)


# ---- McIlroy's adversary against a model of libstdc++'s introselect
class Trace(list):
    pass


def introselect(a, first, nth, last, lt, partition=None, trace=None):
    """std::nth_element of libstdc++ on the list a[first:last) in place: median of three moved to the front, unguarded partition, a
    budget of 2 * floor(log2 n) rounds, then heap select; insertion sort of the last three.  lt(x, y): the comparator on ELEMENTS.
    partition(a, first, last, lt) -> cut replaces the unguarded partition (the wave-parallel form); trace collects what happened"""
    trace = Trace() if trace is None else trace
    if first == last or nth == last:
        return trace
    depth = 2 * ((last - first).bit_length() - 1)
    while last - first > 3:
        if depth == 0:
            trace.append(("heap_select", first, nth, last))
            _heap_select(a, first, nth + 1, last, lt)
            a[first], a[nth] = a[nth], a[first]
            return trace
        depth -= 1
        mid = first + (last - first) // 2
        x, y, z = first + 1, mid, last - 1
        if lt(a[x], a[y]):
            s = y if lt(a[y], a[z]) else (z if lt(a[x], a[z]) else x)
        else:
            s = x if lt(a[x], a[z]) else (z if lt(a[y], a[z]) else y)
        a[first], a[s] = a[s], a[first]
        if partition is None:
            f, l, piv = first + 1, last, a[first]
            while True:
                while lt(a[f], piv):
                    f += 1
                l -= 1
                while lt(piv, a[l]):
                    l -= 1
                if not f < l:
                    break
                a[f], a[l] = a[l], a[f]
                f += 1
        else:
            f = partition(a, first, last, lt)
        trace.append(("partition", first, last, f))
        if f <= nth:
            first = f
        else:
            last = f
    for i in range(first + 1, last):
        v = a[i]
        if lt(v, a[first]):
            a[first + 1:i + 1] = a[first:i]
            a[first] = v
        else:
            j = i
            while lt(v, a[j - 1]):
                a[j] = a[j - 1]
                j -= 1
            a[j] = v
    return trace


def _adjust_heap(a, base, hole, length, value, lt):
    top, child = hole, hole
    while child < (length - 1) // 2:
        child = 2 * (child + 1)
        if lt(a[base + child], a[base + child - 1]):
            child -= 1
        a[base + hole] = a[base + child]
        hole = child
    if length % 2 == 0 and child == (length - 2) // 2:
        child = 2 * (child + 1)
        a[base + hole] = a[base + child - 1]
        hole = child - 1
    parent = (hole - 1) // 2
    while hole > top and lt(a[base + parent], value):
        a[base + hole] = a[base + parent]
        hole = parent
        parent = (hole - 1) // 2
    a[base + hole] = value


def _heap_select(a, first, middle, last, lt):
    length = middle - first
    if length >= 2:
        for parent in range((length - 2) // 2, -1, -1):
            _adjust_heap(a, first, parent, length, a[first + parent], lt)
    for i in range(middle, last):
        if lt(a[i], a[first]):
            v = a[i]
            a[i] = a[first]
            _adjust_heap(a, first, 0, length, v, lt)


def adversary_keys(n):
    """distinct keys 0 .. n-1 for the items 0 .. n-1 (cKDTree's initial index order) that McIlroy's adversary ("A killer adversary for
    quicksort", 1999) fixes while introselect(nth = n / 2) runs on them: every item is "gas" until a comparison forces a value"""
    gas = n
    val = [gas] * n
    state = dict(solid=0, cand=0)

    def freeze(x):
        val[x] = state["solid"]
        state["solid"] += 1

    def lt(x, y):
        if val[x] == gas and val[y] == gas:
            freeze(x if x == state["cand"] else y)
        if val[x] == gas:
            state["cand"] = x
        elif val[y] == gas:
            state["cand"] = y
        return val[x] < val[y]

    introselect(list(range(n)), 0, n // 2, n, lt)
    for x in range(n):
        if val[x] == gas:
            freeze(x)
    assert sorted(val) == list(range(n))
    return np.array(val)


def adversary(seed, n, layer=None):
    """candidates whose rows (the widest dimension) are the adversary's keys in the order cKDTree meets them: blob i (response order)
    gets key[i]; the columns stay within n / 2"""
    rng = np.random.default_rng(seed)
    rows = adversary_keys(n)
    cols = rng.integers(0, max(2, n // 2), n)
    lay = rng.integers(1, 3, n) if layer is None else np.full(n, layer)
    val = (n - np.arange(n)).astype(np.float64) * 1e-4 + 5e-4                  # falling: response order = item order
    rc = pack(rows, cols, lay)
    p = rng.permutation(n)
    return rc[p], val[p]


def ties_values(seed, n, side):
    rng = np.random.default_rng(seed)
    r, c = _uniform_px(rng, n, side)
    return _finish(rng, r, c, rng.integers(1, 3, n), val=rng.choice([5e-4, 1e-3, 2e-3, 4e-3], n))


def ties_both_layers(seed, n, side):
    rng = np.random.default_rng(seed)
    r, c = _uniform_px(rng, n // 2, side)
    return _finish(rng, np.tile(r, 2), np.tile(c, 2), np.repeat([1, 2], n // 2))


def one_line(seed, n, side, axis):
    rng = np.random.default_rng(seed)
    slots = rng.permutation(2 * side)[:n]
    line, lay, fixed = slots % side, slots // side + 1, np.full(n, side // 3)
    return _finish(rng, *((fixed, line) if axis == 0 else (line, fixed)), lay)


def _case(name, gen, side, why, cand_n=None, **want):
    rc, val = gen
    r, c, _ = unpack(rc)
    assert len(rc) == 0 or max(r.max(), c.max()) < side, name
    return Case(name, rc, val, side, cand_n, why, want)


_cases = None


def cases():
    """every case, built once.  Sides: SMALL_SIDE cases fit both engines of the GPU test, the others the W = 2048 engine only"""
    global _cases
    if _cases is not None:
        return _cases
    S = SMALL_SIDE
    L = []
    # ---- candidate counts: empty, one, two, a leaf / the first split (16 / 17), one lane / the wavefront at the root (100 / 101)
    for n in (0, 1, 2, 16, 17, 100, 101):
        L.append(_case("count_%d" % n, uniform(5, n, S), S, "%d candidates" % n, n=n))
    # ---- small -> full class by candidate count (1024 / 1025), the largest list (2048)
    L.append(_case("count_1024", uniform(5, 1024, 1100), 1100, "small class, its last candidate count", n=1024, pairs_max=SMALL_PAIRS, sensitive=True))
    L.append(_case("count_1025", uniform(5, 1025, 1100), 1100, "full class by candidate count", n=1025, pairs_max=SMALL_PAIRS, sensitive=True))
    L.append(_case("count_2048_pairs_10k", uniform(5, 2048, 700), 700, "2048 candidates, set tables in global memory", n=2048, pairs_min=LDS_PAIRS + 1,
                   pairs_max=MAX_PAIRS, sensitive=True))
    L.append(_case("count_2048_pairs_28k", uniform(5, 2048, 420), 420, "2048 candidates, the set grows to 131072 entries", n=2048, pairs_min=20000,
                   pairs_max=MAX_PAIRS, sensitive=True))
    L.append(_case("pairs_3422_of_1024", uniform(5, 1024, 600), 600, "1024 candidates left to the full class by pair count; pairs in global memory, set in LDS",
                   n=1024, pairs_min=NPL + 1, pairs_max=LDS_PAIRS, sensitive=True))
    # ---- pair-count switches, one case on each side
    for tgt, n, why in ((SMALL_PAIRS, 128, "small class, its last pair count"), (SMALL_PAIRS + 1, 128, "full class by pair count"),
                        (NPL, 212, "full class, pairs in LDS: the last count"), (NPL + 1, 212, "full class, pairs in global memory"),
                        (LDS_PAIRS, 258, "set tables in LDS: the last count"), (LDS_PAIRS + 1, 258, "set tables in global memory (bigtab, fenced inserts)")):
        L.append(_case("pairs_%d" % tgt, uniform_with_pairs(tgt, n, S, tgt), S, why, n=n, pairs=tgt, sensitive=True))
    # ---- the sequential prune's second form
    L.append(_case("dense_cluster", cluster(2, 150, 6, 60, layer=None), S, "more overlapping pairs than the LDS list holds (ncl > NCL)", n=150,
                   pairs_min=LDS_PAIRS + 1, pairs_max=MAX_PAIRS, overlaps_min=NCL + 1))
    L.append(_case("dense_field", uniform(0, 680, S), S, "ncl > NCL on an order-sensitive list that fits the small engine", n=680,
                   pairs_min=LDS_PAIRS + 1, pairs_max=MAX_PAIRS, overlaps_min=NCL + 1, sensitive=True))
    # ---- introselect's fallback at the root
    L.append(_case("adversary_100", adversary(1, 100), S, "heap select in bp_nth_element (root built by one lane)", n=100, fallback=True))
    L.append(_case("adversary_101", adversary(1, 101), S, "heap select in rb_nth_element_wave (root built by the wavefront)", n=101, fallback=True))
    L.append(_case("adversary_530", adversary(1, 530), 530, "heap select in rb_nth_element_wave, a real frame's size", n=530, fallback=True))
    L.append(_case("adversary_2048", adversary(1, 2048, layer=1), 2048, "heap select in rb_nth_element_wave, the largest root", n=2048, fallback=True,
                   pairs_max=MAX_PAIRS))
    # ---- slid splits
    for a, b in ((12, 8), (20, 14), (60, 30), (100, 60)):
        L.append(_case("slid_min_%d_%d" % (a, b), at_extreme(a + b, a, b, S), S, "at least half of the root at its minimum", n=a + b, slid=True))
    L.append(_case("slid_min_300_100", at_extreme(400, 300, 100, 1000), 1000, "300 of 400 on one row: the old rule peeled 300 levels", n=400, slid=True))
    # (exactly half at the minimum: the median is the first point ABOVE it - the last layout that does not slide; one more does)
    L.append(_case("half_20_20", at_extreme(40, 20, 20, S), S, "exactly half of the root at its minimum: no slide", n=40, slid=False))
    L.append(_case("half_plus_one_21_19", at_extreme(40, 21, 19, S), S, "half + 1 at the minimum: the first layout that slides", n=40, slid=True))
    L.append(_case("half_101_101", at_extreme(202, 101, 101, S), S, "exactly half at the minimum, built by the wavefront: no slide", n=202, slid=False))
    L.append(_case("half_plus_one_102_100", at_extreme(202, 102, 100, S), S, "half + 1 at the minimum, built by the wavefront", n=202, slid=True))
    L.append(_case("at_max_30_10", at_extreme(41, 30, 10, S, at_max=True), S, "more than half of the root at its maximum (no slide)", n=40, slid=False))
    L.append(_case("at_max_120_60", at_extreme(180, 120, 60, S, at_max=True), S, "more than half at the maximum, built by the wavefront", n=180, slid=False))
    L.append(_case("three_rows", three_rows(3), 901, "keys 0 x 3, 500 x 12, 900 x 5: the 17-point child slides", n=20, slid=True))
    L.append(_case("slid_embedded_60_30", at_extreme(91, 60, 30, 200, embed=1000), 1300, "the slid node inside a 1000-point set", n=1090, slid=True))
    L.append(_case("slid_embedded_200_120", at_extreme(321, 200, 120, 200, embed=1000), 1300, "a wave-built slid node inside a 1000-point set", n=1320, slid=True))
    L.append(_case("slid_flip_20_20", slid_flip(7), 541, "the slid bound decides maxd < ub in float64 (20^2 + 20^2 = 8 sigma^2)", n=160, slid=True, flip=True))
    # ---- ties
    L.append(_case("ties_four_responses", ties_values(4, 300, S), S, "responses of four values: rank ties broken by the C order", n=300))
    L.append(_case("ties_both_layers", ties_both_layers(4, 240, S), S, "every pixel in both layers", n=240))
    L.append(_case("one_row", one_line(4, 120, S, 0), S, "all candidates on one row", n=120))
    L.append(_case("one_column", one_line(5, 120, S, 1), S, "all candidates on one column", n=120))
    L.append(_case("one_pixel_pair", _finish(np.random.default_rng(0), [7, 7], [9, 9], [1, 2]), S, "one pixel in both layers", n=2, pairs=1))
    # ---- overflow: the documented flag, nothing else
    L.append(_case("overflow_pairs", uniform(5, 2048, 300), 300, "more than 32767 pairs", n=2048, pairs_min=MAX_PAIRS + 1, flags=F_PAIR, tasks_max=MAX_TASKS))
    L.append(_case("overflow_pairs_small", uniform(6, 1200, S), S, "more than 32767 pairs within the small engine's image", n=1200, pairs_min=MAX_PAIRS + 1,
                   flags=F_PAIR, tasks_max=MAX_TASKS))
    L.append(_case("overflow_tasks", cluster(3, 2048, 28, 64, layer=None), S, "more than 8192 leaf x leaf blocks", n=2048, flags=F_TREE, tasks_min=MAX_TASKS + 1))
    L.append(_case("overflow_cand", uniform(8, 2048, 2048), 2048, "cand_n = 5000 with 2048 rows", cand_n=5000, n=2048, pairs_max=LDS_PAIRS, flags=F_CAND))
    assert len({c.name for c in L}) == len(L)
    _cases = L
    return L


def by_name(name):
    return next(c for c in cases() if c.name == name)


def flags_of(case):
    return case.want.get("flags", 0)


def dump(path):
    """every case's blobs for the stand-alone sanitizer program (profiles/asan_blob_book.sh): int32 case count, then per case int32 n and
    n x 3 float64 [row, col, sigma] in peak_local_max order"""
    with open(path, "wb") as f:
        f.write(np.int32(len(cases())).tobytes())
        for c in cases():
            b = blobs_of(c.rc, c.val)
            f.write(np.int32(len(b)).tobytes())
            f.write(np.ascontiguousarray(b, np.float64).tobytes())


if __name__ == "__main__":
    import sys
    dump(sys.argv[1])
