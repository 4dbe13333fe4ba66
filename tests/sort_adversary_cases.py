"""Inputs that drive the device argsort (csrc/npsort_wave.h rb_aquicksort_wave, csrc/blobprune.h bp_aquicksort_range) into its
heapsort fallback, for tests/test_sort_adversary_cpu.py (no GPU) and tests/test_gpu_sort_adversary.py (on the GPU).

argsort_model is a sequential Python restatement of NumPy 1.22.3's npy_aquicksort in the shape the device gives it: segments of more
than QS_WAVE_MIN + 1 elements are partitioned "at wave level" (median of three, pivot to pr - 1, the Hoare loop, the larger part to
the stack, a child's depth budget its parent's minus one, the budget 2 * floor(log2 n) checked on what comes off the stack), the
others are collected and sorted afterwards by the sequential loop ("one lane each"), which has npy_aquicksort's own insertion-sort
threshold.  Both thresholds are read off the headers.  npy_aheapsort (1-based sift-down, build phase, extraction) is the fallback
at both levels.  The model compares ITEMS through a callback lt(i, j), so McIlroy's gas adversary ("A Killer Adversary for
Quicksort", 1999) can be run against it (killer), and it returns a trace: which segments were partitioned at wave level and which
were heapsorted, at which level.  Everything is generated and deterministic; nothing is read from disk but the two headers."""
import functools
import os
import re
import warnings

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "radarslampy_amd", "csrc")


def _read_threshold(header, pattern):
    with open(os.path.join(CSRC, header)) as f:
        found = re.findall(pattern, f.read())
    assert len(found) == 1, (header, pattern, found)
    return int(found[0])


QS_WAVE_MIN = _read_threshold("npsort_wave.h", r"#define\s+QS_WAVE_MIN\s+(\d+)")          # pr - pl above it: all lanes partition
SMALL_QUICKSORT = _read_threshold("blobprune.h", r"while \(pr - pl > (\d+)\)")              # pr - pl up to it: insertion sort
WORK_ENTRIES = 128                      # npsort_wave.h: pending + collected segments; a full list sends a segment to one lane
MAX_KEYS = 2047                         # candidates of a 4096-column row (peaks_cond.hip PKC_MAXP is 2048, two are never adjacent)
DISTANCES = [1.7, 3, 5, 10.5, 20, 4096]
VISIBLE_DISTANCES = [3, 5, 10.5]

WAVE, LANE = "wave", "lane"


class Trace:
    """heapsorts: [(pl, pr, level)], level WAVE (a segment the wavefront would have partitioned, off the stack with its budget used
    up) or LANE (inside a collected segment); wave_partitions: [(pl, pr)]; collected: [(pl, pr, budget, popped)], the segments
    handed to one lane each, as the device packs them into small[3k .. 3k + 2]; overflow: segments longer than QS_WAVE_MIN + 1
    that went to one lane because the work list was full; most_entries: the fullest the work list has been"""

    def __init__(self):
        self.heapsorts, self.wave_partitions, self.collected, self.overflow, self.most_entries = [], [], [], 0, 0

    def at(self, level):
        return [(pl, pr) for pl, pr, lv in self.heapsorts if lv == level]


def _aheapsort(ts, off, n, lt):
    """npy_aheapsort on ts[off : off + n]"""
    a = lambda i: ts[off + i - 1]                                                   # noqa: E731  (1-based)

    def put(i, x):
        ts[off + i - 1] = x

    def sift(tmp, i, n):
        j = 2 * i
        while j <= n:
            if j < n and lt(a(j), a(j + 1)):
                j += 1
            if lt(tmp, a(j)):
                put(i, a(j))
                i = j
                j += j
            else:
                break
        put(i, tmp)
    for l in range(n >> 1, 0, -1):
        sift(a(l), l, n)
    while n > 1:
        tmp = a(n)
        put(n, a(1))
        n -= 1
        sift(tmp, 1, n)


def _stable(ts, off, n, lt):
    """what the fallback must NOT be: the segment, as it stands, sorted stably"""
    ts[off:off + n] = sorted(ts[off:off + n], key=functools.cmp_to_key(lambda x, y: -1 if lt(x, y) else (1 if lt(y, x) else 0)))


def _partition(ts, pl, pr, lt):
    """npy_aquicksort's partition of ts[pl .. pr] -> the pivot's final position"""
    pm = pl + ((pr - pl) >> 1)
    if lt(ts[pm], ts[pl]):
        ts[pm], ts[pl] = ts[pl], ts[pm]
    if lt(ts[pr], ts[pm]):
        ts[pr], ts[pm] = ts[pm], ts[pr]
    if lt(ts[pm], ts[pl]):
        ts[pm], ts[pl] = ts[pl], ts[pm]
    vp = ts[pm]
    pi, pj = pl, pr - 1
    ts[pm], ts[pj] = ts[pj], ts[pm]
    while True:
        pi += 1
        while lt(ts[pi], vp):
            pi += 1
        pj -= 1
        while lt(vp, ts[pj]):
            pj -= 1
        if pi >= pj:
            break
        ts[pi], ts[pj] = ts[pj], ts[pi]
    ts[pi], ts[pr - 1] = ts[pr - 1], ts[pi]
    return pi


def _range(ts, pl, pr, cd, popped, lt, trace, fallback):
    """bp_aquicksort_range: npy_aquicksort's loop on one collected segment"""
    stack = []
    while True:
        if popped and cd < 0:
            trace.heapsorts.append((pl, pr, LANE))
            fallback[LANE](ts, pl, pr - pl + 1, lt)
        else:
            while pr - pl > SMALL_QUICKSORT:
                pi = _partition(ts, pl, pr, lt)
                cd -= 1
                if pi - pl < pr - pi:
                    stack.append((pi + 1, pr, cd))
                    pr = pi - 1
                else:
                    stack.append((pl, pi - 1, cd))
                    pl = pi + 1
            for i in range(pl + 1, pr + 1):
                vi, j = ts[i], i
                while j > pl and lt(vi, ts[j - 1]):
                    ts[j] = ts[j - 1]
                    j -= 1
                ts[j] = vi
        if not stack:
            return
        pl, pr, cd = stack.pop()
        popped = True


def argsort_model(n, lt, stable_at=()):
    """-> (permutation, Trace).  lt(i, j): is item i's key below item j's.  stable_at: the levels (WAVE, LANE) whose heapsort is
    replaced by a stable sort of the segment - the wrong fallback the tests must be able to tell from the right one"""
    fallback = {lv: (_stable if lv in stable_at else _aheapsort) for lv in (WAVE, LANE)}
    ts, trace = list(range(n)), Trace()
    if n < 2:
        return ts, trace
    work, small = [], []
    pl, pr, cd, popped = 0, n - 1, 2 * (n.bit_length() - 1), True
    while True:
        full = len(small) + len(work) + 2 >= WORK_ENTRIES
        if pr - pl <= QS_WAVE_MIN or full:
            trace.overflow += pr - pl > QS_WAVE_MIN
            small.append((pl, pr, cd, popped))
        elif popped and cd < 0:
            trace.heapsorts.append((pl, pr, WAVE))
            fallback[WAVE](ts, pl, pr - pl + 1, lt)
        else:
            trace.wave_partitions.append((pl, pr))
            pi = _partition(ts, pl, pr, lt)
            cd -= 1
            if pi - pl < pr - pi:
                work.append((pi + 1, pr, cd))
                pr = pi - 1
            else:
                work.append((pl, pi - 1, cd))
                pl = pi + 1
            popped = False
            trace.most_entries = max(trace.most_entries, len(small) + len(work))
            continue
        trace.most_entries = max(trace.most_entries, len(small) + len(work))
        if not work:
            break
        pl, pr, cd = work.pop()
        popped = True
    trace.collected = list(small)
    for pl, pr, cd, popped in small:
        _range(ts, pl, pr, cd, popped, lt, trace, fallback)
    return ts, trace


def argsort_keys(keys, stable_at=()):
    """the model on a key sequence -> (int64 permutation, Trace)"""
    k = [float(x) for x in keys]
    ts, trace = argsort_model(len(k), lambda i, j: k[i] < k[j], stable_at)
    return np.array(ts, np.int64), trace


@functools.lru_cache(maxsize=None)
def _killer(n):
    gas = n
    val, state = [gas] * n, [0, 0]                                                  # state: solid values handed out, pivot candidate

    def lt(x, y):
        if val[x] == gas and val[y] == gas:
            val[x if x == state[1] else y] = state[0]
            state[0] += 1
        if val[x] == gas:
            state[1] = x
        elif val[y] == gas:
            state[1] = y
        return val[x] < val[y]
    argsort_model(n, lt)
    return tuple(val)


def killer(n):
    """McIlroy's adversary against argsort_model: every key starts as "gas" (n, above every solid value); comparing two gas keys
    freezes the current pivot candidate to the next integer -> the n keys (int64) it ends with"""
    return np.array(_killer(n), np.int64)


def organ_pipe(m):
    """0 .. m // 2 .. 0 (m odd)"""
    return np.concatenate([np.arange(m // 2 + 1), np.arange(m // 2)[::-1]]).astype(np.int64)


ADVERSARIAL, REACHES, CONTROL = "adversarial", "reaches", "control"


class KeyRow:
    """keys: the int64 key sequence; f32: the float32 row (key + 1) / 2048 at the odd columns, 0 at the even ones, 2 M + 1 wide (the
    scaling is exact, so the row's heights tie exactly where the keys do); u8: the same with the codes key + 1, where they fit.
    kind: ADVERSARIAL - reaches the fallback, and the order of its equal heights shows in the peak list; REACHES - reaches the
    fallback, but the peak list cannot tell NumPy 1.22's tie order from this NumPy's (why: key_rows); CONTROL - must not reach
    it.  The CPU test asserts each of these against the trace and the truth."""

    def __init__(self, name, keys, kind, u8=False):
        keys = np.asarray(keys, np.int64)
        assert 1 <= len(keys) <= MAX_KEYS and keys.min() >= 0 and keys.max() < 2048
        self.name, self.keys, self.kind = name, keys, kind
        self.f32 = np.zeros(2 * len(keys) + 1, np.float32)
        self.f32[1::2] = (keys + 1).astype(np.float32) / np.float32(2048)
        self.u8 = None
        if u8:
            assert keys.max() < 255
            self.u8 = np.zeros(2 * len(keys) + 1, np.uint8)
            self.u8[1::2] = keys + 1


@functools.lru_cache(maxsize=None)
def key_rows():
    """-> {name: KeyRow}.  killer(M) // 2: the adversary's keys with ties in pairs (without the halving no two keys are equal and
    no order could be wrong; // 8 no longer reaches the fallback).  M = 64 and 65 stay on one lane, 66 is the smallest row the
    wavefront partitions at all, 80 is partitioned eight times and then heapsorts inside a collected segment, 130 and up heapsort
    one long segment at wave level.  The organ pipes reach many segments at both levels, and are the rows whose collected segments
    carry a used-up budget (a negative one, packed next to the popped bit).
    REACHES rows: organ2047's equal keys are mirror images about the middle, thousands of columns apart except next to the summit,
    which suppresses them first, so no distance condition can see their order; killer64/65/66_half come out the same under NumPy
    1.22's order and this NumPy's at the distances the CPU test looks at, but 65 and 66 differ from a stably sorted fallback."""
    rng = np.random.default_rng(65)
    rows = [KeyRow(f"killer{m}_half", killer(m) // 2, REACHES if m < 80 else ADVERSARIAL)
            for m in (64, 65, 66, 80, 130, 300, 530, 1024, 2047)]
    pipe = organ_pipe(2047)
    rows += [KeyRow("organ2047", pipe, REACHES),
             KeyRow("organ2047_u8", pipe * 254 // 1023, ADVERSARIAL, u8=True),
             KeyRow("organ2047_twice", np.repeat(organ_pipe(1023), 2)[:2047], ADVERSARIAL),
             KeyRow("organ1011_u8", organ_pipe(1011) * 254 // 505, ADVERSARIAL, u8=True),  # fits an Oxford record's 2025 columns
             KeyRow("sorted2047", np.arange(2047), CONTROL),
             KeyRow("reversed2047", np.arange(2047)[::-1], CONTROL),
             KeyRow("equal2047_u8", np.full(2047, 7), CONTROL, u8=True),
             KeyRow("two_valued2047_u8", rng.integers(0, 2, 2047) * 3, CONTROL, u8=True),
             KeyRow("sorted1011_u8", np.arange(1011) // 4, CONTROL, u8=True),
             KeyRow("killer2047_eighth", killer(2047) // 8, CONTROL)]
    return {r.name: r for r in rows}


def _stack(rows, kind, cols=None):
    cols = cols or max(len(getattr(r, kind)) for r in rows)
    img = np.zeros((len(rows), cols), np.float32 if kind == "f32" else np.uint8)
    for i, r in enumerate(rows):
        a = getattr(r, kind)
        img[i, :len(a)] = a
    return img


@functools.lru_cache(maxsize=None)
def images():
    """-> {name: (kind, [row names], image)}: adversarial rows and controls interleaved, shorter rows padded with zeros on the
    right; *_first begins with an adversarial row and ends with a control, *_last is the same image upside down"""
    R = key_rows()
    f32 = ["killer2047_half", "sorted2047", "organ2047", "equal2047_u8", "organ2047_twice", "killer2047_eighth", "killer1024_half",
           "reversed2047", "organ2047_u8", "two_valued2047_u8"]
    small = ["killer65_half", "sorted1011_u8", "killer64_half", "killer66_half", "killer80_half", "killer130_half", "killer300_half",
             "killer530_half"]
    u8 = ["organ2047_u8", "equal2047_u8", "organ1011_u8", "two_valued2047_u8"]
    oxford = ["organ1011_u8", "sorted1011_u8"]
    out = {}
    for name, kind, names, cols in [("f32_first", "f32", f32, 4096), ("f32_last", "f32", f32[::-1], 4095),
                                    ("f32_small", "f32", small, None),
                                    ("u8_first", "u8", u8, 4095), ("u8_last", "u8", u8[::-1], 4096),
                                    ("u8_oxford", "u8", oxford, 2025)]:
        out[name] = (kind, names, _stack([R[n] for n in names], kind, cols))
    return out


def truth_with_order(img, distance, argsort):
    """peaks_cond_cases.truth(img, distance, None) with np.argsort of a 1-D array rebound to argsort(heights) -> permutation"""
    import peaks_cond_cases as pc
    from scipy.signal import find_peaks
    orig = np.argsort

    def patched(a, axis=-1, kind=None, order=None, **kw):
        if kind is None and order is None and not kw and axis in (-1, 0) and np.ndim(a) == 1:
            return argsort(np.asarray(a))
        return orig(a, axis=axis, kind=kind, order=order, **kw)
    np.argsort = patched
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return pc.threshold_rows(img, lambda row: find_peaks(row, distance=distance)[0])
    finally:
        np.argsort = orig
