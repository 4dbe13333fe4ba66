"""Inputs of the back-end edge tests (tests/test_gpu_backend_edges.py on the GPU, tests/test_backend_edges_cpu.py without one,
tests/golden/make_backend_edges.py for the reference's answers): SSC, Kabsch, undistort and the consistency graph away from the
one parameter point the golden fixtures sit at.  Everything is seeded; the fixture file stores a SHA-256 of every input it
answers and the tests recompute it from here.

The module also holds the references the GPU results are judged by (exact rational Kabsch, mpmath undistort, the integer search
for threshold-equality pairs) and the comparison functions themselves, so that the CPU test can hand each comparison a
deliberately wrong result and see it refused."""
import ctypes as C
import hashlib
import math
import os
from fractions import Fraction

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -53                                  # unit roundoff of float64


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()


# ====================================================================================== SSC
SSC_SIZES = [(2024, 2024), (1012, 2024), (2024, 1012), (300, 1000), (64, 64), (4096, 4096)]       # (rows, cols)
SSC_NUM_RET = [2, 10, 50, 200, 500]
SSC_TOL = [0.0, 0.05, 0.1, 0.5]
SSC_DISTS = ["uniform", "clustered", "lattice", "identical", "integer", "edge"]
SSC_BITMAP_BITS = {"stage": 65536 * 8, "batch": 16384 * 8}      # csrc/ssc_body.inc SSC_BITMAP_BYTES / SSC_BATCH_BITMAP_BYTES


def ssc_b_values(num_ret):
    return [1, 2, 63, 64, 65, 127, 128, 129, num_ret - 1, num_ret, num_ret + 1, 2 * num_ret + 1, 1000, 5000]


def ssc_points(dist, B, rows, cols, seed):
    """(B, 3) float64 rows [row, col, sigma] inside [0, rows] x [0, cols]"""
    rng = np.random.default_rng(7000 + seed)
    if dist == "uniform":
        rc = rng.uniform(0, 1, size=(B, 2)) * (rows, cols)
    elif dist == "clustered":
        c = rng.uniform(0.1, 0.9, size=(7, 2)) * (rows, cols)
        rc = np.clip(c[rng.integers(0, 7, B)] + rng.normal(0, 0.02 * max(rows, cols), size=(B, 2)), 0, (rows, cols))
    elif dist == "lattice":
        # a square lattice over the image, row by row: while the square is narrower than the pitch every point survives, then a
        # quarter of them, a ninth ... - the count jumps over [k_min, k_max] unless it starts inside
        g = max(1, int(math.ceil(math.sqrt(B))))
        ii, jj = np.divmod(np.arange(B), g)
        rc = np.column_stack(((ii + 0.5) * rows / g, (jj + 0.5) * cols / g))
    elif dist == "identical":
        rc = np.tile(rng.uniform(0, 1, size=(1, 2)) * (rows, cols), (B, 1))
    elif dist == "integer":
        rc = np.column_stack((rng.integers(0, rows + 1, B), rng.integers(0, cols + 1, B))).astype(np.float64)
    elif dist == "edge":
        rc = np.floor(rng.uniform(0, 1, size=(B, 2)) * (rows, cols))
        k = np.arange(B) % 3
        rc[k == 0, 0] = rows            # the image's last row: cell floor(rows / c), the grid's extra row
        rc[k == 1, 1] = cols
        rc[(np.arange(B) % 7) == 0] = (rows, cols)
    else:
        raise ValueError(dist)
    sig = rng.choice(np.array([0.01, 5.005, 10.0]), size=B)
    return np.ascontiguousarray(np.column_stack((rc, sig)))


def ssc_trace(kp, num_ret, tol, cols, rows, grid=None):
    """ANMS.ssc's binary search, with the covered cells of one pass kept as a set -> (widths visited, indices selected, how it
    ended: "found", "repeat", "empty-range" or "zero-width").  The reference divides by the zero width; the device and the oracle
    return the previous pass there.

    grid="device": the covered cells kept the way the kernel's bitmap keeps them - cell indices clamped into the
    (floor(rows / c) + 1) x (floor(cols / c) + 1) grid, one bit at r * ncols + q.  grid="exchanged": the same with the bit at
    r * nrows + q, the mistake of exchanging the grid's two sizes in the cell index (cells alias on a non-square image) - the
    wrong result the CPU test hands to the comparison."""
    exp1 = rows + cols + 2 * num_ret
    exp2 = 4 * cols + 4 * num_ret + 4 * rows * num_ret + rows * rows + cols * cols - 2 * rows * cols + 4 * rows * cols * num_ret
    sol1, sol2 = -round(float(exp1 + math.sqrt(exp2)) / (num_ret - 1)), -round(float(exp1 - math.sqrt(exp2)) / (num_ret - 1))
    high, low, prev_width = max(sol1, sol2), math.floor(math.sqrt(len(kp) / num_ret)), -1
    k_min, k_max = round(num_ret - num_ret * tol), round(num_ret + num_ret * tol)
    widths, result = [], []
    while True:
        width = low + (high - low) / 2
        if width == prev_width or low > high or width == 0:
            return widths, result, "repeat" if width == prev_width else "empty-range" if low > high else "zero-width"
        widths.append(width)
        c, covered, result = width / 2, set(), []
        w = int(math.floor(width / c))
        cells = np.floor(kp[:, :2] / c).astype(np.int64)
        if grid is None:
            for i, (r, q) in enumerate(cells.tolist()):
                if (r, q) not in covered:
                    result.append(i)
                    covered.update((rr, qq) for rr in range(r - w, r + w + 1) for qq in range(q - w, q + w + 1))
        else:
            nrows, ncols = int(math.floor(rows / c)) + 1, int(math.floor(cols / c)) + 1
            stride = ncols if grid == "device" else nrows
            for i, (r, q) in enumerate(cells.tolist()):
                r, q = min(max(r, 0), nrows - 1), min(max(q, 0), ncols - 1)
                if r * stride + q not in covered:
                    result.append(i)
                    covered.update(rr * stride + qq for rr in range(max(r - w, 0), min(r + w, nrows - 1) + 1)
                                   for qq in range(max(q - w, 0), min(q + w, ncols - 1) + 1))
        if k_min <= len(result) <= k_max:
            return widths, result, "found"
        if len(result) < k_min:
            high = width - 1
        else:
            low = width + 1
        prev_width = width


def ssc_cells(width, cols, rows):
    c = width / 2
    return (math.floor(cols / c) + 1) * (math.floor(rows / c) + 1)


def ssc_crosses(widths, cols, rows, which):
    """does one call use both forms (cell bitmap where the grid fits it, pairwise where it does not) of the kernel `which`?"""
    grid = [ssc_cells(w, cols, rows) <= SSC_BITMAP_BITS[which] for w in widths]
    return any(grid) and not all(grid)


_ssc_cases = None


def ssc_cases():
    """[(name, kp, num_ret, tol, cols, rows)].  One parameter tuple (size, num_ret, tol) carries several (B, distribution) pairs, so
    that the batched kernel gets launches of mixed problem sizes.  The two small images carry more of them: they are the ones the
    reference can be run on (make_backend_edges.py)."""
    global _ssc_cases
    if _ssc_cases is not None:
        return _ssc_cases
    out, seed, t = [], 0, 0
    for si, (rows, cols) in enumerate(SSC_SIZES):
        for ni, num_ret in enumerate(SSC_NUM_RET):
            tol = SSC_TOL[(si + ni) % 4]
            bs = ssc_b_values(num_ret)
            small = max(rows, cols) <= 1100
            nvar = 9 if small else 4
            for v in range(nvar):
                B = bs[(3 * t + 5 * v) % len(bs)]
                if small and v >= 3 and B < num_ret:            # (most of the small-image cases stay reference-pinned)
                    B = bs[8 + (t + v) % 6]
                    B = max(B, num_ret)
                dist = SSC_DISTS[(t + v) % 6]
                B = max(B, 1)
                out.append((f"ssc{seed:03d}-{rows}x{cols}-k{num_ret}-tol{tol}-B{B}-{dist}", ssc_points(dist, B, rows, cols, seed), num_ret, tol, cols, rows))
                seed += 1
            t += 1
    # the grid / pairwise switch: few keypoints for the number asked for drive the width down to where the grid outgrows the bitmap
    for rows, cols in [(2024, 2024), (1012, 2024), (2024, 1012), (4096, 4096)]:
        for num_ret, tol, B, dist in [(200, 0.1, 201, "uniform"), (200, 0.05, 401, "integer"), (50, 0.0, 51, "edge"), (500, 0.1, 1000, "clustered"),
                                      (50, 0.5, 49, "uniform"), (500, 0.0, 501, "lattice")]:
            out.append((f"ssc{seed:03d}-switch-{rows}x{cols}-k{num_ret}-tol{tol}-B{B}-{dist}", ssc_points(dist, B, rows, cols, seed), num_ret, tol, cols, rows))
            seed += 1
    assert len({c[0] for c in out}) == len(out) >= 150
    _ssc_cases = out
    return out


def ssc_reference_pinned(case):
    """the reference can run this case: every width >= 1 (B >= num_ret) and a grid below 5 M cells (sides <= 1100)"""
    _, kp, num_ret, _, cols, rows = case
    return max(rows, cols) <= 1100 and len(kp) >= num_ret


def oracle_ssc_indices(kp, num_ret, tol, cols, rows):
    import oracle
    kp = np.ascontiguousarray(kp, np.float64)
    sel = np.empty(max(len(kp), 1), np.int32)
    n = oracle.lib().oracle_ssc(kp.ctypes.data_as(C.POINTER(C.c_double)), len(kp), int(num_ret), C.c_double(tol), int(cols), int(rows),
                                sel.ctypes.data_as(C.POINTER(C.c_int32)))
    return sel[:n].copy()


def ssc_batches(cases, extra_rows=5):
    """the cases grouped by (num_ret, tol, cols, rows) -> [(params, names, kp (P, kp_cap, 3), count (P,))]; kp_cap is `extra_rows`
    more than the largest problem; the rows past a problem's count hold (0, 0, -1), which the kernel must not read (a count
    clamped to kp_cap does read them: the clamp test compares that with the oracle on all kp_cap rows)"""
    groups = {}
    for name, kp, num_ret, tol, cols, rows in cases:
        groups.setdefault((num_ret, tol, cols, rows), []).append((name, kp))
    out = []
    for params, members in groups.items():
        cap = max(len(kp) for _, kp in members) + extra_rows
        arr = np.zeros((len(members), cap, 3))
        arr[:, :, 2] = -1.0
        for p, (_, kp) in enumerate(members):
            arr[p, :len(kp)] = kp
        out.append((params, [n for n, _ in members], arr, np.array([len(kp) for _, kp in members], np.int32)))
    return out


def compare_ssc(got, want):
    """exact: the same indices in the same order"""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and bool(np.array_equal(got, want))


# ====================================================================================== Kabsch
KABSCH_N = [1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1024, 4097, 100000]
KABSCH_ROT = [0.0, math.pi / 2, -math.pi / 2, math.pi - 5e-10, -math.pi + 5e-10, None]      # None: random
KABSCH_FRAME = [(0.0, 1e3), (1e3, 1e3), (1e6, 1e3), (0.0, 1.0), (1e3, 1.0), (1e6, 1.0)]     # (centroid, spread) px


def _kabsch_pair(n, seed, noise, rot, centroid, spread, collinear=False):
    rng = np.random.default_rng(8000 + seed)
    if collinear:
        d = np.array([math.cos(0.7), math.sin(0.7)])
        tgt = centroid + spread * rng.uniform(-1, 1, size=(n, 1)) * d
    else:
        tgt = centroid + spread * rng.uniform(-1, 1, size=(n, 2))
    th = rng.uniform(-math.pi, math.pi) if rot is None else rot
    R = np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
    src = tgt @ R.T + rng.uniform(-30, 30, 2)
    if noise > 0:
        src = src + rng.normal(0, noise, size=src.shape)
    return np.ascontiguousarray(src), np.ascontiguousarray(tgt)


_kabsch = None


def kabsch_cases():
    """-> (cases, degenerate), both [(name, src, tgt)].  Noise starts at N = 63: below that "all but one point" is itself a
    degenerate or exact fit, and the lost-lane condition of the CPU test has nothing to measure."""
    global _kabsch
    if _kabsch is not None:
        return _kabsch
    cases, t = [], 0
    for n in KABSCH_N[1:]:
        for noise in ((0.0,) if n < 63 else (0.0, 1.5)):
            rot, (cen, spread) = KABSCH_ROT[t % 6], KABSCH_FRAME[(t + t // 6) % 6]
            rname = "random" if rot is None else f"{rot:+.3f}"
            cases.append((f"kabsch-n{n}-noise{noise}-rot{rname}-c{cen:g}-s{spread:g}", *_kabsch_pair(n, t, noise, rot, cen, spread)))
            t += 1
    for n, noise in ((65, 0.0), (257, 1.5)):
        cases.append((f"kabsch-collinear-n{n}-noise{noise}", *_kabsch_pair(n, 100 + n, noise, None, 1e3, 1e3, collinear=True)))
    for name, s, g in (cases[6], cases[13]):
        cases.append((name + "-f32", s.astype(np.float32), g.astype(np.float32)))
    g = np.arange(-4, 5, dtype=np.float64)
    sq = np.array([(x, y) for x in g for y in g]) * 8.0 + 100.0            # invariant under a quarter turn about (100, 100): C00 = -C11
    degenerate = [("kabsch-degenerate-n1", np.array([[3.5, -7.25]]), np.array([[1012.0, 40.0]])),
                  ("kabsch-degenerate-coincident-n64", np.tile([[12.5, 7.0]], (64, 1)), np.tile([[-3.0, 2000.0]], (64, 1))),
                  ("kabsch-degenerate-coincident-tgt-n257", _kabsch_pair(257, 300, 0.0, None, 0.0, 1e3)[0], np.tile([[5.0, 5.0]], (257, 1))),
                  ("kabsch-degenerate-mirror-n81", sq, sq * (1.0, -1.0) + (0.0, 900.0))]
    _kabsch = (cases, degenerate)
    return _kabsch


def kabsch_exact(src, tgt):
    """The fit of the float64 inputs in exact arithmetic up to the last step: exact means, exact centred cross-covariance, one atan2
    of its two combinations (each correctly rounded after scaling by the larger), then h from exact means.  N = 100 000 (too many
    for rationals in a test): the same two passes in np.longdouble.
    -> (theta, h (2,), cond) with cond = dict(S=sum of |products|, z=|(C10 - C01, C00 + C11)|, mt=|mt|, coord=max |coordinate|)"""
    s, t = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    n = len(s)
    if n <= 5000:
        S_, T_ = [[Fraction(v) for v in row] for row in s.tolist()], [[Fraction(v) for v in row] for row in t.tolist()]
        ms = [sum(r[k] for r in S_) / n for k in (0, 1)]
        mt = [sum(r[k] for r in T_) / n for k in (0, 1)]
        c = [[Fraction(0)] * 2 for _ in range(2)]
        Sabs = Fraction(0)
        for a, b in zip(S_, T_):
            ax, ay, bx, by = a[0] - ms[0], a[1] - ms[1], b[0] - mt[0], b[1] - mt[1]
            c[0][0] += ax * bx; c[0][1] += ax * by; c[1][0] += ay * bx; c[1][1] += ay * by
            Sabs += abs(ax * bx) + abs(ay * by) + abs(ax * by) + abs(ay * bx)
        y, x = c[1][0] - c[0][1], c[0][0] + c[1][1]
        m = max(abs(y), abs(x))
        th = math.atan2(float(y / m), float(x / m)) if m else 0.0
        cs, sn = Fraction(math.cos(th)), Fraction(math.sin(th))
        h = np.array([float(ms[0] - (cs * mt[0] - sn * mt[1])), float(ms[1] - (sn * mt[0] + cs * mt[1]))])
        z = math.hypot(float(y), float(x))
        return th, h, dict(S=float(Sabs), z=z, mt=math.hypot(float(mt[0]), float(mt[1])), coord=float(max(np.abs(s).max(), np.abs(t).max())))
    L = np.longdouble
    sl, tl = s.astype(L), t.astype(L)
    ms, mt = sl.sum(axis=0) / L(n), tl.sum(axis=0) / L(n)
    a, b = sl - ms, tl - mt
    c00, c01, c10, c11 = (a[:, 0] * b[:, 0]).sum(), (a[:, 0] * b[:, 1]).sum(), (a[:, 1] * b[:, 0]).sum(), (a[:, 1] * b[:, 1]).sum()
    Sabs = (np.abs(a[:, 0] * b[:, 0]) + np.abs(a[:, 1] * b[:, 1]) + np.abs(a[:, 0] * b[:, 1]) + np.abs(a[:, 1] * b[:, 0])).sum()
    y, x = c10 - c01, c00 + c11
    m = max(abs(y), abs(x))
    th = math.atan2(float(y / m), float(x / m))
    cs, sn = L(math.cos(th)), L(math.sin(th))
    h = np.array([float(ms[0] - (cs * mt[0] - sn * mt[1])), float(ms[1] - (sn * mt[0] + cs * mt[1]))])
    return th, h, dict(S=float(Sabs), z=float(np.hypot(y, x)), mt=float(np.hypot(mt[0], mt[1])), coord=float(max(np.abs(s).max(), np.abs(t).max())))


def kabsch_sequential(src, tgt):
    """the closed form with every sum a plain left-to-right float64 loop: the second CPU order beside oracle.kabsch_closed_form
    (numpy's pairwise sums)"""
    s, t = np.asarray(src, np.float64).tolist(), np.asarray(tgt, np.float64).tolist()
    n = len(s)
    sx = sy = tx = ty = 0.0
    for (a0, a1), (b0, b1) in zip(s, t):
        sx += a0; sy += a1; tx += b0; ty += b1
    msx, msy, mtx, mty = sx / n, sy / n, tx / n, ty / n
    c00 = c01 = c10 = c11 = 0.0
    for (a0, a1), (b0, b1) in zip(s, t):
        ax, ay, bx, by = a0 - msx, a1 - msy, b0 - mtx, b1 - mty
        c00 += ax * bx; c01 += ax * by; c10 += ay * bx; c11 += ay * by
    th = math.atan2(c10 - c01, c00 + c11)
    c, sn = math.cos(th), math.sin(th)
    return np.array([[c, -sn], [sn, c]]), np.array([[msx - (c * mtx - sn * mty)], [msy - (sn * mtx + c * mty)]])


_kabsch_exact = {}


def kabsch_exact_of(case):
    name, s, t = case
    if name not in _kabsch_exact:
        _kabsch_exact[name] = kabsch_exact(s, t)
    return _kabsch_exact[name]


# The largest deviation from the exact reference, in condition units (angle, h), that the two CPU float64 orders show over the
# non-degenerate cases: oracle.kabsch_closed_form (numpy's sums) and kabsch_sequential.  Measured by
# tests/test_backend_edges_cpu.py, which fails when what it measures leaves [1 / 2, 5 / 4] of these records (the figures depend
# on numpy's summation blocks and on libm: another build may move them by a few percent).  The device sums in a third
# order (256 lanes, then wavefronts, then the block): its bar is TOLERANCE_FACTOR times these.
KABSCH_CPU_WORST = (2.46, 68.3)
TOLERANCE_FACTOR = 10.0
KABSCH_K = (TOLERANCE_FACTOR * KABSCH_CPU_WORST[0], TOLERANCE_FACTOR * KABSCH_CPU_WORST[1])
# ... and of the oracle's libm evaluation of undistort from the 50-digit values, in units of the scaled tolerance (xy, dT)
UNDISTORT_CPU_WORST = (3.14, 1.57)
UNDISTORT_K = (TOLERANCE_FACTOR * UNDISTORT_CPU_WORST[0], TOLERANCE_FACTOR * UNDISTORT_CPU_WORST[1])


def wrap_angle(d):
    return (d + math.pi) % (2 * math.pi) - math.pi


def kabsch_units(cond):
    """one condition unit of the angle (rad) and of h (px): what a relative error of u in every product moves them by"""
    ang = U * cond["S"] / cond["z"]
    return ang, ang * cond["mt"] + U * cond["coord"]


def kabsch_deviation(R, h, exact):
    """(angle, h) deviation of a result from the exact reference, in condition units"""
    th, hx, cond = exact
    ua, uh = kabsch_units(cond)
    R, h = np.asarray(R, np.float64), np.asarray(h, np.float64).reshape(2)
    return abs(wrap_angle(math.atan2(R[1, 0], R[0, 0]) - th)) / ua, float(np.abs(h - hx).max()) / uh


def compare_kabsch(R, h, exact, k_ang, k_h):
    da, dh = kabsch_deviation(R, h, exact)
    return bool(np.isfinite(R).all() and np.isfinite(h).all() and da <= k_ang and dh <= k_h and abs(np.linalg.det(R) - 1) < 1e-12)


# ====================================================================================== undistort
UNDISTORT_N = [1, 255, 256, 257, 1000, 65537]
UNDISTORT_OMEGA = [0.0, 0.3, 50.0, 1e6]
UNDISTORT_PERIOD = [0.25, 1.0, 0.01]
_AXIS_POINTS = [(x, y) for r in (1e-3, 1.0, 87.5, 1e4) for x, y in ((r, 0.0), (r, -0.0), (-r, 0.0), (-r, -0.0), (0.0, r), (-0.0, r), (0.0, -r), (-0.0, -r))] \
    + [(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0)]

_undistort = None


def undistort_cases():
    """[(name, v3, pts, period)].  Every set starts with the 36 points on the axes and at the origin (both signs of every zero) as far as
    its N allows; the rest are log-uniform radii in [1e-3, 1e4] at uniform angles.  N = 65 537 repeats 1021 points: the size is there
    for the index arithmetic, and the 50-digit reference is evaluated once per distinct point."""
    global _undistort
    if _undistort is not None:
        return _undistort
    out = []
    t = 0
    for n in UNDISTORT_N:
        for rep in range(2 if n != 65537 else 1):
            rng = np.random.default_rng(9000 + t)
            omega, period = UNDISTORT_OMEGA[t % 4], UNDISTORT_PERIOD[t % 3]
            m = min(n, 1021)
            rad = 10.0 ** rng.uniform(-3, 4, m)
            ang = rng.uniform(-math.pi, math.pi, m)
            pts = np.column_stack((rad * np.cos(ang), rad * np.sin(ang)))
            k = min(m, len(_AXIS_POINTS))
            pts[:k] = np.roll(np.array(_AXIS_POINTS), -t, axis=0)[:k]
            pts = np.ascontiguousarray(np.resize(pts, (n, 2)) if n > m else pts)
            v3 = np.array([rng.uniform(-20, 20), rng.uniform(-3, 3), omega])
            out.append((f"undistort-n{n}-omega{omega:g}-period{period:g}", v3, pts, period))
            t += 1
    for omega, period in ((1e6, 1.0), (50.0, 0.01), (0.3, 0.25), (0.0, 1.0)):           # every axis point under every angular rate
        out.append((f"undistort-axes-omega{omega:g}-period{period:g}", np.array([12.0, -1.5, omega]), np.array(_AXIS_POINTS), period))
    _undistort = out
    return out


def _ieee_atan2_mp(Y, X):
    """atan2 at 50 digits with IEEE 754's rules for signed zeros, which mpmath's numbers do not carry"""
    import mpmath as mp
    if Y == 0:
        at_pi = X < 0 or (X == 0 and math.copysign(1.0, X) < 0)
        return (mp.pi if at_pi else mp.mpf(0)) * int(math.copysign(1.0, Y))
    return mp.atan2(mp.mpf(Y), mp.mpf(X))


_undistort_ref = {}


def undistort_reference(case):
    """-> (xy (N, 2), dT (N,), tol_xy (N,), tol_dT) as float64, the values from mpmath at 50 digits rounded once; tol_*: ONE unit of the
    scaled tolerance, u * period / 2 and u * (|p| (1 + |a|) + |v| |dT|)"""
    name, v3, pts, period = case
    if name in _undistort_ref:
        return _undistort_ref[name]
    import mpmath as mp
    uniq, inv = np.unique(pts.view(np.uint64).reshape(-1, 2), axis=0, return_inverse=True)
    uniq = uniq.view(np.float64).reshape(-1, 2)
    xy, dT, tol = np.empty((len(uniq), 2)), np.empty(len(uniq)), np.empty(len(uniq))
    with mp.workdps(50):
        v0, v1, om, per = (mp.mpf(float(v)) for v in (*v3, period))
        for i, (x, y) in enumerate(uniq.tolist()):
            d = per * _ieee_atan2_mp(-y, -x) / (2 * mp.pi)
            a = om * d
            ca, sa, X, Y = mp.cos(a), mp.sin(a), mp.mpf(x), mp.mpf(y)
            xy[i] = float(ca * X - sa * Y + v0 * d), float(sa * X + ca * Y + v1 * d)
            dT[i] = float(d)
            tol[i] = U * float(mp.hypot(X, Y) * (1 + abs(a)) + mp.hypot(v0, v1) * abs(d))
    inv = np.asarray(inv).reshape(-1)
    _undistort_ref[name] = (xy[inv], dT[inv], tol[inv], U * period / 2)
    return _undistort_ref[name]


def undistort_deviation(xy, dT, ref):
    """(xy, dT) deviation in units of the scaled tolerance; a point whose unit is 0 (the origin under v = 0 ...) must be exact"""
    rxy, rdT, tol, tol_dT = ref
    xy, dT = np.asarray(xy, np.float64)[:, :2], np.asarray(dT, np.float64)
    if xy.shape != rxy.shape or dT.shape != rdT.shape or not (np.isfinite(xy).all() and np.isfinite(dT).all()):
        return math.inf, math.inf
    e = np.abs(xy - rxy).max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        fx = np.where(tol > 0, e / tol, np.where(e > 0, np.inf, 0.0))
    return float(fx.max()), float(np.abs(dT - rdT).max() / tol_dT)


def compare_undistort(xy, dT, ref, k_xy, k_dT):
    fx, fd = undistort_deviation(xy, dT, ref)
    return fx <= k_xy and fd <= k_dT


# ====================================================================================== consistency graph
GRAPH_K = [1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024]


def _lattice_equality(K, seed):
    """K points of a square lattice of multiples of 3 (12, 24 or 40 on a side, the smallest that holds K), `new` stretched by 2 in x:
    many pairs have both distances whole numbers"""
    side = next(g for g in (12, 24, 40) if g * g >= K)
    idx = np.random.default_rng(9500 + seed).permutation(side * side)[:K]
    p = np.column_stack((3 * (idx // side), 3 * (idx % side))).astype(np.float32)
    return p, (p * np.float32([2, 1])).astype(np.float32)


def equality_pairs(prev, new, thr):
    """pairs (i < j) whose two distances are both whole numbers with |d0 - d1| == thr exactly, found in int64 arithmetic"""
    p, n = np.asarray(prev, np.float64), np.asarray(new, np.float64)
    assert np.array_equal(p, np.rint(p)) and np.array_equal(n, np.rint(n)) and thr == int(thr)
    p, n = p.astype(np.int64), n.astype(np.int64)

    def whole(q):
        d2 = ((q[:, None, :] - q[None, :, :]) ** 2).sum(axis=2)
        r = np.rint(np.sqrt(d2.astype(np.float64))).astype(np.int64)
        return r, r * r == d2
    r0, ok0 = whole(p)
    r1, ok1 = whole(n)
    i, j = np.nonzero(np.triu(ok0 & ok1 & (np.abs(r0 - r1) == int(thr)), 1))
    return np.column_stack((i, j))


_graph = None


def graph_cases():
    """-> (cases [(name, prev, new, thr)] float32, equality {name: pairs (m, 2)})"""
    global _graph
    if _graph is not None:
        return _graph
    import oracle
    thr0 = oracle.DIST_THRESHOLD_PX
    out, eq = [], {}
    for t, K in enumerate(GRAPH_K):
        rng = np.random.default_rng(9600 + t)
        p = rng.uniform(0, 2024, size=(K, 2)).astype(np.float32)
        n = (p + rng.normal(0, 3.0 if K <= 129 else 0.3, size=(K, 2))).astype(np.float32)      # (jitter that straddles the threshold makes the
        # clique search exponential: kept to the sizes where the oracle's walk stays quick)
        n[rng.permutation(K)[:K // 5]] += rng.normal(0, 25, size=(K // 5, 2)).astype(np.float32)
        out.append((f"graph-random-K{K}", p, n, thr0))
        kind = t % 6
        pi = rng.integers(0, 2025, size=(K, 2)).astype(np.float32)
        if kind == 0:
            out.append((f"graph-shift-thr0-K{K}", pi, pi + np.float32([3, -7]), 0.0))                 # complete, exactly
        elif kind == 1:
            out.append((f"graph-thr1e9-K{K}", p, n, 1e9))                                              # complete
        elif kind == 2:
            out.append((f"graph-thr-1-K{K}", p, n, -1.0))                                              # empty
        elif kind == 3:
            q, m = p.copy(), n.copy()
            q[K // 2:] = q[0]; m[K // 3:] = m[0]
            out.append((f"graph-coincident-K{K}", q, m, thr0))
        elif kind == 4:
            out.append((f"graph-1e6-K{K}", p + np.float32(1e6), n + np.float32(1e6), thr0))            # float32 spacing 1/16 px there
        else:
            m = n.copy()
            m[K // 2, 1] = np.nan
            out.append((f"graph-nan-K{K}", p, m, thr0))
    byname = {c[0]: c for c in out}
    pi = np.random.default_rng(1).integers(0, 2025, size=(1024, 2)).astype(np.float32)
    out += [("graph-shift-thr0-K1024", pi, pi + np.float32([5, 11]), 0.0),
            ("graph-thr-1-K1", *byname["graph-random-K1"][1:3], -1.0),
            ("graph-thr1e9-K1", *byname["graph-random-K1"][1:3], 1e9),
            ("graph-thr-1-K513", *byname["graph-random-K513"][1:3], -1.0)]
    for K, thr, seed in ((65, 3.0, 0), (129, 6.0, 1), (513, 0.0, 2), (1024, 6.0, 3), (127, 0.0, 4)):
        p, n = _lattice_equality(K, seed)
        name = f"graph-equality-K{K}-thr{thr:g}"
        out.append((name, p, n, thr))
        eq[name] = equality_pairs(p, n, thr)
        assert len(eq[name]) >= 16, (name, len(eq[name]))
    assert len({c[0] for c in out}) == len(out)
    _graph = (out, eq)
    return _graph


def graph_scipy(prev, new, thr):
    """the reference's construction on the live scipy -> dense bool (K, K), diagonal cleared"""
    from scipy.spatial.distance import cdist
    p, n = np.asarray(prev, np.float32), np.asarray(new, np.float32)
    with np.errstate(invalid="ignore"):
        A = np.abs(cdist(p, p) - cdist(n, n)) <= thr
    np.fill_diagonal(A, False)
    return A


def pack_adjacency(A):
    """dense bool (K, K) -> uint64 words (K, max(1, ceil(K / 64))), bit j of word j // 64, unused bits 0"""
    K = A.shape[0]
    nw = max(1, (K + 63) // 64)
    bits = np.zeros((K, nw * 64), np.uint8)
    bits[:, :K] = A
    return np.packbits(bits, axis=1, bitorder="little").view(np.uint64).reshape(K, nw)


def compare_graph(adj, want_adj, pairs=None):
    """exact: every word, the unused high bits of the last one included; the listed pairs adjacent both ways"""
    adj, want_adj = np.asarray(adj), np.asarray(want_adj)
    if adj.shape != want_adj.shape or not np.array_equal(adj, want_adj):
        return False
    for i, j in ([] if pairs is None else np.asarray(pairs).tolist()):
        if not ((int(adj[i, j // 64]) >> (j % 64)) & 1 and (int(adj[j, i // 64]) >> (i % 64)) & 1):
            return False
    return True
