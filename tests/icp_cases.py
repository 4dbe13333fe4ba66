"""Shared, seeded inputs of the ICP tests (test_icp_cpu.py, test_gpu_icp.py).  The model's results are computed once per case and
cached; nothing here touches a device."""
import functools

import numpy as np

import icp_model as model

THREADS, TILE, MAX_POINTS = 512, 4096, 8192        # csrc/icp.hip ICP_THREADS, ICP_TILE; roam_abi.h ROAM_ICP_MAX_POINTS
DUP_DELTA = 1e-8                                    # far below half a float32 ulp of a coordinate of at least 1 m (6e-8)


def rigid(pts, th, tx, ty):
    c, s = np.cos(th), np.sin(th)
    return np.stack([c * pts[:, 0] - s * pts[:, 1] + tx, s * pts[:, 0] + c * pts[:, 1] + ty], 1)


def _scene(rng, n, m, motion, noise=0.0, outliers=0.0, spacing=2.5):
    """src: n points, dst: m points.  A jittered grid of max(n, m) world points `spacing` apart, so that no point has two neighbours
    at nearly one distance; src sees the first n, dst the first m moved by `motion` (th, tx, ty), a share `outliers` of dst replaced
    by uniform clutter, both with Gaussian noise, dst shuffled"""
    k = max(n, m)
    side = int(np.ceil(np.sqrt(k)))
    gx, gy = np.meshgrid(np.arange(side), np.arange(side))
    world = (np.stack([gx.ravel(), gy.ravel()], 1)[:k] - side / 2.0) * spacing + rng.uniform(-0.3, 0.3, (k, 2)) * spacing
    world = world[rng.permutation(k)]
    src = world[:n] + noise * rng.standard_normal((n, 2))
    dst = rigid(world[:m], *motion) + noise * rng.standard_normal((m, 2))
    bad = rng.random(m) < outliers
    dst[bad] = rng.uniform(-side * spacing / 2, side * spacing / 2, (int(bad.sum()), 2))
    return src, dst[rng.permutation(m)]


def _build(name):
    """-> (src, dst, init (th, tx, ty), opts)"""
    rng = np.random.default_rng(4000 + sum(map(ord, "dup" if name.startswith("dup_") else name)))      # the two dup cases share their points
    small = (0.02, 0.15, -0.1)
    if name == "identical_64":
        src = rng.uniform(-20, 20, (64, 2))
        return src, src.copy(), (0.0, 0.0, 0.0), {}
    if name == "rigid_64":                          # an exact motion of 0.3 rad and 0.4 m, seeded with the yaw of three 6-degree sectors
        src, _ = _scene(rng, 64, 64, (0, 0, 0), spacing=3.0)
        return src, rigid(src, 0.3, 0.4 * np.cos(1.0), 0.4 * np.sin(1.0)), (2 * np.pi * 3 / 60, 0.0, 0.0), {}
    if name in ("dup_low_first", "dup_high_first"):
        # every dst point twice: float32-representable coordinates p, and p + 1e-8, which rounds to the same float32.  The search cannot
        # tell them apart; the float64 sums can.  The lowest index must win, so the translation follows the half that comes first
        src = rng.uniform(2.0, 30.0, (48, 2)) * rng.choice([-1.0, 1.0], (48, 2))
        p = rigid(src, 0.01, 0.05, -0.02)
        p = np.where(np.abs(p) < 1.0, np.sign(p) * 1.5, p).astype(np.float32).astype(np.float64)
        q = p + DUP_DELTA
        assert np.array_equal(q.astype(np.float32), p.astype(np.float32))
        return src, (np.concatenate([p, q]) if name == "dup_low_first" else np.concatenate([q, p])), (0.0, 0.0, 0.0), {}
    if name == "n0":
        return np.zeros((0, 2)), rng.uniform(-5, 5, (5, 2)), (0.1, 0.2, 0.3), {}
    if name == "m0":
        return rng.uniform(-5, 5, (5, 2)), np.zeros((0, 2)), (0.1, 0.2, 0.3), {}
    if name == "n1_m3":
        src, dst = _scene(rng, 1, 3, small)
        return src, dst, (0.0, 0.0, 0.0), {}
    if name == "n2_m2_min2":
        src, dst = _scene(rng, 2, 2, small)
        return src, dst, (0.0, 0.0, 0.0), {"min_pairs": 2}
    if name == "n2_m2":                             # two pairs against the default min_pairs = 3
        src, dst = _scene(rng, 2, 2, small)
        return src, dst, (0.0, 0.0, 0.0), {}
    if name == "n3_m3":
        src, dst = _scene(rng, 3, 3, small)
        return src, dst, (0.0, 0.0, 0.0), {}
    if name == "n3_m1":                             # every point has the one partner b, and (b + b + b) / 3 == b exactly for these
        src = rng.uniform(-0.5, 0.5, (3, 2))        # coordinates: the centred sums are exactly zero and theta stays
        return src, np.array([[0.25, -0.125]]), (0.3, 0.0, 0.0), {}
    if name == "n1_m1":
        return np.array([[1.0, 2.0]]), np.array([[1.1, 2.1]]), (0.0, 0.0, 0.0), {}
    for n in (63, 64, 65):
        if name == f"n{n}":
            src, dst = _scene(rng, n, 70, small, noise=0.02)
            return src, dst, (0.0, 0.0, 0.0), {}
    if name == "n513":                              # one over the workgroup's lanes: lane 0 holds two points
        src, dst = _scene(rng, THREADS + 1, 300, small, noise=0.02)
        return src, dst, (0.0, 0.0, 0.0), {}
    if name == "n2049":                             # one over a block of 4 x 512 points: a second sweep of one row
        src, dst = _scene(rng, 4 * THREADS + 1, 200, small, noise=0.02)
        return src, dst, (0.0, 0.0, 0.0), {}
    if name == "n1100":                             # a block of three rows
        src, dst = _scene(rng, 1100, 257, small, noise=0.02)
        return src, dst, (0.0, 0.0, 0.0), {}
    for m in (TILE - 1, TILE + 1):
        if name == f"m{m}":                         # one under / over the LDS tile; the partners of src 0 and 1 are the last two dst
            src, dst = _scene(rng, 150, m, small, noise=0.02)          # points: m - 1 = 4096 is alone in the second tile, 4094 shares its
            for i, pos in ((0, m - 1), (1, m - 2)):                    # 16-byte cell with the padding
                j = int(np.argmin(((dst - rigid(src[i:i + 1], *small)) ** 2).sum(1)))
                dst[[j, pos]] = dst[[pos, j]]
            return src, dst, (0.0, 0.0, 0.0), {}
    if name == "gated_out":
        src, dst = _scene(rng, 40, 40, (0.0, 500.0, 0.0))
        return src, dst, (0.05, 0.1, -0.1), {}
    if name == "max_iterations_1":
        src, dst = _scene(rng, 100, 100, small, noise=0.02)
        return src, dst, (0.0, 0.0, 0.0), {"max_iterations": 1}
    if name == "outliers_400":
        src, dst = _scene(rng, 400, 380, (0.05, 0.5, -0.4), noise=0.05, outliers=0.3)
        return src, dst, (0.0, 0.0, 0.0), {}
    if name == "flat_gate":                         # gate_start = gate_end and no decay: the stopping rule is live from the first update
        src, dst = _scene(rng, 200, 220, (0.004, 0.1, 0.05), noise=0.03)
        return src, dst, (0.0, 0.0, 0.0), {"gate_start": 0.8, "gate_end": 0.8, "gate_decay": 1.0}
    if name == "far_seed":                          # a yaw seed half a sector off and a metre of translation
        src, dst = _scene(rng, 350, 350, (0.6, 0.7, -0.7), noise=0.03, outliers=0.1, spacing=4.0)
        return src, dst, (0.6 - 0.05, 0.0, 0.0), {}
    raise KeyError(name)


CASES = ("identical_64", "rigid_64", "dup_low_first", "dup_high_first", "n0", "m0", "n1_m1", "n1_m3", "n2_m2_min2", "n2_m2", "n3_m3",
         "n3_m1", "n63", "n64", "n65", "n513", "n1100", "n2049", f"m{TILE - 1}", f"m{TILE + 1}", "gated_out", "max_iterations_1",
         "outliers_400", "flat_gate", "far_seed")


@functools.lru_cache(maxsize=None)
def case(name):
    src, dst, init, opts = _build(name)
    src.setflags(write=False)
    dst.setflags(write=False)
    return src, dst, tuple(float(v) for v in init), opts


@functools.lru_cache(maxsize=None)
def case_model(name, search_form="plain", order="kernel", nudge=0):
    src, dst, init, opts = case(name)
    return model.icp(src, dst, init, search_form=search_form, order=order, nudge=nudge, **opts)


VARIANTS = (dict(search_form="fma"), dict(order="sequential"), dict(order="pairwise"), dict(nudge=1), dict(nudge=-1))
TOL_FLOOR, TOL_CAP_M, TOL_CAP_RAD = 1e-9, 1e-2, 1e-3


@functools.lru_cache(maxsize=None)
def tolerance_measured():
    """name -> (metres, radians): the largest difference of the translation or the rms, and of the angle, between the model and its
    variants - a fused multiply-add in the search, two other summation orders, the transformed points one float32 ulp up or down"""
    out = {}
    for name in CASES:
        p0, s0 = case_model(name)
        dm = dr = 0.0
        for v in VARIANTS:
            p, s = case_model(name, **v)
            dr = max(dr, abs(model.normalize_angle(p[0] - p0[0])))
            dm = max(dm, float(np.abs(p[1:] - p0[1:]).max()))
            if np.isfinite(s["rms"]) or np.isfinite(s0["rms"]):
                dm = max(dm, abs(s["rms"] - s0["rms"]))
        out[name] = (dm, dr)
    return out


def tolerance():
    """-> (metres, radians), the bound on |device - model| of a pose (and, in metres, of an rms): ten times the largest difference
    between the model and its variants over every case, floored at 1e-9.  The caps 1e-2 m and 1e-3 rad are a condition, checked by
    test_icp_cpu.py: a case that moves further under those variants is ill-conditioned and does not belong here"""
    t = tolerance_measured()
    return (max(TOL_FLOOR, 10.0 * max(v[0] for v in t.values())), max(TOL_FLOOR, 10.0 * max(v[1] for v in t.values())))


# ---------------------------------------------------------------------------------------------------------------- a batch
def batch130():
    """130 mixed pairs: the cases in turn (with their own init; the options must be one per batch, so only the cases with default
    options), empty ones among them -> (names, pairs, init)"""
    names = [n for n in CASES if not case(n)[3] and not n.startswith("m4")]
    names = [names[k % len(names)] for k in range(130)]
    return names, [case(n)[:2] for n in names], np.array([case(n)[2] for n in names])


# ---------------------------------------------------------------------------------------------------------------- the revisit world
RANGE_RESOLUTION_M = 0.0432
TRUTH_CAP_M, TRUTH_CAP_RAD = 0.2, 0.04


def cloud_from_peaks(peaks, rows=400):
    """(K, 2) [thetaInd, rInd] -> (K, 2) metres, r res (cos phi, sin phi), phi = 2 pi thetaInd / rows: the model's own restatement of
    LoopClosure.polarIndToLocalMetres"""
    phi = 2.0 * np.pi * peaks[:, 0] / rows
    r = peaks[:, 1] * RANGE_RESOLUTION_M
    return np.stack([r * np.cos(phi), r * np.sin(phi)], 1)


@functools.lru_cache(maxsize=None)
def revisit_clouds_oracle():
    """the eleven peak clouds of scan_context_cases.revisit_records() by the oracle's peak extraction, full density"""
    import oracle
    import scan_context_cases as sc
    return [cloud_from_peaks(np.asarray(oracle.peaks_from_record_u8(r), np.float64), r.shape[0]) for r in sc.revisit_records()]


def revisit_truth(t):
    """the true pose (th, tx, ty) that aligns revisit t to its place: x_place^-1 x_revisit"""
    import scan_context_cases as sc
    place, pose = sc.REVISITS[t]
    z = model.relative_pose(sc.place_pose(place), pose)
    return np.array([z[2], z[0], z[1]])


def revisit_seed(t):
    """the yaw a scan-context candidate carries: the true yaw difference rounded to a sector, in (-pi, pi]"""
    import scan_context_cases as sc
    a = 2.0 * np.pi * (round(sc.revisit_true_shift(t)) % sc.REVISIT_S) / sc.REVISIT_S
    return a - 2.0 * np.pi if a > np.pi else a


def pose_error(pose, truth):
    """-> (metres, radians) between two (th, tx, ty)"""
    return float(np.hypot(pose[1] - truth[1], pose[2] - truth[2])), float(abs(model.normalize_angle(pose[0] - truth[0])))


@functools.lru_cache(maxsize=None)
def revisit_model(sub):
    """the model on the three true pairs at every sub-th point -> [(pose, stats)]"""
    import scan_context_cases as sc
    c = revisit_clouds_oracle()
    return [model.icp(c[8 + t][::sub], c[place][::sub], (revisit_seed(t), 0.0, 0.0)) for t, (place, _) in enumerate(sc.REVISITS)]


def truth_bound():
    """-> (metres, radians): 1.5 times the largest error of the model against the ground truth on the three true pairs at every 4th
    point, capped at 0.2 m and 0.04 rad"""
    errs = [pose_error(p, revisit_truth(t)) for t, (p, _) in enumerate(revisit_model(4))]
    return min(TRUTH_CAP_M, 1.5 * max(e[0] for e in errs)), min(TRUTH_CAP_RAD, 1.5 * max(e[1] for e in errs))


WRONG_OFFSETS = (1, 3)


@functools.lru_cache(maxsize=None)
def revisit_fractions(sub):
    """-> (true (3,), wrong (3, 2)): the model's inlier fraction n_inliers / min(n, m) of every revisit against its place and against
    the places (place + 1) % 8 and (place + 3) % 8, at every sub-th point"""
    import scan_context_cases as sc
    c = revisit_clouds_oracle()
    true, wrong = [], []
    for t, (place, _) in enumerate(sc.REVISITS):
        row = []
        for other in [place] + [(place + d) % len(sc.PLACES) for d in WRONG_OFFSETS]:
            src, dst = c[8 + t][::sub], c[other][::sub]
            _, s = model.icp(src, dst, (revisit_seed(t), 0.0, 0.0)) if other != place or sub != 4 else revisit_model(4)[t]
            row.append(s["n_inliers"] / min(len(src), len(dst)))
        true.append(row[0])
        wrong.append(row[1:])
    return np.array(true), np.array(wrong)
