"""Crafted grids, clouds and windows for the map matching (tests/map_match_model.py), each named for the branch of the definition - and of
csrc/map_match.hip - that it reaches; tests/test_map_match_cpu.py counts from the model that it does.  Nothing here touches a device.

A FIELD is what a match field is made from: the grids of a render, the thresholds, the smear.  A MATCH is a call: a field, the clouds,
the priors, the raw window (n_theta, step_rad, kx, ky).  At the prior (0, 0, 0) the angle table's middle row is (1, 0) and a world point
is the cloud's point exactly, so a cloud can be put in chosen cells."""
import functools

import numpy as np

from global_map_cases import GRID_701

RES = 0.5
ORIGIN = (-10.25, -5.5)                                   # multiples of a quarter: cell edges are exact doubles, negative ones among them


# ---------------------------------------------------------------------------------------------------------------- fields
def _grids(W, H, occupied, hits=3, views=2):
    """hits / views (H, W) uint32: `hits` points from `views` keyframes in every cell of the (v, u) list `occupied`, none elsewhere"""
    h, v = np.zeros((H, W), np.uint32), np.zeros((H, W), np.uint32)
    for (y, x) in occupied:
        h[y, x], v[y, x] = hits, views
    return h, v


def _random_cells(W, H, fraction, seed):
    rng = np.random.default_rng(seed)
    n = max(1, int(round(fraction * W * H)))
    flat = rng.choice(W * H, n, replace=False)
    return sorted((int(f // W), int(f % W)) for f in flat)


def _corners(W, H):
    return sorted({(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)})


TWIN_SHAPE = [(0, 0), (0, 2), (1, 1), (3, 0), (4, 3), (2, 4)]          # a cluster of six cells, (dv, du)
TWIN_AT, TWIN_APART = (10, 8), 19                                     # the first cluster's corner (v, u); the second is 19 cells further in u


def _twins():
    return sorted([(TWIN_AT[0] + dv, TWIN_AT[1] + du) for dv, du in TWIN_SHAPE] + [(TWIN_AT[0] + dv, TWIN_AT[1] + TWIN_APART + du) for dv, du in TWIN_SHAPE])


@functools.lru_cache(maxsize=None)
def fields():
    """-> {name: dict(hits, views, origin, res, min_hits, min_views, radius, sigma)}"""
    out = {}

    def add(name, W, H, occupied, radius=2, sigma=1.0, min_hits=1, min_views=1, origin=ORIGIN, res=RES, grids=None):
        h, v = grids if grids is not None else _grids(W, H, occupied)
        out[name] = dict(hits=h, views=v, origin=origin, res=res, min_hits=min_hits, min_views=min_views, radius=radius, sigma=sigma)
    for W, H in ((1, 1), (37, 1), (1, 37), (67, 33), (130, 129)):
        add(f"{W}x{H} empty", W, H, [])
        add(f"{W}x{H} full", W, H, [(y, x) for y in range(H) for x in range(W)])
        add(f"{W}x{H} corners", W, H, _corners(W, H))
        add(f"{W}x{H} random 2 %", W, H, _random_cells(W, H, 0.02, W + H))
    # an occupied cell closer than the radius to each of the four borders (the corners are), at every radius; radius 0: F = 255 occupied
    for r, sigma in ((0, 1.0), (1, 0.5), (2, 1.0), (8, 3.0)):
        add(f"67x33 corners and centre, radius {r}", 67, 33, _corners(67, 33) + [(16, 33), (1, 30), (31, 30), (12, 1), (12, 65)], radius=r, sigma=sigma)
    add("130x129 random 2 %, radius 8", 130, 129, _random_cells(130, 129, 0.02, 8), radius=8, sigma=3.0)
    add("67x33 twins", 67, 33, _twins(), radius=0)
    add("67x33 twins, radius 2", 67, 33, _twins())
    # thresholds: cells with many hits from one keyframe, and cells with one hit each from three
    rng = np.random.default_rng(3)
    h, v = np.zeros((33, 67), np.uint32), np.zeros((33, 67), np.uint32)
    a, b = _random_cells(67, 33, 0.03, 30), _random_cells(67, 33, 0.03, 31)
    for (y, x) in a:
        h[y, x], v[y, x] = 9, 1
    for (y, x) in b:
        h[y, x], v[y, x] = 3, 3
    add("67x33 views decide", 67, 33, None, min_hits=1, min_views=2, grids=(h, v))
    add("67x33 hits decide", 67, 33, None, min_hits=4, min_views=1, grids=(h, v))
    add("67x33 both decide", 67, 33, None, min_hits=4, min_views=2, grids=(h, v))
    W, H = GRID_701[2:]
    add("701x299 random 2 %", W, H, _random_cells(W, H, 0.02, 701), origin=GRID_701[:2], res=0.25)
    # a cell so fine that a point a metre away is 2^30 cells out
    add("130x129 tiny res", 130, 129, _random_cells(130, 129, 0.05, 9), origin=(0.0, 0.0), res=2.0 ** -31)
    return out


def occupied_cells(f):
    """-> (v, u) int arrays of the occupied cells of a field case"""
    return np.nonzero((f["hits"] >= f["min_hits"]) & (f["views"] >= f["min_views"]))


def cell_points(f, v, u, at=0.5):
    """points (n, 2) metres that lie in the cells (v, u) of a field case at the prior (0, 0, 0): `at` of the way across the cell"""
    ox, oy = f["origin"]
    return np.stack([ox + (np.asarray(u, np.float64) + at) * f["res"], oy + (np.asarray(v, np.float64) + at) * f["res"]], axis=1)


# ---------------------------------------------------------------------------------------------------------------- clouds
def _box(f, n, seed, margin):
    """n random points over the grid of a field case and `margin` cells around it"""
    rng = np.random.default_rng(seed)
    H, W = f["hits"].shape
    ox, oy = f["origin"]
    return np.stack([rng.uniform(ox - margin * f["res"], ox + (W + margin) * f["res"], n), rng.uniform(oy - margin * f["res"], oy + (H + margin) * f["res"], n)], axis=1)


def _ring(f, k):
    """the cells within k of the border, inside and outside, one point each: what a shift of up to k carries out of the grid on each of
    the four sides, and into it from each side"""
    H, W = f["hits"].shape
    cells = [(v, u) for v in range(-k, H + k) for u in range(-k, W + k) if not (k <= v < H - k and k <= u < W - k)]
    v, u = np.array(cells).T
    return cell_points(f, v, u, 0.25)


def _edges(f):
    """points exactly on cell edges and corners, negative coordinates among them (ORIGIN is negative)"""
    H, W = f["hits"].shape
    u, v = np.meshgrid(np.arange(-1, W + 2, 3), np.arange(-1, H + 2, 2))
    return cell_points(f, v.ravel(), u.ravel(), 0.0)


IDENT = (0.0, 0.0, 0.0)
BATCH = 48
WINDOWS = [(1, 0.0, 0, 0), (1, 0.01, 5, 0), (1, 0.01, 0, 5), (3, 0.01, 2, 2), (25, 0.01, 12, 12), (5, 0.02, 3, 64)]      # (n_theta, step_rad, kx, ky)
ROW_LENGTHS = [(1, 0.0, 31, 1), (1, 0.0, 32, 1), (3, 0.01, 63, 2), (1, 0.0, 64, 20)]       # 2 kx + 1 = 63, 65, 127 and 129; the last has 41 rows of 129 candidates, more than a workgroup holds


@functools.lru_cache(maxsize=None)
def matches():
    """-> {name: dict(field, clouds [(n, 2)], priors (n, 3), window, reaches: the branches test_map_match_cpu.py counts)}"""
    F = fields()
    out = {}

    def add(name, field, clouds, priors, window, reaches=()):
        priors = np.tile(np.asarray(priors, np.float64), (len(clouds), 1)) if np.ndim(priors) == 1 else np.asarray(priors, np.float64)
        out[name] = dict(field=field, clouds=clouds, priors=priors, window=window, reaches=tuple(reaches))
    rnd = F["67x33 random 2 %"]
    tilt = (0.3, -0.2, 0.05)                              # a prior that is no multiple of anything
    # sizes: one wavefront more or less, more than one chunk of 2048 points, the ceiling
    for n in (0, 1, 63, 64, 65, 4097, 8192):
        cloud = _box(rnd, n, n, 3) if n != 1 else cell_points(rnd, *[c[:1] for c in occupied_cells(rnd)])
        add(f"{n} points", "67x33 random 2 %", [cloud], tilt if n != 1 else IDENT, (3, 0.01, 2, 2), ["whole"] if n > 1 else ["cut"] * n)
    # windows, on a cloud with points on every list
    base = _box(rnd, 300, 7, 8)
    for w in WINDOWS:
        add(f"window {w[0]} x {2 * w[3] + 1} x {2 * w[2] + 1}", "67x33 random 2 %", [base], tilt, w, (["whole"] if 2 * w[3] < 33 else []) + (["cut", "dropped"] if w[2] or w[3] else []))         # 129 rows of shift: no window fits 33
    big = F["701x299 random 2 %"]
    for w in ROW_LENGTHS:
        add(f"row length {2 * w[2] + 1}", "701x299 random 2 %", [_box(big, 200, w[2], 40)], (0.1, 0.05, -0.02), w, ["whole", "cut"])
    add("the largest window", "130x129 random 2 %", [_box(F["130x129 random 2 %"], 63, 5, 10)], IDENT, (1, 0.0, 128, 128), ["cut"])
    # where the points are
    v, u = occupied_cells(rnd)
    mid = np.flatnonzero((v > 5) & (v < 27) & (u > 5) & (u < 61))[:1]           # an occupied cell well inside
    add("all points in one cell", "67x33 random 2 %", [np.repeat(cell_points(rnd, v[mid], u[mid]), 500, axis=0)], IDENT, (3, 0.01, 2, 2), ["whole"])
    add("points on cell edges", "67x33 random 2 %", [_edges(rnd)], IDENT, (1, 0.0, 2, 2), ["edges", "cut"])
    add("leaving and entering on four sides", "67x33 full", [_ring(F["67x33 full"], 3)], IDENT, (1, 0.0, 3, 3),
        ["leaves left", "leaves right", "leaves low", "leaves high", "enters left", "enters right", "enters low", "enters high", "cut"])
    tiny = F["130x129 tiny res"]
    far = np.concatenate([cell_points(tiny, *occupied_cells(tiny)), [[1.0, 0.0], [0.0, -1.0], [-0.75, 0.5], [0.5, 2.0 ** -31 * 7]]])      # the last: dx = 2^30 exactly
    far = np.concatenate([far, [[np.nextafter(0.5, 0.0), 0.0], [-0.5, 0.0]]])      # the last doubles that are not far: 2^30 - ulp, and -2^30
    add("far points", "130x129 tiny res", [far], IDENT, (3, 0.0, 2, 2), ["far", "whole", "dropped"])
    # degenerate grids
    for name in ("1x1 full", "37x1 corners", "1x37 random 2 %", "1x1 empty", "130x129 empty"):
        f = F[name]
        add(f"grid {name}", name, [_box(f, 40, 11, 2)], IDENT, (3, 0.3, 3, 3), ["cut"])
    add("radius 8", "130x129 random 2 %, radius 8", [_box(F["130x129 random 2 %, radius 8"], 400, 12, 6)], tilt, (5, 0.02, 6, 6), ["whole", "cut"])
    # the planted tie: the cloud is the cluster's shape, and the window holds both clusters
    tw = F["67x33 twins"]
    shape = np.array(TWIN_SHAPE)
    cluster = cell_points(tw, TWIN_AT[0] + shape[:, 0], TWIN_AT[1] + shape[:, 1])
    add("a planted tie", "67x33 twins", [cluster], (10 * RES, 0.0, 0.0), (1, 0.0, 12, 2), ["tie"])
    add("a planted tie, radius 2", "67x33 twins, radius 2", [cluster], (10 * RES, RES, 0.0), (3, 0.2, 12, 2), ["tie"])
    # batches: queries of different sizes in one call; one query at several positions of a batch
    mixed = [_box(rnd, n, 40 + n, 3) for n in (0, 1, 65, 4097, 300)]
    add("a batch of different sizes", "67x33 random 2 %", mixed, [tilt, IDENT, (0.0, 0.4, -0.03), tilt, (1.0, 1.0, 0.1)], (3, 0.01, 2, 3), ["whole"])
    # batches large enough that a device of up to 300 compute units gives a workgroup as many rows as it holds (BATCH x 25 pairs of query
    # and angle >= 4 per unit): 625 candidates in one block, three accumulators; and 65 rows of 65 in blocks of 31, 31 and 3, all eight
    r130 = F["130x129 random 2 %"]
    rng = np.random.default_rng(48)
    pri = np.stack([rng.uniform(-1.0, 1.0, BATCH), rng.uniform(-1.0, 1.0, BATCH), rng.uniform(-0.1, 0.1, BATCH)], axis=1)
    add("a batch of 48, window 25 x 25 x 25", "67x33 random 2 %", [_box(rnd, 40 + 3 * q, 100 + q, 4) for q in range(BATCH)], pri, (25, 0.01, 12, 12), ["whole", "cut"])
    add("a batch of 48, window 25 x 65 x 65", "130x129 random 2 %", [_box(r130, 30 + q, 200 + q, 4) for q in range(BATCH)], pri, (25, 0.01, 32, 32), ["whole", "cut"])
    other = _box(rnd, 200, 50, 3)
    add("one query at three positions", "67x33 random 2 %", [base, other, base, other, other, base], [tilt, IDENT, tilt, tilt, IDENT, tilt], (3, 0.01, 4, 2), ["whole"])
    return out


# ---------------------------------------------------------------------------------------------------------------- what a case reaches
def reached(f, xy, prior, cs, kx, ky):
    """count, from the definition alone, the branches a query takes over all its angles -> dict of counts"""
    import map_match_model as model
    H, W = f["hits"].shape
    ox, oy = f["origin"]
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    c = dict.fromkeys(["far", "dropped", "cut", "whole", "edges", "leaves left", "leaves right", "leaves low", "leaves high", "enters left", "enters right",
                       "enters low", "enters high"], 0)
    for row in cs:
        u, v = model.cells(xy, prior, row, f["res"], ox, oy)
        c["far"] += len(xy) - len(u)
        gone = (u + kx < 0) | (u - kx >= W) | (v + ky < 0) | (v - ky >= H)
        whole = (u - kx >= -1) & (u + kx <= W) & (v - ky >= -1) & (v + ky <= H)
        c["dropped"] += int(gone.sum())
        c["whole"] += int((whole & ~gone).sum())
        c["cut"] += int((~whole & ~gone).sum())
        inside = (u >= 0) & (u < W) & (v >= 0) & (v < H)
        c["leaves left"] += int((inside & (u - kx < 0)).sum())
        c["leaves right"] += int((inside & (u + kx >= W)).sum())
        c["leaves low"] += int((inside & (v - ky < 0)).sum())
        c["leaves high"] += int((inside & (v + ky >= H)).sum())
        rows_in = (v >= 0) & (v < H)
        cols_in = (u >= 0) & (u < W)
        c["enters left"] += int((rows_in & (u < 0) & (u + kx >= 0)).sum())
        c["enters right"] += int((rows_in & (u >= W) & (u - kx < W)).sum())
        c["enters low"] += int((cols_in & (v < 0) & (v + ky >= 0)).sum())
        c["enters high"] += int((cols_in & (v >= H) & (v - ky < H)).sum())
        wx, wy = model.world(xy, prior, row)
        dx, dy = (wx - ox) / f["res"], (wy - oy) / f["res"]
        c["edges"] += int(((dx == np.floor(dx)) | (dy == np.floor(dy))).sum())
    return c


# ---------------------------------------------------------------------------------------------------------------- the synthetic world
WORLD_CELL_M, WORLD_RADIUS = 0.25, 2
WORLD_WINDOW = dict(reachM=3.0, reachRad=0.12, stepRad=0.01)
WORLD_MAP_POSES = [(2.0 * k, 0.3 * np.sin(0.7 * k), 0.02 * k) for k in range(8)]          # eight scans 2 m apart
# four held-out scans between and beside the map's, and how far off their priors are: 2 to 3 m per axis, 0.05 to 0.12 rad
WORLD_QUERY_POSES = [(3.1, 0.45, 0.031), (6.9, -0.35, 0.072), (10.7, 0.6, -0.044), (13.2, -0.15, 0.118)]
WORLD_PRIOR_OFF = [(2.13, -2.71, 0.0537), (-2.87, 2.29, -0.0911), (2.44, 2.06, 0.1163), (-2.31, -2.93, -0.0768)]


@functools.lru_cache(maxsize=None)
def world_records():
    """twelve Oxford records (400 x 3779 uint8) of StreamWorld(5, per_tile=40): the eight map scans, then the four queries"""
    from radarslampy_amd import synth
    w = synth.StreamWorld(5, per_tile=40)
    return [synth.render_stream_record(w, pose, t_index=t) for t, pose in enumerate(WORLD_MAP_POSES + WORLD_QUERY_POSES)]


@functools.lru_cache(maxsize=None)
def world_clouds_oracle():
    """the twelve peak clouds by the oracle's peak extraction, metres in the sensor frame; thinned as a loop database thins them to at most
    8192 points: every step-th peak, step = ceil(peaks / 8192)"""
    import oracle
    from icp_cases import cloud_from_peaks
    out = []
    for r in world_records():
        c = cloud_from_peaks(np.asarray(oracle.peaks_from_record_u8(r), np.float64), r.shape[0])
        out.append(c[::max(1, -(-len(c) // 8192))])
    return out


def world_priors():
    return np.array(WORLD_QUERY_POSES) + np.array(WORLD_PRIOR_OFF)


# ---------------------------------------------------------------------------------------------------------------- the model's answers
@functools.lru_cache(maxsize=None)
def expected_field(name):
    """the model's field of a field case, smeared with the library's own table (host code, no device) -> (table, F (H, W) uint8)"""
    import map_match_model as model
    from radarslampy_amd import _ffi
    f = fields()[name]
    table = _ffi.map_field_table(f["sigma"], f["radius"])
    return table, model.field(f["hits"], f["views"], f["min_hits"], f["min_views"], f["radius"], table)


@functools.lru_cache(maxsize=None)
def expected_match(name):
    """the model's answer to a match case, multiplying with the library's own angle table (host code, no device), computed once and
    shared -> (poses (n, 3) float64, info (n, 6) int32, [volume per query])"""
    import map_match_model as model
    from radarslampy_amd import _ffi
    m = matches()[name]
    f = fields()[m["field"]]
    _, F = expected_field(m["field"])
    n_theta, step, kx, ky = m["window"]
    cs = _ffi.map_match_angles(m["priors"], n_theta, step)
    rows = [model.match(F, xy, m["priors"][q], cs[q], step, f["res"], f["origin"][0], f["origin"][1], kx, ky) for q, xy in enumerate(m["clouds"])]
    return np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), [r[2] for r in rows]
