"""CPU: the global map's NumPy contract (tests/global_map_model.py) against an independent restatement, the two host entries of the
library (roam_map_plan, roam_map_pose_table), the argument checks of the Python entries and GlobalMap.cellOf.  No device: every check
here must raise before a device is asked for."""
import ctypes
import math
import os

import numpy as np
import pytest

import global_map_cases as cases
import global_map_model as model

ULP_OF_ONE = 2.0 ** -52


# ---------------------------------------------------------------------------------------------------------------- the model
def _loop_render(clouds, poses, cs, res, extent, min_hits, min_views, use):
    """the definition again, point by point in Python floats: a dict of cells, a set of entries per cell"""
    ox, oy, W, H = extent
    cells, outside = {}, 0
    for e, cloud in enumerate(clouds):
        if use is not None and not use[e]:
            continue
        c, s, x, y = float(cs[e][0]), float(cs[e][1]), float(poses[e][0]), float(poses[e][1])
        for px, py in np.asarray(cloud, np.float64).reshape(-1, 2).tolist():
            wx = ((c * px) - (s * py)) + x
            wy = ((s * px) + (c * py)) + y
            dx, dy = (wx - ox) / res, (wy - oy) / res
            if not (0.0 <= dx < W and 0.0 <= dy < H):
                outside += 1
                continue
            u, v = math.floor(dx), math.floor(dy)
            cell = cells.setdefault((v, u), [0, set(), 0, 0])
            cell[0] += 1
            cell[1].add(e)
            cell[2] += math.floor((dx - u) * 65536.0)
            cell[3] += math.floor((dy - v) * 65536.0)
    points = []
    for (v, u) in sorted(cells):
        hits, entries, sx, sy = cells[(v, u)]
        if hits >= min_hits and len(entries) >= min_views:
            mx, my = (2 * sx + hits) / (131072.0 * hits), (2 * sy + hits) / (131072.0 * hits)
            points.append((ox + res * (u + mx), oy + res * (v + my), hits, len(entries)))
    return cells, outside, points


SMALL_ENTRIES = [cases.SINGLE, cases.N65, cases.N63, cases.EDGES, cases.PAIR_A, cases.PAIR_B, cases.EMPTY]


def _small_cases():
    """the renders whose clouds are small enough for the loop: all of SMALL, and BIG with its large entries masked out"""
    out = [("small", name, kw) for name, kw in cases.small_renders()]
    keep = np.zeros(12, np.int8)
    keep[SMALL_ENTRIES] = 1
    for name, kw in cases.big_renders():
        use = keep if kw["use"] is None else kw["use"] & keep
        out.append(("big", name, {**kw, "use": use}))
    return out


@pytest.mark.parametrize("which,name,kw", _small_cases(), ids=lambda v: v if isinstance(v, str) else None)
def test_model_against_the_loop(which, name, kw):
    from radarslampy_amd import _ffi
    clouds = cases.small_clouds() if which == "small" else cases.big_clouds()
    cs = _ffi.map_pose_table(kw["poses"])
    extent, b, n, got = cases.expected(clouds, kw, cs)
    cells, outside, points = _loop_render(clouds, kw["poses"], cs, kw["res"], extent, kw["min_hits"], kw["min_views"], kw["use"])
    W, H = extent[2:]
    print(f"{which} / {name}: extent {extent}, {n} points, {len(cells)} cells occupied, {outside} outside, {len(points)} map points")
    assert got["outside"] == outside and got["hits"].shape == (H, W) and got["hits"].dtype == got["views"].dtype == np.uint32
    assert int(np.count_nonzero(got["hits"])) == len(cells) and int(got["hits"].sum()) + outside == n
    for (v, u), (hits, entries, sx, sy) in cells.items():
        assert (got["hits"][v, u], got["views"][v, u], got["sx"][v, u], got["sy"][v, u]) == (hits, len(entries), sx, sy)
    assert got["points"].shape == (len(points), 2)
    want = np.array([p[:2] for p in points], np.float64).reshape(-1, 2)
    assert got["points"].tobytes() == want.tobytes()
    assert got["point_hits"].tolist() == [p[2] for p in points] and got["point_views"].tolist() == [p[3] for p in points]
    if kw["extent"] is None:
        assert outside == 0                               # a planned extent holds every point


def test_the_cases_hold_what_they_are_for():
    """the figures the crafted clouds were built to give, by the model under the identity pose (cos 1, sin 0)"""
    clouds = cases.big_clouds()
    by_name = dict(cases.big_renders())
    cs = np.tile([1.0, 0.0], (12, 1))

    def run(name):
        return cases.expected(clouds, by_name[name], cs)

    assert [len(c) for c in clouds] == [0, 1, 8192, 8192, 8191, 513, 65, 63, 513, 81, cases.PAIR_K, cases.PAIR_K]
    _, _, _, r = run("one cell")
    assert r["hits"].max() == 8192 and np.count_nonzero(r["hits"]) == 1 and r["views"].max() == 1 and len(r["points"]) == 1
    _, _, _, r = run("8192 distinct cells")
    assert np.count_nonzero(r["hits"]) == 8192 and r["hits"].max() == 1
    _, _, _, r = run("cell edges")                        # 9 x 9 multiples of the cell from -2 m to 2 m on an 8 x 8 grid from -2 m: dx = 8 is outside
    assert r["outside"] == 17 and np.all(r["hits"] == 1) and not r["sx"].any() and not r["sy"].any()
    _, _, _, r = run("cell edges, cut on four sides")
    assert r["outside"] == 81 - 6 and np.all(r["hits"] == 1)
    ext, _, _, r = run("outside on four sides")
    pts = np.concatenate([clouds[cases.N8191], clouds[cases.N513]])
    x1, y1 = ext[0] + ext[2] * 0.5, ext[1] + ext[3] * 0.5
    sides = [np.count_nonzero(pts[:, 0] < ext[0]), np.count_nonzero(pts[:, 0] >= x1), np.count_nonzero(pts[:, 1] < ext[1]), np.count_nonzero(pts[:, 1] >= y1)]
    assert min(sides) > 100 and 0 < r["outside"] < len(pts) and r["hits"].sum() + r["outside"] == len(pts)
    ext, _, _, r = run("701 x 299")
    assert ext[2:] == (701, 299) and r["outside"] == 0
    assert r["hits"][0, 0] and r["hits"][0, 700] and r["hits"][298, 0] and r["hits"][298, 700]
    _, _, _, r = run("1 x 1")
    assert r["hits"].tolist() == [[sum(len(c) for c in clouds)]] and r["views"].tolist() == [[11]] and r["outside"] == 0
    for name, shape in (("1 x N", (121, 1)), ("N x 1", (1, 203))):
        _, _, _, r = run(name)
        assert r["hits"].shape == shape and r["outside"] > 0 and np.count_nonzero(r["hits"]) > 20
    _, _, _, r2 = run("thresholds")
    _, _, _, r1 = run("identity, all entries, planned")
    assert 0 < len(r2["points"]) < len(r1["points"]) and r2["point_hits"].min() >= 2 and r2["point_views"].min() >= 2
    assert np.count_nonzero((r1["hits"] >= 2) & (r1["views"] < 2)) > 0            # min_views decides for some cells
    _, _, _, r = run("nothing used")
    assert not r["hits"].any() and len(r["points"]) == 0 and r["outside"] == 0
    # the twins share a pose, so wherever one lands the other does
    tw = by_name["twins at one far pose"]
    _, _, _, r = cases.expected(clouds, tw, model.pose_table(tw["poses"]))
    assert np.all(r["views"][r["hits"] > 0] == 2) and np.all(r["hits"] % 2 == 0)


# ---------------------------------------------------------------------------------------------------------------- the host entries
def test_pose_table_is_libm_of_the_angles():
    from radarslampy_amd import _ffi
    poses = cases.far_poses(64, 3)
    poses[5:9, 2] = [0.0, np.pi / 2, -np.pi / 2, 1e5]
    cs = _ffi.map_pose_table(poses)
    d = np.abs(cs - model.pose_table(poses))
    print(f"{np.count_nonzero(d)} of {d.size} table entries differ from NumPy's, largest {d.max():.3g}")
    assert cs.dtype == np.float64 and cs.shape == (64, 2) and d.max() <= ULP_OF_ONE
    assert cs[5].tolist() == [1.0, 0.0] and cs[0, 0] == -1.0
    assert _ffi.map_pose_table(np.zeros((0, 3))).shape == (0, 2)
    for bad in (np.zeros((3, 2)), [[0.0, 0.0, np.nan]], [[0.0, 0.0, np.inf]]):
        with pytest.raises(ValueError, match="poses"):
            _ffi.map_pose_table(bad)


def _plan_cases():
    rng = np.random.default_rng(17)
    out = [(0.0, 10.0, -3.0, 4.0, 0.5), (-7.5, -7.5, 2.0, 2.0, 0.5), (1.5, 1.5, -1.5, -1.5, 0.5), (-1e6, 1e6, -1e6, 1e6, 400.0), (0.0, 0.0, 0.0, 0.0, 1e-3),
           (0.1 * 3, 0.1 * 3 + 1.0, -0.1 * 7, 5.0, 0.1), (-2e6, -2e6 + 1.0, 2e6 - 1.0, 2e6, 1e-3)]
    for _ in range(300):
        res = float(10.0 ** rng.uniform(-2.0, 1.5))
        lo = rng.uniform(-2e3, 2e3, 2)
        if rng.random() < 0.4:                            # a minimum that is an exact multiple of the cell
            lo = np.round(lo / res) * res
        span = rng.uniform(0.0, 60.0, 2) * (rng.random(2) < 0.9)
        out.append((float(lo[0]), float(lo[0] + span[0]), float(lo[1]), float(lo[1] + span[1]), res))
    return out


def test_plan_against_the_model_and_its_margin():
    from radarslampy_amd import _ffi
    for minx, maxx, miny, maxy, res in _plan_cases():
        got = _ffi.map_plan((minx, maxx, miny, maxy), res)
        assert got == model.plan(minx, maxx, miny, maxy, res), (minx, maxx, miny, maxy, res)
        ox, oy, W, H = got
        for lo, hi, o, n in ((minx, maxx, ox, W), (miny, maxy, oy, H)):
            d_lo, d_hi = (lo - o) / res, (hi - o) / res   # both bounding points fall inside, off the first and the last cell
            assert 0.0 <= d_lo < n and 0.0 <= d_hi < n, (lo, hi, res, o, n)
            assert math.floor(d_lo) >= 0 and math.floor(d_hi) <= n - 1 and n <= (hi - lo) / res + 4


def test_plan_refusals():
    from radarslampy_amd import _ffi
    lib = _ffi.load_library()
    ox, oy, W, H = ctypes.c_double(), ctypes.c_double(), ctypes.c_int32(), ctypes.c_int32()
    outs = (ctypes.byref(ox), ctypes.byref(oy), ctypes.byref(W), ctypes.byref(H))
    nan, inf = float("nan"), float("inf")
    arg = [(nan, 1.0, 0.0, 1.0, 0.5), (0.0, inf, 0.0, 1.0, 0.5), (inf, -inf, inf, -inf, 0.5), (2.0, 1.0, 0.0, 1.0, 0.5), (0.0, 1.0, 3.0, 2.5, 0.5),
           (0.0, 1.0, 0.0, 1.0, 0.0), (0.0, 1.0, 0.0, 1.0, -1.0), (0.0, 1.0, 0.0, 1.0, nan), (0.0, 1.0, 0.0, 1.0, inf), (1e6, 1e6, 0.0, 0.0, 1e-12)]
    for a in arg:
        assert lib.roam_map_plan(*a, *outs) == _ffi.ROAM_E_ARG, a
        with pytest.raises(ValueError, match="arg"):
            model.plan(*a)
        with pytest.raises(ValueError, match="global map"):
            _ffi.map_plan(a[:4], a[4])
    for a in [(0.0, 8192.0, 0.0, 8192.0, 1.0), (0.0, 2.0 ** 26, 0.0, 0.0, 1.0), (-1e6, 1e6, -1e6, 1e6, 1.0)]:
        assert lib.roam_map_plan(*a, *outs) == _ffi.ROAM_E_CAPACITY, a
        with pytest.raises(ValueError, match="capacity"):
            model.plan(*a)
        with pytest.raises(ValueError, match="cells"):
            _ffi.map_plan(a[:4], a[4])
    assert _ffi.map_plan((0.0, 8189.0, 0.0, 8189.0), 1.0) == (-1.0, -1.0, 8192, 8192)        # 2^26 cells exactly
    assert lib.roam_map_plan(0.0, 1.0, 0.0, 1.0, 0.5, None, *outs[1:]) == _ffi.ROAM_E_ARG
    with pytest.raises(ValueError, match="bounds"):
        _ffi.map_plan((0.0, 1.0, 2.0), 0.5)
    with pytest.raises(ValueError, match="res"):
        _ffi.map_plan((0.0, 1.0, 0.0, 1.0), "0.5")


# ---------------------------------------------------------------------------------------------------------------- the Python checks
def _no_device(monkeypatch):
    from radarslampy_amd import _ffi

    def no_device(*a, **k):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(_ffi, "default_context", no_device)
    monkeypatch.setattr(_ffi, "Context", no_device)


GOOD = dict(poses=np.zeros((4, 3)), use=None, res=0.5, extent=(0.0, 0.0, 10, 10), min_hits=1, min_views=1)


@pytest.mark.parametrize("kw,match", [
    (dict(poses=[[0.0, 0.0, np.nan]] * 4), "poses"), (dict(poses=[[np.inf, 0.0, 0.0]] * 4), "poses"), (dict(poses=[[0.0, -2e6, 0.0]] * 4), "poses"),
    (dict(poses=np.zeros((3, 3))), "poses"), (dict(poses=np.zeros((4, 2))), "poses"), (dict(poses=np.zeros(12)), "poses"), (dict(poses=[["a"] * 3] * 4), "poses"),
    (dict(res=0), "res"), (dict(res=0.0), "res"), (dict(res=-0.5), "res"), (dict(res=float("nan")), "res"), (dict(res=float("inf")), "res"), (dict(res="1"), "res"),
    (dict(extent=(0.0, 0.0, 8193, 8192)), "W H"), (dict(extent=(0.0, 0.0, 0, 5)), "W and H"), (dict(extent=(0.0, 0.0, 5, -1)), "W and H"),
    (dict(extent=(0.0, 0.0, 5.0, 5)), "W and H"), (dict(extent=(np.nan, 0.0, 5, 5)), "origin"), (dict(extent=(0.0, 0.0, 5)), "extent"),
    (dict(min_hits=0), "min_hits"), (dict(min_views=0), "min_views"), (dict(min_hits=1.0), "min_hits"), (dict(min_views=True), "min_views"),
    (dict(use=np.ones(3, np.int8)), "use"), (dict(use=np.ones(5, np.int8)), "use"), (dict(use=np.ones((4, 1), np.int8)), "use"), (dict(use=np.ones(4)), "use")])
def test_map_arguments_raise_before_a_device_is_asked_for(kw, match, monkeypatch):
    from radarslampy_amd import _ffi
    from radarslampy_amd.LoopClosure import LoopDetector
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match=match):
        _ffi.loop_map_args(4, **{**GOOD, **kw})
    # and through the detector: a LoopDetector that never reached the device
    det = LoopDetector.__new__(LoopDetector)
    det.keepClouds = True
    det.db = [None] * 4                                   # len() is all the checks ask of it
    names = dict(res="cellM", min_hits="minHits", min_views="minViews")
    with pytest.raises(ValueError, match=match):
        det.renderMap(**{names.get(k, k): v for k, v in {**GOOD, **kw}.items()})


def test_map_arguments_that_pass():
    from radarslampy_amd import _ffi
    p, u, res, extent, mh, mv = _ffi.loop_map_args(2, [[1, 2, 3], [4, 5, 6]], [True, False], 1, (0, -1, 8192, 8192), 2, 3)
    assert p.dtype == np.float64 and p.flags.c_contiguous and p.tolist() == [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]
    assert u.dtype == np.int8 and u.tolist() == [1, 0] and (res, extent, mh, mv) == (1.0, (0.0, -1.0, 8192, 8192), 2, 3)
    assert _ffi.loop_map_args(2, np.zeros((2, 3)), np.array([0, 7]))[1].tolist() == [0, 1]
    p, u, _, extent, _, _ = _ffi.loop_map_args(0, [])
    assert p.shape == (0, 3) and u is None and extent is None


def test_a_detector_or_database_without_clouds_refuses_before_the_library():
    from radarslampy_amd import _ffi
    from radarslampy_amd.LoopClosure import LoopDetector
    det = LoopDetector.__new__(LoopDetector)
    det.keepClouds = False
    with pytest.raises(ValueError, match="keeps no clouds"):
        det.renderMap(np.zeros((0, 3)))
    db = _ffi.LoopDb.__new__(_ffi.LoopDb)
    db.h = db.ctx = None
    db.cloud_rows = db.max_points = None
    for call in (lambda: db.map_bounds(np.zeros((0, 3))), lambda: db.map_render(np.zeros((0, 3)), 0.5, (0.0, 0.0, 1, 1)),
                 lambda: db.time_map(np.zeros((0, 3)), 0.5, (0.0, 0.0, 1, 1))):
        with pytest.raises(ValueError, match="keeps no clouds"):
            call()


# ---------------------------------------------------------------------------------------------------------------- the entry points
def test_the_library_exports_the_entries_and_refuses_a_null_context():
    from radarslampy_amd import _ffi
    from radarslampy_amd import LoopClosure, Mapping
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    names = ("roam_map_pose_table", "roam_map_plan", "roam_loop_db_map_bounds", "roam_loop_db_map_render", "roam_time_loop_db_map")
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "roam_abi.h")).read()
    for name in names:
        assert hasattr(lib, name), name
        assert name in _ffi.ABI_SYMBOLS and f" {name}(" in txt
    assert "#define ROAM_MAP_MAX_CELLS (1 << 26)" in txt and _ffi.MAP_MAX_CELLS == model.MAX_CELLS == 1 << 26
    lib = _ffi.load_library()
    n, n64, ms = ctypes.c_int32(), ctypes.c_int64(), (ctypes.c_float * 3)()
    assert lib.roam_loop_db_map_bounds(None, None, None, None, None, ctypes.byref(n64)) == _ffi.ROAM_E_ARG
    assert lib.roam_loop_db_map_render(None, None, None, None, 0.5, 0.0, 0.0, 1, 1, 1, 1, None, None, None, None, None, 0, ctypes.byref(n),
                                       ctypes.byref(n64)) == _ffi.ROAM_E_ARG
    assert lib.roam_time_loop_db_map(None, None, None, None, 0.5, 0.0, 0.0, 1, 1, 1, 1, 1, ms) == _ffi.ROAM_E_ARG
    assert lib.roam_map_pose_table(-1, None, None) == _ffi.ROAM_E_ARG and lib.roam_map_pose_table(1, None, None) == _ffi.ROAM_E_ARG
    assert lib.roam_map_pose_table(0, None, None) == _ffi.ROAM_OK
    for cls, name in ((_ffi.LoopDb, "map_bounds"), (_ffi.LoopDb, "map_render"), (_ffi.LoopDb, "time_map"), (LoopClosure.LoopDetector, "renderMap"),
                      (LoopClosure, "mapFromGraph"), (Mapping, "GlobalMap")):
        assert callable(getattr(cls, name))


def test_cell_of_follows_the_rule():
    from radarslampy_amd.Mapping import GlobalMap
    m = GlobalMap((-1.0, 2.0), 0.5, (4, 6), None, None, np.zeros((0, 2)), np.zeros(0, np.uint32), np.zeros(0, np.uint32), 3)
    assert m.nPoints == 0 and m.outside == 3 and m.origin == (-1.0, 2.0) and m.cellM == 0.5 and m.shape == (4, 6)
    xy = [[-1.0, 2.0], [-0.75, 2.25], [-0.5, 2.5], [np.nextafter(-0.5, -1.0), np.nextafter(2.5, 0.0)], [-1.01, 1.99], [-1.5, 1.5], [-1.75, 1.25],
          [2.0, 4.0], [1.99, 3.99]]
    got = m.cellOf(xy)
    assert got.dtype == np.int64 and got.tolist() == [[0, 0], [0, 0], [1, 1], [0, 0], [-1, -1], [-1, -1], [-2, -2], [6, 4], [5, 3]]
    # the same cells as the model's, for points inside
    rng = np.random.default_rng(2)
    pts = np.stack([rng.uniform(-1.0, 2.0, 500), rng.uniform(2.0, 4.0, 500)], axis=1)
    inside, u, v, _, _ = model.cells(pts[:, 0], pts[:, 1], 0.5, -1.0, 2.0, 6, 4)
    assert inside.all() and np.array_equal(m.cellOf(pts), np.stack([u, v], axis=1))
    assert m.cellOf([0.0, 3.0]).tolist() == [[2, 2]]
