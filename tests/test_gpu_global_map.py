"""GPU (-m gpu): the global map (csrc/loop_map.hip, LoopDetector.renderMap, LoopClosure.mapFromGraph) against tests/global_map_model.py.
Parity is unpinned: nothing in the reference computes a map.

Every comparison is bit for bit.  The pose table the model multiplies with is the library's own (_ffi.map_pose_table, the host's libm);
from there on a world point is four multiplies, three additions, a subtraction and a division per coordinate pair, each rounded once on
both sides, and what a cell holds are integers - there is nothing left to round differently, so no tolerance appears below."""
import ctypes
import types

import numpy as np
import pytest

import global_map_cases as cases
import scan_context_cases as sc
from gen_inputs import ENGINE_LAYOUTS, layout_sequence

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from radarslampy_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


def _detector(ctx, clouds, max_points):
    from radarslampy_amd.LoopClosure import LoopDetector
    det = LoopDetector(len(clouds), cases.SECTORS, cases.RINGS, min_gap=1, ctx=ctx, keepClouds=True, rows=400, maxPoints=max_points)
    assert det.addDescriptors(cases.descriptors(len(clouds)), clouds=clouds) == 0 and len(det) == len(clouds)
    return det


@pytest.fixture(scope="module")
def big(ctx):
    clouds = cases.big_clouds()
    det = _detector(ctx, clouds, 8192)
    yield det, clouds
    det.close()


@pytest.fixture(scope="module")
def small(ctx):
    clouds = cases.small_clouds()
    det = _detector(ctx, clouds, 64)
    yield det, clouds
    det.close()


_EXPECTED = {}


def _expected(which, name, clouds, kw):
    """the model's render of a case, computed once"""
    from radarslampy_amd import _ffi
    if (which, name) not in _EXPECTED:
        _EXPECTED[which, name] = cases.expected(clouds, kw, _ffi.map_pose_table(kw["poses"]))
    return _EXPECTED[which, name]


def _render(det, kw, **more):
    return det.renderMap(kw["poses"], cellM=kw["res"], extent=kw["extent"], minHits=kw["min_hits"], minViews=kw["min_views"], use=kw["use"], **more)


def _same_points(m, want):
    return (m.points.dtype == np.float64 and m.points.shape == want["points"].shape and m.points.tobytes() == want["points"].tobytes()
            and m.pointHits.dtype == np.uint32 and m.pointHits.tobytes() == want["point_hits"].tobytes()
            and m.pointViews.dtype == np.uint32 and m.pointViews.tobytes() == want["point_views"].tobytes())


def _same(m, extent, want):
    """a GlobalMap against the model's render, bit for bit"""
    return (m.origin == tuple(extent[:2]) and m.shape == (extent[3], extent[2]) and m.hits.dtype == m.views.dtype == np.uint32
            and m.hits.shape == m.shape and m.hits.tobytes() == want["hits"].tobytes() and m.views.tobytes() == want["views"].tobytes()
            and _same_points(m, want) and m.outside == want["outside"] and m.nPoints == len(want["points"]))


def _p32(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _p64(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


RENDERS = [("big", name, kw) for name, kw in cases.big_renders()] + [("small", name, kw) for name, kw in cases.small_renders()]


# ---------------------------------------------------------------------------------------------------------------- 1: crafted clouds
@pytest.mark.parametrize("which,name,kw", RENDERS, ids=lambda v: v if isinstance(v, str) else None)
def test_crafted_clouds(which, name, kw, big, small):
    det, clouds = big if which == "big" else small
    extent, bounds, n, want = _expected(which, name, clouds, kw)
    got_b, got_n = det.db.map_bounds(kw["poses"], kw["use"])
    print(f"{which} / {name}: bounds {got_b.tolist()}, {got_n} points; extent {extent}: {np.count_nonzero(want['hits'])} cells occupied, "
          f"{len(want['points'])} map points, {want['outside']} outside")
    assert got_n == n and got_b.tobytes() == np.asarray(bounds, np.float64).tobytes()
    m = _render(det, kw)
    assert m.cellM == kw["res"] and _same(m, extent, want)
    if kw["extent"] is None:
        assert m.outside == 0                             # a planned extent holds every point
    if name == "one cell":
        assert m.hits.max() == 8192 and m.views.max() == 1 and m.nPoints == 1 and m.pointHits.tolist() == [8192]
    if name == "twins at one far pose":
        assert np.all(m.views[m.hits > 0] == 2) and np.all(m.pointViews == 2)
    # the points are where cellOf says: each in its own cell, in row-major order
    uv = m.cellOf(m.points)
    flat = uv[:, 1] * m.shape[1] + uv[:, 0]
    assert np.array_equal(flat, np.flatnonzero((want["hits"] >= kw["min_hits"]) & (want["views"] >= kw["min_views"])))


def test_capacity_one_short_and_no_grids(big):
    from radarslampy_amd import _ffi
    det, clouds = big
    name, kw = cases.big_renders()[0]
    extent, _, _, want = _expected("big", name, clouds, kw)
    M = len(want["points"])
    assert M > 8192
    with pytest.raises(_ffi.RoamError) as e:
        det.db.map_render(kw["poses"], kw["res"], extent, cap=M - 1)
    assert e.value.code == _ffi.ROAM_E_CAPACITY and e.value.required == M and "capacity" in str(e.value)
    # the raw call writes no point
    pts, ph, pv = np.full((M - 1, 2), -7.0), np.full(M - 1, 7, np.uint32), np.full(M - 1, 7, np.uint32)
    n, out = np.zeros(1, np.int32), np.zeros(1, np.int64)
    p = np.ascontiguousarray(kw["poses"], np.float64)
    rc = det.db.ctx.lib.roam_loop_db_map_render(det.db.ctx.h, det.db.h, _ffi._ptr(p), None, kw["res"], extent[0], extent[1], extent[2], extent[3], 1, 1, None,
                                                None, _ffi._ptr(pts), _ffi._ptr(ph), _ffi._ptr(pv), M - 1, _p32(n), _p64(out))
    assert rc == _ffi.ROAM_E_CAPACITY and n[0] == M and np.all(pts == -7.0) and np.all(ph == 7) and np.all(pv == 7)
    exact = det.db.map_render(kw["poses"], kw["res"], extent, cap=M)
    assert exact["points"].tobytes() == want["points"].tobytes() and exact["hits"].tobytes() == want["hits"].tobytes()
    m = _render(det, kw, grids=False)
    assert m.hits is None and m.views is None and m.shape == (extent[3], extent[2]) and _same_points(m, want) and m.outside == 0


# ---------------------------------------------------------------------------------------------------------------- 2: the same bits
def test_the_same_call_twice_and_an_entry_alone_or_among_others(big, small):
    det, clouds = big
    name, kw = next((n, k) for n, k in cases.big_renders() if n == "far poses, all entries")
    extent, _, _, want = _expected("big", name, clouds, kw)
    a, b = _render(det, kw), _render(det, kw)
    assert _same(a, extent, want) and _same(b, extent, want)
    hits, views = np.zeros_like(want["hits"]), np.zeros_like(want["views"])
    outside = 0
    for e in range(len(clouds)):                          # every entry alone on the same extent: its share of the grids
        use = np.zeros(len(clouds), np.int8)
        use[e] = 1
        r = det.db.map_render(kw["poses"], kw["res"], extent, use=use)
        assert int(r["hits"].sum()) + r["outside"] == len(clouds[e]) and r["views"].max() <= 1
        assert np.array_equal(r["views"] > 0, r["hits"] > 0)
        hits += r["hits"]
        views += r["views"]
        outside += r["outside"]
    assert hits.tobytes() == want["hits"].tobytes() and views.tobytes() == want["views"].tobytes() and outside == want["outside"]
    # SMALL holds its five clouds twice, the second time in reverse order, and the poses go with the clouds: the same map
    det, clouds = small
    by_name = dict(cases.small_renders())
    first, again = _render(det, by_name["small, first five"]), _render(det, by_name["small, the five again, reversed"])
    assert first.origin == again.origin and first.shape == again.shape and first.hits.any()
    assert first.hits.tobytes() == again.hits.tobytes() and first.views.tobytes() == again.views.tobytes()
    assert first.points.tobytes() == again.points.tobytes() and first.pointHits.tobytes() == again.pointHits.tobytes()
    both = _render(det, by_name["small, all"])
    assert np.array_equal(both.hits, 2 * first.hits) and np.array_equal(both.views, 2 * first.views)


# ---------------------------------------------------------------------------------------------------------------- 3: what it is for
def test_a_wrong_pose_shows_as_single_views(big):
    """two entries hold one cloud of K points, six cells apart.  At the true poses K cells are occupied, each seen twice; with the
    second pose off by exactly three cells in x there are 2 K occupied cells, each seen once, and minViews = 2 leaves no map point"""
    det, clouds = big
    K = cases.PAIR_K
    use = np.zeros(12, np.int8)
    use[[cases.PAIR_A, cases.PAIR_B]] = 1
    poses = np.zeros((12, 3))
    extent = (-10.0, -10.0, 120, 120)
    true = det.renderMap(poses, cellM=cases.RES, extent=extent, use=use, minViews=2)
    assert np.count_nonzero(true.hits) == K and np.all(true.views[true.hits > 0] == 2) and np.all(true.hits[true.hits > 0] == 2)
    assert true.nPoints == K and true.outside == 0
    # a map point is the mean of the sub-cell positions, each known to 2^-16 of a cell and reported at the middle of that step
    pair = clouds[cases.PAIR_A][np.lexsort((clouds[cases.PAIR_A][:, 0], clouds[cases.PAIR_A][:, 1]))]
    assert np.abs(true.points - pair).max() <= cases.RES * 2.0 ** -16
    poses[cases.PAIR_B, 0] = 3 * cases.RES
    off = det.renderMap(poses, cellM=cases.RES, extent=extent, use=use, minViews=2)
    assert np.count_nonzero(off.hits) == 2 * K and np.all(off.views[off.hits > 0] == 1) and off.nPoints == 0 and off.outside == 0
    assert det.renderMap(poses, cellM=cases.RES, extent=extent, use=use).nPoints == 2 * K


# ---------------------------------------------------------------------------------------------------------------- 4: the engine
def test_clouds_from_the_engine():
    from radarslampy_amd import _ffi
    from radarslampy_amd.engine import Engine
    from radarslampy_amd.LoopClosure import LoopDetector
    layout = (497, 399, 504, 5)
    assert layout in ENGINE_LAYOUTS
    clip, rows, stride_b, off = layout
    recs, _ = layout_sequence(clip + 1, 4, rows, clip, stride_b, off, n_movers=6)
    order = [2, 0, 3, 3, 1]
    c = _ffi.Context(0)
    eng = Engine(1, 4, ctx=c, rows=rows, stride=stride_b, payload_off=off, clip=clip, retrack_on_device=False)
    for t in range(4):
        eng.upload_scan(t, recs[t])
    det = LoopDetector(8, 60, 20, clip_px=400, min_gap=1, ctx=c, keepClouds=True, rows=rows)
    assert eng.loop_db_add(det, order) == 0 and len(det) == 5
    clouds = [det.cloud(i)[0] for i in range(5)]
    assert min(len(x) for x in clouds) > 1000
    for seed, kw in ((1, dict(cellM=0.5)), (2, dict(cellM=0.25, minHits=2)), (3, dict(cellM=1.0, minViews=2, use=np.array([1, 1, 0, 1, 1], np.int8)))):
        poses = cases.far_poses(5, seed)
        poses[:, :2] *= 0.02                              # a few metres apart: the scans overlap
        full = dict(poses=poses, res=kw["cellM"], extent=None, min_hits=kw.get("minHits", 1), min_views=kw.get("minViews", 1), use=kw.get("use"))
        extent, _, n, want = cases.expected(clouds, full, _ffi.map_pose_table(poses))
        m = det.renderMap(poses, **kw)
        print(f"engine clouds, {kw}: {n} points on {extent[2]} x {extent[3]} cells, {m.nPoints} map points, views up to {m.views.max()}")
        assert _same(m, extent, want) and m.outside == 0 and m.nPoints > 0
    det.close()
    eng.close()
    c.close()


# ---------------------------------------------------------------------------------------------------------------- 5: after closeLoops
def test_map_from_graph_after_closing_loops():
    """the revisit world of test_gpu_loop_cloud.py, its drift and its weights: the map at the optimised poses"""
    from radarslampy_amd import _ffi
    from radarslampy_amd.engine import Engine
    from radarslampy_amd.LoopClosure import LoopDetector, closeLoops, mapFromGraph
    recs = sc.revisit_records()
    n, n_places = len(recs), len(sc.PLACES)
    c = _ffi.Context(0)
    eng = Engine(1, n, ctx=c, retrack_on_device=False)
    for t in range(n):
        eng.upload_scan(t, recs[t])
    det = LoopDetector(16, sc.REVISIT_S, sc.REVISIT_R, clip_px=sc.REVISIT_CLIP, min_gap=1, max_distance=np.inf, k=2, ctx=c, keepClouds=True,
                       rows=recs[0].shape[0])
    assert eng.loop_db_add(det, np.arange(n)) == 0
    true = np.array([sc.place_pose(i) for i in range(n_places)] + [p for _, p in sc.REVISITS])
    drift = np.cumsum(np.tile([0.35, -0.25, 0.006], (len(true), 1)), axis=0) - [0.35, -0.25, 0.006]
    kfs = [types.SimpleNamespace(pose=true[k] + drift[k]) for k in range(len(true))]
    graph, edges, _ = closeLoops(kfs, det, loopInformation=1e4 * np.eye(3), odomInformation=np.diag([1e-4, 1e-4, 1.0]), ctx=c)
    assert len(edges) == len(sc.REVISITS)
    poses = np.array([graph.get_pose(k) for k in range(n)])
    m = mapFromGraph(det, graph, cellM=1.0, minViews=2)
    want = det.renderMap(poses, cellM=1.0, minViews=2)
    print(f"map from the graph: {m.shape[1]} x {m.shape[0]} cells, {np.count_nonzero(m.hits)} occupied, {m.nPoints} seen from two keyframes")
    assert m.origin == want.origin and m.shape == want.shape and m.hits.tobytes() == want.hits.tobytes() and m.views.tobytes() == want.views.tobytes()
    assert m.points.tobytes() == want.points.tobytes() and m.pointViews.tobytes() == want.pointViews.tobytes() and m.outside == want.outside == 0
    assert int(m.hits.sum()) == int(det.db.cloud_counts()[0].sum())
    det.close()
    eng.close()
    c.close()


# ---------------------------------------------------------------------------------------------------------------- 6: refusals, timing
def test_raw_abi_refuses_bad_calls_and_leaves_the_database_usable(ctx, small):
    from radarslampy_amd import _ffi
    det, clouds = small
    lib, db = ctx.lib, det.db
    err = lambda: lib.roam_last_error(ctx.h)              # noqa: E731
    name, kw = cases.small_renders()[0]
    extent, _, _, want = _expected("small", name, clouds, kw)
    before = _render(det, kw)
    assert _same(before, extent, want)
    W, H = extent[2:]
    good = dict(poses=np.ascontiguousarray(kw["poses"], np.float64), use=None, res=0.5, ox=extent[0], oy=extent[1], W=W, H=H, min_hits=1, min_views=1, cap=64)
    pts, ph, pv = np.zeros((64, 2)), np.zeros(64, np.uint32), np.zeros(64, np.uint32)
    n, out = np.zeros(1, np.int32), np.zeros(1, np.int64)

    def render(handle=None, n_out=n, pts_out=pts, **kw):
        a = {**good, **kw}
        return lib.roam_loop_db_map_render(ctx.h, db.h if handle is None else handle, _ffi._ptr(a["poses"]), _ffi._ptr(a["use"]), a["res"], a["ox"], a["oy"],
                                           a["W"], a["H"], a["min_hits"], a["min_views"], None, None, _ffi._ptr(pts_out), _ffi._ptr(ph), _ffi._ptr(pv),
                                           a["cap"], _p32(n_out), _p64(out))

    nan_pose, far_pose, inf_theta = good["poses"].copy(), good["poses"].copy(), good["poses"].copy()
    nan_pose[3, 1], far_pose[9, 0], inf_theta[0, 2] = np.nan, 1.5e6, np.inf
    for kw_bad, text in ((dict(poses=None), b"poses"), (dict(poses=nan_pose), b"poses of entry 3"), (dict(poses=far_pose), b"poses of entry 9"),
                         (dict(poses=inf_theta), b"poses of entry 0"), (dict(res=0.0), b"res"), (dict(res=float("nan")), b"res"), (dict(ox=float("inf")), b"origin"),
                         (dict(W=0), b"W and H"), (dict(H=-3), b"W and H"), (dict(W=8193, H=8192), b"W H"), (dict(min_hits=0), b"min_hits"),
                         (dict(min_views=0), b"min_views"), (dict(cap=-1), b"cap"), (dict(n_out=None), b"n_points_out"), (dict(pts_out=None), b"points_out")):
        assert render(**kw_bad) == _ffi.ROAM_E_ARG and text in err(), (kw_bad.keys(), err())
    bounds, n64 = np.zeros(4), np.zeros(1, np.int64)
    assert lib.roam_loop_db_map_bounds(ctx.h, db.h, None, None, _ffi._ptr(bounds), _p64(n64)) == _ffi.ROAM_E_ARG and b"poses" in err()
    assert lib.roam_loop_db_map_bounds(ctx.h, db.h, _ffi._ptr(good["poses"]), None, None, _p64(n64)) == _ffi.ROAM_E_ARG and b"bounds_out" in err()
    assert render(handle=0) == _ffi.ROAM_E_ARG and b"db" in err()
    plain = _ffi.LoopDb(ctx, 10, cases.SECTORS, cases.RINGS)                      # a database that keeps no clouds
    plain.add_desc(cases.descriptors(10))
    assert render(handle=plain.h) == _ffi.ROAM_E_STATE and b"keeps no clouds" in err()
    assert lib.roam_loop_db_map_bounds(ctx.h, plain.h, _ffi._ptr(good["poses"]), None, _ffi._ptr(bounds), _p64(n64)) == _ffi.ROAM_E_STATE
    with pytest.raises(ValueError, match="keeps no clouds"):
        plain.map_render(kw["poses"], 0.5, extent)
    plain.close()
    assert not pts.any() and not n[0]
    assert _same(_render(det, kw), extent, want)          # every refusal left the database as it was
    # an empty database that keeps clouds: an all-zero grid and no points
    empty = _ffi.LoopDb(ctx, 4, cases.SECTORS, cases.RINGS)
    empty.keep_clouds(400, 64)
    b, cnt = empty.map_bounds(np.zeros((0, 3)))
    assert cnt == 0 and b.tolist() == [np.inf, -np.inf, np.inf, -np.inf]
    r = empty.map_render(np.zeros((0, 3)), 0.5, (0.0, 0.0, 3, 2))
    assert r["hits"].shape == (2, 3) and not r["hits"].any() and not r["views"].any() and len(r["points"]) == 0 and r["outside"] == 0
    empty.close()


def test_timing_entry_reports_three_parts_and_changes_nothing(big):
    det, clouds = big
    name, kw = cases.big_renders()[0]
    extent, _, _, want = _expected("big", name, clouds, kw)
    ms = det.db.time_map(kw["poses"], kw["res"], extent, reps=2)
    print(f"clear {ms[0]:.4f} ms, splat {ms[1]:.4f} ms, compaction {ms[2]:.4f} ms for {extent[2]} x {extent[3]} cells and 12 entries")
    assert len(ms) == 3 and all(np.isfinite(v) and v > 0.0 for v in ms)
    assert _same(_render(det, kw), extent, want)
