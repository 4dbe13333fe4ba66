"""CPU (-m "not gpu"): the contract of the map matching (tests/map_match_model.py) held against itself and against the host half of the
library (roam_map_field_table, roam_map_match_angles), the crafted cases (tests/map_match_cases.py) held to the branches they are named
for, two known answers, the argument checks of the Python entries, and the synthetic world: what the definition localises to.  No
device: every check that reaches the library uses host-only entries."""
import ctypes
import os
import re

import numpy as np
import pytest

import global_map_model as map_model
import map_match_cases as cases
import map_match_model as model

MATCHES = list(cases.matches())
FIELDS = list(cases.fields())


def _angles(m):
    from radarslampy_amd import _ffi
    return _ffi.map_match_angles(m["priors"], m["window"][0], m["window"][1])


# ---------------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("name", MATCHES)
def test_both_forms_of_the_volume_agree(name):
    m = cases.matches()[name]
    f = cases.fields()[m["field"]]
    _, F = cases.expected_field(m["field"])
    _, info, vols = cases.expected_match(name)
    n_theta, step, kx, ky = m["window"]
    cs = _angles(m)
    for q, xy in enumerate(m["clouds"]):
        if len(m["clouds"]) > 8 and q not in ((0, len(m["clouds"]) - 1) if vols[q].size < 50000 else (0,)):
            continue                                      # a large batch: its first and its last query, or the first alone (the literal loop is slow)
        if len(xy) * vols[q].size > 3e7:                  # the literal loop on a thinned cloud: the same code paths at a tenth of the time
            xy = xy[::16]
            fast = model.volume(F, xy, m["priors"][q], cs[q], f["res"], *f["origin"], kx, ky)
        else:
            fast = vols[q]
        slow = model.volume_loops(F, xy, m["priors"][q], cs[q], f["res"], *f["origin"], kx, ky)
        assert fast.dtype == slow.dtype == np.uint32 and fast.shape == (n_theta, 2 * ky + 1, 2 * kx + 1) and np.array_equal(fast, slow)
        assert int(vols[q].max()) == info[q, 0] <= 255 * len(m["clouds"][q])


@pytest.mark.parametrize("name", FIELDS)
def test_field_model_against_the_definition_cell_by_cell(name):
    f = cases.fields()[name]
    table, F = cases.expected_field(name)
    occ = (f["hits"] >= f["min_hits"]) & (f["views"] >= f["min_views"])
    H, W = occ.shape
    r = f["radius"]
    rng = np.random.default_rng(len(name))
    picks = {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)} | {(int(rng.integers(H)), int(rng.integers(W))) for _ in range(200)}
    for v, u in picks:
        want = 0
        for dv in range(-r, r + 1):
            for du in range(-r, r + 1):
                if 0 <= v + dv < H and 0 <= u + du < W and occ[v + dv, u + du]:
                    want = max(want, int(table[dv + r, du + r]))
        assert F[v, u] == want, (v, u)
    assert F.dtype == np.uint8 and np.array_equal(F == 255, occ) and table[r, r] == 255
    if r == 0:
        assert np.array_equal(F, np.where(occ, 255, 0))
    if name == "67x33 views decide":
        other = cases.fields()["67x33 hits decide"]
        o2 = (other["hits"] >= other["min_hits"]) & (other["views"] >= other["min_views"])
        assert occ.any() and o2.any() and not (occ & o2).any()        # each threshold keeps its own cells and drops the other's
        assert not ((f["hits"] >= 4) & (f["views"] >= 2)).any() and not cases.expected_field("67x33 both decide")[1].any()


# ---------------------------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("name", MATCHES)
def test_every_case_reaches_the_branch_it_names(name):
    m = cases.matches()[name]
    f = cases.fields()[m["field"]]
    n_theta, step, kx, ky = m["window"]
    cs = _angles(m)
    count = {}
    for q, xy in enumerate(m["clouds"]):
        for k, n in cases.reached(f, xy, m["priors"][q], cs[q], kx, ky).items():
            count[k] = count.get(k, 0) + n
    _, info, vols = cases.expected_match(name)
    print(name, {k: n for k, n in count.items() if n}, "best", info[:, :4].tolist())
    for branch in m["reaches"]:
        if branch == "tie":
            top = np.flatnonzero(vols[0].reshape(-1) == vols[0].max())
            flat = (info[0, 1] * (2 * ky + 1) + info[0, 2]) * (2 * kx + 1) + info[0, 3]
            assert len(top) == 2 and flat == top[0] and info[0, 0] == 255 * 6         # the tie exists and the lower index wins
            assert top[1] - top[0] == cases.TWIN_APART                                # the other cluster, the same row
        else:
            assert count[branch] > 0, (branch, count)
    assert np.all(info[:, 4] == [len(c) for c in m["clouds"]])
    if name == "leaving and entering on four sides":
        k = 3
        H, W = f["hits"].shape
        assert count["leaves left"] == count["leaves right"] == k * H and count["leaves low"] == count["leaves high"] == k * W
        assert count["enters left"] == count["enters right"] == k * H and count["enters low"] == count["enters high"] == k * W
    if name == "far points":
        assert count["far"] == 3 * 4 and count["dropped"] == 3 * 2                    # four far points, two that just are not, three angles
    if name == "one query at three positions":
        poses, _, _ = cases.expected_match(name)
        assert poses[0].tobytes() == poses[2].tobytes() == poses[5].tobytes() and np.array_equal(vols[0], vols[5]) and np.array_equal(info[0], info[2])


def _most_least(kx, ky):
    rowlen, nb = 2 * kx + 1, 2 * ky + 1
    return rowlen, nb, min(nb, 2048 // rowlen), -(-256 // rowlen)


def test_the_plan_of_the_row_blocks(monkeypatch):
    """roam_map_match_plan, the host code that cuts a window into workgroups (what the kernel's launch uses): at most 2048 candidates to a
    workgroup whatever is asked, every row in exactly one block, the batches of the cases at the rows a workgroup holds, and
    ROAM_MATCH_ROWS forcing the rows (clamped)"""
    from radarslampy_amd import _ffi
    monkeypatch.delenv("ROAM_MATCH_ROWS", raising=False)
    for cu in (1, 64, 256, 304, 4096):
        for nq in (1, 2, 48, 64, 1000, 65535):
            for n_theta, kx, ky in ((1, 0, 0), (1, 5, 0), (1, 0, 5), (3, 2, 2), (25, 12, 12), (5, 3, 64), (25, 32, 32), (61, 32, 32), (1, 64, 20), (1, 128, 128),
                                    (1025, 128, 128), (1, 0, 128), (1, 128, 0), (3, 3, 1)):
                rows, n_blk = _ffi.map_match_plan(cu, nq, (n_theta, 0.01, kx, ky))
                rowlen, nb, most, least = _most_least(kx, ky)
                assert 1 <= rows <= most and rows * rowlen <= 2048 and (n_blk - 1) * rows < nb <= n_blk * rows, (cu, nq, n_theta, kx, ky, rows, n_blk)
                assert rows >= min(least, most)
                if nq * n_theta >= 4 * cu:
                    assert rows == most                   # enough pairs of query and angle: a workgroup takes all it holds
    assert _ffi.map_match_plan(256, 1, (25, 0.01, 12, 12)) == (11, 3) and _ffi.map_match_plan(256, 1, (1, 0.0, 64, 20)) == (2, 21)
    assert _ffi.map_match_plan(256, cases.BATCH, (25, 0.01, 12, 12)) == (25, 1) and _ffi.map_match_plan(256, 64, (61, 0.01, 32, 32)) == (31, 3)
    assert _ffi.map_match_plan(256, cases.BATCH, (25, 0.01, 32, 32)) == (31, 3) == _ffi.map_match_plan(300, cases.BATCH, (25, 0.01, 32, 32))
    for forced, want in ((1, (1, 65)), (4, (4, 17)), (31, (31, 3)), (40, (31, 3)), (1024, (31, 3))):
        monkeypatch.setenv("ROAM_MATCH_ROWS", str(forced))
        assert _ffi.map_match_plan(256, 1, (25, 0.01, 32, 32)) == want == _ffi.map_match_plan(4096, 999, (1, 0.0, 32, 32))
    for ignored in ("0", "-3", "x", "", "1025"):
        monkeypatch.setenv("ROAM_MATCH_ROWS", ignored)
        assert _ffi.map_match_plan(256, 1, (25, 0.01, 12, 12)) == (11, 3)
    monkeypatch.delenv("ROAM_MATCH_ROWS")
    lib = _ffi.load_library()
    r, n = ctypes.c_int32(7), ctypes.c_int32(7)
    for args in ((0, 1, 3, 1, 1), (256, 0, 3, 1, 1), (256, 65536, 3, 1, 1), (256, 1, 2, 1, 1), (256, 1, 3, 129, 1), (256, 1, 3, 1, -1)):
        assert lib.roam_map_match_plan(*args, ctypes.byref(r), ctypes.byref(n)) == _ffi.ROAM_E_ARG and (r.value, n.value) == (7, 7)
    assert lib.roam_map_match_plan(256, 1, 3, 1, 1, None, ctypes.byref(n)) == lib.roam_map_match_plan(256, 1, 3, 1, 1, ctypes.byref(r), None) == _ffi.ROAM_E_ARG


# ---------------------------------------------------------------------------------------------------------------- known answers
def _own_points():
    f = cases.fields()["130x129 random 2 %"]
    _, F = cases.expected_field("130x129 random 2 %")
    v, u = cases.occupied_cells(f)
    return f, F, cases.cell_points(f, v, u)


def test_a_maps_own_points_at_the_identity_score_255_n_at_the_centre():
    f, F, pts = _own_points()
    n_theta, step, kx, ky = 5, 0.01, 4, 3
    cs = _angles(dict(priors=np.zeros((1, 3)), window=(n_theta, step)))[0]
    assert cs[2].tolist() == [1.0, 0.0]
    pose, info, vol = model.match(F, pts, (0.0, 0.0, 0.0), cs, step, f["res"], *f["origin"], kx, ky)
    assert info.tolist() == [255 * len(pts), 2, ky, kx, len(pts), len(pts)] and pose.tolist() == [0.0, 0.0, 0.0]
    assert np.count_nonzero(vol == vol.max()) == 1


def test_the_same_cloud_displaced_puts_the_peak_where_it_was_moved_to():
    """the truth is (x, y, th); the prior is 3 cells short in x, 2 cells over in y and two angle steps short: the peak is at
    i = c + 2, b = ky - 2, a = kx + 3"""
    f, F, world_pts = _own_points()
    n_theta, step, kx, ky = 7, 0.02, 5, 4
    truth = np.array([7.5, 3.0, 0.3])
    c, s = np.cos(truth[2]), np.sin(truth[2])
    d = world_pts - truth[:2]
    cloud = np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1]], axis=1)        # R(-th) (w - t): back into the sensor frame
    prior = truth + [-3 * f["res"], 2 * f["res"], -2 * step]
    cs = _angles(dict(priors=prior[None], window=(n_theta, step)))[0]
    pose, info, vol = model.match(F, cloud, prior, cs, step, f["res"], *f["origin"], kx, ky)
    assert info.tolist() == [255 * len(cloud), 3 + 2, ky - 2, kx + 3, len(cloud), len(cloud)]
    assert np.abs(pose - truth).max() < 1e-12 and np.count_nonzero(vol == vol.max()) == 1


# ---------------------------------------------------------------------------------------------------------------- the host half
def test_tables_are_libm_of_the_definition():
    from radarslampy_amd import _ffi
    for sigma, r in ((1.0, 2), (0.5, 1), (3.0, 8), (1.0, 0), (0.3, 8), (100.0, 8)):
        t = _ffi.map_field_table(sigma, r)
        assert t.dtype == np.uint8 and t.shape == (2 * r + 1, 2 * r + 1) and t[r, r] == 255
        assert np.abs(t.astype(int) - model.field_table(sigma, r).astype(int)).max() <= 1
        assert np.array_equal(t, t.T) and np.array_equal(t, t[::-1]) and np.array_equal(t, t[:, ::-1])
    priors = np.array([[1.0, 2.0, 0.3], [0.0, 0.0, -3.1], [5.0, 5.0, 1e3]])
    cs = _ffi.map_match_angles(priors, 25, 0.01)
    for q in range(3):
        want = model.angles(priors[q], 25, 0.01)
        assert np.abs(cs[q] - want).max() <= np.spacing(1.0)
        th = model.thetas(priors[q, 2], 25, 0.01)
        assert th[12] == priors[q, 2] and th[0] == priors[q, 2] + (-12.0) * 0.01
    assert _ffi.map_match_angles((0.0, 0.0, 0.0), 1, 0.0).tolist() == [[[1.0, 0.0]]]


def test_constants_are_the_headers():
    from radarslampy_amd import _abi
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "roam_abi.h")).read()
    for name, mine in (("RADIUS", _abi.MAP_MATCH_MAX_RADIUS), ("ANGLES", _abi.MAP_MATCH_MAX_ANGLES), ("SHIFT", _abi.MAP_MATCH_MAX_SHIFT)):
        assert int(re.search(rf"#define ROAM_MATCH_MAX_{name} (\d+)", txt)[1]) == mine
    assert re.search(r"#define ROAM_MATCH_MAX_VOLUME \(1 << 26\)", txt) and _abi.MAP_MATCH_MAX_VOLUME == 1 << 26
    assert (model.MAX_RADIUS, model.MAX_ANGLES, model.MAX_SHIFT, model.MAX_VOLUME) == (8, 1025, 128, 1 << 26)
    assert _abi.MATCH_TABLE.names == ("x", "y", "theta", "score", "fraction", "nPoints", "nInside", "i", "b", "a", "found")


def test_the_library_exports_the_entries_and_refuses_without_a_context():
    from radarslampy_amd import _ffi
    lib = _ffi.load_library()
    t = np.zeros(289, np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)       # noqa: E731
    for sigma, r in ((0.0, 2), (-1.0, 2), (np.nan, 2), (np.inf, 2), (1.0, -1), (1.0, 9)):
        assert lib.roam_map_field_table(sigma, r, p(t)) == _ffi.ROAM_E_ARG
    assert lib.roam_map_field_table(1.0, 2, None) == _ffi.ROAM_E_ARG and not t.any()
    pri, cs = np.zeros((2, 3)), np.zeros((2, 3, 2))
    assert lib.roam_map_match_angles(2, p(pri), 3, 0.01, p(cs)) == _ffi.ROAM_OK
    for n_theta, step in ((0, 0.01), (2, 0.01), (1027, 0.01), (3, -0.01), (3, np.nan), (3, np.inf)):
        assert lib.roam_map_match_angles(2, p(pri), n_theta, step, p(cs)) == _ffi.ROAM_E_ARG
    assert lib.roam_map_match_angles(2, None, 3, 0.01, p(cs)) == lib.roam_map_match_angles(2, p(pri), 3, 0.01, None) == _ffi.ROAM_E_ARG
    assert lib.roam_map_match_angles(2, p(np.array([[0.0, 0.0, 0.0], [0.0, 0.0, np.nan]])), 3, 0.01, p(cs)) == _ffi.ROAM_E_ARG
    for name in ("roam_map_field_create", "roam_map_field_read", "roam_map_field_destroy", "roam_map_match_clouds", "roam_loop_db_map_match",
                 "roam_time_map_match"):
        assert hasattr(lib, name)
    assert lib.roam_map_field_read(None, None, None) == lib.roam_map_field_destroy(None, None) == _ffi.ROAM_E_ARG


# ---------------------------------------------------------------------------------------------------------------- the Python checks
def _no_device(monkeypatch):
    from radarslampy_amd import _ffi

    def no_device(*a, **k):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(_ffi, "default_context", no_device)
    monkeypatch.setattr(_ffi, "Context", no_device)
    monkeypatch.setattr(_ffi, "load_library", no_device)


def _map(hits=None, views=None, grids=True):
    from radarslampy_amd.Mapping import GlobalMap
    h = np.ones((4, 5), np.uint32) if hits is None else hits
    v = np.ones((4, 5), np.uint32) if views is None else views
    return GlobalMap((0.0, 0.0), 0.25, (4, 5), h if grids else None, v if grids else None, np.zeros((0, 2)), np.zeros(0, np.uint32), np.zeros(0, np.uint32), 0)


@pytest.mark.parametrize("kw,match", [
    (dict(minHits=0), "minHits"), (dict(minViews=0), "minViews"), (dict(minHits=1.5), "minHits"), (dict(minViews=True), "minViews"),
    (dict(sigmaCells=0.0), "sigmaCells"), (dict(sigmaCells=np.nan), "sigmaCells"), (dict(sigmaCells=-1.0), "sigmaCells"), (dict(sigmaCells="1"), "sigmaCells"),
    (dict(radiusCells=-1), "radiusCells"), (dict(radiusCells=9), "radiusCells"), (dict(radiusCells=2.0), "radiusCells")])
def test_localizer_arguments_raise_before_the_library(kw, match, monkeypatch):
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match=match):
        _map().localizer(**kw)


def test_a_map_without_grids_or_with_bad_grids_is_refused(monkeypatch):
    from radarslampy_amd import _ffi
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match="grids=False"):
        _map(grids=False).localizer()
    for h, v in ((np.ones((4, 5)), None), (np.ones((4, 6), np.uint32), None), (np.ones(20, np.uint32), np.ones(20, np.uint32)),
                 (-np.ones((4, 5), np.int64), None), (np.zeros((0, 5), np.uint32), np.zeros((0, 5), np.uint32))):
        with pytest.raises(ValueError, match="hits and views"):
            _map(h, v).localizer()
    with pytest.raises(ValueError, match="table"):
        _ffi.map_field_args(np.ones((4, 5), np.uint32), np.ones((4, 5), np.uint32), (0.0, 0.0), 0.25, radius=2, table=np.zeros((3, 3), np.uint8))
    with pytest.raises(ValueError, match="origin"):
        _ffi.map_field_args(np.ones((4, 5), np.uint32), np.ones((4, 5), np.uint32), (0.0, np.inf), 0.25)
    with pytest.raises(ValueError, match="cellM"):
        _ffi.map_field_args(np.ones((4, 5), np.uint32), np.ones((4, 5), np.uint32), (0.0, 0.0), 0.0)


def _localizer():
    """a MapLocalizer that never reached the device"""
    from radarslampy_amd import _ffi
    from radarslampy_amd.Mapping import MapLocalizer
    loc = MapLocalizer.__new__(MapLocalizer)
    loc.origin, loc.cellM, loc.shape = (0.0, 0.0), 0.25, (4, 5)
    loc._field = _ffi.MapField.__new__(_ffi.MapField)     # its checks run; a call that passes them fails on the missing context
    loc._field.ctx = loc._field.h = None
    return loc


CLOUD = np.zeros((5, 2))


@pytest.mark.parametrize("kw,match", [
    (dict(reachM=-1.0), "reachM"), (dict(reachM=np.nan), "reachM"), (dict(reachM=(1.0, 2.0, 3.0)), "reachM"), (dict(reachM=32.25), "reachM"),
    (dict(reachM=(1.0, 40.0)), "reachM"), (dict(reachRad=-0.1), "reachRad"), (dict(reachRad=np.inf), "reachRad"), (dict(stepRad=0.0), "stepRad"),
    (dict(stepRad=-0.01), "stepRad"), (dict(stepRad=np.nan), "stepRad"), (dict(reachRad=6.0, stepRad=0.01), "angles"),
    (dict(priors=(0.0, 0.0)), "priors"), (dict(priors=np.zeros((2, 3))), "priors"), (dict(priors=(np.nan, 0.0, 0.0)), "priors"),
    (dict(priors=(0.0, 2e6, 0.0)), "priors"), (dict(priors=(0.0, 0.0, np.inf)), "priors"), (dict(priors=("a", "b", "c")), "priors"),
    (dict(clouds=np.zeros((5, 3))), "cloud"), (dict(clouds=[np.zeros((8193, 2))]), "8193"), (dict(clouds=[np.full((2, 2), np.nan)]), "coordinate"),
    (dict(clouds=[np.full((2, 2), 2e6)]), "coordinate"), (dict(clouds=[]), "no cloud"), (dict(clouds=[np.zeros((2, 2), object)]), "cloud"),
    (dict(clouds=[CLOUD] * 70000), "queries"), (dict(clouds=[CLOUD] * 200, reachM=32.0, reachRad=0.12, volume=True), "volume")])
def test_match_arguments_raise_before_the_library(kw, match, monkeypatch):
    _no_device(monkeypatch)
    full = {**dict(clouds=[CLOUD], priors=(0.0, 0.0, 0.0)), **kw}
    with pytest.raises(ValueError, match=match):
        _localizer().match(**full)


def test_localize_arguments_raise_before_the_library(monkeypatch):
    from radarslampy_amd import _ffi
    from radarslampy_amd.LoopClosure import LoopDetector
    _no_device(monkeypatch)
    det = LoopDetector.__new__(LoopDetector)
    det.keepClouds = False
    with pytest.raises(ValueError, match="keeps no clouds"):
        det.localize(_localizer())
    for count, idx, match in ((0, None, "empty"), (4, [4], "indices"), (4, [-1], "indices"), (4, [], "indices"), (4, [0.5], "indices")):
        with pytest.raises(ValueError, match=match):
            _ffi.map_match_indices(count, idx)
    assert _ffi.map_match_indices(4, None).tolist() == [3] and _ffi.map_match_indices(4, [[2, 0]]).tolist() == [2, 0]


def test_arguments_that_pass():
    from radarslampy_amd import _ffi
    assert _ffi.map_match_window(0.25) == (25, 0.01, 12, 12) and _ffi.map_match_window(0.5, (3.0, 1.2), 0.0, 0.0) == (1, 0.0, 6, 2)
    assert _ffi.map_match_window(0.25, 32.0, 5.12, 0.01) == (1025, 0.01, 128, 128) and _ffi.map_match_window(0.1, 0.3, 0.03, 0.01)[2:] == (3, 3)
    xy, off = _ffi.map_match_clouds([np.ones((3, 2)), np.zeros((0, 2)), [[1, 2]]])
    assert xy.dtype == np.float64 and xy.shape == (4, 2) and off.dtype == np.int64 and off.tolist() == [0, 3, 3, 4]
    assert _ffi.map_match_clouds(np.ones((3, 2)))[1].tolist() == [0, 3]
    p = _ffi.map_match_priors((1, 2, 3), 2, (3, 0.01, 1, 1))
    assert p.dtype == np.float64 and p.tolist() == [[1.0, 2.0, 3.0]] * 2
    t = _ffi.match_table(np.array([[1.0, 2.0, 0.5], [0.0, 0.0, 0.0]]), np.array([[510, 1, 2, 3, 4, 3], [0, 0, 0, 0, 0, 0]], np.int32))
    assert t["fraction"].tolist() == [0.5, 0.0] and t["found"].tolist() == [True, False] and t["nInside"].tolist() == [3, 0] and t["a"][0] == 3


# ---------------------------------------------------------------------------------------------------------------- the synthetic world
def test_the_definition_localises_held_out_scans_in_the_synthetic_world():
    """Eight scans of StreamWorld(5, per_tile=40), 2 m apart, rendered at their true poses into a map of 0.25 m cells (the global map's
    model); four held-out scans with priors 2 to 3 m per axis and 0.05 to 0.12 rad off, no multiples of the cell or the angle step.
    The bound is a condition, not a measurement: the model's estimate within ONE CELL per axis and ONE ANGLE STEP of the truth (half
    a step of discretisation plus one node), and the best score unique.  Measured with the oracle's peak extraction (printed below,
    recorded in docs/PARITY.md): errors of at most 0.12 m per axis and 0.0037 rad, best score 1.83 to 2.11 times the prior's."""
    from radarslampy_amd import _ffi
    clouds = cases.world_clouds_oracle()
    map_poses = np.array(cases.WORLD_MAP_POSES)
    res = cases.WORLD_CELL_M
    cs = _ffi.map_pose_table(map_poses)
    b, n = map_model.bounds(clouds[:8], map_poses, cs)
    extent = map_model.plan(*b, res)
    r = map_model.render(clouds[:8], map_poses, cs, res, extent)
    table = _ffi.map_field_table(1.0, cases.WORLD_RADIUS)
    F = model.field(r["hits"], r["views"], 1, 1, cases.WORLD_RADIUS, table)
    window = _ffi.map_match_window(res, *(cases.WORLD_WINDOW[k] for k in ("reachM", "reachRad", "stepRad")))
    assert window == (25, 0.01, 12, 12)
    priors = cases.world_priors()
    angles = _ffi.map_match_angles(priors, window[0], window[1])
    for q in range(4):
        truth = np.array(cases.WORLD_QUERY_POSES[q])
        off = priors[q] - truth
        assert np.all((np.abs(off[:2]) >= 2.0) & (np.abs(off[:2]) <= 3.0)) and 0.05 <= abs(off[2]) <= 0.12
        assert np.all(np.abs(off[:2] / res - np.round(off[:2] / res)) > 0.05) and abs(off[2] / 0.01 - round(off[2] / 0.01)) > 0.05
        pose, info, vol = model.match(F, clouds[8 + q], priors[q], angles[q], window[1], res, extent[0], extent[1], window[2], window[3])
        err = pose - truth
        at_prior = int(vol[12, 12, 12])
        print(f"query {q}: {info[4]} points, error {err[0]:+.4f} m, {err[1]:+.4f} m, {err[2]:+.5f} rad; score {info[0]} = {info[0] / at_prior:.2f} x the prior's "
              f"{at_prior}; fraction {info[0] / (255.0 * info[4]):.3f}; best at i, b, a = {info[1:4].tolist()}")
        assert np.count_nonzero(vol == vol.max()) == 1
        assert abs(err[0]) <= res and abs(err[1]) <= res and abs(err[2]) <= window[1]
