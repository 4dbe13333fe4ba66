"""CPU: the motion compensation of the loop database's peak clouds (tests/loop_cloud_motion_model.py) - the model against the oracle's
MotionDistortionSolver.undistort, the library's host-only table against the model, the host conversion, the argument checks of the
Python entries (each must raise before a device is asked for) and what the compensation is worth to the model ICP on three moving
pairs.  No device."""
import ctypes
import types

import numpy as np
import pytest

import icp_cases
import loop_cloud_model as plain
import loop_cloud_motion_cases as cases
import loop_cloud_motion_model as model

RES = 0.0438                                          # the issue's grid: bins of 0.0438 m up to 4095
ROWS = (64, 399, 400, 1020)
VELOCITIES = [(15.0, 3.0, 0.5), (-30.0, 10.0, -1.5), (2.0, -1.0, 0.05), (0.0, 0.0, 1.5), (30.0, -10.0, 0.0)]


def _grid(rows, seed):
    """peaks [theta, r] on every row of a scan, ranges from 1 to 4095 bins (a point AT the sensor has no azimuth for atan2 to find)"""
    rng = np.random.default_rng(seed)
    th = np.concatenate([np.arange(rows), rng.integers(0, rows, 3000)])
    r = np.concatenate([np.full(rows, 4095), rng.integers(1, 4096, 3000)])
    r[:rows:3] = 1
    return np.stack([th, r], axis=1)


# ---------------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("rows", ROWS)
def test_model_is_the_oracle_s_undistort_with_the_time_of_the_row(rows):
    """one ulp at 180 m is 2.8e-14 m and the two computations differ in about ten roundings: 1e-12 m; the row time against atan2 of
    the rounded point: 1e-16 s"""
    import oracle
    from radarslampy_amd import _ffi
    trig = _ffi.polar_cloud_table(rows)
    peaks = _grid(rows, rows)
    xy0 = plain.metres(peaks, *trig, RES)
    tau = model.row_times(rows)[peaks[:, 0]]
    d_tau = np.abs(tau - oracle.MotionDistortionSolver.compute_time_deltas(0.25, xy0)).max()
    worst = 0.0
    for v in VELOCITIES:
        got = model.metres(peaks, *trig, RES, model.table(rows, v))
        want = oracle.MotionDistortionSolver.undistort(np.array(v), xy0, 0.25)[:, :2]
        worst = max(worst, float(np.abs(got - want).max()))
    print(f"rows {rows}: model against undistort {worst:.3g} m, row time against compute_time_deltas {d_tau:.3g} s")
    assert worst <= 1e-12 and d_tau <= 1e-16
    assert model.row_times(rows)[0] == -0.125 and (rows % 2 or model.row_times(rows)[rows // 2] == 0.0)


@pytest.mark.parametrize("rows", ROWS)
def test_zero_velocity_equals_the_plain_model_numerically(rows):
    from radarslampy_amd import _ffi
    trig = _ffi.polar_cloud_table(rows)
    peaks = _grid(rows, 7)
    zero = model.metres(peaks, *trig, RES, model.table(rows, (0.0, 0.0, 0.0)))
    want = plain.metres(peaks, *trig, RES)
    assert np.array_equal(zero, want)                     # ==: a -0.0 may have become +0.0, which is why None is the plain path
    none = model.cloud(peaks, *trig, RES, 512, 1, None)
    assert none[0].tobytes() == plain.cloud(peaks, *trig, RES, 512, 1)[0].tobytes() and none[1] == len(peaks)
    assert np.isnan(model.table(rows, None)).all()


# ---------------------------------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize("rows", ROWS + (1, 65536))
def test_table_is_the_model_s_bit_for_bit(rows):
    from radarslampy_amd import _ffi
    cos, sin = cases.libm()
    vel = VELOCITIES[:2] + [None] if rows > 1020 else VELOCITIES + [None]
    got = _ffi.cloud_motion_table(rows, vel)
    assert got.shape == (len(vel), rows, 4) and got.dtype == np.float64
    for i, v in enumerate(vel):
        assert got[i].tobytes() == model.table(rows, v, cos=cos, sin=sin).tobytes(), (rows, v)
    other = _ffi.cloud_motion_table(rows, np.array(VELOCITIES[1]), period=0.1)
    assert other.shape == (1, rows, 4) and other[0].tobytes() == model.table(rows, VELOCITIES[1], 0.1, cos, sin).tobytes()
    marked = _ffi.cloud_motion_table(rows, np.array([[np.nan, 1.0, 2.0], VELOCITIES[0]]))       # NaN in vx: the ABI's marker
    assert np.isnan(marked[0]).all() and marked[1].tobytes() == got[0].tobytes()


def test_table_symmetry_and_odd_rows():
    from radarslampy_amd import _ffi
    for rows in (64, 400, 1020):
        t = _ffi.cloud_motion_table(rows, VELOCITIES[0])[0]
        a, b = t[1:], t[1:][::-1]                         # t <-> rows - t
        assert np.array_equal(a[:, 0], b[:, 0]) and np.array_equal(a[:, 1:], -b[:, 1:])
        assert t[rows // 2].tolist() == [1.0, 0.0, 0.0, 0.0]
    assert np.all(model.row_times(399) != 0.0)
    t = _ffi.cloud_motion_table(399, (1.0, 1.0, 1.0))[0]
    assert np.all(t[:, 2] != 0.0) and np.all(t[:, 1] != 0.0)


def test_table_refusals():
    from radarslampy_amd import _ffi
    lib = _ffi.load_library()
    v, out = np.array([[1.0, 2.0, 3.0]]), np.zeros((1, 4, 4))
    assert lib.roam_cloud_motion_table(4, 0.25, 1, _ffi._ptr(v), _ffi._ptr(out)) == _ffi.ROAM_OK
    for rows, period, n, vp, op in ((0, 0.25, 1, v, out), (65537, 0.25, 1, v, out), (4, 0.0, 1, v, out), (4, -1.0, 1, v, out),
                                    (4, float("nan"), 1, v, out), (4, float("inf"), 1, v, out), (4, 0.25, 0, v, out), (4, 0.25, 1, None, out),
                                    (4, 0.25, 1, v, None), (4, 0.25, 1, np.array([[1.0, np.nan, 0.0]]), out),
                                    (4, 0.25, 1, np.array([[np.inf, 0.0, 0.0]]), out), (4, 0.25, 1, np.array([[0.0, 0.0, -np.inf]]), out)):
        assert lib.roam_cloud_motion_table(rows, period, n, _ffi._ptr(vp), _ffi._ptr(op)) == _ffi.ROAM_E_ARG, (rows, period, n)
    for args, match in (((0, (1, 2, 3)), "rows"), ((400.0, (1, 2, 3)), "rows"), ((4, None), "velocities"), ((4, (1, 2, 3), 0.0), "period"),
                        ((4, (1, np.inf, 3)), "finite"), ((4, [(1, 2)]), "velocities"), ((4, np.zeros((2, 2))), "velocities")):
        with pytest.raises(ValueError, match=match):
            _ffi.cloud_motion_table(*args)


# ---------------------------------------------------------------------------------------------------------------- the host conversion
@pytest.mark.parametrize("rows", ROWS)
def test_polar_ind_to_local_metres_with_a_velocity(rows):
    from radarslampy_amd import _ffi
    from radarslampy_amd.LoopClosure import polarIndToLocalMetres
    trig = _ffi.polar_cloud_table(rows)
    peaks = _grid(rows, 3)
    worst = 0.0
    for v in VELOCITIES:
        for period in (0.25, 0.1):
            got = polarIndToLocalMetres(peaks, rows, RES, velocity=v, period=period)
            want = model.metres(peaks, *trig, RES, model.table(rows, v, period))
            worst = max(worst, float(np.abs(got - want).max()))
    print(f"rows {rows}: polarIndToLocalMetres(velocity=) against the model {worst:.3g} m")
    assert worst <= 1e-12
    assert polarIndToLocalMetres(peaks, rows, RES, velocity=None).tobytes() == polarIndToLocalMetres(peaks, rows, RES).tobytes()
    assert polarIndToLocalMetres(np.zeros((0, 2), int), rows, RES, velocity=(1, 2, 3)).shape == (0, 2)
    for kw, match in ((dict(velocity=(1, 2)), "velocities"), (dict(velocity=(1, 2, np.nan)), "finite"), (dict(velocity=(1, 2, 3), period=0), "period")):
        with pytest.raises(ValueError, match=match):
            polarIndToLocalMetres(peaks, rows, RES, **kw)


# ---------------------------------------------------------------------------------------------------------------- argument checks
def test_motion_args_shapes():
    from radarslampy_amd import _ffi
    assert _ffi.loop_motion_args(None, "not read", 3) == (None, 0.25)
    v, p = _ffi.loop_motion_args((1, 2, 3), 0.25, 1)
    assert v.dtype == np.float64 and v.flags.c_contiguous and v.tolist() == [[1.0, 2.0, 3.0]] and p == 0.25
    v, _ = _ffi.loop_motion_args([(1, 2, 3), None, np.array([4.0, 5.0, 6.0])], 0.5, 3)
    assert v[0].tolist() == [1, 2, 3] and np.isnan(v[1]).all() and v[2].tolist() == [4, 5, 6]
    v, _ = _ffi.loop_motion_args([None, None, None], 0.25, 3)
    assert np.isnan(v).all()
    src = np.array([[np.nan, 7.0, np.inf], [1.0, 2.0, 3.0]])
    v, _ = _ffi.loop_motion_args(src, 0.25, 2)            # the marker: whatever else the row holds
    assert v is not src and np.isnan(v[0, 0]) and v[1].tolist() == [1, 2, 3]
    for vel, n, match in (((1, 2, 3), 2, "velocities"), ([(1, 2, 3)], 2, "velocities"), (np.zeros((2, 2)), 2, "velocities"),
                          (np.zeros((3, 3)), 2, "velocities"), ([(1, 2, 3), "x"], 2, "velocities"), ([(1, 2, np.inf)], 1, "finite"),
                          ([(np.nan, 2, 3)], 1, "finite"), (np.array([[1.0, np.nan, 0.0]]), 1, "finite"), (np.array([["a", "b", "c"]]), 1, "velocities")):
        with pytest.raises(ValueError, match=match):
            _ffi.loop_motion_args(vel, 0.25, n)
    for period in (0, -0.25, np.nan, np.inf, "0.25", None, True):
        with pytest.raises(ValueError, match="period"):
            _ffi.loop_motion_args((1, 2, 3), period, 1)
    with pytest.raises(ValueError, match="keeps no clouds"):
        _ffi.loop_motion_args((1, 2, 3), 0.25, 1, keeps_clouds=False)
    # |v| period / 2 plus the largest range within 1e6 m
    far = (8e6 - 8 * 3768 * 0.0432, 0.0, 0.0)
    assert _ffi.loop_motion_args(far, 0.25, 1, True, 3768, 0.0432)[0][0, 0] == far[0]
    for vel in ((8.1e6, 0.0, 0.0), (0.0, -8.1e6, 100.0), (6e6, 6e6, 0.0)):
        with pytest.raises(ValueError, match="beyond"):
            _ffi.loop_motion_args(vel, 0.25, 1, True, 3768, 0.0432)
    assert _ffi.loop_motion_args((8.1e6, 0, 0), 0.125, 1, True, 3768, 0.0432)[1] == 0.125


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library's {name} was called")


def _offline_db(keeps_clouds=True):
    """a LoopDb that never reached the device, and whose every library call fails the test"""
    from radarslampy_amd import _ffi
    db = _ffi.LoopDb.__new__(_ffi.LoopDb)
    db.h = None
    db.ctx = types.SimpleNamespace(lib=_NoLibrary(), h=None, check=lambda rc: None)
    db.capacity, db.sectors, db.rings = 8, 16, 8
    db.cloud_rows, db.max_points, db.range_resolution_m = (64, 512, 0.0432) if keeps_clouds else (None, None, None)
    db.offsets_m = None
    return db


BAD_ADDS = [(dict(velocities=(1, 2, 3)), False, "keeps no clouds"), (dict(velocities=(1, 2, 3), period=0.0), True, "period"),
            (dict(velocities=(1, 2, 3), period=float("nan")), True, "period"), (dict(velocities=(1, np.inf, 3)), True, "finite"),
            (dict(velocities=[(np.nan, 0, 0)]), True, "finite"), (dict(velocities=(8.1e6, 0, 0)), True, "beyond"),
            (dict(velocities=[(1, 2, 3), None]), True, "velocities")]


@pytest.mark.parametrize("kw,keeps,match", BAD_ADDS)
def test_adds_refuse_before_the_library_is_called(kw, keeps, match, monkeypatch):
    from radarslampy_amd import _ffi
    from radarslampy_amd.engine import Engine
    from radarslampy_amd.LoopClosure import LoopDetector

    def no_device(*a, **k):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(_ffi, "default_context", no_device)
    monkeypatch.setattr(_ffi, "Context", no_device)
    db = _offline_db(keeps)
    img = np.zeros((64, 100), np.float32)
    with pytest.raises(ValueError, match=match):
        db.add_f32(img, **kw)
    det = LoopDetector.__new__(LoopDetector)
    det.db, det.clip_px, det.floor, det.keepClouds = db, None, 0.0, keeps
    with pytest.raises(ValueError, match=match):
        det.add(img, velocity=kw["velocities"], **{k: v for k, v in kw.items() if k == "period"})
    eng = Engine.__new__(Engine)
    eng.ctx, eng.lib, eng.pool_scans, eng.rows = db.ctx, db.ctx.lib, 4, 64
    eng.cfg = types.SimpleNamespace(clip=100)
    with pytest.raises(ValueError, match=match):
        eng.loop_db_add(db, [2], floor_code=0, **kw)
    with pytest.raises(ValueError, match=match):
        eng.time_loop_cloud(db, [2], **kw)
    for call in (lambda: db.add_f32(img), lambda: eng.loop_db_add(db, [2], floor_code=0), lambda: eng.time_loop_cloud(db, [2])):
        with pytest.raises(AssertionError, match="was called"):      # without velocities the arguments pass and the library is reached
            call()


def test_the_library_exports_the_entries_and_refuses_a_null_context():
    from radarslampy_amd import _ffi
    lib = _ffi.load_library()
    for name in ("roam_cloud_motion_table", "roam_loop_db_add_f32_motion", "roam_engine_loop_db_add_motion", "roam_engine_time_loop_cloud_motion"):
        assert hasattr(lib, name) and name in _ffi.ABI_SYMBOLS, name
    v = np.array([[1.0, 2.0, 3.0]])
    assert lib.roam_loop_db_add_f32_motion(None, None, None, 1, 8, 8, 8, 64, 0, 0.0, _ffi._ptr(v), 0.25, None) == _ffi.ROAM_E_ARG
    assert lib.roam_engine_loop_db_add_motion(None, None, 1, None, 0, 0, _ffi._ptr(v), 0.25, None) == _ffi.ROAM_E_ARG
    ms = ctypes.c_float()
    assert lib.roam_engine_time_loop_cloud_motion(None, None, 1, None, _ffi._ptr(v), 0.25, 1, ctypes.byref(ms), ctypes.byref(ms)) == _ffi.ROAM_E_ARG


# ---------------------------------------------------------------------------------------------------------------- closeLoops
def test_close_loops_undistorts_the_clouds_it_aligns(monkeypatch):
    from radarslampy_amd import LoopClosure, _ffi
    rows = 64
    kfs = [types.SimpleNamespace(pose=np.zeros(3), velocity=np.array(VELOCITIES[k]), pointCloud=_grid(rows, k)[:200 + k]) for k in range(3)]
    seen = []

    def align(pairs, init, opts):
        seen.append(pairs)
        stats = np.zeros(len(pairs), _ffi.ICP_STATS)
        stats["status"] = _ffi.ICP_FEW_PAIRS
        return np.asarray(init, np.float64), stats
    monkeypatch.setattr(LoopClosure, "_align_batch", align)
    monkeypatch.setattr(LoopClosure, "_optimise", lambda keyframes, edges, table, *a: (None, edges, table))
    class Det:
        keepClouds = False

        def __len__(self):
            return 3

        def query(self, idx):                            # keyframe 1 -> candidate 0, keyframe 2 -> candidate 1
            return np.array([[-1], [0], [1]], np.int32), np.zeros((3, 1)), np.full((3, 1), 0.1)
    det = Det()
    trig = _ffi.polar_cloud_table(rows)
    for undistort, period in ((True, 0.25), (True, 0.1), (False, 0.25)):
        seen.clear()
        _, edges, table = LoopClosure.closeLoops(kfs, det, rows=rows, rangeResolutionM=RES, undistort=undistort, period=period)
        assert edges == [] and len(table) == 2 and len(seen) == 1 and len(seen[0]) == 2
        for (src, dst), (q, c) in zip(seen[0], ((1, 0), (2, 1))):
            for got, k in ((src, q), (dst, c)):
                tab = model.table(rows, kfs[k].velocity, period) if undistort else None
                want = model.metres(kfs[k].pointCloud, *trig, RES, tab)
                assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12
                assert undistort == (np.abs(got - plain.metres(kfs[k].pointCloud, *trig, RES)).max() > 0.1)


# ---------------------------------------------------------------------------------------------------------------- what it is worth
def test_compensated_clouds_give_the_model_icp_the_true_edge():
    """three pairs of one place seen twice while moving (loop_cloud_motion_cases): from the raw model clouds the model ICP reports
    success more than TRUTH_CAP_M = 0.2 m off the truth (0.46 to 1.43 m measured), from the compensated ones it is within 0.2 m and
    0.04 rad (0.027 to 0.063 m measured)"""
    raw, comp = cases.numpy_model()
    truth = cases.truth()
    for p in range(len(cases.MOVING_PAIRS)):
        (r_m, r_rad), (c_m, c_rad) = icp_cases.pose_error(raw[p][0], truth), icp_cases.pose_error(comp[p][0], truth)
        print(f"pair {p}: raw {r_m:.4f} m, {r_rad:.5f} rad (status {raw[p][1]['status']}, rms {raw[p][1]['rms']:.3f} m); "
              f"compensated {c_m:.4f} m, {c_rad:.5f} rad (status {comp[p][1]['status']}, rms {comp[p][1]['rms']:.3f} m)")
        assert r_m > icp_cases.TRUTH_CAP_M
        assert c_m < icp_cases.TRUTH_CAP_M and c_rad < icp_cases.TRUTH_CAP_RAD
