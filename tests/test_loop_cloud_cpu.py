"""CPU: the loop database's peak-cloud store (tests/loop_cloud_model.py) and the argument checks of its Python entries.  No device: the
table entry is host code, and every check here must raise before a device is asked for."""
import ctypes
import os

import numpy as np
import pytest

import loop_cloud_model as model

ULP_OF_ONE = 2.0 ** -52


@pytest.mark.parametrize("rows", [64, 399, 400, 1020, 65536])
def test_table_is_libm_of_the_numpy_angles(rows):
    """|cos| and |sin| are at most 1, so a correctly rounded result and a faithfully rounded one differ by at most one ulp of 1.0"""
    from radarslampy_amd import _ffi
    c, s = _ffi.polar_cloud_table(rows)
    phi = 2.0 * np.pi * np.arange(rows, dtype=np.float64) / rows
    dc, ds = np.abs(c - np.cos(phi)), np.abs(s - np.sin(phi))
    print(f"rows {rows}: {np.count_nonzero(dc)} cos and {np.count_nonzero(ds)} sin entries differ from NumPy's, largest {max(dc.max(), ds.max()):.3g}")
    assert c.dtype == np.float64 and c.shape == s.shape == (rows,)
    assert dc.max() <= ULP_OF_ONE and ds.max() <= ULP_OF_ONE
    assert c[0] == 1.0 and s[0] == 0.0


def test_table_refuses_rows_outside_the_limits():
    from radarslampy_amd import _ffi
    lib = _ffi.load_library()
    buf = np.zeros(4)
    for rows in (0, -1, 65537):
        assert lib.roam_polar_cloud_table(rows, _ffi._ptr(buf), _ffi._ptr(buf)) == _ffi.ROAM_E_ARG
        with pytest.raises(ValueError, match="rows"):
            _ffi.polar_cloud_table(rows)
    assert lib.roam_polar_cloud_table(4, None, _ffi._ptr(buf)) == _ffi.ROAM_E_ARG
    with pytest.raises(ValueError, match="rows"):
        _ffi.polar_cloud_table(400.0)


def test_model_agrees_with_polar_ind_to_local_metres():
    from radarslampy_amd import _ffi
    from radarslampy_amd.LoopClosure import polarIndToLocalMetres
    from radarslampy_amd.parseData import RANGE_RESOLUTION_M
    rng = np.random.default_rng(11)
    for rows, cols in ((400, 3768), (399, 497), (64, 1000)):
        peaks = np.stack([rng.integers(0, rows, 5000), rng.integers(0, cols, 5000)], axis=1)
        peaks[:4] = [[0, 0], [rows - 1, cols - 1], [0, cols - 1], [rows - 1, 0]]
        got = model.metres(peaks, *_ffi.polar_cloud_table(rows), RANGE_RESOLUTION_M)
        want = polarIndToLocalMetres(peaks, rows)
        bound = 4 * ULP_OF_ONE * peaks[:, 1:2] * RANGE_RESOLUTION_M
        d = np.abs(got - want)
        print(f"rows {rows}: the model and polarIndToLocalMetres differ by at most {d.max():.3g} m on {np.count_nonzero(d)} coordinates")
        assert got.dtype == np.float64 and np.all(d <= bound)


SELECT_CASES = [(0, 8, 1), (1, 8, 1), (8, 8, 1), (9, 8, 1), (16, 8, 1), (17, 8, 1), (17, 8, 3), (1680, 512, 1), (1680, 2048, 4), (8193, 8192, 1)]


@pytest.mark.parametrize("n,max_points,stride", SELECT_CASES)
def test_selection_rule(n, max_points, stride):
    idx = model.select(n, max_points, stride)
    st = model.step(n, max_points, stride)
    assert st >= stride and st >= 1
    assert len(idx) == -(-n // st) and len(idx) <= max_points
    if n:
        assert idx[0] == 0 and idx[-1] < n and n - idx[-1] <= st                 # from the first peak to the last stretch
        assert np.all(np.diff(idx) == st)
    # the smallest step that fits: one less (where the stride allows it) would overflow the slot
    if st > stride:
        assert -(-n // (st - 1)) > max_points
    expect = {(9, 8, 1): 2, (16, 8, 1): 2, (17, 8, 1): 3, (17, 8, 3): 3, (1680, 512, 1): 4, (1680, 2048, 4): 4, (8193, 8192, 1): 2}
    assert st == expect.get((n, max_points, stride), 1)
    pk = np.stack([np.arange(n) % 7, np.arange(n)], axis=1)
    xy, full = model.cloud(pk, np.ones(7), np.zeros(7), 0.5, max_points, stride)
    assert full == n and xy.shape == (len(idx), 2) and np.array_equal(xy[:, 0], 0.5 * idx) and not xy[:, 1].any()


def _no_device(monkeypatch):
    from radarslampy_amd import _ffi

    def no_device(*a, **k):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(_ffi, "default_context", no_device)
    monkeypatch.setattr(_ffi, "Context", no_device)


@pytest.mark.parametrize("kw,match", [
    (dict(rows=None), "rows"), (dict(rows=0), "rows"), (dict(rows=65537), "rows"), (dict(rows=400.0), "rows"), (dict(rows=True), "rows"),
    (dict(rows=400, maxPoints=0), "max_points"), (dict(rows=400, maxPoints=8193), "max_points"), (dict(rows=400, maxPoints=2.5), "max_points"),
    (dict(rows=400, pointStride=0), "point_stride"), (dict(rows=400, pointStride=1.0), "point_stride"),
    (dict(rows=400, rangeResolutionM=0.0), "range_resolution_m"), (dict(rows=400, rangeResolutionM=float("nan")), "range_resolution_m"),
    (dict(rows=400, rangeResolutionM=float("inf")), "range_resolution_m"), (dict(rows=400, rangeResolutionM="1"), "range_resolution_m"),
    (dict(rows=400, capacity=16001), "capacity")])
def test_detector_arguments_raise_before_a_device_is_asked_for(kw, match, monkeypatch):
    from radarslampy_amd.LoopClosure import LoopDetector
    _no_device(monkeypatch)
    kw = dict(kw)
    capacity = kw.pop("capacity", 16)
    with pytest.raises(ValueError, match=match):
        LoopDetector(capacity, keepClouds=True, **kw)


def test_capacity_limit_is_the_database_s_2000_mib():
    from radarslampy_amd import _ffi
    assert _ffi.loop_cloud_args(16000, 400, 8192, 1, 0.0432) == (400, 8192, 1, 0.0432)      # 16000 x 8192 x 16 = 2000 MiB exactly
    with pytest.raises(ValueError, match="capacity"):
        _ffi.loop_cloud_args(16001, 400, 8192, 1, 0.0432)


def test_cloud_and_pair_arguments():
    from radarslampy_amd import _ffi
    for bad, match in ((np.zeros((3, 3)), r"\(n, 2\)"), (np.zeros((9, 2)), "max_points"), ([[0.0, np.nan]], "finite"), ([[2e6, 0.0]], "finite"),
                       (np.array([["a", "b"]]), "numbers")):
        with pytest.raises(ValueError, match=match):
            _ffi.loop_cloud_points(bad, 8)
    a = _ffi.loop_cloud_points([[1, 2], [3, 4]], 8)
    assert a.dtype == np.float64 and a.flags.c_contiguous and a.tolist() == [[1.0, 2.0], [3.0, 4.0]]
    assert _ffi.loop_cloud_points([], 8).shape == (0, 2)
    for args, match in ((([0], [4], None), "indices"), (([-1], [0], None), "indices"), (([0, 1], [0], None), "length"), (([], [], None), "length"),
                        (([0], [1], [0.0, 0.0]), "init"), (([0], [1], [np.inf, 0.0, 0.0]), "pose"), (([0], [1], [0.0, 2e6, 0.0]), "pose")):
        with pytest.raises(ValueError, match=match):
            _ffi.loop_verify_args(4, *args)
    si, di, x0 = _ffi.loop_verify_args(4, [0, 3], [1, 1], (0.5, 1, 2))
    assert si.dtype == di.dtype == np.int32 and x0.shape == (2, 3) and np.array_equal(x0[1], [0.5, 1, 2])


def test_methods_of_a_database_without_clouds_raise_before_the_library(monkeypatch):
    """a LoopDb object that never reached the device: every cloud method refuses on its own state"""
    from radarslampy_amd import _ffi
    db = _ffi.LoopDb.__new__(_ffi.LoopDb)
    db.h = db.ctx = None
    db.cloud_rows = db.max_points = None
    for call in (lambda: db.set_cloud(0, np.zeros((1, 2))), lambda: db.get_cloud(0), lambda: db.cloud_counts(), lambda: db.verify([0], [0]),
                 lambda: db.query_verify([0], [0]), lambda: db.time_verify([0], [0])):
        with pytest.raises(ValueError, match="keeps no clouds"):
            call()


def test_close_loops_and_add_descriptors_refuse_mismatched_clouds(monkeypatch):
    from radarslampy_amd.LoopClosure import LoopDetector
    det = LoopDetector.__new__(LoopDetector)
    det.keepClouds = False
    with pytest.raises(ValueError, match="keeps none"):
        det.addDescriptors(np.zeros((60, 20), np.float32), clouds=[np.zeros((1, 2))])


def test_the_library_exports_the_entries_and_refuses_a_null_context():
    from radarslampy_amd import _ffi
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    names = ("roam_polar_cloud_table", "roam_loop_db_keep_clouds", "roam_loop_db_set_cloud", "roam_loop_db_get_cloud", "roam_loop_db_cloud_counts",
             "roam_loop_db_verify", "roam_loop_db_query_verify", "roam_engine_time_loop_cloud", "roam_time_loop_db_verify")
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "roam_abi.h")).read()
    for name in names:
        assert hasattr(lib, name), name
        assert name in _ffi.ABI_SYMBOLS and f" {name}(" in txt
    lib = _ffi.load_library()
    assert lib.roam_loop_db_keep_clouds(None, None, 400, 8192, 1, 0.0432) == _ffi.ROAM_E_ARG
    assert lib.roam_loop_db_set_cloud(None, None, 0, None, 0) == _ffi.ROAM_E_ARG
    assert lib.roam_loop_db_get_cloud(None, None, 0, None, 0, None, None) == _ffi.ROAM_E_ARG
    assert lib.roam_loop_db_cloud_counts(None, 0, 0, None, None) == _ffi.ROAM_E_ARG
    assert lib.roam_loop_db_verify(None, None, 1, None, None, None, None, None, None) == _ffi.ROAM_E_ARG
    assert lib.roam_loop_db_query_verify(None, None, 1, None, None, 1, 1.0, None, None, None, None, None, None) == _ffi.ROAM_E_ARG
    ms = ctypes.c_float()
    assert lib.roam_time_loop_db_verify(None, None, 1, None, None, None, None, 1, ctypes.byref(ms)) == _ffi.ROAM_E_ARG
    assert lib.roam_engine_time_loop_cloud(None, None, 1, None, 1, ctypes.byref(ms), ctypes.byref(ms)) == _ffi.ROAM_E_ARG
