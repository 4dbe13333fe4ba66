"""CPU (-m "not gpu"): the seeded tracker's C entries exist, and the Python argument errors are raised without a device."""
import ctypes

import numpy as np
import pytest


def test_new_symbols_are_exported_and_declared():
    from radarslampy_amd import _ffi
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for s in ("roam_klt_track_u8_flow", "roam_klt_track_f32_flow", "roam_engine_set_motion_prior"):
        assert hasattr(lib, s) and s in _ffi.ABI_SYMBOLS, s
    assert len(_ffi._SIGS["roam_klt_track_u8_flow"][1]) == len(_ffi._SIGS["roam_klt_track_u8"][1]) + 1
    lib = _ffi.load_library()
    assert lib.roam_engine_set_motion_prior(None, None, None) == _ffi.ROAM_E_ARG
    assert lib.roam_klt_track_u8_flow(None, None, None, 16, 16, None, None, 0, None, None, None) == _ffi.ROAM_E_ARG


def test_klt_flow_argument_errors_need_no_device():
    from radarslampy_amd import _ffi
    pts = np.zeros((5, 2), np.float32)
    p, g = _ffi.klt_flow_args(pts, None)
    assert g is None and p.shape == (5, 2)
    p, g = _ffi.klt_flow_args(pts, pts + 3.0)
    assert g.dtype == np.float32 and g.flags.c_contiguous
    for bad in (np.zeros((4, 2)), np.zeros((5, 3)), np.zeros(10)):
        with pytest.raises(ValueError):
            _ffi.klt_flow_args(pts, bad)
    for v in (np.nan, np.inf, -np.inf, 2.0 ** 20 + 1, -2.0 ** 21):
        g = pts.copy()
        g[3, 1] = v
        with pytest.raises(ValueError):
            _ffi.klt_flow_args(pts, g)
    g = pts.copy()
    g[0, 0] = 2.0 ** 20
    _ffi.klt_flow_args(pts, g)          # the bound itself is allowed
    # the checks run before the context is asked for anything: a stand-in without a library
    class NoDevice(_ffi.Context):
        def __init__(self):
            pass
    with pytest.raises(ValueError):
        NoDevice().klt_track(np.zeros((16, 16), np.uint8), np.zeros((16, 16), np.uint8), pts, np.full((5, 2), np.nan))


def test_motion_prior_argument_errors_need_no_device():
    from radarslampy_amd import _ffi
    eye = np.tile(np.float32([[1, 0, 0], [0, 1, 0]]), (3, 1, 1))
    a, u = _ffi.motion_prior_args(eye, None, 3)
    assert a.shape == (3, 6) and a.dtype == np.float32 and u is None
    a, u = _ffi.motion_prior_args(eye.reshape(3, 6), [0, 2, 0], 3)
    assert u.dtype == np.uint8 and u.tolist() == [0, 1, 0]
    for bad in (eye[:2], eye.reshape(3, 3, 2), np.zeros(18)):
        with pytest.raises(ValueError):
            _ffi.motion_prior_args(bad, None, 3)
    with pytest.raises(ValueError):
        _ffi.motion_prior_args(eye, [1, 1], 3)
    for idx, v in (((0, 0, 0), np.nan), ((1, 1, 2), np.inf), ((2, 0, 1), 65.0), ((0, 1, 2), 2.0 ** 20 + 1)):
        m = eye.copy()
        m[idx] = v
        with pytest.raises(ValueError):
            _ffi.motion_prior_args(m, None, 3)


def test_tracker_signatures_keep_the_reference_call():
    import inspect
    from radarslampy_amd import FMT, Tracker, getTransformKLT
    from radarslampy_amd.engine import Engine
    sig = inspect.signature(getTransformKLT.getTrackedPointsKLT)
    assert list(sig.parameters) == ["srcImg", "targetImg", "blobCoordSrc", "initialFlow"] and sig.parameters["initialFlow"].default is None
    assert inspect.signature(FMT.flowPriorFromFMT).parameters["cols"].default == 2025
    assert callable(Engine.set_motion_prior) and callable(Tracker.flowFromPrior)
    assert "initialFlow" in inspect.signature(Tracker.getTrackedPointsKLT).parameters
    with pytest.raises(ValueError):
        getTransformKLT.getTrackedPointsKLT(None, None, np.zeros((70, 2)), initialFlow=np.zeros((69, 2)))
