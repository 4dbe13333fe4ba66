"""CPU (-m "not gpu"): the contract of getPointCloudPolarInd(polarImage, peakDistance, peakProminence) - find_peaks' distance /
prominence conditions - without a GPU: the fixtures against live scipy with NumPy 1.22.3's argsort, why that argsort matters,
the drop-in's argument checks (raised before any device call) and the two new C-ABI symbols."""
import ctypes
import os

import numpy as np
import pytest

import peaks_cond_cases as pc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def cases():
    return pc.load_cases(np.load(os.path.join(GOLDEN, "peaks_cond.npz")), GOLDEN)


def test_fixture_covers_the_grid(cases):
    names = {c[0] for c in cases}
    assert {"real0_u8", "real1_u8", "hand_u8", "hand_f32", "alt4096_u8"} <= names
    assert {c[3] for c in cases} >= {1.7, 3.0, 5.0, 10.5, 20.0, 4096.0}
    assert any(isinstance(c[4], tuple) and c[4][0] is None for c in cases)
    assert any(len(c[5]) == 0 for c in cases)                        # conditions that remove every peak
    assert all(c[2].shape[1] == 4096 for c in cases if c[0] == "alt4096_u8")


def test_live_scipy_with_numpy122_argsort_reproduces_every_case(cases):
    pytest.importorskip("scipy")
    for name, u8, f32, d, p, want in cases:
        got = pc.truth(f32, d, p)
        assert np.array_equal(got, want), (name, d, p)


def test_tie_order_is_material(cases):
    """NumPy >= 2's own argsort orders equal heights differently: the fixtures would not hold with it"""
    pytest.importorskip("scipy")
    differ = [(name, d, p) for name, u8, f32, d, p, want in cases
              if name.startswith("real") and d is not None and d > 2 and not np.array_equal(pc.truth(f32, d, p, numpy122=False), want)]
    assert differ


def test_distance_up_to_two_and_prominence_zero_change_nothing(cases):
    """two candidates are never adjacent, every candidate has a prominence > 0: (1.7, 0) is the plain detection"""
    pytest.importorskip("scipy")
    plain = {name: pc.truth(f32) for name, u8, f32, d, p, want in cases if name.startswith("real")}
    for name, u8, f32, d, p, want in cases:
        if name.startswith("real") and d in (None, 1.7) and p in (None, 0) and (d, p) != (None, None):
            assert np.array_equal(want, plain[name]), (name, d, p)


def test_dropin_argument_errors_need_no_gpu():
    from radarslampy_amd import getPointCloud
    img = np.zeros((4, 64), np.float32)
    with pytest.raises(ValueError, match="distance"):
        getPointCloud.getPointCloudPolarInd(img, peakDistance=0.5)
    with pytest.raises(ValueError, match="distance"):
        getPointCloud.getPointCloudFromRecord(np.zeros((4, 64), np.uint8), 0, 64, peakDistance=0.5)
    with pytest.raises(NotImplementedError):
        getPointCloud.getPointCloudPolarInd(img, peakProminence=np.full(64, 0.1))
    with pytest.raises(NotImplementedError):
        getPointCloud.getPointCloudPolarInd(img, peakProminence=(np.zeros(64), None))


def test_condition_unpacking_follows_scipy():
    from radarslampy_amd._ffi import peak_conditions
    d, lo, hi = peak_conditions(3)
    assert d == 3.0 and np.isnan(lo) and np.isnan(hi)
    d, lo, hi = peak_conditions(None, 0.1)
    assert d == 0.0 and lo == 0.1 and np.isnan(hi)
    d, lo, hi = peak_conditions(None, (None, 0.05))
    assert np.isnan(lo) and hi == 0.05
    assert peak_conditions(1, np.array([0.02, 0.2]))[1:] == (0.02, 0.2)      # a 2-element array unpacks like a tuple in scipy
    d, lo, hi = peak_conditions(None, (None, None))
    assert np.isnan(lo) and np.isnan(hi)


def test_new_symbols_are_exported():
    from radarslampy_amd import _ffi
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for s in ("roam_peaks_polar_f32_cond", "roam_peaks_record_u8_cond"):
        assert hasattr(lib, s) and s in _ffi.ABI_SYMBOLS, s


def test_new_entry_points_check_the_context_first():
    from radarslampy_amd import _ffi
    lib = _ffi.load_library()
    n = ctypes.c_int64(0)
    assert lib.roam_peaks_polar_f32_cond(None, None, 1, 8, 3.0, float("nan"), float("nan"), None, 0, ctypes.byref(n)) == _ffi.ROAM_E_ARG
    assert lib.roam_peaks_record_u8_cond(None, None, 1, 8, 0, 8, 0.0, 0.1, float("nan"), None, 0, ctypes.byref(n)) == _ffi.ROAM_E_ARG
