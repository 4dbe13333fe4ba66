"""GPU (-m gpu): getPointCloudPolarInd(polarImage, peakDistance, peakProminence) on the MI355X (peaks_cond.hip) - the float32
drop-in and the fused u8 record path against every case of peaks_cond.npz (the reference under NumPy 1.22.3's argsort), against
live scipy on tie-heavy random rows, and against the plain kernel where the conditions cannot remove a peak."""
import os

import numpy as np
import pytest

import peaks_cond_cases as pc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ctx():
    from radarslampy_amd import _ffi
    c = _ffi.default_context(0)
    assert "gfx950" in c.device_info()["arch"]
    return c


@pytest.fixture(scope="module")
def cases():
    return pc.load_cases(np.load(os.path.join(GOLDEN, "peaks_cond.npz")), GOLDEN)


def _record(u8, off, stride):
    rng = np.random.default_rng(u8.shape[1])
    rec = rng.integers(0, 256, size=(u8.shape[0], stride), dtype=np.uint8)
    rec[:, off:off + u8.shape[1]] = u8
    return rec


def test_f32_dropin_matches_every_case(ctx, cases):
    from radarslampy_amd.getPointCloud import getPointCloudPolarInd
    for name, u8, f32, d, p, want in cases:
        got = getPointCloudPolarInd(f32, peakDistance=d, peakProminence=p)
        assert got.dtype == np.int64 and np.array_equal(got, want), (name, d, p)


def test_fused_u8_path_matches_every_case(ctx, cases):
    from radarslampy_amd.getPointCloud import getPointCloudFromRecord
    for name, u8, f32, d, p, want in cases:
        if u8 is None:
            continue
        cols = u8.shape[1]
        got = getPointCloudFromRecord(u8, 0, cols, peakDistance=d, peakProminence=p)
        assert np.array_equal(got, want), (name, d, p, "payload_off 0")
        if cols == 2025:                                             # the Oxford record: 11 metadata bytes + 3768 power bins
            got = getPointCloudFromRecord(_record(u8, 11, 3779), 11, 2025, peakDistance=d, peakProminence=p)
            assert np.array_equal(got, want), (name, d, p, "Oxford layout")


def test_live_scipy_on_tie_heavy_random_rows(ctx):
    pytest.importorskip("scipy")
    rng = np.random.default_rng(2026)
    for it in range(24):
        rows, cols = int(rng.integers(1, 40)), int(rng.integers(3, 700))
        u8 = rng.integers(0, int(rng.choice([2, 3, 5, 40, 256])), (rows, cols)).astype(np.uint8)
        d = [None, float(rng.uniform(1, 4)), int(rng.integers(2, 40)), float(rng.uniform(1, 200))][it % 4]
        p = [None, float(rng.uniform(0, 0.02)), (None, float(rng.uniform(0, 0.05))),
             (float(rng.uniform(0, 0.01)), float(rng.uniform(0.01, 0.5)))][(it // 4) % 4]
        if d is None and p is None:
            p = 0.004
        want = pc.truth(pc.decode(u8), d, p)
        got = ctx.peaks_record_u8(u8, payload_off=0, clip=cols, distance=d, prominence=p)
        assert np.array_equal(got, want), (it, rows, cols, d, p)
        f32 = (rng.integers(0, 6, (rows, cols)) / 5).astype(np.float32)
        want = pc.truth(f32, d, p)
        got = ctx.peaks_polar_f32(f32, distance=d, prominence=p)
        assert np.array_equal(got, want), (it, "f32", rows, cols, d, p)


def test_no_op_conditions_equal_the_plain_kernel(ctx, golden):
    g = golden("peaks")
    for i in (0, 1):
        u8 = g[f"real{i}_u8"]
        plain = ctx.peaks_record_u8(u8, payload_off=0, clip=u8.shape[1])
        assert np.array_equal(plain, g[f"real{i}_out"])
        got = ctx.peaks_record_u8(u8, payload_off=0, clip=u8.shape[1], distance=1.7, prominence=0)
        assert np.array_equal(got, plain), f"real{i} u8"
        got = ctx.peaks_polar_f32(pc.decode(u8), distance=1.7, prominence=0)
        assert np.array_equal(got, plain), f"real{i} f32"


def test_widest_and_narrowest_rows(ctx):
    pytest.importorskip("scipy")
    a = pc.alt4096_u8()
    for d, p in [(None, 0), (2, None), (3, None), (4096, None), (7, 0.001), (None, (0.005, None))]:
        want = pc.truth(pc.decode(a), d, p)
        assert np.array_equal(ctx.peaks_record_u8(a, payload_off=0, clip=4096, distance=d, prominence=p), want), (d, p)
        assert np.array_equal(ctx.peaks_polar_f32(pc.decode(a), distance=d, prominence=p), want), (d, p)
    three = np.array([[0, 5, 0], [5, 0, 5], [1, 1, 1], [0, 1, 1], [3, 4, 3]], np.uint8)
    for d, p in [(1, None), (3, 0), (None, 0.01), (5, (None, 0.001))]:
        want = pc.truth(pc.decode(three), d, p)
        assert np.array_equal(ctx.peaks_record_u8(three, payload_off=0, clip=3, distance=d, prominence=p), want), (d, p)
        assert np.array_equal(ctx.peaks_polar_f32(pc.decode(three), distance=d, prominence=p), want), (d, p)


def test_bad_distance_is_an_argument_error(ctx):
    from radarslampy_amd import _ffi
    import ctypes
    img = np.zeros((2, 16), np.float32)
    out = np.empty((16, 2), np.int32)
    n = ctypes.c_int64(0)
    rc = ctx.lib.roam_peaks_polar_f32_cond(ctx.h, img.ctypes.data, 2, 16, 0.5, float("nan"), float("nan"), out.ctypes.data, 16,
                                           ctypes.byref(n))
    assert rc == _ffi.ROAM_E_ARG
