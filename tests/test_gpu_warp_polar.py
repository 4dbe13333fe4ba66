"""GPU (-m gpu): cv2.warpPolar in all four modes (warppolar.hip, roam_warp_polar_f32) bit for bit against the NumPy model of
tests/warp_polar_model.py, and against the oracle's C where it covers the mode (inverse linear, forward semilog,
convertPolarImgToLogPolar); at the live geometry against warp.hip's roam_polar_to_cart_f32 on the 11 real scans of
tests/golden/tiny_track.npz.  Through parseData: every downsampleFactor / logPolarMode of convertPolarImageToCartesian,
convertCartesianImageToPolar with OpenCV's default and explicit sizes, the reference FMT script's round trip, strided and batched
input, getCartImageFromImgPaths."""
import ctypes as C

import numpy as np
import pytest

import oracle
import warp_polar_model as M
from radarslampy_amd import parseData

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from radarslampy_amd import _ffi
    c = _ffi.default_context()
    assert "gfx950" in c.device_info()["arch"]
    return c


@pytest.fixture(scope="module")
def scans(golden):
    return golden("tiny_track")["payload"].astype(np.float32) / np.float32(255.)


_plans = {}


def _inverse_plan(rows, cols, df, log):
    R = cols // df if df > 1 else cols
    key = ("inv", rows, cols, R, log)
    if key not in _plans:
        _plans[key] = M.polar_to_cart_plan(rows, cols, df, log)
    return _plans[key]


def _forward_plan(W, ds, log):
    key = ("fwd", W, ds, log)
    if key not in _plans:
        mx, my = M.forward_maps(ds[0], ds[1], W / 2, W / 2, W / 2, log)
        _plans[key] = M.Remap(mx, my, W, W, False)
    return _plans[key]


def _oracle_inverse(img, R):
    img = np.ascontiguousarray(img, np.float32)
    rows, cols = img.shape
    out = np.empty((2 * R, 2 * R), np.float32)
    oracle.lib().oracle_warp_polar_inverse(oracle._p(img, C.c_float), rows, cols, C.c_int64(cols), 2 * R, 2 * R, C.c_float(R), C.c_float(R),
                                           C.c_double(R), oracle._p(out, C.c_float))
    return out


def _oracle_forward_log(img, ds):
    img = np.ascontiguousarray(img, np.float32)
    W = img.shape[0]
    out = np.empty((ds[1], ds[0]), np.float32)
    oracle.lib().oracle_warp_polar_forward_log(oracle._p(img, C.c_float), W, W, ds[0], ds[1], C.c_float(W / 2), C.c_float(W / 2),
                                               C.c_double(W / 2), oracle._p(out, C.c_float))
    return out


@pytest.mark.timeout(300)
def test_live_geometry_equals_polar_to_cart_on_real_scans(ctx, scans):
    rows, cols = scans[0].shape
    R = cols // 2
    plan = _inverse_plan(rows, cols, 2, False)
    for k, p in enumerate(scans):
        got = ctx.warp_polar_f32(p, (2 * R, 2 * R), (R, R), R, inverse=True)
        assert np.array_equal(got, ctx.polar_to_cart_f32(p)[0]), k
        assert np.array_equal(got, plan(p)), k


@pytest.mark.timeout(600)
@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("df", [0, 1, 3, 20])
def test_polar_to_cartesian_modes(scans, df, log):
    rows, cols = scans[0].shape
    plan = _inverse_plan(rows, cols, df, log)
    R = cols // df if df > 1 else cols
    for k in ((0, 5) if df < 3 else range(len(scans))):
        got = parseData.convertPolarImageToCartesian(scans[k], logPolarMode=log, downsampleFactor=df)
        assert got.shape == (2 * R, 2 * R) and got.dtype == np.float32
        assert np.array_equal(got, plan(scans[k])), (df, log, k)
        if not log and k == 0:
            assert np.array_equal(got, _oracle_inverse(scans[k], R)), (df, k)


@pytest.mark.timeout(300)
def test_peaks_image_all_modes(golden):
    img = golden("peaks")["f32img"]                                # 37 x 513
    for df in (1, 2, 3, 7):
        for log in (False, True):
            got = parseData.convertPolarImageToCartesian(img, logPolarMode=log, downsampleFactor=df)
            assert np.array_equal(got, M.convertPolarImageToCartesian(img, log, df)), (df, log)
    cart = M.convertPolarImageToCartesian(img, False, 1)
    for shapeHW in (None, (400, 1012), (0, 300)):
        for log in (False, True):
            got = parseData.convertCartesianImageToPolar(cart, logPolarMode=log, shapeHW=shapeHW)
            assert np.array_equal(got, M.convertCartesianImageToPolar(cart, log, shapeHW)), (shapeHW, log)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("width", [2024, 513])
def test_cartesian_to_polar_modes(ctx, scans, width):
    carts = [ctx.polar_to_cart_f32(scans[k])[0] for k in (0, 7)]
    if width != 2024:
        o = (2024 - width) // 2
        carts = [np.ascontiguousarray(c[o:o + width, o:o + width]) for c in carts]
    for shapeHW in (None, (400, 1012), (0, 300)):
        ds = M.dsize(width / 2) if shapeHW is None else M.dsize(width / 2, shapeHW[1], shapeHW[0])
        for log in (False, True):
            plan = _forward_plan(width, ds, log)
            for k, c in enumerate(carts):
                got = parseData.convertCartesianImageToPolar(c, logPolarMode=log, shapeHW=shapeHW)
                assert got.shape == (ds[1], ds[0]) and got.dtype == np.float32
                assert np.array_equal(got, plan(c)), (width, shapeHW, log, k)
                if log:
                    assert np.array_equal(got, _oracle_forward_log(c, ds)), (width, shapeHW, k)


@pytest.mark.timeout(300)
def test_log_polar_equals_oracle(scans):
    for k, cols in [(0, 101), (3, 202), (6, 57), (9, 2025)]:
        img = scans[k][:, :cols]
        assert np.array_equal(parseData.convertPolarImgToLogPolar(img), oracle.convertPolarImgToLogPolar(img)), (k, cols)


@pytest.mark.timeout(300)
def test_fmt_script_round_trip_df20(scans):
    # FMT.py:191-198: to Cartesian at downsampleFactor 20, then back with shapeHW = the polar image's shape
    polar = scans[2]
    cart = parseData.convertPolarImageToCartesian(polar, downsampleFactor=20)
    assert np.array_equal(cart, M.convertPolarImageToCartesian(polar, False, 20))
    back = parseData.convertCartesianImageToPolar(cart, shapeHW=polar.shape)
    assert back.shape == polar.shape
    assert np.array_equal(back, M.convertCartesianImageToPolar(cart, False, polar.shape))


@pytest.mark.timeout(300)
def test_strided_slice_and_batch(ctx, scans):
    # a record as the data set stores it: 11 bytes of metadata, then 3768 range bins; extractDataFromRadarImage returns a column slice
    rec = np.zeros((400, 3779), np.uint8)
    rec[:, 11:11 + 2025] = (scans[4] * 255).round().astype(np.uint8)
    polar = parseData.extractDataFromRadarImage(rec)[0]
    assert not polar.flags.c_contiguous and polar.strides[1] == 4
    want = ctx.warp_polar_f32(np.ascontiguousarray(polar), (1350, 1350), (675, 675), 675, log=True, inverse=True)
    assert np.array_equal(ctx.warp_polar_f32(polar, (1350, 1350), (675, 675), 675, log=True, inverse=True), want)
    assert np.array_equal(parseData.convertPolarImageToCartesian(polar, downsampleFactor=3, logPolarMode=True), want)
    batch = scans[1:4]
    got = ctx.warp_polar_f32(batch, (404, 404), (202, 202), 202, inverse=True)
    assert got.shape == (3, 404, 404)
    for i in range(3):
        assert np.array_equal(got[i], ctx.warp_polar_f32(batch[i], (404, 404), (202, 202), 202, inverse=True)), i
    carts = got[:, 1:, 1:]                                         # (a non-contiguous batch: made contiguous on the way)
    fwd = ctx.warp_polar_f32(carts, (250, 700), (201.5, 201.5), 201.5, log=True)
    for i in range(3):
        assert np.array_equal(fwd[i], M.warp_polar(carts[i], (250, 700), (201.5, 201.5), 201.5, log=True)), i


@pytest.mark.timeout(300)
def test_change_global_range_resolution_and_path_helpers(scans, tmp_path):
    from PIL import Image
    old = parseData.RANGE_RESOLUTION_CART_M
    try:
        parseData.convertPolarImageToCartesian(scans[0], downsampleFactor=20, changeGlobalRangeResolution=True)
        assert parseData.RANGE_RESOLUTION_CART_M == parseData.RANGE_RESOLUTION_M * 20
        parseData.convertPolarImageToCartesian(scans[0], changeGlobalRangeResolution=True)
        assert parseData.RANGE_RESOLUTION_CART_M == old
    finally:
        parseData.RANGE_RESOLUTION_CART_M = old
    rec = np.zeros((400, 3779), np.uint8)
    rec[:, 11:11 + 2025] = (scans[8] * 255).round().astype(np.uint8)
    Image.fromarray(rec, mode="L").save(tmp_path / "1547131046353776.png")
    cart = parseData.getCartImageFromImgPaths([str(tmp_path / "1547131046353776.png")], 0)
    assert np.array_equal(cart, oracle.convertPolarImageToCartesian(parseData.extractDataFromRadarImage(rec)[0]))
