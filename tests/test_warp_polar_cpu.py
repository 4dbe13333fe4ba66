"""CPU (-m "not gpu"): the NumPy model of cv2.warpPolar in tests/warp_polar_model.py against the oracle's C restatement where the
oracle covers a mode (inverse linear, forward semilog, the live df=2 geometry, convertPolarImgToLogPolar); OpenCV's dsize rules;
the argument errors of parseData's warps, raised before any device call; the names the reference's FMT.py and RawROAMSystem.py import
from parseData; the host helpers that read records from PNG files."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle
import warp_polar_model as M
from radarslampy_amd import parseData


def _oracle_inverse(img, dw, dh, cx, cy, R, row_stride=None):
    img = np.asarray(img, np.float32)
    rows, cols = img.shape
    if row_stride is None:
        img = np.ascontiguousarray(img)
        row_stride = cols
    out = np.empty((dh, dw), np.float32)
    oracle.lib().oracle_warp_polar_inverse(img.ctypes.data_as(C.POINTER(C.c_float)), rows, cols, C.c_int64(row_stride), dw, dh,
                                           C.c_float(cx), C.c_float(cy), C.c_double(R), oracle._p(out, C.c_float))
    return out


def _oracle_forward_log(img, dw, dh, cx, cy, R):
    img = np.ascontiguousarray(img, np.float32)
    H, W = img.shape
    out = np.empty((dh, dw), np.float32)
    oracle.lib().oracle_warp_polar_forward_log(oracle._p(img, C.c_float), W, H, dw, dh, C.c_float(cx), C.c_float(cy), C.c_double(R),
                                               oracle._p(out, C.c_float))
    return out


@pytest.fixture(scope="module")
def scans(golden):
    return golden("tiny_track")["payload"].astype(np.float32) / np.float32(255.)


def test_model_inverse_linear_equals_oracle_random():
    rng = np.random.default_rng(3)
    for rows, cols, dw, dh, cx, cy, R in [(37, 51, 103, 97, 51.5, 48.5, 50.3), (5, 3, 9, 11, 4.5, 5.5, 4.0), (64, 101, 202, 202, 101, 101, 101),
                                          (29, 77, 61, 40, 30.5, 19.5, 33.25), (400, 13, 27, 27, 13.5, 13.5, 13.5)]:
        img = rng.random((rows, cols), np.float32)
        got = M.warp_polar(img, (dw, dh), (cx, cy), R, log=False, inverse=True)
        assert np.array_equal(got, _oracle_inverse(img, dw, dh, cx, cy, R)), (rows, cols, dw, dh, cx, cy, R)


def test_model_inverse_linear_equals_oracle_real_scans(scans):
    for k, p in enumerate(scans):
        img = p[:, :1013] if k % 2 else p[:, :101]                  # odd widths
        cols = img.shape[1]
        R = cols // 3 if k % 3 else cols
        c = R + 0.5 * (k % 2)                                       # half-pixel centres on every other scan
        got = M.warp_polar(img, (2 * R + 1, 2 * R), (c, c), R, log=False, inverse=True)
        assert np.array_equal(got, _oracle_inverse(img, 2 * R + 1, 2 * R, c, c, R)), k


def test_model_inverse_reads_a_strided_view_like_the_oracle(scans):
    view = scans[0][:, 7:7 + 303]                                  # the oracle reads it in place, with its row stride
    want = _oracle_inverse(view, 203, 202, 101.5, 101, 101, row_stride=view.strides[0] // 4)
    assert np.array_equal(M.warp_polar(view, (203, 202), (101.5, 101), 101, inverse=True), want)


def test_model_forward_log_equals_oracle():
    rng = np.random.default_rng(4)
    for H, W, dw, dh, cx, cy, R in [(97, 97, 48, 151, 48.5, 48.5, 48.5), (40, 61, 33, 70, 30.5, 20.0, 25.3), (7, 7, 3, 9, 3.5, 3.5, 3.5),
                                    (202, 202, 101, 317, 101, 101, 101), (513, 513, 300, 942, 256.5, 256.5, 256.5)]:
        img = rng.random((H, W), np.float32)
        got = M.warp_polar(img, (dw, dh), (cx, cy), R, log=True, inverse=False)
        assert np.array_equal(got, _oracle_forward_log(img, dw, dh, cx, cy, R)), (H, W, dw, dh)


def test_model_forward_log_equals_oracle_real_cartesian(scans):
    for k in (0, 5, 10):
        cart = oracle.convertPolarImageToCartesian(scans[k][:, :675])
        W = cart.shape[0]
        for ds in [M.dsize(W / 2), (400, 1012), M.dsize(W / 2, 300, 0)]:
            got = M.warp_polar(cart, ds, (W / 2, W / 2), W / 2, log=True, inverse=False)
            assert np.array_equal(got, _oracle_forward_log(cart, ds[0], ds[1], W / 2, W / 2, W / 2)), (k, ds)


def test_model_live_geometry_equals_oracle(scans, golden):
    plan = M.polar_to_cart_plan(*scans[0].shape, 2)
    for k in (0, 4, 10):
        assert np.array_equal(plan(scans[k]), oracle.convertPolarImageToCartesian(scans[k])), k
    peaks = golden("peaks")["f32img"]
    assert np.array_equal(M.convertPolarImageToCartesian(peaks), oracle.convertPolarImageToCartesian(peaks))


def test_model_log_polar_equals_oracle(scans):
    for k, cols in [(0, 101), (3, 202), (7, 57)]:
        img = scans[k][:, :cols]
        assert np.array_equal(M.convertPolarImgToLogPolar(img), oracle.convertPolarImgToLogPolar(img)), (k, cols)


def test_forward_tables_are_libm_values():
    br, cp, sp = M.forward_tables(5, 4, 7.5, log=True)
    assert br[0] == 0 and br[1] == np.float32(math.exp(1 * (math.log(7.5) / 5)) - 1.0)
    assert cp[1] == math.cos(2 * math.pi / 4) and sp[3] == math.sin(3 * (2 * math.pi / 4))
    brl, _, _ = M.forward_tables(5, 4, 7.5, log=False)
    assert np.array_equal(brl, np.array([r * (7.5 / 5) for r in range(5)], np.float32))


def test_dsize_rules():
    for f in (M.dsize, lambda r, w=0, h=0: parseData.warpPolarDsize(r, (w, h))):
        assert f(256.5) == (256, 806)                               # cvRound(256.5) = 256: half to even
        assert f(257.5) == (258, round(257.5 * math.pi))
        assert f(1012.0) == (1012, 3179)
        assert f(100, 300, 0) == (300, 942)
        assert f(100, 300, -5) == (300, 942)
        assert f(100, 1012, 400) == (1012, 400)
        assert f(100, -1, -1) == (100, 314)
        with pytest.raises(ValueError):
            f(100, 0, 300)
    assert parseData.warpPolarDsize(256.5) == (256, 806) == parseData.warpPolarDsize(256.5, None)


def test_argument_errors_need_no_device():
    img = np.zeros((8, 16), np.float32)
    with pytest.raises(ValueError):
        parseData.convertPolarImageToCartesian(np.zeros((2, 8, 16), np.float32), downsampleFactor=3)
    with pytest.raises(ValueError):
        parseData.convertPolarImageToCartesian(np.zeros(16, np.float32))
    with pytest.raises(ValueError):
        parseData.convertPolarImageToCartesian(np.zeros((2, 8, 16), np.float32))            # the live configuration too
    with pytest.raises(TypeError):
        parseData.convertPolarImageToCartesian(img, downsampleFactor=2.0)
    with pytest.raises(TypeError):
        parseData.convertPolarImageToCartesian(img, downsampleFactor=1.5)
    with pytest.raises(ValueError):
        parseData.convertPolarImageToCartesian(img, downsampleFactor=17)                    # maxRadius 0: empty output
    with pytest.raises(ValueError):
        parseData.convertPolarImageToCartesian(np.zeros((8, 1), np.float32), downsampleFactor=2)   # live: maxRadius 0
    with pytest.raises(ValueError):
        parseData.convertPolarImageToCartesian(img, logPolarMode=True, downsampleFactor=16)  # maxRadius 1: log(1) = 0
    with pytest.raises(ValueError):
        parseData.convertPolarImageToCartesian(np.zeros((8, 9000), np.float32), downsampleFactor=1)   # 18000 > 16384
    with pytest.raises(ValueError):
        parseData.convertPolarImageToCartesian(np.zeros((0, 16), np.float32), downsampleFactor=3)
    with pytest.raises(AssertionError):
        parseData.convertCartesianImageToPolar(np.zeros((8, 9), np.float32))
    with pytest.raises(ValueError):
        parseData.convertCartesianImageToPolar(np.zeros((2, 8, 8), np.float32))
    with pytest.raises(ValueError):
        parseData.convertCartesianImageToPolar(np.zeros((8, 8), np.float32), shapeHW=(300, 0))   # width 0, height 300
    with pytest.raises(ValueError):
        parseData.convertCartesianImageToPolar(np.zeros((2, 2), np.float32), logPolarMode=True)  # maxRadius 1
    with pytest.raises(ValueError):
        parseData.convertCartesianImageToPolar(np.zeros((0, 0), np.float32))
    with pytest.raises(ValueError):
        parseData.convertCartesianImageToPolar(np.zeros((8, 8), np.float32), shapeHW=(20000, 10))
    with pytest.raises(ValueError):
        parseData.convertPolarImgToLogPolar(np.zeros((4, 1), np.float32))                  # Cartesian 2 x 2: maxRadius 1


def test_reference_imports_exist():
    # FMT.py:7 and RawROAMSystem.py:8 of the reference
    for name in ["RANGE_RESOLUTION_CART_M", "convertCartesianImageToPolar", "convertPolarImageToCartesian", "getCartImageFromImgPaths",
                 "getPolarImageFromImgPaths", "getRadarImgPaths", "convertPolarImgToLogPolar", "getDataFromImgPathsByIndex",
                 "getRadarStreamPolar"]:
        assert callable(getattr(parseData, name)) or name == "RANGE_RESOLUTION_CART_M", name


def _write_sequence(tmp_path, n):
    from PIL import Image
    rng = np.random.default_rng(9)
    recs = [rng.integers(0, 256, (16, 11 + 40), dtype=np.uint8) for _ in range(n)]
    lines = []
    for i, r in enumerate(recs):
        stamp = str(1547131046353776 + 250000 * i)
        Image.fromarray(r, mode="L").save(tmp_path / f"{stamp}.png")
        lines.append(f"{stamp} 1\n")
    (tmp_path / "radar.timestamps").write_text("".join(lines))
    return recs


def test_host_helpers_read_records(tmp_path):
    recs = _write_sequence(tmp_path, 3)
    paths = parseData.getRadarImgPaths(str(tmp_path), str(tmp_path / "radar.timestamps"))
    for i, r in enumerate(recs):
        got = parseData.getDataFromImgPathsByIndex(paths, i)
        want = oracle.extractDataFromRadarImage(r)
        assert len(got) == 6
        for a, b in zip(got, want):
            assert np.array_equal(np.asarray(a), np.asarray(b)), i
    stream = parseData.getRadarStreamPolar(str(tmp_path), str(tmp_path / "radar.timestamps"))
    assert stream.shape == (16, 40, 3) and stream.dtype == np.float32
    for i, r in enumerate(recs):
        assert np.array_equal(stream[:, :, i], oracle.extractDataFromRadarImage(r)[0])
