"""CPU side of warpAffine / FMT.rotateImg (no GPU): known answers of the NumPy model the GPU test is judged by, the model's edge
cases, rotateImg's name and argument errors raised before any device call, the ABI declaration, and the reference's perfect-image
test (FMT.py:190-208) on the project's models - the expectation the GPU chain is held to.

Perfect-image chain, measured here (real scan 0 of tests/golden/peaks.npz, downsampleFactor 20, oracle.getRotationUsingFMT(polar,
polar of the rotated image)): the recovered angle has the SIGN of the angle given to rotateImg, and recovered - applied is
+2.750e-3 rad at +5 deg, +1.220e-3 at -5, +2.041e-3 at +20, -0.909e-3 at -20.  The bound is the worst of these plus one log-polar
row, 2 pi / 317 rad, the estimator's own resolution: 2.257e-2 rad."""
import inspect
import math
import os
import re

import numpy as np
import pytest

import oracle
import warp_affine_cases as cases
import warp_affine_model as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [8, 202, 2024])
def test_model_known_answers(n):
    a = np.random.default_rng(n).random((n, n), dtype=np.float32)
    for deg, want in cases.known_answers(a).items():
        assert np.array_equal(A.rotateImg(a, deg), want), (n, deg)


def test_model_singular_matrix_reads_the_first_pixel():
    a = np.random.default_rng(1).random((9, 14), dtype=np.float32)
    assert A.invert_affine(cases.SINGULAR_M) == [0.0] * 6
    out = A.warp_affine(a, cases.SINGULAR_M, (11, 6))
    assert out.shape == (6, 11) and np.array_equal(out, np.full((6, 11), a[0, 0], np.float32))


def test_model_inverse_map_equals_the_default_path():
    a = np.random.default_rng(2).random((40, 56), dtype=np.float32)
    M = cases.GENERAL_M
    inv = np.array(A.invert_affine(M)).reshape(2, 3)
    want = A.warp_affine(a, M, (70, 33))
    assert want.any() and np.array_equal(A.warp_affine(a, inv, (70, 33), inverse_map=True), want)
    # the inversion really inverts: source -> destination -> source is the identity
    full = np.vstack([M, [0, 0, 1]]) @ np.vstack([inv, [0, 0, 1]])
    assert np.allclose(full, np.eye(3), atol=1e-12)


@pytest.mark.parametrize("shift", [40000.0, -40000.0, 2.0 ** 20 - 64])
def test_model_int16_saturation(shift):
    """a translation past +-32768 px (inside the 2^20 limit): the unsaturated tap index leaves int16, the saturated one lies
    outside any source of at most 16384 columns, every tap reads the border"""
    from radarslampy_amd import _ffi
    a = np.ones((5, 7), np.float32)
    M = np.array([[1.0, 0.0, shift], [0.0, 1.0, 0.0]])
    _ffi.warp_affine_args(a, M, (7, 5), inverse_map=True)              # accepted: below the limit
    X, Y = A.fixed_coords(M.ravel(), 7, 5)
    assert (np.abs(X >> 5) > 32767).all() and np.array_equal(Y >> 5, np.arange(5)[:, None] * np.ones(7, np.int64))
    assert not A.warp_affine(a, M, (7, 5), inverse_map=True).any()
    assert np.array_equal(A.warp_affine(a, np.array([[1.0, 0, 2.5], [0, 1.0, 0]]), (7, 5))[:, 3:], np.ones((5, 4), np.float32))


def test_rotation_matrix_2d():
    from radarslampy_amd import FMT
    for center, angle, scale in (((101, 101), 5.0, 1.0), ((0.1, 1012.5), -29.8, 1.0), ((3.0, 4.0), 33.3, 0.7), ((0, 0), 90, 2.0)):
        M = FMT.getRotationMatrix2D(center, angle, scale)
        assert M.shape == (2, 3) and M.dtype == np.float64
        assert np.array_equal(M, A.rotation_matrix_2d(center, angle, scale))
        cx, cy = float(np.float32(center[0])), float(np.float32(center[1]))
        assert np.allclose(M @ [cx, cy, 1.0], [cx, cy], atol=1e-9)        # the centre stays
        assert np.isclose(np.linalg.det(M[:, :2]), scale * scale)
    assert np.allclose(FMT.getRotationMatrix2D((0, 0), 90, 1.0)[:, :2], [[0, 1], [-1, 0]], atol=1e-15)
    assert FMT.getRotationMatrix2D((0.1, 0), 0, 1.0)[0, 2] == 0.0 and A.rotation_matrix_2d((0.1, 3), 180, 1.0)[0, 2] != 0.2


def test_names_import_with_the_reference_signature():
    from radarslampy_amd import FMT, _ffi
    assert list(inspect.signature(FMT.rotateImg).parameters) == ["image", "angle_degrees"]
    assert list(inspect.signature(FMT.getRotationMatrix2D).parameters) == ["center", "angle", "scale"]
    assert list(inspect.signature(_ffi.Context.warp_affine_f32).parameters) == ["self", "src", "M", "dsize_wh", "inverse_map"]
    assert "2^20" in _ffi.Context.warp_affine_f32.__doc__
    assert "roam_warp_affine_f32" in _ffi.ABI_SYMBOLS


def test_header_declares_the_entry():
    txt = open(os.path.join(ROOT, "include", "roam_abi.h")).read()
    m = re.search(r"int32_t\s+roam_warp_affine_f32\s*\(([^;]*)\)\s*;", txt)
    assert m, "include/roam_abi.h does not declare roam_warp_affine_f32"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["ctx", "src", "n", "rows", "cols", "src_row_stride", "src_image_stride", "M",
                                                          "m_count", "dst", "dw", "dh", "flags"]
    assert re.search(r"#define\s+ROAM_WARP_AFFINE_INVERSE_MAP\s+1\b", txt)


def test_argument_errors_come_before_any_device_call(monkeypatch):
    from radarslampy_amd import FMT, _ffi

    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_ffi, "default_context", no_device)
    monkeypatch.setattr(_ffi, "load_library", no_device)
    img = np.zeros((16, 24), np.float32)
    for bad in (img[0], img[None, None], np.float32(3)):                       # neither 2-D nor 3-D
        with pytest.raises(ValueError):
            FMT.rotateImg(bad, 5.0)
    for bad in (np.zeros((0, 24), np.float32), np.zeros((16, 0), np.float32), np.zeros((0, 16, 24), np.float32)):     # empty
        with pytest.raises(ValueError):
            FMT.rotateImg(bad, 5.0)
    for bad in (np.zeros((1, 16385), np.float32), np.zeros((16385, 1), np.uint8)):      # a side above 16384
        with pytest.raises(ValueError):
            FMT.rotateImg(bad, 5.0)
    for bad in (float("nan"), float("inf"), [1.0, float("nan"), 2.0]):          # a non-finite angle = a non-finite matrix
        with pytest.raises(ValueError):
            FMT.rotateImg(np.stack([img] * 3), bad)
    for im, ang in ((img, [1.0]), (np.stack([img] * 3), [1.0, 2.0]), (np.stack([img] * 3), np.zeros((3, 1)))):   # angles that match no batch
        with pytest.raises(ValueError):
            FMT.rotateImg(im, ang)
    with pytest.raises(AssertionError, match="device call"):                   # valid arguments do reach the device
        FMT.rotateImg(img, 5.0)
    with pytest.raises(AssertionError, match="device call"):
        FMT.rotateImg(np.stack([img] * 3), [1.0, 2.0, 3.0])

    ctx = object.__new__(_ffi.Context)                                         # no library, no device behind it
    eye = np.array([[1.0, 0, 0], [0, 1.0, 0]])
    batch = np.stack([img] * 3)
    with pytest.raises(ValueError):
        ctx.warp_affine_f32(img[0], eye, (24, 16))
    with pytest.raises(ValueError):
        ctx.warp_affine_f32(np.zeros((2, 3, 4, 5), np.float32), eye, (24, 16))
    for badM in (np.eye(3), np.zeros(6), np.zeros((3, 2)), np.stack([eye] * 3), np.zeros((1, 2, 3))):   # wrong M shapes for a 2-D image
        with pytest.raises(ValueError):
            ctx.warp_affine_f32(img, badM, (24, 16))
    with pytest.raises(ValueError):
        ctx.warp_affine_f32(batch, np.stack([eye] * 2), (24, 16))             # 2 matrices for 3 images
    for v in (np.nan, np.inf, -np.inf):
        M = eye.copy(); M[1, 2] = v
        with pytest.raises(ValueError):
            ctx.warp_affine_f32(img, M, (24, 16))
    for ds in ((0, 16), (24, 0), (-1, 5), (16385, 4), (4, 16385)):             # an empty output, a side above 16384
        with pytest.raises(ValueError):
            ctx.warp_affine_f32(img, eye, ds)
    with pytest.raises(ValueError):
        ctx.warp_affine_f32(np.zeros((0, 24), np.float32), eye, (24, 16))
    # the 2^20 px limit at the four corners of the output, through the inverted matrix
    far = np.array([[1.0, 0, 2.0 ** 20], [0, 1.0, 0]])
    with pytest.raises(ValueError, match="2\\^20"):
        ctx.warp_affine_f32(img, far, (24, 16), inverse_map=True)
    with pytest.raises(ValueError, match="2\\^20"):
        ctx.warp_affine_f32(img, far, (24, 16))                                # inverted: -2^20
    with pytest.raises(ValueError, match="2\\^20"):
        ctx.warp_affine_f32(img, np.array([[1.0, 0, 0], [0, 70.0, 0]]), (24, 16384), inverse_map=True)    # only the far corners
    with pytest.raises(ValueError, match="2\\^20"):
        ctx.warp_affine_f32(img, np.array([[1e-9, 0, 0], [0, 1.0, 0]]), (24, 16))   # a tiny scale: its inverse is huge
    with pytest.raises(ValueError, match="2\\^20"):
        ctx.warp_affine_f32(img, np.array([[1e-160, 0, 1e160], [0, 1e-160, 0]]), (24, 16))   # the inverse overflows to inf
    with pytest.raises(ValueError, match="2\\^20"):
        ctx.warp_affine_f32(batch, np.stack([eye, eye, far]), (24, 16), inverse_map=True)   # the last matrix of a stack
    # accepted just inside the limit, and the singular matrix (it inverts to zeros): these do reach the library
    for M, inv in ((np.array([[1.0, 0, 2.0 ** 20 - 24], [0, 1.0, 0]]), True), (cases.SINGULAR_M, False)):
        a, m, dw, dh = _ffi.warp_affine_args(img, M, (24, 16), inverse_map=inv)
        assert a is img and m.shape == (1, 6) and m.dtype == np.float64 and (dw, dh) == (24, 16)
    assert _ffi.warp_affine_args(batch, np.stack([eye] * 3), (5, 4))[1].shape == (3, 6)
    assert np.array_equal(_ffi.invert_affine(cases.GENERAL_M), A.invert_affine(cases.GENERAL_M))
    ctx.h = None


def test_perfect_image_chain():
    """FMT.py:190-208 on the models: polar -> Cartesian (downsampleFactor 20) -> rotateImg -> polar of the scan's shape ->
    getRotationUsingFMT(scan, that).  Sign and error as the module docstring records them."""
    polar = cases.real_scan0()
    assert polar.shape == (400, 2025)
    worst = 0.0
    for deg in (5, -5, 20, -20):
        cart, rot, back = cases.cpu_chain(deg)
        assert cart.shape == rot.shape == (202, 202) and back.shape == polar.shape
        angle, scale, response = oracle.getRotationUsingFMT(polar, back)
        err = angle - math.radians(deg)
        print(f"perfect image {deg:+d} deg: recovered {angle:+.6f} rad ({math.degrees(angle):+.4f} deg), error {err:+.3e} rad, "
              f"scale {scale:.6f}, response {response:.4f}")
        worst = max(worst, abs(err))
        assert math.copysign(1.0, angle) == math.copysign(1.0, deg), (deg, angle)
        assert abs(err) <= cases.CHAIN_BOUND_RAD, (deg, angle, err)
        assert abs(err - cases.CHAIN_MEASURED_ERR[deg]) < 5e-6, (deg, err)      # the record in the docstring is this run's
    print(f"worst error {worst:.3e} rad, bound {cases.CHAIN_BOUND_RAD:.3e} rad")
