"""GPU (-m gpu): cv2.warpAffine (warpaffine.hip, roam_warp_affine_f32) and FMT.rotateImg bit for bit against the NumPy model of
tests/warp_affine_model.py - rotations of images smaller than a tile, odd, not a multiple of a tile side and 2024 x 2024; a general
matrix into another size, WARP_INVERSE_MAP, the singular matrix, a strided view, batches with one matrix and with one per image,
other dtypes; the four known answers; the reference's perfect-image chain (FMT.py:190-208) against the CPU chain of
test_warp_affine_cpu.py; the C entry's own refusals; and the kernel's time (printed, docs/KERNELS.md records it)."""
import ctypes as C
import math

import numpy as np
import pytest

import warp_affine_cases as cases
import warp_affine_model as A
from radarslampy_amd import FMT, parseData

pytestmark = pytest.mark.gpu

ANGLES = (0, 90, -90, 180, 5, -29.8, 33.3, 45)
SHAPES = ((8, 8), (3, 5), (1, 1), (300, 700), (700, 300), (202, 202), (257, 1031))


@pytest.fixture(scope="module")
def ctx():
    from radarslampy_amd import _ffi
    c = _ffi.default_context()
    assert "gfx950" in c.device_info()["arch"]
    return c


def _image(shape, seed=0):
    return np.random.default_rng(seed).random(shape, dtype=np.float32)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rotations_equal_the_model(shape):
    a = _image(shape, shape[0])
    for deg in ANGLES:
        got = FMT.rotateImg(a, deg)
        assert got.shape == shape and got.dtype == np.float32
        assert np.array_equal(got, A.rotateImg(a, deg)), (shape, deg)


def test_2024_equals_the_model():
    a = _image((2024, 2024), 7)
    assert np.array_equal(FMT.rotateImg(a, 5), A.rotateImg(a, 5))


def test_general_inverse_singular(ctx):
    a = _image((257, 1031), 3)
    M = cases.GENERAL_M
    got = ctx.warp_affine_f32(a, M, (700, 300))
    assert got.shape == (300, 700) and got.any() and np.array_equal(got, A.warp_affine(a, M, (700, 300)))
    inv = np.array(A.invert_affine(M)).reshape(2, 3)
    assert np.array_equal(ctx.warp_affine_f32(a, inv, (700, 300), inverse_map=True), got)
    assert np.array_equal(ctx.warp_affine_f32(a, M, (700, 300), inverse_map=True), A.warp_affine(a, M, (700, 300), inverse_map=True))
    got = ctx.warp_affine_f32(a, cases.SINGULAR_M, (33, 9))
    assert np.array_equal(got, np.full((9, 33), a[0, 0], np.float32)) and np.array_equal(got, A.warp_affine(a, cases.SINGULAR_M, (33, 9)))
    # a translation past the int16 range of the tap index: every tap is the border
    far = np.array([[1.0, 0, -40000.0], [0, 1.0, 0]])
    assert not ctx.warp_affine_f32(a, far, (64, 8), inverse_map=True).any()


def test_strided_view_batches_and_dtypes(ctx):
    wide = _image((300, 700), 4)
    view = wide[::2, 5:406]                                           # read in place: unit column stride, a longer row stride
    assert not view.flags.c_contiguous and view.strides[1] == 4
    M = A.rotation_matrix_2d((200.5, 75), 33.3, 1.0)
    assert np.array_equal(ctx.warp_affine_f32(view, M, (401, 150)), A.warp_affine(np.ascontiguousarray(view), M, (401, 150)))
    batch = np.stack([_image((101, 67), 10 + i) for i in range(5)])
    got = ctx.warp_affine_f32(batch, cases.GENERAL_M, (80, 90))
    assert got.shape == (5, 90, 80)
    for i in range(5):
        assert np.array_equal(got[i], A.warp_affine(batch[i], cases.GENERAL_M, (80, 90))), i
    angles = np.array([5, -29.8, 33.3, 90, 0.2])
    got = FMT.rotateImg(batch, angles)
    assert got.shape == batch.shape
    for i in range(5):
        assert np.array_equal(got[i], FMT.rotateImg(batch[i], angles[i])), i
        assert np.array_equal(got[i], A.rotateImg(batch[i], angles[i])), i
    one = FMT.rotateImg(batch, 45)
    for i in range(5):
        assert np.array_equal(one[i], A.rotateImg(batch[i], 45)), i
    assert np.array_equal(FMT.rotateImg(batch[:, ::-1, ::2], 5)[2], A.rotateImg(batch[2, ::-1, ::2], 5))     # made contiguous on the way
    f64 = np.random.default_rng(5).random((57, 91)) * 3 - 1
    u8 = np.random.default_rng(6).integers(0, 256, (57, 91), dtype=np.uint8)
    for img in (f64, u8):
        got = FMT.rotateImg(img, -29.8)
        assert got.dtype == np.float32 and np.array_equal(got, A.rotateImg(img.astype(np.float32), -29.8))
        assert np.array_equal(got, A.rotateImg(img, -29.8))


def test_rotate_img_is_the_stage_call_and_known_answers(ctx):
    a = _image((202, 202), 202)
    for deg in (5, -29.8):
        M = FMT.getRotationMatrix2D((101.0, 101.0), deg, 1.0)
        assert np.array_equal(FMT.rotateImg(a, deg), ctx.warp_affine_f32(a, M, (202, 202)))
    b = _image((120, 202), 9)
    assert np.array_equal(FMT.rotateImg(b, 33.3), ctx.warp_affine_f32(b, FMT.getRotationMatrix2D((101.0, 60.0), 33.3, 1.0), (202, 120)))
    for deg, want in cases.known_answers(a).items():
        assert np.array_equal(FMT.rotateImg(a, deg), want), deg


@pytest.mark.parametrize("deg", [5, -20])
def test_perfect_image_chain(deg):
    """FMT.py:190-208 on the device: every intermediate image equals the CPU chain's, the angle agrees with the oracle's on the CPU
    chain to the 1e-5 rad of test_fmt_rotation_matches_oracle, and so meets the sign and the bound fixed on the CPU"""
    import oracle
    polar = cases.real_scan0()
    cart_cpu, rot_cpu, back_cpu = cases.cpu_chain(deg)
    cart = parseData.convertPolarImageToCartesian(polar, downsampleFactor=cases.CHAIN_DOWNSAMPLE)
    assert np.array_equal(cart, cart_cpu)
    rot = FMT.rotateImg(cart, deg)
    assert np.array_equal(rot, rot_cpu)
    back = parseData.convertCartesianImageToPolar(rot, shapeHW=polar.shape)
    assert np.array_equal(back, back_cpu)
    angle, scale, response = FMT.getRotationUsingFMT(polar, back)
    want, _, _ = oracle.getRotationUsingFMT(polar, back_cpu)
    print(f"perfect image {deg:+d} deg on the device: {angle:+.9f} rad, CPU chain {want:+.9f} rad ({angle - want:+.3g})")
    assert abs(angle - want) <= 1e-5, (deg, angle, want)
    assert math.copysign(1.0, angle) == math.copysign(1.0, deg)
    assert abs(angle - math.radians(deg)) <= cases.CHAIN_BOUND_RAD, (deg, angle)


def test_argument_errors_on_the_device_side(ctx):
    """the C entry's own refusals (the Python wrapper checks the same things first)"""
    from radarslampy_amd import _ffi
    a = np.zeros((8, 8), np.float32)
    out = np.zeros((2, 8, 8), np.float32)
    M = np.array([1.0, 0, 0, 0, 1.0, 0] * 2)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    call = lambda *args: ctx.lib.roam_warp_affine_f32(ctx.h, *args)
    assert call(p(a), 1, 8, 8, 8, 64, p(M), 1, p(out), 8, 8, 0) == _ffi.ROAM_OK
    assert call(p(a), 1, 8, 8, 8, 64, p(M), 1, p(out), 8, 8, 1) == _ffi.ROAM_OK
    assert call(p(a), 2, 4, 8, 8, 32, p(M), 2, p(out), 8, 8, 0) == _ffi.ROAM_OK
    assert call(None, 1, 8, 8, 8, 64, p(M), 1, p(out), 8, 8, 0) == _ffi.ROAM_E_ARG
    assert call(p(a), 1, 8, 8, 8, 64, None, 1, p(out), 8, 8, 0) == _ffi.ROAM_E_ARG
    assert call(p(a), 1, 8, 8, 8, 64, p(M), 1, None, 8, 8, 0) == _ffi.ROAM_E_ARG
    assert call(p(a), 0, 8, 8, 8, 64, p(M), 1, p(out), 8, 8, 0) == _ffi.ROAM_E_ARG
    assert call(p(a), 1, 0, 8, 8, 64, p(M), 1, p(out), 8, 8, 0) == _ffi.ROAM_E_ARG
    assert call(p(a), 1, 8, 0, 8, 64, p(M), 1, p(out), 8, 8, 0) == _ffi.ROAM_E_ARG
    assert call(p(a), 1, 8, 8, 8, 64, p(M), 1, p(out), 0, 8, 0) == _ffi.ROAM_E_ARG
    assert call(p(a), 1, 8, 8, 8, 64, p(M), 1, p(out), 8, 16385, 0) == _ffi.ROAM_E_ARG
    assert call(p(a), 1, 16385, 8, 8, 64, p(M), 1, p(out), 8, 8, 0) == _ffi.ROAM_E_ARG
    assert call(p(a), 1, 8, 8, 8, 64, p(M), 2, p(out), 8, 8, 0) == _ffi.ROAM_E_ARG        # m_count not in {1, n}
    assert call(p(a), 2, 4, 8, 8, 32, p(M), 0, p(out), 8, 8, 0) == _ffi.ROAM_E_ARG
    assert call(p(a), 1, 8, 8, 8, 64, p(M), 1, p(out), 8, 8, 2) == _ffi.ROAM_E_ARG        # an unknown flag
    assert call(p(a), 1, 8, 8, 7, 64, p(M), 1, p(out), 8, 8, 0) == _ffi.ROAM_E_ARG        # a row stride below cols
    assert call(p(a), 2, 4, 8, 8, 31, p(M), 1, p(out), 8, 8, 0) == _ffi.ROAM_E_ARG        # overlapping images
    assert b"bad argument" in ctx.lib.roam_last_error(ctx.h)


def test_timing(ctx):
    """one 2024 x 2024 rotation by 5 degrees and a batch of 16, the kernel alone between HIP events after warm runs, best of three;
    GB/s counts one read and one write of the image.  Printed; no bar - there is no earlier figure to hold it to."""
    M = FMT.getRotationMatrix2D((1012, 1012), 5, 1.0)
    for n in (1, 16):
        ms = [ctx.time_warp_affine(n, 2024, 2024, M, 50) for _ in range(3)]
        print(f"warp_affine_kernel {n} x 2024x2024 by 5 deg: {ms} ms, best {min(ms):.4f} ms, "
              f"{8.0 * n * 2024 * 2024 / (min(ms) * 1e-3) / 1e9:.0f} GB/s")
        assert min(ms) > 0
    M45 = FMT.getRotationMatrix2D((1012, 1012), 45, 1.0)
    print(f"warp_affine_kernel 16 x 2024x2024 by 45 deg: {min(ctx.time_warp_affine(16, 2024, 2024, M45, 50) for _ in range(3)):.4f} ms")
