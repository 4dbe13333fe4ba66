"""NumPy restatement of cv2.warpAffine(src, M, dsize, INTER_LINEAR [| WARP_INVERSE_MAP], BORDER_CONSTANT 0) on float32 images,
operation by operation as warpaffine.hip computes it, of cv2.getRotationMatrix2D and of the reference's rotateImg (FMT.py:93-100).
OpenCV 4's CV_32F path: the matrix inverted in float64 in OpenCV's operation order; per output pixel the two terms of each source
coordinate rounded to 1/1024 px (half to even, saturated to int32) and added in int32 - here in int64 with an explicit wrap to
int32 - then shifted to 1/32 px; tap indices saturated to int16; bilinear weights wy * wx in float32; taps outside the source read 0;
the four products added in OpenCV's order.  cos / sin come from Python's math module (glibc's libm), as the library's host code
takes them."""
import math

import numpy as np

F = np.float32
AB_SCALE = 1024.0


def invert_affine(M):
    """warpAffine's in-place inversion of the 2 x 3 matrix (Python floats: IEEE double, one rounding per operation) -> 6 coefficients;
    a singular matrix gives all zeros"""
    M0, M1, M2, M3, M4, M5 = (float(v) for v in np.asarray(M, np.float64).ravel())
    D = M0 * M4 - M1 * M3
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = M4 * D, M0 * D
    M0, M1, M3, M4 = A11, M1 * -D, M3 * -D, A22
    b1 = -M0 * M2 - M1 * M5
    b2 = -M3 * M2 - M4 * M5
    return [M0, M1, b1, M3, M4, b2]


def _sat_round(v):
    """saturate_cast<int>(double): nearest, half to even, saturated to int32 -> int64"""
    return np.clip(np.rint(v), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


def _wrap32(v):
    """an int64 sum as int32 arithmetic leaves it"""
    return ((v + 2 ** 31) & (2 ** 32 - 1)) - 2 ** 31


def fixed_coords(M6, dw, dh):
    """the 1/32-px source coordinates (X, Y), int64 holding int32 values, of every pixel of a dh x dw destination for the
    destination -> source coefficients M6"""
    M0, M1, M2, M3, M4, M5 = M6
    x = np.arange(dw, dtype=np.float64)
    y = np.arange(dh, dtype=np.float64)
    adelta = _sat_round(M0 * x * AB_SCALE)
    bdelta = _sat_round(M3 * x * AB_SCALE)
    X0 = _sat_round((M1 * y + M2) * AB_SCALE) + 16
    Y0 = _sat_round((M4 * y + M5) * AB_SCALE) + 16
    X = _wrap32(X0[:, None] + adelta[None, :]) >> 5
    Y = _wrap32(Y0[:, None] + bdelta[None, :]) >> 5
    return X, Y


def remap_fixed(src, X, Y):
    """the bilinear remap of one float32 image at the 1/32-px coordinates (X, Y)"""
    src = np.ascontiguousarray(src, F)
    rows, cols = src.shape
    flat = src.ravel()
    ix, iy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
    wx1, wy1 = (X & 31).astype(F) * F(1 / 32), (Y & 31).astype(F) * F(1 / 32)
    wx0, wy0 = F(1) - wx1, F(1) - wy1
    v = None
    for dy, dx, w in ((0, 0, wy0 * wx0), (0, 1, wy0 * wx1), (1, 0, wy1 * wx0), (1, 1, wy1 * wx1)):
        yy, xx = iy + dy, ix + dx
        ok = (xx >= 0) & (xx < cols) & (yy >= 0) & (yy < rows)
        t = np.where(ok, flat[np.where(ok, yy * cols + xx, 0)], F(0)) * w
        v = t if v is None else v + t
    return v.astype(F)


def warp_affine(src, M, dsize_wh, inverse_map=False):
    """cv2.warpAffine on one image (any dtype: converted to float32 first, the package's convention) -> (dh, dw) float32"""
    dw, dh = dsize_wh
    M6 = [float(v) for v in np.asarray(M, np.float64).ravel()] if inverse_map else invert_affine(M)
    X, Y = fixed_coords(M6, dw, dh)
    return remap_fixed(np.asarray(src).astype(F), X, Y)


def rotation_matrix_2d(center, angle, scale):
    """cv2.getRotationMatrix2D: the centre as cv::Point2f (float32), everything else in float64"""
    cx, cy = float(F(center[0])), float(F(center[1]))
    rad = float(angle) * math.pi / 180.0
    a, b = math.cos(rad) * float(scale), math.sin(rad) * float(scale)
    return np.array([[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy]], np.float64)


def rotateImg(image, angle_degrees):
    """FMT.py:93-100 on one 2-D image"""
    h, w = image.shape
    return warp_affine(image, rotation_matrix_2d((w / 2, h / 2), angle_degrees, 1.0), (w, h))
