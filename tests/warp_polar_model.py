"""NumPy restatement of cv2.warpPolar(src, dsize, center, maxRadius, INTER_LINEAR | WARP_FILL_OUTLIERS [| WARP_POLAR_LOG]
[| WARP_INVERSE_MAP]) on float32 images, all four modes, operation by operation as warppolar.hip computes them, and of OpenCV's dsize
rules.  The host tables of the forward mode (radius per column, cos / sin per row) and the logarithms are computed with Python's
math module - glibc's libm, like the oracle's C and the library's host code - never with vectorised np.exp / np.cos / np.log, whose
SIMD forms may round differently.  The inverse semilog mode takes (float)log((double)(mag + 1)) where OpenCV uses hal::log32f."""
import math

import numpy as np

F = np.float32
CV_2PI = 6.283185307179586476925286766559


def cv_round(v: float) -> int:
    """cvRound of a double: nearest, half to even"""
    return int(np.rint(v))


def dsize(maxRadius, w=0, h=0):
    """OpenCV's output size (dw, dh) of warpPolar for the requested (w, h)"""
    if w <= 0 and h <= 0:
        return cv_round(maxRadius), cv_round(maxRadius * math.pi)
    if h <= 0:
        return w, cv_round(w * math.pi)
    if w <= 0:
        raise ValueError("width <= 0 with a positive height")
    return w, h


def fast_atan2_deg(y, x):
    sc = F(180 / math.pi)
    p1, p3, p5, p7 = F(0.9997878412794807) * sc, F(-0.3258083974640975) * sc, F(0.1555786518463281) * sc, F(-0.04432655554792128) * sc
    eps = F(2.220446049250313e-16)
    ax, ay = np.abs(x), np.abs(y)
    m = ax >= ay
    c = np.where(m, ay / (ax + eps), ax / (ay + eps)).astype(F)
    c2 = c * c
    a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
    a = np.where(m, a, F(90) - a)
    a = np.where(x < 0, F(180) - a, a)
    a = np.where(y < 0, F(360) - a, a)
    return a.astype(F)


def _log_f32(v):
    """(float)log((double)v) with glibc's log, once per distinct value"""
    u, inv = np.unique(v, return_inverse=True)
    lu = np.array([math.log(float(t)) for t in u], np.float64).astype(F)
    return lu[inv].reshape(v.shape)


def inverse_maps(rows, cols, dw, dh, cx, cy, maxRadius, log=False):
    """polar (rows x cols) -> Cartesian dh x dw: the float maps (mx, my) into the source padded by one wrapped row each side"""
    Kangle = CV_2PI / rows
    Kmag = (math.log(maxRadius) if log else maxRadius) / cols
    fx = (np.arange(dw).astype(F) - F(cx))[None, :]
    fy = (np.arange(dh).astype(F) - F(cy))[:, None]
    fx, fy = np.broadcast_arrays(fx, fy)
    mag = np.sqrt(fx * fx + fy * fy)
    ang = fast_atan2_deg(fy, fx) * F(math.pi / 180.0)
    p = _log_f32(mag + F(1)) if log else mag
    mx = (p.astype(np.float64) / Kmag).astype(F)
    my = (ang.astype(np.float64) / Kangle).astype(F) + F(1)
    return mx, my


def forward_tables(dw, dh, maxRadius, log=False):
    """OpenCV's host tables: br (dw) float32, cp, sp (dh) float64"""
    Kangle = CV_2PI / dh
    if log:
        Kmag = math.log(maxRadius) / dw
        br = [F(math.exp(rho * Kmag) - 1.0) for rho in range(dw)]
    else:
        Kmag = maxRadius / dw
        br = [F(rho * Kmag) for rho in range(dw)]
    cp = [math.cos(Kangle * phi) for phi in range(dh)]
    sp = [math.sin(Kangle * phi) for phi in range(dh)]
    return np.array(br, F), np.array(cp, np.float64), np.array(sp, np.float64)


def forward_maps(dw, dh, cx, cy, maxRadius, log=False):
    """Cartesian -> polar dh x dw (rows of angle, columns of radius): the float maps (mx, my)"""
    br, cp, sp = forward_tables(dw, dh, maxRadius, log)
    b = br.astype(np.float64)[None, :]
    mx = (b * cp[:, None] + float(F(cx))).astype(F)
    my = (b * sp[:, None] + float(F(cy))).astype(F)
    return mx, my


class Remap:
    """cv2.remap(src, mx, my, INTER_LINEAR, BORDER_CONSTANT 0) of float32 images of one size, the fixed-point plan built once:
    1/32-px coordinates (cvRound), int16 tap indices, weights wy * wx, taps outside the source read 0; padded: the polar source
    with one wrapped row above and one below"""

    def __init__(self, mx, my, rows, cols, padded):
        def fixed(m):
            s = np.clip(np.rint(m * F(32)).astype(np.float64), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)
            return np.clip(s >> 5, -32768, 32767), (s & 31).astype(F) * F(1 / 32)
        ix, wx1 = fixed(mx)
        iy, wy1 = fixed(my)
        wx0, wy0 = F(1) - wx1, F(1) - wy1
        self.w = [wy0 * wx0, wy0 * wx1, wy1 * wx0, wy1 * wx1]
        self.idx, self.ok = [], []
        prow = rows + 2 if padded else rows
        for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
            y, x = iy + dy, ix + dx
            ok = (x >= 0) & (x < cols) & (y >= 0) & (y < prow)
            r = y - 1 if padded else y
            r = np.where(r < 0, r + rows, np.where(r >= rows, r - rows, r))
            self.idx.append(np.where(ok, r * cols + x, 0).astype(np.int32))
            self.ok.append(ok)

    def __call__(self, src):
        flat = np.ascontiguousarray(src, F).ravel()
        t = [np.where(ok, flat[i], F(0)) for i, ok in zip(self.idx, self.ok)]
        v = t[0] * self.w[0]
        v = v + t[1] * self.w[1]
        v = v + t[2] * self.w[2]
        v = v + t[3] * self.w[3]
        return v.astype(F)


def warp_polar(src, dsize_wh, center, maxRadius, log=False, inverse=False):
    """cv2.warpPolar on one float32 image with a resolved dsize = (dw, dh)"""
    rows, cols = src.shape
    dw, dh = dsize_wh
    if inverse:
        mx, my = inverse_maps(rows, cols, dw, dh, center[0], center[1], maxRadius, log)
    else:
        mx, my = forward_maps(dw, dh, center[0], center[1], maxRadius, log)
    return Remap(mx, my, rows, cols, inverse)(src)


def polar_to_cart_plan(rows, cols, downsampleFactor=2, log=False):
    """convertPolarImageToCartesian's geometry (parseData.py:100-135) as a reusable Remap"""
    R = cols // downsampleFactor if downsampleFactor > 1 else cols
    mx, my = inverse_maps(rows, cols, 2 * R, 2 * R, R, R, R, log)
    return Remap(mx, my, rows, cols, True)


def convertPolarImageToCartesian(imgPolar, logPolarMode=False, downsampleFactor=2):
    rows, cols = imgPolar.shape
    return polar_to_cart_plan(rows, cols, downsampleFactor, logPolarMode)(imgPolar)


def convertCartesianImageToPolar(imgCart, logPolarMode=False, shapeHW=None):
    h, w = imgCart.shape
    assert w == h
    R = w / 2
    ds = dsize(R) if shapeHW is None else dsize(R, shapeHW[1], shapeHW[0])
    return warp_polar(imgCart, ds, (h / 2, w / 2), R, log=logPolarMode, inverse=False)


def convertPolarImgToLogPolar(imgPolar):
    return convertCartesianImageToPolar(convertPolarImageToCartesian(imgPolar, False, 1), True, None)
