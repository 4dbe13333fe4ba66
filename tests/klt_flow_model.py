"""NumPy restatement of the pyramidal Lucas-Kanade tracker, operation by operation in float32 / integer arithmetic as
oracle_klt_track (oracle/c/warp_klt.c) and klt_kernel (csrc/pyrklt.hip) do it, with the one thing the oracle does not have: an optional
start of the search, cv2.calcOpticalFlowPyrLK's OPTFLOW_USE_INITIAL_FLOW.  OpenCV's rule (lkpyramid.cpp, restated): at the top
level only, nextPt = init_pts * 2^-maxLevel in place of prevPt; everything else is the unseeded tracker.

Unseeded it is tied to the oracle bit for bit by tests/test_klt_flow_cpu.py; apply_affine is the float32 order in which the kernel
turns a lane's affine prior into guesses."""
import numpy as np

F = np.float32
WIN = 15
W_BITS = 14
MAX_LEVEL = 3
MAX_ITER = 10
EPS = F(0.03)
MIN_EIG = F(1e-4)
ERR_THRESHOLD = 10


def apply_affine(A, pts):
    """(a00 x + a01 y) + a02, (a10 x + a11 y) + a12 in float32, every operation rounded: A six numbers or (2, 3), pts (K, 2)"""
    a = np.asarray(A, F).reshape(6)
    p = np.ascontiguousarray(pts, F).reshape(-1, 2)
    x, y = p[:, 0], p[:, 1]
    gx = (a[0] * x + a[1] * y) + a[2]
    gy = (a[3] * x + a[4] * y) + a[5]
    return np.stack([gx, gy], axis=1).astype(F)


def reflect101(p, n):
    """BORDER_REFLECT_101 of any integer index (the oracle's loop, closed form)"""
    p = np.asarray(p, np.int64)
    if n == 1:
        return np.zeros_like(p)
    period = 2 * (n - 1)
    q = np.mod(p, period)
    return np.where(q >= n, period - q, q)


def pyr_down(img):
    """cv2.pyrDown on u8: 5 x 5 binomial, REFLECT_101, (sum + 128) >> 8"""
    h, w = img.shape
    dh, dw = (h + 1) // 2, (w + 1) // 2
    k = np.array([1, 4, 6, 4, 1], np.int64)
    src = img.astype(np.int64)
    cols = reflect101(2 * np.arange(dw)[:, None] + np.arange(5)[None, :] - 2, w)        # (dw, 5)
    rows = reflect101(2 * np.arange(dh)[:, None] + np.arange(5)[None, :] - 2, h)        # (dh, 5)
    horiz = (src[:, cols] * k).sum(axis=2)                                               # (h, dw)
    acc = (horiz[rows] * k[None, :, None]).sum(axis=1)                                   # (dh, dw)
    return ((acc + 128) >> 8).astype(np.uint8)


def build_pyramid(img_u8, max_level=MAX_LEVEL):
    pyr = [np.ascontiguousarray(img_u8, np.uint8)]
    for _ in range(max_level):
        pyr.append(pyr_down(pyr[-1]))
    return pyr


def _scharr(img):
    """Scharr derivatives of the whole level (REFLECT_101 taps), int64"""
    p = np.pad(img.astype(np.int64), 1, mode="reflect") if min(img.shape) > 1 else np.pad(img.astype(np.int64), 1, mode="edge")
    a00, a01, a02 = p[:-2, :-2], p[:-2, 1:-1], p[:-2, 2:]
    a10, a12 = p[1:-1, :-2], p[1:-1, 2:]
    a20, a21, a22 = p[2:, :-2], p[2:, 1:-1], p[2:, 2:]
    dx = 3 * (a02 + a22 - a00 - a20) + 10 * (a12 - a10)
    dy = 3 * (a20 + a22 - a00 - a02) + 10 * (a21 - a01)
    return dx, dy


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _weights(a, b):
    S = F(1 << W_BITS)
    one = F(1.0)
    iw00 = int(np.rint((one - a) * (one - b) * S))
    iw01 = int(np.rint(a * (one - b) * S))
    iw10 = int(np.rint((one - a) * b * S))
    return iw00, iw01, iw10, (1 << W_BITS) - iw00 - iw01 - iw10


def _patch(img, x0, y0, n):
    """n x n pixels from (x0, y0), REFLECT_101, int64"""
    h, w = img.shape
    return img[np.ix_(reflect101(y0 + np.arange(n), h), reflect101(x0 + np.arange(n), w))].astype(np.int64)


def _patch_zero(d, x0, y0, n):
    """n x n values of a derivative image from (x0, y0), zero outside the image"""
    h, w = d.shape
    ys, xs = y0 + np.arange(n), x0 + np.arange(n)
    out = d[np.ix_(np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1))].copy()
    out[(ys < 0) | (ys >= h), :] = 0
    out[:, (xs < 0) | (xs >= w)] = 0
    return out


def _bilin(t, iw, shift):
    """the four-tap fixed-point interpolation of a (WIN + 1)^2 patch -> WIN x WIN"""
    return _descale(t[:-1, :-1] * iw[0] + t[:-1, 1:] * iw[1] + t[1:, :-1] * iw[2] + t[1:, 1:] * iw[3], shift)


def _ifloor(v):
    return int(np.floor(v))


def track_on_pyramids(pp, npyr, pts, init_pts=None):
    """-> (nextPts (K, 2) f32, status (K, 1) u8, err (K, 1) f32); init_pts (K, 2) or None"""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 2)
    K = len(pts)
    guess = pts if init_pts is None else np.ascontiguousarray(init_pts, F).reshape(-1, 2)
    assert guess.shape == pts.shape
    L = len(pp)
    nxt = np.zeros((K, 2), F)
    status = np.ones(K, np.uint8)
    err = np.zeros(K, F)
    half = F((WIN - 1) * 0.5)
    FLT_SCALE = F(1.0 / (1 << 20))
    eps2 = EPS * EPS
    two, half_f, four = F(2.0), F(0.5), F(4.0)
    for level in range(L - 1, -1, -1):
        I, J = pp[level], npyr[level]
        h, w = I.shape
        Dx, Dy = _scharr(I)
        scale = F(1.0 / (1 << level))
        for k in range(K):
            px, py = pts[k, 0] * scale, pts[k, 1] * scale
            if level == L - 1:
                nx, ny = guess[k, 0] * scale, guess[k, 1] * scale
            else:
                nx, ny = nxt[k, 0] * two, nxt[k, 1] * two
            nxt[k] = (nx, ny)
            px, py = px - half, py - half
            ipx, ipy = _ifloor(px), _ifloor(py)
            if ipx < -WIN or ipx >= w or ipy < -WIN or ipy >= h:
                if level == 0:
                    status[k] = 0
                    err[k] = 0
                continue
            iw = _weights(px - F(ipx), py - F(ipy))
            Iv = _bilin(_patch(I, ipx, ipy, WIN + 1), iw, W_BITS - 5)
            Ix = _bilin(_patch_zero(Dx, ipx, ipy, WIN + 1), iw, W_BITS)
            Iy = _bilin(_patch_zero(Dy, ipx, ipy, WIN + 1), iw, W_BITS)
            A11 = F(int((Ix * Ix).sum())) * FLT_SCALE
            A12 = F(int((Ix * Iy).sum())) * FLT_SCALE
            A22 = F(int((Iy * Iy).sum())) * FLT_SCALE
            D = A11 * A22 - A12 * A12
            dA = A11 - A22
            minEig = (A22 + A11 - np.sqrt(dA * dA + four * A12 * A12)) / F(2 * WIN * WIN)
            if minEig < MIN_EIG or D < F(1.1920929e-07):
                if level == 0:
                    status[k] = 0
                continue
            D = F(1.0) / D
            nx, ny = nx - half, ny - half
            pdx = pdy = F(0.0)
            for j in range(MAX_ITER):
                inx, iny = _ifloor(nx), _ifloor(ny)
                if inx < -WIN or inx >= w or iny < -WIN or iny >= h:
                    if level == 0:
                        status[k] = 0
                    break
                jw = _weights(nx - F(inx), ny - F(iny))
                diff = _bilin(_patch(J, inx, iny, WIN + 1), jw, W_BITS - 5) - Iv
                b1 = F(int((diff * Ix).sum())) * FLT_SCALE
                b2 = F(int((diff * Iy).sum())) * FLT_SCALE
                dx = (A12 * b2 - A22 * b1) * D
                dy = (A12 * b1 - A11 * b2) * D
                nx, ny = nx + dx, ny + dy
                nxt[k] = (nx + half, ny + half)
                if dx * dx + dy * dy <= eps2:
                    break
                if j > 0 and abs(dx + pdx) < F(0.01) and abs(dy + pdy) < F(0.01):
                    nxt[k, 0] -= dx * half_f
                    nxt[k, 1] -= dy * half_f
                    break
                pdx, pdy = dx, dy
            if status[k] and level == 0:
                ex, ey = nxt[k, 0] - half, nxt[k, 1] - half
                iex, iey = _ifloor(ex), _ifloor(ey)
                if iex < -WIN or iex >= w or iey < -WIN or iey >= h:
                    status[k] = 0
                    continue
                ew = _weights(ex - F(iex), ey - F(iey))
                diff = _bilin(_patch(J, iex, iey, WIN + 1), ew, W_BITS - 5) - Iv
                err[k] = F(int(np.abs(diff).sum())) * (F(1.0) / F(32 * WIN * WIN))
    return nxt, status.reshape(-1, 1), err.reshape(-1, 1)


def track(prev_u8, next_u8, pts, init_pts=None):
    """cv2.calcOpticalFlowPyrLK(prev, next, pts[, init_pts, OPTFLOW_USE_INITIAL_FLOW]) with the reference's LK_PARAMS"""
    return track_on_pyramids(build_pyramid(prev_u8), build_pyramid(next_u8), pts, init_pts)


def count_good(status, err):
    """features the reference keeps: status & (err < ERR_THRESHOLD) (getTransformKLT.py:365)"""
    return int(((status.reshape(-1) != 0) & (err.reshape(-1) < ERR_THRESHOLD)).sum())
