"""NumPy restatement of the pyramidal Lucas-Kanade tracker, operation by operation in float32 / integer arithmetic as
oracle_klt_track (oracle/c/warp_klt.c) and klt_kernel (csrc/pyrklt.hip) do it, with the one thing the oracle does not have: an optional
start of the search, cv2.calcOpticalFlowPyrLK's OPTFLOW_USE_INITIAL_FLOW.  OpenCV's rule (lkpyramid.cpp, restated): at the top
level only, nextPt = init_pts * 2^-maxLevel in place of prevPt; everything else is the unseeded tracker.

Unseeded it is tied to the oracle bit for bit by tests/test_klt_flow_cpu.py; apply_affine is the float32 order in which the kernel
turns a lane's affine prior into guesses.  An optional trace says which branch each (point, level) took and how large its window sums
were (tests/klt_branch_cases.py); the tile bookkeeping in it restates klt_kernel's rule and takes no part in any result."""
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


def _wsum(p, what):
    """an exact window sum (Python int) of the normal matrix (what = "A") or the mismatch vector ("b"): the one place a test swaps for
    narrower arithmetic, to see that its cases would notice"""
    return int(p.sum())


GROUP_ROWS = ((0, 4), (4, 8), (8, 12), (12, 15))      # window rows summed in 32 bits by one 16-lane DPP row of klt_kernel
SUM_NAMES = ("IxIx", "IxIy", "IyIy", "dIx", "dIy")
TILE = 32                                              # klt_kernel's cached neighbourhood of the next image
TILE_KEEP = 15                                         # the tile is kept while 0 <= inx - tx0 <= TILE_KEEP, likewise in y


def _note_sums(e, names, prods):
    """largest |sum| per 4-window-row group and over the whole window, kept in the trace entry e"""
    for name, p in zip(names, prods):
        g = max(abs(int(p[a:b].sum())) for a, b in GROUP_ROWS)
        e["group"][name] = max(e["group"][name], g)
        e["whole"][name] = max(e["whole"][name], abs(int(p.sum())))


def _tile_sides(tx0, ty0, w, h):
    """the sides on which a TILE x TILE tile at (tx0, ty0) leaves a w x h image: empty = load_j_tile's interior path"""
    return frozenset(n for n, out in (("left", tx0 < 0), ("right", tx0 + TILE > w), ("top", ty0 < 0), ("bottom", ty0 + TILE > h)) if out)


def _tile_step(e, tile, ix, iy, w, h):
    """klt_kernel's tile rule restated (trace only): reload with origin (ix - 8, iy - 8) unless the window origin is 0 ... 15 from the
    cached one; -> (tile origin, the directions in which the window left the old tile: None = kept, () = the level's first load)"""
    if tile is not None and 0 <= ix - tile[0] <= TILE_KEEP and 0 <= iy - tile[1] <= TILE_KEEP:
        return tile, None
    dirs = ()
    if tile is not None:
        dirs = tuple(n for n, out in (("+x", ix - tile[0] > TILE_KEEP), ("-x", ix < tile[0]), ("+y", iy - tile[1] > TILE_KEEP),
                                      ("-y", iy < tile[1])) if out)
    tile = (ix - 8, iy - 8)
    e["tiles"].append(_tile_sides(tile[0], tile[1], w, h))
    return tile, dirs


def track_on_pyramids(pp, npyr, pts, init_pts=None, trace=None):
    """-> (nextPts (K, 2) f32, status (K, 1) u8, err (K, 1) f32); init_pts (K, 2) or None.
    trace: None, or a list that receives one dict per (point, level), levels from the top down, which changes no result:
      k, level; exit: "prev_outside", "mineig", "d_only" (minEig passes, D < FLT_EPSILON), "eps0" (|d|^2 <= eps^2 at j == 0), "eps"
      (at j >= 1), "backoff", "maxiter" or "left" (the window left the image in mid-iteration); iters: mismatch vectors formed;
      reloads: per reload after the level's first load, the directions in which the window left the tile; tiles: per loaded tile, the
      sides on which it leaves the image (empty: interior path), the error patch's load included; err_reload: the error patch needed a
      load; err_outside: the final position was outside the image after iterations inside it; group / whole: largest |sum| of SUM_NAMES
      per group of GROUP_ROWS and over the window"""
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
            e = None
            if trace is not None:
                e = dict(k=k, level=level, exit="prev_outside", iters=0, reloads=[], tiles=[], err_reload=False, err_outside=False,
                         group=dict.fromkeys(SUM_NAMES, 0), whole=dict.fromkeys(SUM_NAMES, 0))
                trace.append(e)
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
            A11 = F(_wsum(Ix * Ix, "A")) * FLT_SCALE
            A12 = F(_wsum(Ix * Iy, "A")) * FLT_SCALE
            A22 = F(_wsum(Iy * Iy, "A")) * FLT_SCALE
            D = A11 * A22 - A12 * A12
            dA = A11 - A22
            minEig = (A22 + A11 - np.sqrt(dA * dA + four * A12 * A12)) / F(2 * WIN * WIN)
            if e is not None:
                _note_sums(e, SUM_NAMES[:3], (Ix * Ix, Ix * Iy, Iy * Iy))
                e["exit"] = "mineig" if minEig < MIN_EIG else "d_only" if D < F(1.1920929e-07) else "maxiter"
            if minEig < MIN_EIG or D < F(1.1920929e-07):
                if level == 0:
                    status[k] = 0
                continue
            D = F(1.0) / D
            nx, ny = nx - half, ny - half
            pdx = pdy = F(0.0)
            tile = None
            for j in range(MAX_ITER):
                inx, iny = _ifloor(nx), _ifloor(ny)
                if inx < -WIN or inx >= w or iny < -WIN or iny >= h:
                    if level == 0:
                        status[k] = 0
                    if e is not None:
                        e["exit"] = "left"
                    break
                if e is not None:
                    tile, dirs = _tile_step(e, tile, inx, iny, w, h)
                    if dirs:
                        e["reloads"].append(dirs)
                jw = _weights(nx - F(inx), ny - F(iny))
                diff = _bilin(_patch(J, inx, iny, WIN + 1), jw, W_BITS - 5) - Iv
                if e is not None:
                    e["iters"] = j + 1
                    _note_sums(e, SUM_NAMES[3:], (diff * Ix, diff * Iy))
                b1 = F(_wsum(diff * Ix, "b")) * FLT_SCALE
                b2 = F(_wsum(diff * Iy, "b")) * FLT_SCALE
                dx = (A12 * b2 - A22 * b1) * D
                dy = (A12 * b1 - A11 * b2) * D
                nx, ny = nx + dx, ny + dy
                nxt[k] = (nx + half, ny + half)
                if dx * dx + dy * dy <= eps2:
                    if e is not None:
                        e["exit"] = "eps0" if j == 0 else "eps"
                    break
                if j > 0 and abs(dx + pdx) < F(0.01) and abs(dy + pdy) < F(0.01):
                    nxt[k, 0] -= dx * half_f
                    nxt[k, 1] -= dy * half_f
                    if e is not None:
                        e["exit"] = "backoff"
                    break
                pdx, pdy = dx, dy
            if status[k] and level == 0:
                ex, ey = nxt[k, 0] - half, nxt[k, 1] - half
                iex, iey = _ifloor(ex), _ifloor(ey)
                if iex < -WIN or iex >= w or iey < -WIN or iey >= h:
                    status[k] = 0
                    if e is not None:
                        e["err_outside"] = True
                    continue
                if e is not None:
                    assert tile is not None                 # status 1 at level 0: an iteration ran and loaded a tile
                    e["err_reload"] = _tile_step(e, tile, iex, iey, w, h)[1] is not None
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
