"""The NumPy contract of the map matching (csrc/map_match.hip, include/roam_abi.h "map matching"): a scan placed in a rendered global map
by correlative scan-to-map matching.  PARITY UNPINNED: nothing in the reference computes this (its Map.mapPoints is an empty list with
a TODO).  Every floating-point step is one float64 operation rounded once, in the order written here; everything accumulated is an
integer, so no order of arrival can show.  The two tables that need libm - the smear table (exp) and the angle table (cos, sin) - are
inputs: the tests take them from the library (_ffi.map_field_table, _ffi.map_match_angles, the host's libm), so nothing can round
differently; field_table and angles below are NumPy's own, what the library's are compared with.

A translation is an exact shift of the cell index: candidate (i, b, a) reads the field at (v + b - ky, u + a - kx) for the cell (u, v)
that the point has at angle i and at the prior's position.  It is not a re-binning of a translated point, which would round again."""
import numpy as np

from global_map_model import world

MAX_RADIUS, MAX_ANGLES, MAX_SHIFT, MAX_VOLUME = 8, 1025, 128, 1 << 26
FAR = 2.0 ** 30


def field_table(sigma, radius):
    """NumPy's own smear table (2 r + 1, 2 r + 1) uint8 - compared with the library's to a count, not what the model smears with"""
    d = np.arange(-radius, radius + 1, dtype=np.float64)
    d2 = d[:, None] * d[:, None] + d[None, :] * d[None, :]
    return np.floor(255.0 * np.exp(-d2 / (2.0 * np.float64(sigma) * np.float64(sigma))) + 0.5).astype(np.uint8)


def field(hits, views, min_hits, min_views, radius, table):
    """F[v][u] = the maximum of table[dv + r][du + r] over the occupied cells (v + dv, u + du) inside the grid, |dv|, |du| <= r; 0
    without one -> (H, W) uint8"""
    occ = (np.asarray(hits) >= min_hits) & (np.asarray(views) >= min_views)
    H, W = occ.shape
    table = np.asarray(table, np.uint8).reshape(2 * radius + 1, 2 * radius + 1)
    big = np.zeros((H + 2 * radius, W + 2 * radius), bool)
    big[radius:radius + H, radius:radius + W] = occ
    out = np.zeros((H, W), np.uint8)
    for dv in range(-radius, radius + 1):
        for du in range(-radius, radius + 1):
            shifted = big[radius + dv:radius + dv + H, radius + du:radius + du + W]      # shifted[v][u] = occ[v + dv][u + du]
            out = np.maximum(out, np.where(shifted, table[dv + radius, du + radius], np.uint8(0)))
    return out


def thetas(th0, n_theta, step_rad):
    """th_i = th0 + float(i - c) * step_rad, c = (n_theta - 1) / 2: two operations"""
    c = (n_theta - 1) // 2
    return np.float64(th0) + (np.arange(n_theta) - c).astype(np.float64) * np.float64(step_rad)


def angles(prior, n_theta, step_rad):
    """NumPy's own (n_theta, 2) rows (cos th_i, sin th_i) - compared with the library's to an ulp, not what the model multiplies with"""
    th = thetas(prior[2], n_theta, step_rad)
    return np.stack([np.cos(th), np.sin(th)], axis=1)


def cells(xy, prior, cs_row, res, ox, oy):
    """the cloud at the prior's position and the angle of cs_row = (c, s) -> (u, v) int64 of the points that are not far, and their
    number; far: not -2^30 <= dx < 2^30, or dy likewise, compared in float64 before any conversion"""
    wx, wy = world(xy, prior, cs_row)
    dx, dy = (wx - np.float64(ox)) / np.float64(res), (wy - np.float64(oy)) / np.float64(res)
    near = (dx >= -FAR) & (dx < FAR) & (dy >= -FAR) & (dy < FAR)
    return np.floor(dx[near]).astype(np.int64), np.floor(dy[near]).astype(np.int64)


def _lookup(F, u, v):
    """F[v][u] as uint32, 0 outside the grid"""
    H, W = F.shape
    ok = (u >= 0) & (u < W) & (v >= 0) & (v < H)
    out = np.zeros(len(u), np.uint32)
    out[ok] = F[v[ok], u[ok]]
    return out


def volume_loops(F, xy, prior, cs, res, ox, oy, kx, ky):
    """the definition as the literal triple loop -> (n_theta, 2 ky + 1, 2 kx + 1) uint32"""
    out = np.zeros((len(cs), 2 * ky + 1, 2 * kx + 1), np.uint32)
    for i in range(len(cs)):
        u, v = cells(xy, prior, cs[i], res, ox, oy)
        for b in range(2 * ky + 1):
            for a in range(2 * kx + 1):
                out[i, b, a] = _lookup(F, u + (a - kx), v + (b - ky)).sum(dtype=np.uint32)
    return out


def volume(F, xy, prior, cs, res, ox, oy, kx, ky):
    """the same, vectorised: the points' cells are counted into a grid the size of the field plus the window, and a score is the sum of
    count times field over the overlap - integers throughout"""
    H, W = F.shape
    out = np.zeros((len(cs), 2 * ky + 1, 2 * kx + 1), np.uint32)
    Fp = np.zeros((H + 4 * ky, W + 4 * kx), np.int64)                     # the field with 2 k zeros on every side
    Fp[2 * ky:2 * ky + H, 2 * kx:2 * kx + W] = F
    for i in range(len(cs)):
        u, v = cells(xy, prior, cs[i], res, ox, oy)
        keep = (u >= -kx) & (u < W + kx) & (v >= -ky) & (v < H + ky)      # a point further out reaches the grid under no shift
        if not keep.any():
            continue
        cnt = np.zeros((H + 2 * ky, W + 2 * kx), np.int64)                # cnt[v + ky][u + kx]
        np.add.at(cnt, (v[keep] + ky, u[keep] + kx), 1)
        rows, cols = np.nonzero(cnt)
        w = cnt[rows, cols]
        B, A = np.arange(2 * ky + 1)[None, :, None], np.arange(2 * kx + 1)[None, None, :]
        acc = np.zeros(out.shape[1:], np.int64)
        for k in range(0, len(w), 1024):                                  # Fp[(v + ky) + b][(u + kx) + a] = F[v + b - ky][u + a - kx]
            r, c = rows[k:k + 1024, None, None], cols[k:k + 1024, None, None]
            acc += (w[k:k + 1024, None, None] * Fp[r + B, c + A]).sum(axis=0)
        out[i] = acc
    return out


def best(vol):
    """the largest score, among ties the lowest flat index -> (score, i, b, a)"""
    flat = int(np.argmax(vol.reshape(-1)))                                # argmax returns the first of the maxima
    i, rem = divmod(flat, vol.shape[1] * vol.shape[2])
    b, a = divmod(rem, vol.shape[2])
    return int(vol[i, b, a]), i, b, a


def match(F, xy, prior, cs, step_rad, res, ox, oy, kx, ky, vol=None):
    """one query -> (pose (3,) float64, info (6,) int32: score, i, b, a, n_points, n_inside, the volume)"""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    vol = volume(F, xy, prior, cs, res, ox, oy, kx, ky) if vol is None else vol
    score, i, b, a = best(vol)
    u, v = cells(xy, prior, cs[i], res, ox, oy)
    H, W = F.shape
    x, y = u + (a - kx), v + (b - ky)
    n_inside = int(np.count_nonzero((x >= 0) & (x < W) & (y >= 0) & (y < H)))
    pose = np.array([np.float64(prior[0]) + np.float64(a - kx) * np.float64(res), np.float64(prior[1]) + np.float64(b - ky) * np.float64(res),
                     thetas(prior[2], len(cs), step_rad)[i]], np.float64)
    return pose, np.array([score, i, b, a, len(xy), n_inside], np.int32), vol
