"""The NumPy contract of the global map (csrc/loop_map.hip, include/roam_abi.h "global map"): the loop database's stored clouds taken to
the world frame at given poses and binned on a grid.  PARITY UNPINNED: nothing in the reference computes this (its Map.mapPoints is an
empty list).  Every operation is one float64 operation rounded once, in the order written here; what a cell accumulates are integers,
so no order of arrival can show.  The pose table (cos theta, sin theta) is an input: the tests take it from the library
(_ffi.map_pose_table, the host's libm), so nothing can round differently."""
import numpy as np

MAX_CELLS = 1 << 26
MAX_INDEX = 2.0 ** 50
ICP_MAX_COORD = 1e6


def pose_table(poses):
    """NumPy's own cosines and sines - what the library's table is compared with (to an ulp), not what the model multiplies with"""
    th = np.asarray(poses, np.float64).reshape(-1, 3)[:, 2]
    return np.stack([np.cos(th), np.sin(th)], axis=1)


def world(xy, pose, cs):
    """stored points (n, 2) of an entry with the pose (x, y, theta) and its table row (c, s) -> (wx, wy)"""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    px, py = xy[:, 0], xy[:, 1]
    c, s = np.float64(cs[0]), np.float64(cs[1])
    wx = ((c * px) - (s * py)) + np.float64(pose[0])
    wy = ((s * px) + (c * py)) + np.float64(pose[1])
    return wx, wy


def cells(wx, wy, res, ox, oy, W, H):
    """-> (inside mask, u, v, qx, qy of the points inside; int64)"""
    res, ox, oy = np.float64(res), np.float64(ox), np.float64(oy)
    dx, dy = (wx - ox) / res, (wy - oy) / res
    inside = (dx >= 0.0) & (dx < np.float64(W)) & (dy >= 0.0) & (dy < np.float64(H))
    dx, dy = dx[inside], dy[inside]
    fu, fv = np.floor(dx), np.floor(dy)
    qx, qy = np.floor((dx - fu) * 65536.0), np.floor((dy - fv) * 65536.0)
    return inside, fu.astype(np.int64), fv.astype(np.int64), qx.astype(np.int64), qy.astype(np.int64)


def _used(n, use):
    return [e for e in range(n) if use is None or use[e]]


def render(clouds, poses, cs, res, extent, min_hits=1, min_views=1, use=None):
    """clouds: one (n, 2) array per entry; poses (count, 3); cs (count, 2); extent (ox, oy, W, H) -> dict: hits, views (H, W) uint32,
    sx, sy (H, W) uint64, points (M, 2) float64, point_hits, point_views (M,) uint32, outside"""
    ox, oy, W, H = extent
    hits, views = np.zeros(W * H, np.uint32), np.zeros(W * H, np.uint32)
    sx, sy = np.zeros(W * H, np.uint64), np.zeros(W * H, np.uint64)
    outside = 0
    for e in _used(len(clouds), use):
        wx, wy = world(clouds[e], poses[e], cs[e])
        inside, u, v, qx, qy = cells(wx, wy, res, ox, oy, W, H)
        outside += int(np.count_nonzero(~inside))
        if not len(u):
            continue
        k, inv, cnt = np.unique(v * W + u, return_inverse=True, return_counts=True)
        hits[k] += cnt.astype(np.uint32)
        views[k] += np.uint32(1)
        bx, by = np.bincount(inv, weights=qx.astype(np.float64)), np.bincount(inv, weights=qy.astype(np.float64))      # < 8192 * 65536: exact
        sx[k] += bx.astype(np.uint64)
        sy[k] += by.astype(np.uint64)
    q = np.flatnonzero((hits >= min_hits) & (views >= min_views))             # row-major: v major
    h = hits[q].astype(np.uint64)
    den = 131072.0 * h.astype(np.float64)
    mx, my = (2 * sx[q] + h).astype(np.float64) / den, (2 * sy[q] + h).astype(np.float64) / den
    res = np.float64(res)
    cx = np.float64(ox) + res * ((q % W).astype(np.float64) + mx)
    cy = np.float64(oy) + res * ((q // W).astype(np.float64) + my)
    return dict(hits=hits.reshape(H, W), views=views.reshape(H, W), sx=sx.reshape(H, W), sy=sy.reshape(H, W), points=np.stack([cx, cy], axis=1),
                point_hits=hits[q], point_views=views[q], outside=outside)


def bounds(clouds, poses, cs, use=None):
    """-> ((min wx, max wx, min wy, max wy) float64 - a zero is +0; +inf, -inf, +inf, -inf without a point -, the number of points)"""
    b, n = np.array([np.inf, -np.inf, np.inf, -np.inf]), 0
    for e in _used(len(clouds), use):
        wx, wy = world(clouds[e], poses[e], cs[e])
        if len(wx):
            wx, wy = wx + 0.0, wy + 0.0
            b = np.array([min(b[0], wx.min()), max(b[1], wx.max()), min(b[2], wy.min()), max(b[3], wy.max())])
            n += len(wx)
    return b, n


def plan(minx, maxx, miny, maxy, res):
    """the automatic extent -> (ox, oy, W, H).  ValueError("arg") / ValueError("capacity") where roam_map_plan returns ROAM_E_ARG /
    ROAM_E_CAPACITY"""
    v = [np.float64(t) for t in (minx, maxx, miny, maxy, res)]
    minx, maxx, miny, maxy, res = v
    if not all(np.isfinite(t) for t in v) or minx > maxx or miny > maxy or not res > 0.0:
        raise ValueError("arg")
    fx, fy = np.floor(minx / res), np.floor(miny / res)
    if not (abs(fx) <= MAX_INDEX and abs(fy) <= MAX_INDEX):
        raise ValueError("arg")
    ox, oy = (fx - 1.0) * res, (fy - 1.0) * res
    w, h = np.floor((maxx - ox) / res) + 2.0, np.floor((maxy - oy) / res) + 2.0
    if not (w <= MAX_CELLS and h <= MAX_CELLS and w * h <= MAX_CELLS):
        raise ValueError("capacity")
    return float(ox), float(oy), int(w), int(h)
