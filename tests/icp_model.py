"""NumPy model of the batched 2-D ICP (include/roam_abi.h roam_icp2d_batch, csrc/icp.hip): the contract of the loop-closure
verification, which has no counterpart in the reference.  Nothing here touches a device.

icp(src, dst, init, **opts) restates the kernel operation by operation:
  * q = R(th) src + t in float64, (c x - s y) + tx and (s x + c y) + ty with every operation rounded, then rounded to float32; dst
    rounded to float32;
  * d2 = fl32(fl32(dx dx) + fl32(dy dy)) on float32 differences, no fused multiply-add; np.argmin returns the lowest index of the minimum;
  * kept: d2 <= fl32(g g);
  * sums in the kernel's order (`order="kernel"`): lane l of 512 adds its points i = l, l + 512, ... from zero, a wave of 64 lanes adds
    by the xor butterfly 32, 16, ... 1, the eight waves are added in order; centroids first, then the centred sums in a second pass;
  * th' = atan2(S_sin, S_cos), th when both are exactly zero; t' = bm - R(th') am;
  * the stopping rule and the scoring pass at gate_end.
The variants measure how much the freedoms a device has move the result (tests/icp_cases.py tolerance()): `search_form="fma"` contracts
dx dx + dy dy to a fused multiply-add (emulated in float64: the product of two float32 is exact there), `order="sequential"` /
`order="pairwise"` sum in other orders, `nudge` moves every transformed float32 point by one ulp."""
import numpy as np

OK, MAX_ITERATIONS, FEW_PAIRS = 0, 1, 2
DEFAULTS = dict(gate_start=3.0, gate_end=0.5, gate_decay=0.8, max_iterations=40, eps_trans=1e-4, eps_rot=1e-5, min_pairs=3)
THREADS, WAVE = 512, 64
_XOR = [np.arange(WAVE) ^ d for d in (32, 16, 8, 4, 2, 1)]


def _sum(v, order):
    """the sum of a float64 vector v - one entry per src point, zero where the pair is not kept - in the given order"""
    v = np.asarray(v, np.float64)
    if order == "pairwise":
        return float(np.sum(v))
    if order == "sequential":
        s = 0.0
        for x in v.tolist():
            s += x
        return s
    rows = -(-len(v) // THREADS)
    pad = np.zeros(rows * THREADS)
    pad[:len(v)] = v
    lanes = np.zeros(THREADS)
    for r in pad.reshape(rows, THREADS):          # a lane's points in ascending i; a point that is not kept adds +0.0, which changes nothing
        lanes = lanes + r
    w = lanes.reshape(THREADS // WAVE, WAVE)
    for idx in _XOR:
        w = w + w[:, idx]
    s = w[0, 0]
    for k in range(1, THREADS // WAVE):
        s = s + w[k, 0]
    return float(s)


def normalize_angle(th):
    """utils.normalize_angles / roam_normalize_angle: (th + pi) % (2 pi) - pi with Python's modulo"""
    return (th + np.pi) % (2.0 * np.pi) - np.pi


def transform(src, th, tx, ty):
    c, s = np.cos(th), np.sin(th)
    return (c * src[:, 0] - s * src[:, 1]) + tx, (s * src[:, 0] + c * src[:, 1]) + ty


def search(src, dst32, th, tx, ty, gate2, search="plain", nudge=0, block=512):
    """-> (partner (n,) int64, kept (n,) bool): the float32 nearest neighbour of every transformed point and the gate"""
    qx, qy = transform(src, th, tx, ty)
    qx, qy = qx.astype(np.float32), qy.astype(np.float32)
    if nudge:
        to = np.float32(np.inf if nudge > 0 else -np.inf)
        qx, qy = np.nextafter(qx, to), np.nextafter(qy, to)
    n = len(src)
    part = np.zeros(n, np.int64)
    best = np.zeros(n, np.float32)
    bx, by = dst32[:, 0][None, :], dst32[:, 1][None, :]
    for i0 in range(0, n, block):
        dx = qx[i0:i0 + block, None] - bx
        dy = qy[i0:i0 + block, None] - by
        if search == "fma":
            d2 = (dx.astype(np.float64) * dx.astype(np.float64) + (dy * dy).astype(np.float64)).astype(np.float32)
        else:
            d2 = dx * dx + dy * dy                 # float32 throughout: each product and the sum rounded once
        j = np.argmin(d2, axis=1)
        part[i0:i0 + block] = j
        best[i0:i0 + block] = d2[np.arange(len(j)), j]
    return part, best <= np.float32(gate2)


def icp(src, dst, init=(0.0, 0.0, 0.0), search_form="plain", order="kernel", nudge=0, trace=None, **opts):
    """-> (pose (3,) [th, tx, ty], stats dict(status, iterations, n_pairs_last, n_inliers, rms))"""
    o = dict(DEFAULTS, **opts)
    src = np.ascontiguousarray(src, np.float64).reshape(-1, 2)
    dst = np.ascontiguousarray(dst, np.float64).reshape(-1, 2)
    th, tx, ty = (float(v) for v in init)
    n, m = len(src), len(dst)
    status, iterations, n_last = MAX_ITERATIONS, 0, 0
    if n < 1 or m < 1:
        return np.array([th, tx, ty]), dict(status=FEW_PAIRS, iterations=0, n_pairs_last=0, n_inliers=0, rms=np.inf)
    dst32 = dst.astype(np.float32)
    g = float(o["gate_start"])
    for it in range(o["max_iterations"]):
        part, kept = search(src, dst32, th, tx, ty, np.float32(g * g), search_form, nudge)
        if trace is not None:
            trace.append((part.copy(), kept.copy()))
        k = kept.astype(np.float64)
        a, b = src, dst[part]
        cnt = _sum(k, order)
        n_last = int(cnt)
        if n_last < o["min_pairs"]:
            status = FEW_PAIRS
            break
        amx, amy = _sum(a[:, 0] * k, order) / cnt, _sum(a[:, 1] * k, order) / cnt
        bmx, bmy = _sum(b[:, 0] * k, order) / cnt, _sum(b[:, 1] * k, order) / cnt
        ax, ay, bx, by = a[:, 0] - amx, a[:, 1] - amy, b[:, 0] - bmx, b[:, 1] - bmy
        s_cos = _sum(np.where(kept, ax * bx + ay * by, 0.0), order)
        s_sin = _sum(np.where(kept, ax * by - ay * bx, 0.0), order)
        th2 = th if (s_cos == 0.0 and s_sin == 0.0) else float(np.arctan2(s_sin, s_cos))
        c2, s2 = np.cos(th2), np.sin(th2)
        tx2, ty2 = bmx - (c2 * amx - s2 * amy), bmy - (s2 * amx + c2 * amy)
        dth = abs(normalize_angle(th2 - th))
        ex, ey = tx2 - tx, ty2 - ty
        dt = np.sqrt(ex * ex + ey * ey)
        th, tx, ty = th2, float(tx2), float(ty2)
        iterations = it + 1
        if g == o["gate_end"] and dth < o["eps_rot"] and dt < o["eps_trans"]:
            status = OK
            break
        g = max(float(o["gate_end"]), g * o["gate_decay"])
    ge = float(o["gate_end"])
    part, kept = search(src, dst32, th, tx, ty, np.float32(ge * ge), search_form, nudge)
    qx, qy = transform(src, th, tx, ty)
    ex, ey = qx - dst[part, 0], qy - dst[part, 1]
    n_in = int(_sum(kept.astype(np.float64), order))
    rms = float(np.sqrt(_sum(np.where(kept, ex * ex + ey * ey, 0.0), order) / n_in)) if n_in else np.inf
    return np.array([th, tx, ty]), dict(status=status, iterations=iterations, n_pairs_last=n_last, n_inliers=n_in, rms=rms)


def relative_pose(pi, pj):
    """x_i^-1 x_j of two poses (x, y, theta) -> (tx, ty, theta)"""
    c, s = np.cos(pi[2]), np.sin(pi[2])
    dx, dy = pj[0] - pi[0], pj[1] - pi[1]
    return np.array([c * dx + s * dy, c * dy - s * dx, normalize_angle(pj[2] - pi[2])])
