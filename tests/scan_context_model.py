"""The contract of the loop-closure candidates (radarslampy_amd/csrc/loop_describe.hip, loop_query.hip, radarslampy_amd/LoopClosure.py): the radar scan
context of Kim et al. (the MulRan data set) in NumPy, float64.  Nothing in the reference computes this (Mapping.py:7 is a
commented-out "import m2dp"), so parity is unpinned and this file is what the device is held to.

Bins.  clip = clip_px if 0 < clip_px < cols else cols; sector s covers the rows [floor(s rows / S), floor((s + 1) rows / S)), ring r
the columns [floor(r clip / R), floor((r + 1) clip / R)), integer arithmetic; rows >= S and clip >= R, so no bin is empty.
Descriptor D[s][r], float32.  u8 codes k, integer floor f: (float)((double)sum max(k - f, 0) / (255.0 count)) - the sum is an exact
integer.  float32 values v, float floor f >= 0: (float)(sum max((double)v - (double)f, 0) / count), the sum in float64.
Distance.  Sector s is valid at shift k when |q[s]| |c[(s + k) mod S]| > 0; d_k = 1 - (1 / count_k) sum over the valid s of
q[s] . c[(s + k) mod S] / (|q[s]| |c[(s + k) mod S]|), 1 when count_k = 0; distance = min_k d_k, shift = the lowest such k.
Candidates of query i: among the entries j < max_index[i] with distance <= max_distance the k smallest by (distance, index);
unused slots hold -1, +inf, 0."""
import numpy as np


def clip_of(cols, clip_px):
    return int(clip_px) if clip_px is not None and 0 < clip_px < cols else int(cols)


def bin_edges(rows, cols, clip_px, S, R):
    """-> (row_edges (S + 1,), col_edges (R + 1,)) int"""
    clip = clip_of(cols, clip_px)
    assert rows >= S and clip >= R
    return np.array([s * rows // S for s in range(S + 1)]), np.array([r * clip // R for r in range(R + 1)])


def _bin_sums(vals, re, ce):
    """vals (rows, >= clip) of an exact or float64 type -> (S, R) sums and the cell counts"""
    rows_cum = np.add.reduceat(vals[:, :ce[-1]], re[:-1], axis=0)
    sums = np.add.reduceat(rows_cum, ce[:-1], axis=1)
    return sums, np.outer(np.diff(re), np.diff(ce))


def describe_u8(codes, S, R, clip_px=None, floor_code=0):
    """codes: (rows, cols) uint8 record payload -> (S, R) float32"""
    codes = np.asarray(codes)
    assert codes.dtype == np.uint8 and 0 <= floor_code <= 254
    re, ce = bin_edges(codes.shape[0], codes.shape[1], clip_px, S, R)
    sums, cnt = _bin_sums(np.maximum(codes.astype(np.int64) - int(floor_code), 0), re, ce)
    return (sums.astype(np.float64) / (255.0 * cnt)).astype(np.float32)


def describe_f32(img, S, R, clip_px=None, floor=0.0):
    """img: (rows, cols) float32 -> (S, R) float32"""
    img = np.asarray(img)
    assert img.dtype == np.float32 and floor >= 0
    re, ce = bin_edges(img.shape[0], img.shape[1], clip_px, S, R)
    sums, cnt = _bin_sums(np.maximum(img.astype(np.float64) - np.float64(floor), 0.0), re, ce)
    return (sums / cnt).astype(np.float32)


def _diagonals(M2):
    """M2 (n, S, 2S), a matrix [j, s, t] doubled along t -> a view V (n, S, S): V[j, s, k] = M2[j, s, s + k] = M[j, s, (s + k) mod S]"""
    n, S, S2 = M2.shape
    a, b, c = M2.strides
    return np.lib.stride_tricks.as_strided(M2, shape=(n, S, S), strides=(a, b + c, c), writeable=False)


def _doubled_t(C):
    """C (n, S, ...) -> (n, ..., 2S): the sector axis last and doubled"""
    return np.ascontiguousarray(np.concatenate([C, C], axis=1).swapaxes(1, -1)) if C.ndim == 3 else np.concatenate([C, C], axis=1)


def prepare(C):
    """what the two evaluations below need of the candidates C (n, S, R), made once for many queries"""
    C = np.asarray(C, np.float64)
    nc = np.sqrt((C * C).sum(axis=2))
    Cn = np.where(nc[:, :, None] > 0, C / np.where(nc > 0, nc, 1.0)[:, :, None], 0.0)
    return _doubled_t(C), _doubled_t(nc), _doubled_t(Cn)


def shift_distances(q, C, prep=None):
    """q (S, R), C (n, S, R) float32 descriptors -> d (n, S) float64: d[j, k] = d_k of (q, C[j])"""
    q = np.asarray(q, np.float64)
    C2, nc2, _ = prep or prepare(C)
    nq = np.sqrt((q * q).sum(axis=1))
    M = np.matmul(q, C2)                                         # raw dots [j, s, t], t < 2S
    den = nq[None, :, None] * nc2[:, None, :]
    ok = den > 0
    term = np.where(ok, M / np.where(ok, den, 1.0), 0.0)
    cnt = _diagonals(ok).sum(axis=1)
    tot = _diagonals(term).sum(axis=1)
    return np.where(cnt > 0, 1.0 - tot / np.maximum(cnt, 1), 1.0)


def distances(Q, C):
    """Q (m, S, R), C (n, S, R) -> (dist (m, n) float64, shift (m, n) int32, second (m, n): the second smallest d_k, +inf for S = 1)"""
    m, n = len(Q), len(C)
    dist, shift, second = np.empty((m, n)), np.empty((m, n), np.int32), np.empty((m, n))
    prep = prepare(C)
    for i in range(m):
        d = shift_distances(Q[i], C, prep)
        shift[i] = d.argmin(axis=1)                              # the first of equal minima
        dist[i] = d[np.arange(n), shift[i]]
        second[i] = np.partition(d, 1, axis=1)[:, 1] if d.shape[1] > 1 else np.inf
    return dist, shift, second


def distance(q, c):
    d, s, _ = distances(np.asarray(q)[None], np.asarray(c)[None])
    return float(d[0, 0]), int(s[0, 0])


def distance_brute(q, c):
    """the same definition, loop by loop (an independent evaluation for the CPU test) -> (distance, shift, d_k list)"""
    S, R = q.shape
    out = []
    for k in range(S):
        tot, cnt = 0.0, 0
        for s in range(S):
            t = (s + k) % S
            nq = float(np.sqrt(sum(float(q[s, r]) ** 2 for r in range(R))))
            nc = float(np.sqrt(sum(float(c[t, r]) ** 2 for r in range(R))))
            if nq * nc > 0:
                tot += sum(float(q[s, r]) * float(c[t, r]) for r in range(R)) / (nq * nc)
                cnt += 1
        out.append(1.0 - tot / cnt if cnt else 1.0)
    k = min(range(S), key=lambda kk: (out[kk], kk))
    return out[k], k, out


# ---- the device's arithmetic: float64, normalised columns, the order of loop_distance_kernel
LDS_BYTES = 32768


def phase_rings(S, R):
    """rings of one LDS phase of the distance kernel (csrc/loop_query.hip sc_phase_rings): R padded to a multiple of four, or the
    largest multiple of four whose doubled candidate (2S + 1 float64 per ring) fits 32 KiB"""
    Rp = (R + 3) & ~3
    return min(Rp, (LDS_BYTES // (8 * (2 * S + 1))) & ~3)


def shift_distances_kernel_order(q, C, prep=None):
    """shift_distances in the order the kernel sums in: columns divided by their norms first; per phase of phase_rings(S, R) rings
    and per sector the dot of the phase's rings, those added serially (phase-major, sector ascending) to the shift's accumulator;
    d_k = 1 - sum / count.  (The dots of at most 32 rings are left to the BLAS: their rounding is far below the serial sum's.)"""
    q = np.asarray(q, np.float64)
    S, R = q.shape
    _, nc2, Cn2 = prep or prepare(C)
    nq = np.sqrt((q * q).sum(axis=1))
    qn = np.where(nq[:, None] > 0, q / np.where(nq > 0, nq, 1.0)[:, None], 0.0)
    RL = phase_rings(S, R)
    tot = np.zeros((len(C), S))
    for r0 in range(0, R, RL):
        Md = _diagonals(np.matmul(qn[:, r0:r0 + RL], Cn2[:, r0:r0 + RL, :]))
        for s in range(S):                                       # one serial chain per (candidate, shift)
            tot += Md[:, s, :]
    cnt = _diagonals((nq > 0)[None, :, None] & (nc2 > 0)[:, None, :]).sum(axis=1)
    return np.where(cnt > 0, 1.0 - tot / np.maximum(cnt, 1), 1.0)


def candidates(dist, shift, max_index, max_distance, k):
    """dist, shift (m, n); max_index (m,) -> (index (m, k) int32, distance (m, k) float64, shift (m, k) int32)"""
    m, n = dist.shape
    ci, cd, cs = np.full((m, k), -1, np.int32), np.full((m, k), np.inf), np.zeros((m, k), np.int32)
    for i in range(m):
        lim = int(min(max(max_index[i], 0), n))
        js = [j for j in range(lim) if dist[i, j] <= max_distance]
        js.sort(key=lambda j: (dist[i, j], j))
        for slot, j in enumerate(js[:k]):
            ci[i, slot], cd[i, slot], cs[i, slot] = j, dist[i, j], shift[i, j]
    return ci, cd, cs


def shift_to_yaw(shift, S):
    """yaw(query) - yaw(candidate) in (-pi, pi] for rows = atan2(y, x) rows / 2 pi"""
    a = 2.0 * np.pi * np.asarray(shift, np.float64) / S
    return np.where(a > np.pi, a - 2.0 * np.pi, a)
