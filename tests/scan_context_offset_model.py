"""The contract of the origin-shifted scan context (radarslampy_amd/csrc/loop_offset.hip, the offset entries of loop_query.hip and
loop_verify.hip, LoopClosure.LoopDetector(originOffsetsM=...)): the augmentation of Scan Context++ (Kim, Choi, Kim, T-RO 2021) in
NumPy, float64, on top of scan_context_model.py.  Nothing in the reference computes this: parity is unpinned and this file is what the
device is held to.

Shifted descriptor of a scan for the origin offset o = (ox, oy), in range bins in the sensor frame of polarIndToLocalMetres
(x = r cos phi, y = r sin phi); o = offset_m / rangeResolutionM, one float64 division.
Samples.  Every (a, c), a < rows, c < clip, at its centre: phi_a = (2.0 * pi * (a + 0.5)) / rows, (C_a, S_a) = (cos, sin)(phi_a) from
a table of the host's libm (trig_tables: math.cos / math.sin, which are the C library's - the library's
roam_scan_context_offset_table gives the same bits, asserted on the CPU), rho_c = c + 0.5.
Arithmetic.  x = rho_c C_a - ox, y = rho_c S_a - oy, q = x x + y y; every product, sum and difference rounded once in float64, no
fused multiply-add.
Ring.  r with E_r^2 <= q < E_{r+1}^2, E_r the integer column edges of scan_context_model.bin_edges (their squares are exact); a sample
with q >= clip^2 is dropped.  No square root.
Sector.  b_s = (cos, sin)((2.0 * pi * row_edges[s]) / rows) from the same libm; k_s = b_s.x y - b_s.y x; the sample belongs to the
lowest s with k_s >= 0 and k_{(s + 1) mod S} < 0, and is dropped when there is none (it sits on the new origin, or in a sector wider
than pi).  The sign of k_s is the sign of the exact difference of the two rounded products, the computed signs are >= 0 on one arc of
the boundaries and < 0 on the other (a rounding can move an end of an arc by one boundary, not split it), so at most one s
satisfies the rule: sector_keys finds it from an arctan2 guess, checks the rule there and walks the rest literally;
sector_keys_literal is the rule loop by loop and the CPU test compares the two.
Value.  count = the samples that landed in the bin; a bin with none holds 0.  u8 codes k, integer floor f:
(float)((double)sum max(k - f, 0) / (255.0 count)), the sum an exact integer.  float32 values v: (float)(sum max((double)v - floor, 0)
/ count), summed in float64 (any order of at most 2^28 non-negative terms is within 1e-10 relative of any other, far below half a
float32 ulp, so the device's fixed order is within 1 float32 ulp of this one).
With o = (0, 0) the rule gives describe_u8 / describe_f32 (a centre is never within rounding of an edge): check_offset_zero asserts it.

Variants.  Variant 0 of an entry is its plain descriptor; variant a >= 1 the descriptor shifted by the a-th offset.  D(i, j) = min
over a of d(variant a of i, plain j) with d scan_context_model's; ties take the lowest a (a result equal to the plain one reports
variant 0); the shift is that variant's.  Candidates: scan_context_model.candidates on D.
Seed.  A candidate with yaw psi and winning offset o_m (metres) seeds the ICP with (psi, t), t = -R(psi) o_m, in the convention
dst ~ R(theta) src + t, src = the query."""
import math

import numpy as np

import scan_context_model as base

MAX_OFFSETS = 48                                    # roam_abi.h ROAM_LOOP_MAX_OFFSETS


def trig_tables(rows, row_edges):
    """-> (C (rows,), S (rows,), bx (S,), by (S,)) float64 by the C library's cos / sin"""
    phi = [(2.0 * math.pi * (a + 0.5)) / rows for a in range(rows)]
    beta = [(2.0 * math.pi * float(e)) / rows for e in row_edges[:-1]]
    return (np.array([math.cos(p) for p in phi]), np.array([math.sin(p) for p in phi]),
            np.array([math.cos(b) for b in beta]), np.array([math.sin(b) for b in beta]))


def offsets_bins(offsets_m, range_resolution_m):
    return np.asarray(offsets_m, np.float64).reshape(-1, 2) / np.float64(range_resolution_m)


def sample_xyq(rows, clip, o, tab):
    C, S = tab[0], tab[1]
    rho = np.arange(clip, dtype=np.float64) + 0.5
    x = rho[None, :] * C[:, None] - np.float64(o[0])
    y = rho[None, :] * S[:, None] - np.float64(o[1])
    return x, y, x * x + y * y


def ring_keys(q, ce):
    """q (...) -> ring (...) int, -1 for a dropped sample"""
    e2 = (ce.astype(np.int64) * ce.astype(np.int64)).astype(np.float64)
    r = np.searchsorted(e2, q, side="right") - 1
    return np.where(q >= e2[-1], -1, r)


def sector_keys_literal(x, y, bx, by):
    """the rule, loop by loop over the sectors -> sector (...) int, -1 where no s satisfies it"""
    S = len(bx)
    k = [bx[s] * y - by[s] * x for s in range(S)]
    out = np.full(x.shape, -1, np.int64)
    for s in range(S - 1, -1, -1):                                # descending, so the lowest s is written last
        out = np.where((k[s] >= 0) & (k[(s + 1) % S] < 0), s, out)
    return out


def sector_keys(x, y, bx, by):
    """the same result: a guess from arctan2, the rule checked there, the samples that fail it by the literal loop"""
    S = len(bx)
    beta = np.arctan2(by, bx) % (2.0 * np.pi)
    beta[0] = 0.0
    th = np.arctan2(y, x) % (2.0 * np.pi)
    g = np.clip(np.searchsorted(beta, th, side="right") - 1, 0, S - 1)
    n = (g + 1) % S
    ok = (bx[g] * y - by[g] * x >= 0) & (bx[n] * y - by[n] * x < 0)
    out = np.where(ok, g, -1)
    if not ok.all():
        out[~ok] = sector_keys_literal(x[~ok], y[~ok], bx, by)
    return out


def bin_keys(rows, cols, clip_px, S, R, o, tab=None, literal=False):
    """-> (key (rows, clip) int64: s R + r, or -1 for a dropped sample)"""
    clip = base.clip_of(cols, clip_px)
    re, ce = base.bin_edges(rows, cols, clip_px, S, R)
    tab = tab or trig_tables(rows, re)
    x, y, q = sample_xyq(rows, clip, o, tab)
    ring = ring_keys(q, ce)
    sec = (sector_keys_literal if literal else sector_keys)(x, y, tab[2], tab[3])
    return np.where((ring >= 0) & (sec >= 0), sec * R + ring, -1)


def _means(key, vals, S, R, scale):
    live = key >= 0
    cnt = np.bincount(key[live], minlength=S * R)
    tot = np.bincount(key[live], weights=vals[live], minlength=S * R)
    return np.where(cnt > 0, tot / (scale * np.maximum(cnt, 1)), 0.0).astype(np.float32).reshape(S, R)


def describe_offsets_u8(codes, S, R, clip_px, floor_code, o_bins, tab=None, literal=False):
    """codes (rows, cols) uint8, o_bins (n, 2) -> (n, S, R) float32"""
    codes = np.asarray(codes)
    assert codes.dtype == np.uint8 and 0 <= floor_code <= 254
    rows, cols = codes.shape
    clip = base.clip_of(cols, clip_px)
    vals = np.maximum(codes[:, :clip].astype(np.int64) - int(floor_code), 0).astype(np.float64)      # sums < 2^53: exact
    return np.stack([_means(bin_keys(rows, cols, clip_px, S, R, o, tab, literal), vals, S, R, 255.0) for o in np.reshape(o_bins, (-1, 2))])


def describe_offsets_f32(img, S, R, clip_px, floor, o_bins, tab=None, literal=False):
    """img (rows, cols) float32, o_bins (n, 2) -> (n, S, R) float32"""
    img = np.asarray(img)
    assert img.dtype == np.float32 and floor >= 0
    rows, cols = img.shape
    clip = base.clip_of(cols, clip_px)
    vals = np.maximum(img[:, :clip].astype(np.float64) - np.float64(floor), 0.0)
    return np.stack([_means(bin_keys(rows, cols, clip_px, S, R, o, tab, literal), vals, S, R, 1.0) for o in np.reshape(o_bins, (-1, 2))])


def describe_literal_u8(codes, S, R, clip_px, floor_code, o):
    """one offset, sample by sample in Python (an independent evaluation for the CPU test; small images only)"""
    rows, cols = codes.shape
    clip = base.clip_of(cols, clip_px)
    re, ce = base.bin_edges(rows, cols, clip_px, S, R)
    tot = [[0] * R for _ in range(S)]
    cnt = [[0] * R for _ in range(S)]
    bx = [math.cos((2.0 * math.pi * float(e)) / rows) for e in re[:-1]]
    by = [math.sin((2.0 * math.pi * float(e)) / rows) for e in re[:-1]]
    for a in range(rows):
        phi = (2.0 * math.pi * (a + 0.5)) / rows
        ca, sa = math.cos(phi), math.sin(phi)
        for c in range(clip):
            x, y = (c + 0.5) * ca - float(o[0]), (c + 0.5) * sa - float(o[1])
            q = x * x + y * y
            if q >= float(clip * clip):
                continue
            r = max(rr for rr in range(R) if float(int(ce[rr]) ** 2) <= q)
            ks = [bx[s] * y - by[s] * x for s in range(S)]
            ss = [s for s in range(S) if ks[s] >= 0 and ks[(s + 1) % S] < 0]
            if not ss:
                continue
            tot[ss[0]][r] += max(int(codes[a, c]) - floor_code, 0)
            cnt[ss[0]][r] += 1
    return np.array([[np.float32(tot[s][r] / (255.0 * cnt[s][r])) if cnt[s][r] else np.float32(0) for r in range(R)] for s in range(S)],
                    np.float32)


def check_offset_zero(arr, S, R, clip_px, floor):
    """the rule at o = (0, 0) against the plain descriptor, bit for bit (uint8 codes with an integer floor, or a float32 image)"""
    arr = np.asarray(arr)
    if arr.dtype == np.uint8:
        got, want = describe_offsets_u8(arr, S, R, clip_px, floor, [(0.0, 0.0)])[0], base.describe_u8(arr, S, R, clip_px, floor)
    else:
        got, want = describe_offsets_f32(arr, S, R, clip_px, floor, [(0.0, 0.0)])[0], base.describe_f32(arr, S, R, clip_px, floor)
    assert np.array_equal(got, want), "the offset rule at (0, 0) is not the plain descriptor"
    return got


# ---------------------------------------------------------------------------------------------------------------- variants
def distances_variants(V, C):
    """V (m, A, S, R): the variants of m queries, variant 0 first; C (n, S, R) plain candidates ->
    (dist (m, n) float64, shift (m, n) int32, variant (m, n) int32: the lowest a of the minimum)"""
    m, n = len(V), len(C)
    dist, shift, var = np.empty((m, n)), np.empty((m, n), np.int32), np.empty((m, n), np.int32)
    for i in range(m):
        d, s, _ = base.distances(V[i], C)                        # (A, n)
        a = d.argmin(axis=0)                                     # the first of equal minima
        var[i], dist[i], shift[i] = a, d[a, np.arange(n)], s[a, np.arange(n)]
    return dist, shift, var


def variant_offsets(var, offsets_m):
    """variant indices (...) -> their offsets in metres (..., 2); variant 0 is (0, 0)"""
    table = np.concatenate([np.zeros((1, 2)), np.asarray(offsets_m, np.float64).reshape(-1, 2)])
    return table[np.asarray(var)]


def seed(yaw, o_m):
    """-> (psi, tx, ty), t = -R(psi) o_m"""
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([yaw, -(c * o_m[0] - s * o_m[1]), -(s * o_m[0] + c * o_m[1])])


def offset_grid(reach_m, step_m):
    """the grid of multiples of step_m within +-reach_m on both axes, x-major, without its centre -> (n, 2) float64"""
    k = int(math.floor(reach_m / step_m + 1e-9))
    return np.array([(i * step_m, j * step_m) for i in range(-k, k + 1) for j in range(-k, k + 1) if (i, j) != (0, 0)], np.float64).reshape(-1, 2)
