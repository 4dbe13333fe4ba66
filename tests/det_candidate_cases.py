"""Inputs and a small float64 model for the candidate lists of rt_det_strip_kernel (csrc/retrack_det.hip) and of the fused kernel
(csrc/retrack_fused.inc): seeded polar payloads, the oracle's candidates packed like the device's keys (rc = row << 16 | col << 2 |
layer, float64 determinant), and a classifier that says which of the kernel's special paths a candidate list passes through - the
seam rows, the row-clipped first and last steps, the clipped corner columns, the strip's edge columns, the partial last strip and
step, the dark-step table, exact ties, the pruned dxy term.  No GPU and no engine import: tests/test_det_candidates_cpu.py holds the
class minima with the oracle alone, so that tests/test_gpu_det_candidates.py cannot pass by having nothing to compare.

The binary families (codes 0 and 255 only) matter: every Cartesian pixel of theirs is a multiple of 2^-10 (bilinear weights in 1/32
steps on samples of exactly 0 or 1), so the integral image and every box sum are exact and neighbouring determinants above the
threshold are EXACTLY equal by the hundred - only there does a `>=` in place of `>` in the maxima rule, or a seam row compared the
wrong way, show.  Grey-level families have no such ties."""
from collections import namedtuple

import numpy as np

import oracle

SIGMAS = np.linspace(0.01, 10, 3)                # the engine's detector parameters (getFeatures.py:13-18); layer 0 has box size 0: skipped
THRESHOLD = 0.0005
SIZES = (0, 15, 30)                              # int(3 sigma) per layer
CAP = 2048                                       # BP_MAX_PTS: candidates a detection keeps (beyond it the kept subset depends on arrival order)
SD_T, SD_OUT, SD_PC, SD_HL, SD_HR = 16, 62, 64, 14, 16    # retrack_geom.h: rows per step, outputs / positions per strip, box offsets -14 .. +16

CLIPS = (132, 188, 497, 560)

# (clip, family, seed, n_oracle[, overflow]): n_oracle = the oracle's number of 3 x 3 x 3 maxima, recorded; tests/test_det_candidates_cpu.py
# holds it.  overflow: the one case beyond the cap - uniform u8 noise at clip 400 (the kernel counts every maximum and keeps 2048)
Case = namedtuple("Case", "clip family seed n_oracle overflow", defaults=(False,))
CASES = [Case(*c) for c in [
    (132, "blobs", 1, 42), (132, "u8_speckle", 1, 20), (132, "bin_rings", 1, 651), (132, "bin_band", 1, 318), (132, "bin_squares", 1, 73), (132, "bin_noise", 1, 26), (132, "bin_diag", 1, 150),
    (188, "blobs", 1, 50), (188, "u8_speckle", 1, 39), (188, "bin_rings", 1, 882), (188, "bin_band", 1, 496), (188, "bin_squares", 1, 175), (188, "bin_noise", 1, 50), (188, "bin_diag", 1, 187),
    (497, "blobs", 1, 151), (497, "u8_speckle", 1, 489), (497, "bin_rings", 1, 1684), (497, "bin_band", 1, 624), (497, "bin_squares", 1, 1041), (497, "bin_noise", 1, 156), (497, "bin_diag", 1, 468),
    (560, "blobs", 1, 180), (560, "u8_speckle", 1, 558), (560, "bin_rings", 1, 1918), (560, "bin_band", 1, 1204), (560, "bin_squares", 1, 1459), (560, "bin_noise", 1, 217), (560, "bin_diag", 1, 531),
    (400, "u8_noise", 1, 2429, True),
]]
OVERFLOW_CASE = CASES[-1]
BINARY = ("bin_rings", "bin_band", "bin_squares", "bin_noise", "bin_diag")


def cases_of(clip):
    return [c for c in CASES if c.clip == clip and not c.overflow]


def blob_payload(clip, seed, rows=400):
    """speckle + Gaussian blobs in (azimuth, range), a third of them at the far end of the range axis = along the borders of the
    Cartesian image, where the box corners of the determinant are clipped"""
    rng = np.random.default_rng(seed)
    img = rng.exponential(6.0, size=(rows, clip))
    for i in range(max(18, clip // 5)):
        a, A = rng.uniform(0, rows), rng.uniform(80, 200)
        r = rng.uniform(clip - 24, clip - 2) if i % 3 == 0 else rng.uniform(4, clip - 2)
        sa, sr = max(1.5, 240.0 / max(r, 4.0)), rng.uniform(2.0, 7.0)
        aa = np.arange(int(a - 4 * sa), int(a + 4 * sa) + 1)
        rr = np.arange(max(0, int(r - 4 * sr)), min(clip, int(r + 4 * sr) + 1))
        img[np.ix_(aa % rows, rr)] += A * np.exp(-0.5 * ((aa - a) / sa) ** 2)[:, None] * np.exp(-0.5 * ((rr - r) / sr) ** 2)[None, :]
    return np.clip(np.floor(img), 0, 255).astype(np.uint8)


def payload(name, clip, rows=400, seed=0):
    """uint8 (rows, clip) polar scan of family `name`, a function of (name, clip, rows, seed) alone"""
    if name == "blobs":
        return blob_payload(clip, seed, rows)
    rng = np.random.default_rng([seed, clip, sum(map(ord, name))])
    pay = np.zeros((rows, clip), np.uint8)
    if name == "u8_speckle":                     # speckle of low amplitude + bright squares, a fifth of them in the last range bins
        pay = (rng.random((rows, clip)) * 10).astype(np.uint8)
        for i in range(max(24, clip // 6)):
            a = int(rng.integers(0, rows))
            r = int(rng.integers(clip - 12, clip - 2)) if i % 5 == 0 else int(rng.integers(6, clip - 2))
            h = int(rng.integers(2, 5))
            pay[max(0, a - h):a + h, max(0, r - h):r + h] = rng.integers(120, 256)
    elif name == "bin_rings":                    # whole-azimuth range bands, one of them over the last range bins
        thin = clip >= 300                       # (at the larger sizes two thick bands have more than 2048 maxima)
        pay[:, clip - (4 if thin else 5):] = 255
        pay[:, int(0.45 * clip):int(0.45 * clip) + (1 if thin else 3)] = 255
    elif name == "bin_band":                     # one whole-azimuth band of 3 bins at a range where maxima tie ACROSS a step boundary (found by search)
        r0 = {132: 98, 188: 176, 497: 236, 560: 434}.get(clip, int(0.475 * clip))
        pay[:, r0:r0 + 3] = 255
    elif name == "bin_squares":                  # 7 x 7 polar squares, every fourth in the last range bins
        for i in range(max(30, clip // 4)):
            a = int(rng.integers(0, rows))
            r = int(rng.integers(clip - 9, clip - 6)) if i % 4 == 0 else int(rng.integers(4, clip - 8))
            pay[np.arange(a, a + 7) % rows, r:r + 7] = 255
    elif name == "bin_noise":                    # a few per cent of the samples lit
        pay[rng.random((rows, clip)) < (0.04 if clip < 300 else 0.012)] = 255
    elif name == "bin_diag":                     # elongated diagonal bars in the CARTESIAN image (drawn through polar coordinates): large dxy
        R = clip / 2.0
        for i in range(max(10, clip // 24)):
            x0, y0 = rng.uniform(-0.62 * R, 0.62 * R, size=2)
            L, s = rng.uniform(10, 26), (1.0 if i % 2 else -1.0)
            for u in np.arange(-L, L, 0.2):
                for v in (-1.0, 0.0, 1.0):
                    x, y = x0 + (u + v) * 0.7071, y0 + s * (u - v) * 0.7071
                    rad, ang = 2.0 * np.hypot(x, y), np.arctan2(y, x) % (2 * np.pi)
                    if rad < clip - 1:
                        pay[int(ang / (2 * np.pi) * rows) % rows, int(rad)] = 255
    elif name == "u8_noise":
        pay = rng.integers(0, 256, size=(rows, clip), dtype=np.uint8)
    else:
        raise KeyError(name)
    return pay


def pack(rows, cols, layers):
    return (np.asarray(rows, np.uint32) << 16) | (np.asarray(cols, np.uint32) << 2) | np.asarray(layers, np.uint32)


def unpack(rc):
    rc = np.asarray(rc, np.uint32)
    return (rc >> 16).astype(np.int64), ((rc >> 2) & 0x3fff).astype(np.int64), (rc & 3).astype(np.int64)


def cartesian(pay):
    return oracle.convertPolarImageToCartesian(pay.astype(np.float32) / np.float32(255.))


def want(pay):
    """the oracle's candidates of a payload with the engine's parameters -> (rc uint32 (n,), val float64 (n,), layers): keys packed like
    the device's, in the oracle's C (row, column, layer) order = ascending key order"""
    rcs, val, layers = oracle.doh_maxima(cartesian(pay), SIGMAS, THRESHOLD)
    return pack(rcs[:, 0], rcs[:, 1], rcs[:, 2]), val.copy(), layers


_TRUTH = {}


def truth(case):
    """(payload, rc, val, layers) of a (clip, family, seed, ...) entry, computed once and shared read-only among the tests"""
    key = tuple(case[:3])
    if key not in _TRUTH:
        pay = payload(case[1], case[0], seed=case[2])
        rc, val, layers = want(pay)
        for a in (pay, rc, val, layers[1], layers[2]):
            a.setflags(write=False)
        _TRUTH[key] = (pay, rc, val, layers)
    return _TRUTH[key]


def integral(cart):
    """skimage's integral image: cumsum over rows, then over columns, float64"""
    return np.cumsum(np.cumsum(cart.astype(np.float64), axis=0), axis=1)


def _integ(S, r, c, rl, cl):
    H, W = S.shape
    r, c = np.clip(r, 0, H - 1), np.clip(c, 0, W - 1)
    r2, c2 = np.clip(r + rl, 0, H - 1), np.clip(c + cl, 0, W - 1)
    a = S[np.ix_(r, c)] + S[np.ix_(r2, c2)] - S[np.ix_(r, c2)] - S[np.ix_(r2, c)]
    return np.maximum(a, 0.0)


def hessian_parts(S, size):
    """dxx, dyy, dxy of every position: oracle/c/doh.c's boxes (skimage _hessian_matrix_det) restated in NumPy.  Classifies positions
    (where does the bare product dxx * dyy pass the threshold while the determinant does not); never an expected value."""
    H, W = S.shape
    r, c = np.arange(H), np.arange(W)
    s2, s3, w = (size - 1) // 2, size // 3, size
    w_i = 1.0 / size / size
    tl, br = _integ(S, r - s3, c - s3, s3, s3), _integ(S, r + 1, c + 1, s3, s3)
    bl, tr = _integ(S, r - s3, c + 1, s3, s3), _integ(S, r + 1, c - s3, s3, s3)
    dxy = -(bl + tr - tl - br) * w_i
    dxx = -(_integ(S, r - s3 + 1, c - s2, 2 * s3 - 1, w) - 3 * _integ(S, r - s3 + 1, c - s3 // 2, 2 * s3 - 1, s3)) * w_i
    dyy = -(_integ(S, r - s2, c - s3 + 1, w, 2 * s3 - 1) - 3 * _integ(S, r - s3 // 2, c - s3 + 1, s3, 2 * s3 - 1)) * w_i
    return dxx, dyy, dxy


_DARK = {}


def dark_steps(clip, rows=400):
    """bool (strips, steps): the whole window of the step - position rows 16 t .. 16 t + 15 with box rows -14 .. +16, the strip's 64
    position columns (from 62 s - 1) with box columns -14 .. +16, clipped to the image - lies where the warp of an all-ones scan is 0,
    i.e. beyond the maximum range.  The rule documented above rt_darktab_kernel, restated; classifies only."""
    if (clip, rows) not in _DARK:
        lit = oracle.convertPolarImageToCartesian(np.ones((rows, clip), np.float32)) != 0
        W = lit.shape[0]
        ns, nt = -(-W // SD_OUT), W // SD_T + 1
        dark = np.zeros((ns, nt), bool)
        for s in range(ns):
            xa, xb = max(SD_OUT * s - 1 - SD_HL, 0), min(SD_OUT * s - 1 + SD_PC - 1 + SD_HR, W - 1)
            for t in range(nt):
                ra, rb = max(SD_T * t - SD_HL, 0), min(SD_T * t + SD_T - 1 + SD_HR, W - 1)
                dark[s, t] = not lit[ra:rb + 1, xa:xb + 1].any()
        _DARK[(clip, rows)] = dark
    return _DARK[(clip, rows)]


def _edges(dark):
    """per strip: has dark steps (and lit ones), first lit step, last lit step"""
    t = np.arange(dark.shape[1])[None, :]
    return dark.any(axis=1) & ~dark.all(axis=1), np.where(~dark, t, dark.shape[1]).min(axis=1), np.where(~dark, t, -1).max(axis=1)


def _count(lit, ra, rb, ca, cb):
    """per position the lit pixels in rows r + ra .. r + rb, columns c + ca .. c + cb (clipped to the image)"""
    H, W = lit.shape
    I = np.zeros((H + 1, W + 1), np.int64)
    I[1:, 1:] = np.cumsum(np.cumsum(lit, axis=0), axis=1)
    r, c = np.arange(H), np.arange(W)
    r0, r1, c0, c1 = np.clip(r + ra, 0, H), np.clip(r + rb + 1, 0, H), np.clip(c + ca, 0, W), np.clip(c + cb + 1, 0, W)
    return I[np.ix_(r1, c1)] - I[np.ix_(r0, c1)] - I[np.ix_(r1, c0)] + I[np.ix_(r0, c0)]


_EDGE = {}


def edge_step_positions(clip, rows=400, inward=0):
    """how many positions in the first / last lit step of a strip that has dark steps (inward = 1: in the step next to it) could hold
    a determinant above the threshold at all.  Pixels are at most 1, so |dxx| <= max(lit pixels in the two outer thirds of its box, 2 x those in the centre third) / size^2,
    the same for dyy, and det <= dxx * dyy: a position where that bound stays at or below the threshold for both box sizes has no
    candidate whatever the scan holds.  The step before the first lit one is dark, i.e. no pixel within 16 rows below its positions is
    lit: the positions of an edge step are 12 pixels and more away from the lit disc, and the bound says so: 0 positions at clip 188 and
    497, 1 at clip 560.  Such a step is lit because a corner of its window is, not because it could hold a maximum."""
    if (clip, rows, inward) not in _EDGE:
        lit = oracle.convertPolarImageToCartesian(np.ones((rows, clip), np.float32)) != 0
        W, dark = lit.shape[0], dark_steps(clip, rows)
        bound = np.zeros((W, W))
        for size in SIZES[1:]:
            s2, s3 = (size - 1) // 2, size // 3
            b = []
            for tr in (False, True):
                box = lambda a, n: _count(lit, a, a + n - 1, -s3 + 1, s3 - 1) if tr else _count(lit, -s3 + 1, s3 - 1, a, a + n - 1)
                mid, cen = box(-s2, size), box(-(s3 // 2), s3)
                b.append(np.maximum(mid - cen, 2 * cen))
            bound = np.maximum(bound, b[0] * b[1] / float(size) ** 4)
        has, first, last = _edges(dark)
        n = 0
        for s in np.nonzero(has)[0]:
            for t in {first[s] + inward, last[s] - inward}:
                n += int((bound[SD_T * t:SD_T * t + SD_T, SD_OUT * s:SD_OUT * s + SD_OUT] > THRESHOLD).sum())
        _EDGE[(clip, rows, inward)] = n
    return _EDGE[(clip, rows, inward)]


def _cube(layers):
    """layers 1 and 2 with a border of zeros (scipy's mode='constant'), (2, H + 2, W + 2)"""
    H, W = layers[1].shape
    cube = np.zeros((2, H + 2, W + 2))
    cube[0, 1:-1, 1:-1], cube[1, 1:-1, 1:-1] = layers[1], layers[2]
    return cube


def _neighbours():
    return [(dl, dr, dc) for dl in (-1, 0, 1) for dr in (-1, 0, 1) for dc in (-1, 0, 1) if (dl, dr, dc) != (0, 0, 0)]


def possible(clip, rows=400):
    """the classes an image of this size can populate at all.  Not among them at any size: both_layers - each layer is the other's
    neighbour, so two maxima at one (row, column) need determinants of box 15 and box 30 that are equal bit for bit; the class is
    counted and reported, no minimum is set.  dark_edge_step only where at least three positions of such steps can hold a candidate
    (edge_step_positions: none of these sizes).  What the dark-step table can get wrong with a visible effect is populated instead:
    the strips that have dark steps (dark_strip), the steps next to the edge steps where at least 100 positions can hold a candidate
    (dark_next_step), and from step 32 on the lit steps that the table's first word calls dark (second_word: a kernel that did not
    reload the word would lose them).  seam_ties: exact ties whose equal neighbour lies in another step."""
    W, dark = 2 * (clip // 2), dark_steps(clip, rows)
    out = {"layer1", "layer2", "strip_edge_col", "seam_row", "rows_top", "rows_bottom", "cols_left", "cols_right", "near_threshold",
           "ties", "seam_ties"}
    if W % SD_OUT:
        out.add("last_partial_strip")
    if W % SD_T:
        out.add("last_partial_step")
    if W > 512:
        out.add("row_ge_512")
    has, first, last = _edges(dark)
    if has.any():
        out.add("dark_strip")
        if edge_step_positions(clip, rows) >= 3:
            out.add("dark_edge_step")
        if edge_step_positions(clip, rows, 1) >= 100:
            out.add("dark_next_step")
        if any(dark[s, t & 31] for s in np.nonzero(has)[0] for t in range(32, last[s] + 1)):
            out.add("second_word")
    return out


def classes(rc, val, layers, W, dark, S=None):
    """name -> number of candidates of the list (rc, val) in each class; layers: the oracle's determinant layers; dark: dark_steps();
    S: the integral image - given, the pruned-and-failed POSITIONS next to a candidate are counted too"""
    r, c, l = unpack(rc)
    n = {}
    n["layer1"], n["layer2"] = int((l == 1).sum()), int((l == 2).sum())
    pos = r * W + c
    n["both_layers"] = int(np.intersect1d(pos[l == 1], pos[l == 2]).size)
    n["strip_edge_col"] = int(np.isin(c % SD_OUT, (0, SD_OUT - 1)).sum())
    n["seam_row"] = int(np.isin(r % SD_T, (0, SD_T - 2, SD_T - 1)).sum())
    n["rows_top"], n["rows_bottom"] = int((r < SD_HL).sum()), int((r >= W - SD_HR).sum())
    n["cols_left"], n["cols_right"] = int((c < SD_HL).sum()), int((c >= W - SD_HR).sum())
    n["last_partial_strip"] = int((c >= SD_OUT * (W // SD_OUT)).sum()) if W % SD_OUT else 0
    n["last_partial_step"] = int((r >= SD_T * (W // SD_T)).sum()) if W % SD_T else 0
    n["row_ge_512"] = int((r >= 512).sum())
    s, t = c // SD_OUT, r // SD_T
    has, first, last = _edges(dark)
    n["dark_strip"] = int(has[s].sum())
    n["dark_edge_step"] = int((has[s] & ((t == first[s]) | (t == last[s]))).sum())
    n["dark_next_step"] = int((has[s] & ((t == first[s] + 1) | (t == last[s] - 1))).sum())
    n["second_word"] = int(((t >= 32) & dark[s, t & 31]).sum())            # a lit step that the table's FIRST word would call dark
    n["near_threshold"] = int((val <= 1.1 * THRESHOLD).sum())
    cube = _cube(layers)
    tie, seam = np.zeros(len(rc), bool), np.zeros(len(rc), bool)
    for dl, dr, dc in _neighbours():
        ll = l - 1 + dl
        ok = (ll >= 0) & (ll < 2)
        u = cube[np.clip(ll, 0, 1), r + 1 + dr, c + 1 + dc]
        tie |= ok & (u == val)
        seam |= ok & (u == val) & ((r + dr) // SD_T != t)                  # the equal neighbour lies in another step: decided through the seam
    n["ties"], n["seam_ties"] = int(tie.sum()), int(seam.sum())
    if S is not None:
        iscand = np.zeros((2, W + 2, W + 2), bool)
        iscand[l - 1, r + 1, c + 1] = True
        near = np.zeros_like(iscand)                                       # a candidate among the 26 neighbours
        for dl, dr, dc in _neighbours():
            sh = np.roll(iscand, (dl, dr, dc), axis=(0, 1, 2))
            if dl:
                sh[0 if dl > 0 else 1] = False                             # (np.roll wraps the two layers around)
            near |= sh
        cnt = 0
        for k in (1, 2):
            dxx, dyy, dxy = hessian_parts(S, SIZES[k])
            failed = (dxx * dyy > THRESHOLD) & ~(layers[k] > THRESHOLD)
            cnt += int((failed & near[k - 1, 1:-1, 1:-1]).sum())
        n["pruned_failed"] = cnt
    return n
