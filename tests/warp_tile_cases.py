"""Cases and a tile model for warp_gather_kernel (radarslampy_amd/csrc/warp.hip), the kernel that makes level 0 of every lane's pyramid.

The kernel cuts the W x W Cartesian image into tiles of 64 x 16 pixels and treats a tile by the polar footprint of its pixels:
dark (no pixel inside the scan's range), direct (the footprint does not fit the 4096 staged floats: next to the centre and across the
0 / 2 pi seam) or box (the footprint is staged in LDS, for `per` scans of the batch in one pass).  classify() restates those decisions in
NumPy on the oracle's sampling map; GEOMETRIES are the smallest record shapes that between them reach every class; records() and
lane_maps() make scans and lane -> scan assignments on which a wrong clamp, a wrong pass remainder or a wrong scan inside a pass changes
bytes.  tests/test_warp_tiles_cpu.py holds the conditions the cases must meet, tests/test_gpu_warp_tiles.py runs them on the device."""
import numpy as np

import oracle

# the kernel's constants (warp.hip)
WG_LB = 32              # lanes of the batch per workgroup
WG_TW, WG_TH = 64, 16   # tile width and height
WG_BOX_ELEMS = 4096     # floats staged per pass
WG_FILL_U = 4           # largest fill unit

DARK, DIRECT, BOX = 0, 1, 2
CLASS_NAMES = ("dark", "direct", "box")

# (rows, clip, stride, payload_off)
GEOMETRIES = [
    (8, 200, 200, 0),
    (3, 132, 139, 5),
    (2, 132, 132, 0),
    (200, 300, 317, 11),
    (1020, 520, 520, 0),
    (64, 1000, 1003, 3),
]
# the batch sizes of the GPU test: every geometry at 70 lanes (groups of 32, 32 and 6), two of them also at 1, 31 and 33
BATCH = 70
PARTIAL_GEOMETRIES = [GEOMETRIES[0], GEOMETRIES[3]]
PARTIAL_BATCHES = (1, 31, 33)

RECORD_NAMES = ("noise", "ones", "rowcode", "seam", "rim", "noise2")


def geometry_id(g):
    return "rows%d_clip%d_stride%d_off%d" % g


def device_map(rows, clip):
    """(ix, iy, fx, fy) per pixel as warp_map_kernel packs them: the oracle's sampling map with the kernel's clamps (ix outside
    [0, 4095] -> 4095, which is out of range for every clip the engine takes; iy into [0, 1022])"""
    sx, sy = oracle.polar_sampling_map(rows, clip)
    ix = np.clip(sx >> 5, -32768, 32767)
    iy = np.clip(sy >> 5, -32768, 32767)
    ix = np.where((ix > 4095) | (ix < 0), 4095, ix)
    iy = np.clip(iy, 0, 1022)
    return ix.astype(np.int64), iy.astype(np.int64), (sx & 31).astype(np.int64), (sy & 31).astype(np.int64)


def grid(clip, B):
    """(gx, gy, gz) of launch_warp_gather"""
    W = 2 * (clip // 2)
    return (W + WG_TW - 1) // WG_TW, (W + WG_TH - 1) // WG_TH, (B + WG_LB - 1) // WG_LB


def _tiles(a, W, gx, gy, fill):
    """(W, W) -> (gy, gx, 16 * 64) with `fill` outside the image"""
    p = np.full((gy * WG_TH, gx * WG_TW), fill, a.dtype)
    p[:W, :W] = a
    return p.reshape(gy, WG_TH, gx, WG_TW).transpose(0, 2, 1, 3).reshape(gy, gx, -1)


def classify(rows, clip):
    """The kernel's per-tile decisions (warp.hip: the box extent over the in-range pixels, `any`, `use_box`, `chk`, `per`) -> dict of
    (gy, gx) arrays:
      cls          DARK / DIRECT / BOX
      all_in       every pixel of the tile that lies in the image is in range (ix < cols)
      wraps        a polar row the tile reads is wrapped: for a box tile a staged row index mny - 1 < 0 (wrap_lo) or mxy >= rows
                   (wrap_hi: the index reaches rows or more); for a direct tile a pixel with iy == 0 or iy >= rows
      iy_top       an in-range pixel has iy == rows + 1 (the zero-weight tap row rows + 2 of the padded image is staged as row 1)
      mnx, mxx, mny, mxy, bw, bh, bp, elems, chk, per    the box geometry (meaningful where cls != DARK; chk and per where cls == BOX)"""
    W = 2 * (clip // 2)
    cols = clip
    gx, gy, _ = grid(clip, 1)
    ix, iy, _, _ = device_map(rows, clip)
    inimg = _tiles(np.ones((W, W), bool), W, gx, gy, False)
    tix, tiy = _tiles(ix, W, gx, gy, 4095), _tiles(iy, W, gx, gy, 0)
    in0 = inimg & (tix < cols)
    big = np.int64(0x7fffffff)
    mnx = np.where(in0, tix, big).min(-1); mxx = np.where(in0, tix, -1).max(-1)
    mny = np.where(in0, tiy, big).min(-1); mxy = np.where(in0, tiy, -1).max(-1)
    any_ = mxx >= 0
    bw, bh = mxx - mnx + 2, mxy - mny + 2
    bp = (bw + 3) & ~3
    elems = np.where(any_, bp * bh, 0)
    use_box = any_ & (elems <= WG_BOX_ELEMS)
    cls = np.where(~any_, DARK, np.where(use_box, BOX, DIRECT))
    per = np.maximum(1, np.minimum(WG_LB, WG_BOX_ELEMS // np.maximum(elems, 1)))
    wrap_lo, wrap_hi = any_ & (mny == 0), any_ & (mxy >= rows)
    return dict(cls=cls, all_in=(in0 | ~inimg).all(-1), wrap_lo=wrap_lo, wrap_hi=wrap_hi, wraps=wrap_lo | wrap_hi,
                iy_top=(in0 & (tiy == rows + 1)).any(-1), mnx=mnx, mxx=mxx, mny=mny, mxy=mxy, bw=bw, bh=bh, bp=bp, elems=elems,
                chk=use_box & (mnx + bp > cols), per=np.where(use_box, per, 0))


def fill_units(n_lanes_in_group, per):
    """the box fills of one workgroup with n_lanes_in_group lanes (l1 - l0): a list of passes, each the tuple of fill units (scans per
    box_fill call: 4, 2 or 1) in the order the kernel's qb loop issues them"""
    passes = []
    for lb in range(0, n_lanes_in_group, per):
        nq = min(per, n_lanes_in_group - lb)
        units, qb = [], 0
        while qb < nq:
            rem = nq - qb
            u = 4 if rem >= 4 and WG_FILL_U >= 4 else 2 if rem >= 2 and WG_FILL_U >= 2 else 1
            units.append(u)
            qb += u
        passes.append(tuple(units))
    return passes


def group_sizes(B):
    return [min(WG_LB, B - l0) for l0 in range(0, B, WG_LB)]


def class_table(geometries=GEOMETRIES):
    """per geometry the number of tiles of every class the conditions of tests/test_warp_tiles_cpu.py name, and the pass sizes"""
    out = []
    for g in geometries:
        rows, clip = g[0], g[1]
        c = classify(rows, clip)
        box, direct = c["cls"] == BOX, c["cls"] == DIRECT
        out.append(dict(
            geometry=g, W=2 * (clip // 2), tiles=int(c["cls"].size), dark=int((c["cls"] == DARK).sum()),
            direct_all_in=int((direct & c["all_in"]).sum()), direct_part_out=int((direct & ~c["all_in"]).sum()),
            box_nochk=int((box & ~c["chk"]).sum()), box_chk=int((box & c["chk"]).sum()), box_part_out=int((box & ~c["all_in"]).sum()),
            box_wide=int((box & (c["bw"] > 64)).sum()), box_tall=int((box & (c["bh"] > 16)).sum()),
            box_wraps=int((box & c["wrap_hi"]).sum()), direct_wraps=int((direct & c["wraps"]).sum()),
            box_iy_top=int((box & c["iy_top"]).sum()), per=sorted(set(int(p) for p in c["per"][box]))))
    return out


TABLE_COLUMNS = ("dark", "direct_all_in", "direct_part_out", "box_nochk", "box_chk", "box_part_out", "box_wide", "box_tall", "box_wraps",
                 "direct_wraps", "box_iy_top")


def format_table(table):
    lines = ["%-22s %5s %6s " % ("rows,clip,stride,off", "W", "tiles") + " ".join("%15s" % c for c in TABLE_COLUMNS) + "  per"]
    for t in table:
        lines.append("%-22s %5d %6d " % (",".join(map(str, t["geometry"])), t["W"], t["tiles"]) +
                     " ".join("%15d" % t[c] for c in TABLE_COLUMNS) + "  " + ",".join(map(str, t["per"])))
    return "\n".join(lines)


def records(geometry):
    """six u8 records (rows, stride) in the order of RECORD_NAMES.  In every record every byte outside the payload columns
    [payload_off, payload_off + clip) is 255 (metadata, padding and - through `ones` and `rim` where stride == clip - the first columns
    of the next row): a staged column past the last range bin that is not zeroed lights the rim of the image"""
    rows, clip, stride, off = geometry
    r, c = np.arange(rows)[:, None], np.arange(clip)[None, :]
    seed = rows * 100003 + clip * 101 + stride
    pay = {}
    pay["noise"] = np.random.default_rng(seed).integers(0, 256, (rows, clip), dtype=np.uint8)
    pay["ones"] = np.full((rows, clip), 255, np.uint8)
    pay["rowcode"] = ((37 * r + 11 * c) & 255).astype(np.uint8)
    seam = np.zeros((rows, clip), np.uint8)
    seam[0] = 255
    seam[rows - 1] = 128
    pay["seam"] = seam
    rim = np.zeros((rows, clip), np.uint8)
    rim[:, [0, clip - 2, clip - 1]] = 255
    pay["rim"] = rim
    pay["noise2"] = np.random.default_rng(seed + 1).integers(0, 256, (rows, clip), dtype=np.uint8)
    out = []
    for name in RECORD_NAMES:
        rec = np.full((rows, stride), 255, np.uint8)
        rec[:, off:off + clip] = pay[name]
        out.append(rec)
    return out


def lane_maps(B):
    """two lane -> record maps (int32 (B,)): neither is monotone, both repeat records, every full group of 32 lanes holds all six
    records in both, and the two differ in every lane"""
    b = np.arange(B)
    first = (5 * b + 2 * (b // 32)) % 6          # 4 b + 2 (b // 32) is even, so first - second = 4 b + 2 (b // 32) - 3 is never 0 mod 6
    second = (b + 3) % 6
    return first.astype(np.int32), second.astype(np.int32)


_EXPECTED = {}


def expected_images(geometry):
    """the oracle's u8 Cartesian image of each of the six records, computed once per geometry (read-only)"""
    if geometry not in _EXPECTED:
        rows, clip, stride, off = geometry
        imgs = []
        for rec in records(geometry):
            img = oracle.convertPolarImageToCartesian(rec[:, off:off + clip].astype(np.float32) / np.float32(255.), want_u8=True)[1]
            img.setflags(write=False)
            imgs.append(img)
        _EXPECTED[geometry] = imgs
    return _EXPECTED[geometry]


def remap_numpy(polar, rows, clip):
    """convertPolarImageToCartesian restated on polar_sampling_map: four taps of the padded image (zero outside it), the weights and the
    summation order of oracle/c/warp_klt.c, all in float32 -> (cart f32, cart u8)"""
    f32 = np.float32
    polar = np.ascontiguousarray(polar, f32)
    sx, sy = oracle.polar_sampling_map(rows, clip)
    ix, iy = (sx >> 5).astype(np.int64), (sy >> 5).astype(np.int64)
    wx1 = (sx & 31).astype(f32) * f32(1.0 / 32.0); wx0 = f32(1) - wx1
    wy1 = (sy & 31).astype(f32) * f32(1.0 / 32.0); wy0 = f32(1) - wy1

    def tap(py, px):
        ok = (px >= 0) & (px < clip) & (py >= 0) & (py < rows + 2)
        r = py - 1
        r = np.where(r < 0, r + rows, np.where(r >= rows, r - rows, r))
        return np.where(ok, polar[np.clip(r, 0, rows - 1), np.clip(px, 0, clip - 1)], f32(0))

    v = tap(iy, ix) * (wy0 * wx0)
    v = v + tap(iy, ix + 1) * (wy0 * wx1)
    v = v + tap(iy + 1, ix) * (wy1 * wx0)
    v = v + tap(iy + 1, ix + 1) * (wy1 * wx1)
    assert v.dtype == np.float32
    return v, (v * f32(255.0)).astype(np.int32).astype(np.uint8)


def describe_pixel(geometry, y, x, cls=None):
    """'tile (by, bx) box chk per=...' of the tile that holds pixel (y, x): for the message of a failed comparison"""
    rows, clip = geometry[0], geometry[1]
    c = classify(rows, clip) if cls is None else cls
    by, bx = int(y) // WG_TH, int(x) // WG_TW
    k = int(c["cls"][by, bx])
    s = "tile (by=%d, bx=%d) %s" % (by, bx, CLASS_NAMES[k])
    if k != DARK:
        s += " all_in=%d wraps=%d iy_top=%d" % (c["all_in"][by, bx], c["wraps"][by, bx], c["iy_top"][by, bx])
    if k == BOX:
        s += " bw=%d bh=%d bp=%d elems=%d chk=%d per=%d" % tuple(int(c[n][by, bx]) for n in ("bw", "bh", "bp", "elems", "chk", "per"))
    return s
