"""Image pairs that drive klt_kernel (csrc/pyrklt.hip) through its data-dependent branches, and the classes they reach
(test_klt_branches_cpu.py, test_gpu_klt_branches.py).  Every other tracker comparison of the suite moves one kind of image - a smooth
texture, a rendered or a real scan - by a few pixels and varies where the points lie; here the content varies: noise, 0 / 255 blocks,
flat images, one step edge, stripes at the per-pixel maximum of every window product, textures moved further than a tile holds.
Seeded generators, no files; u8 images of 128 x 160 (a few 160 x 128), at most 200 points per case and 64 per seeded case.
Everything is computed once per process and never modified."""
import numpy as np

import klt_flow_model as M

HW = (128, 160)
HW_T = (160, 128)
MAX_GUESS = 1e6             # seeded guesses stay finite and within this: beyond, int(floor()) and the C conversion are not defined alike

_cache = {}


# ------------------------------------------------------------------------------------------------------------------ images
def noise(seed, hw=HW):
    return np.random.default_rng(seed).integers(0, 256, hw, dtype=np.uint8)


def blocks(seed, hw=HW, b=8):
    """0 / 255 in b x b blocks"""
    h, w = hw
    bits = np.random.default_rng(seed).integers(0, 2, ((h + b - 1) // b, (w + b - 1) // b), dtype=np.uint8)
    return np.ascontiguousarray(np.kron(bits, np.ones((b, b), np.uint8))[:h, :w] * np.uint8(255))


def box(hw=HW, level=0, value=255, y0=40, y1=90, x0=60, x1=110):
    a = np.full(hw, level, np.uint8)
    a[y0:y1, x0:x1] = value
    return a


def step_edge(hw=HW, x=80):
    a = np.zeros(hw, np.uint8)
    a[:, x:] = 255
    return a


def stripes(hw=HW, split=40):
    """rows above `split`: vertical stripes [0, 255, 255, 0][x % 4]; from `split` on: horizontal stripes [0, 255, 255, 0][y % 4].  Every
    pixel of the upper part has |Scharr dx| = 4080, and against the image rolled by one column |diff| = 8160 on half of them: the
    per-pixel maximum of diff * Ix.  Two pyrDowns turn it grey, so the upper levels fail minEig and level 0 starts on the point."""
    h, w = hw
    pat = np.array([0, 255, 255, 0], np.uint8)
    a = np.empty(hw, np.uint8)
    a[:split] = pat[np.arange(w) % 4][None, :]
    a[split:] = pat[np.arange(split, h) % 4][:, None]
    return a


def smooth(seed, hw=HW, shift=(0.0, 0.0)):
    """a sum of 14 plane waves of 18 ... 70 px, sampled at (x - shift[0], y - shift[1]): the texture moved by `shift`, any fraction"""
    h, w = hw
    rng = np.random.default_rng(seed)
    lam = rng.uniform(18.0, 70.0, 14)
    th = rng.uniform(0.0, 2 * np.pi, 14)
    ph = rng.uniform(0.0, 2 * np.pi, 14)
    amp = rng.uniform(0.5, 1.0, 14)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    x, y = x - shift[0], y - shift[1]
    v = sum(a * np.sin(2 * np.pi * (x * np.cos(t) + y * np.sin(t)) / l + p) for a, l, t, p in zip(amp, lam, th, ph))
    v = 127.5 + v * (110.0 / np.abs(v).max())
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------ points
def spread(seed, hw, K, beyond=4.0):
    """K points over the image and `beyond` px past it"""
    h, w = hw
    rng = np.random.default_rng(seed)
    return np.column_stack((rng.uniform(-beyond, w + beyond, K), rng.uniform(-beyond, h + beyond, K))).astype(np.float32)


def near_border(seed, hw, K, side, depth=16.0):
    """K points within `depth` px of one border"""
    h, w = hw
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(0, w - 1, K), rng.uniform(0, h - 1, K)
    d = rng.uniform(0, depth, K)
    if side == "left": x = d
    elif side == "right": x = w - 1 - d
    elif side == "top": y = d
    else: y = h - 1 - d
    return np.column_stack((x, y)).astype(np.float32)


def whole_grid(xs, ys):
    return np.array([(x, y) for y in ys for x in xs], np.float32)


def _t(case):
    """the case transposed: images (h, w) -> (w, h), x and y exchanged"""
    out = dict(case, name=case["name"] + "_T", prev=np.ascontiguousarray(case["prev"].T), next=np.ascontiguousarray(case["next"].T),
               pts=np.ascontiguousarray(case["pts"][:, ::-1]))
    if case.get("init") is not None:
        out["init"] = np.ascontiguousarray(case["init"][:, ::-1])
    return out


# ------------------------------------------------------------------------------------------------------------------ cases
OUTWARD = {"left": (-12.0, 0.0), "right": (12.0, 0.0), "top": (0.0, -12.0), "bottom": (0.0, 12.0)}
FAR = {"+x": (34.0, 0.0), "-x": (-34.0, 0.0), "+y": (0.0, 30.0), "-y": (0.0, -30.0), "+x+y": (24.0, 22.0), "-x-y": (-26.0, -21.0)}
ERR_OUTSIDE_NOISE = ((1.9429277181625366, 0.31508323550224304), (2.143702745437622, 0.48497745394706726),
                     (150.2034912109375, 118.61947631835938), (154.0832977294922, 63.00767135620117),
                     (158.93507385253906, 56.52833938598633), (158.8685760498047, 56.988128662109375),
                     (154.1676025390625, 54.79212951660156), (153.5968017578125, 51.81904983520508),
                     (153.7967987060547, 51.81633758544922), (149.60427856445312, 1.8460750579833984),
                     (153.71315002441406, 55.881534576416016), (158.4517364501953, 22.003509521484375))
ERR_OUTSIDE_FAR_T = ((9.122515678405762, 105.37213897705078), (9.584144592285156, 95.92642974853516),
                     (1.2421058416366577, 91.0526123046875), (1.4325451850891113, 89.88329315185547),
                     (9.974452018737793, 92.80314636230469), (2.0310349464416504, 90.8586654663086),
                     (0.1504417508840561, 91.521728515625), (5.7479166984558105, 42.550594329833984),
                     (8.83857536315918, 104.79016876220703), (7.0430402755737305, 90.21903228759766),
                     (3.600018262863159, 90.74524688720703), (4.680995464324951, 91.24110412597656))


def _make_cases():
    out = []

    def add(name, prev, nxt, pts, init=None):
        pts = np.ascontiguousarray(pts, np.float32)
        assert prev.dtype == np.uint8 and nxt.dtype == np.uint8 and prev.shape == nxt.shape and prev.shape in (HW, HW_T)
        assert len(pts) <= (200 if init is None else 64)
        if init is not None:
            init = np.ascontiguousarray(init, np.float32)
            assert init.shape == pts.shape and np.isfinite(init).all() and float(np.abs(init).max()) <= MAX_GUESS
        out.append(dict(name=name, prev=prev, next=nxt, pts=pts, init=init))
        return out[-1]

    def addT(*a):
        out.append(_t(out.pop(out.index(add(*a)))))

    # unrelated noise: nothing converges; windows wander, reload their tile and leave the image
    add("noise", noise(1), noise(2), spread(10, HW, 150))
    addT("noise_b", noise(3), noise(4), spread(11, HW, 60))
    # 0 / 255 blocks against the inverse: flat windows (minEig), the largest mismatches, many reloads
    b = blocks(5)
    add("blocks_inverse", b, 255 - b, spread(12, HW, 150))
    # ... against itself rolled a few pixels in each direction: convergence, the back-off, eps at once
    for name, (ry, rx) in (("right_up", (-5, 3)), ("left_down", (4, -3)), ("right", (0, 6)), ("left", (0, -6)), ("down", (7, 0)),
                           ("up", (-7, 0))):
        add("blocks_roll_" + name, b, np.roll(b, (ry, rx), axis=(0, 1)), spread(13 + abs(ry) + 10 * abs(rx), HW, 60))
    add("blocks_same", b, b.copy(), spread(14, HW, 40))
    bt = blocks(6, HW_T)
    add("blocks_roll_T", bt, np.roll(bt, (3, -5), axis=(0, 1)), spread(15, HW_T, 60))
    # flat with one box: minEig fails at every level away from the box, corners track
    add("box", box(), box(x0=63, x1=113, y0=38, y1=88), np.vstack((spread(16, HW, 70), whole_grid((58, 60, 62, 108, 110, 112), (38, 40, 42, 88, 90, 92)))))
    add("box_grey", box(level=100, value=140), box(level=100, value=140, x0=58, x1=108, y0=43, y1=93),
        whole_grid((50, 60, 70, 85, 100, 110, 120), (30, 40, 50, 65, 80, 90, 100)))
    # all 0, all 255
    for v in (0, 255):
        add("flat_%d" % v, np.full(HW, v, np.uint8), np.full(HW, v, np.uint8), spread(17 + v, HW, 24))
    add("flat_0_to_255", np.zeros(HW, np.uint8), np.full(HW, 255, np.uint8), spread(18, HW, 24))
    # one vertical step edge: rank-one windows (A22 = A12 = 0 away from the borders)
    e = step_edge()
    add("edge", e, np.roll(e, 3, axis=1), np.vstack((spread(19, HW, 40), whole_grid((72, 76, 78, 80, 82, 86), (5, 30.5, 64, 100.25, 124)))))
    addT("edge_back", e, np.roll(e, -2, axis=1), whole_grid((74, 77.5, 80, 81.25, 85), (0, 20, 64, 127)))
    # the stripes: window sums near the limits the kernel's 32-bit row sums rely on, in both roll directions and transposed
    s = stripes()
    grid = whole_grid(range(21, 141, 8), (28, 30, 32, 33, 36))
    for name, r in (("plus", 1), ("minus", -1)):
        out.append(_t(add("stripes_" + name, s, np.roll(s, r, axis=1), grid)))
    # a smooth texture moved further than half a tile at some level
    for name, sh in FAR.items():
        add("far_" + name, smooth(20), smooth(20, shift=sh), spread(21, HW, 60, beyond=0.0))
    add("far_T", smooth(22, HW_T), smooth(22, HW_T, shift=(-28.0, 33.0)), spread(23, HW_T, 60, beyond=0.0))
    # features within 16 px of a border whose true motion points out of the image
    for side, sh in OUTWARD.items():
        add("outward_" + side, smooth(24), smooth(24, shift=sh), near_border(25, HW, 40, side))
    add("outward_T", smooth(26, HW_T), smooth(26, HW_T, shift=(9.5, 11.25)), np.vstack((near_border(27, HW_T, 30, "right"), near_border(28, HW_T, 30, "bottom"))))
    # noise around the borders: ten iterations whose last step leaves the image (the error position outside)
    for i, side in enumerate(("left", "right", "top", "bottom")):
        add("noise_border_" + side, noise(30 + i), noise(40 + i), near_border(50 + i, HW, 100, side, depth=6.0))
    # ... found by search (ERR_OUTSIDE_*): 100 000 points within 10 px of the borders of each pair, 25 000 per side, the oracle's
    # status-0 points whose final window lies outside traced by the model; all leave with the step of the tenth iteration
    add("err_outside_noise", noise(30), noise(40), np.vstack((np.float32(ERR_OUTSIDE_NOISE), near_border(54, HW, 20, "right", depth=6.0))))
    add("err_outside_far_T", smooth(22, HW_T), smooth(22, HW_T, shift=(-28.0, 33.0)), np.float32(ERR_OUTSIDE_FAR_T))
    # points 9 ... 60 px outside the image: no window at level 0 (status 0, err 0), tracked in the levels above it
    g = np.random.default_rng(29)
    far_out = np.vstack([np.column_stack((g.uniform(-60, -9, 10), g.uniform(0, HW[0], 10))), np.column_stack((g.uniform(HW[1] + 8, HW[1] + 50, 10), g.uniform(0, HW[0], 10))),
                         np.column_stack((g.uniform(0, HW[1], 10), g.uniform(-60, -9, 10))), np.column_stack((g.uniform(0, HW[1], 10), g.uniform(HW[0] + 8, HW[0] + 50, 10))),
                         [(-8.0, 64.0), (-8.001, 64.0), (-64.0, 64.0), (-64.001, 64.0), (HW[1] + 7.0, 3.0), (HW[1] + 6.999, 3.0), (5.0, HW[0] + 7.0), (5.0, -8.5)]])
    add("beyond", smooth(24), smooth(24, shift=(2.5, 1.75)), far_out)

    # ---- seeded entry
    a0, a1 = smooth(60), smooth(60, shift=(3.25, -2.5))
    p = spread(61, HW, 64, beyond=2.0)
    i = np.arange(64)
    outside = p.copy()
    outside[i % 4 == 0, 0] = -140.0
    outside[i % 4 == 1, 0] = HW[1] + 130.5
    outside[i % 4 == 2, 1] = -129.25
    outside[i % 4 == 3, 1] = HW[0] + 300.0
    add("seed_same", a0, a1, p, p.copy())
    add("seed_outside_top_level", a0, a1, p, outside)
    huge = p.copy()
    huge[i % 2 == 0, 0] = np.where(i[i % 2 == 0] % 4 == 0, MAX_GUESS, -MAX_GUESS)
    huge[i % 2 == 1, 1] = np.where(i[i % 2 == 1] % 4 == 1, 99999.5, -65536.0)
    add("seed_huge", a0, a1, p, huge)
    truth = p + np.float32([3.25, -2.5])
    ang = np.random.default_rng(62).uniform(0, 2 * np.pi, 64)
    add("seed_30_from_truth", a0, a1, p, truth + 30.0 * np.column_stack((np.cos(ang), np.sin(ang))))
    for name, sh in (("+x", (64.0, 0.0)), ("-x", (-68.0, 0.0)), ("+y", (0.0, 64.0)), ("-y", (0.0, -68.0))):
        # seeded 64 px short of the truth: the top level has 8 px to walk and reloads in that direction
        q = spread(64, HW, 32, beyond=0.0)
        add("seed_walk_" + name, a0, a1, q, (q + np.float32([3.25, -2.5]) - np.float32(sh)).astype(np.float32))
    bs = blocks(7)
    add("seed_blocks", bs, 255 - bs, p, (p + np.float32([-9.0, 14.5])).astype(np.float32))
    addT("seed_noise", noise(8), noise(9), p[:32], (p[:32] + np.float32([20.0, -6.0])).astype(np.float32))
    return out


def cases():
    if "cases" not in _cache:
        cs = _make_cases()
        assert len({c["name"] for c in cs}) == len(cs)
        for c in cs:
            for a in (c["prev"], c["next"], c["pts"]) + (() if c["init"] is None else (c["init"],)):
                a.setflags(write=False)
        _cache["cases"] = cs
    return _cache["cases"]


def unseeded():
    return [c for c in cases() if c["init"] is None]


def seeded():
    return [c for c in cases() if c["init"] is not None]


def traced(case):
    """-> ((next, status, err), trace) of the model on the case, once per process"""
    key = ("trace", case["name"])
    if key not in _cache:
        tr = []
        res = M.track_on_pyramids(M.build_pyramid(case["prev"]), M.build_pyramid(case["next"]), case["pts"], case["init"], trace=tr)
        _cache[key] = (res, tr)
    return _cache[key]


# ------------------------------------------------------------------------------------------------------------------ classes
SIDES = ("left", "right", "top", "bottom")
CLASSES = (("mineig_l%d_tracked" % l for l in (3, 2, 1)), ("mineig_l0", "d_only", "eps_j0", "eps_j1", "backoff"),
           ("maxiter_l%d" % l for l in (3, 2, 1, 0)), ("left_upper", "left_l0", "err_outside"),
           ("reload_" + d for d in ("+x", "-x", "+y", "-y")), ("reloads_0", "reloads_2"), ("tile_" + s for s in SIDES),
           ("tile_corner", "tile_interior", "err_reload", "prev_outside_upper_l0_inside", "prev_outside_l0_upper_inside", "start_outside"))
CLASSES = tuple(n for g in CLASSES for n in g)


def entry_classes(e, status_k, l0_exit):
    """the classes one trace entry (point, level) belongs to; status_k: the point's final status, l0_exit: its level-0 exit"""
    c, lv, ex = [], e["level"], e["exit"]
    if ex == "prev_outside":
        if lv >= 1 and l0_exit != "prev_outside": c.append("prev_outside_upper_l0_inside")
        return c
    if lv >= 1 and l0_exit == "prev_outside": c.append("prev_outside_l0_upper_inside")
    if ex == "mineig":
        if lv == 0: c.append("mineig_l0")
        elif status_k: c.append("mineig_l%d_tracked" % lv)
    elif ex == "d_only": c.append("d_only")
    elif ex == "eps0": c.append("eps_j0")
    elif ex == "eps": c.append("eps_j1")
    elif ex == "backoff": c.append("backoff")
    elif ex == "maxiter": c.append("maxiter_l%d" % lv)
    elif ex == "left": c.append("start_outside" if e["iters"] == 0 else "left_l0" if lv == 0 else "left_upper")
    if e["err_outside"]: c.append("err_outside")
    if e["err_reload"]: c.append("err_reload")
    for dirs in e["reloads"]:
        c.extend("reload_" + d for d in dirs)
    if e["iters"] >= 1:
        n = len(e["reloads"])
        if n == 0: c.append("reloads_0")
        if n >= 2: c.append("reloads_2")
    for sides in e["tiles"]:
        # the levels in which a tile fits: from 32 x 40 down every tile leaves the image on two opposite sides at least
        if not sides: c.append("tile_interior")
        elif len(sides) == 1: c.append("tile_" + next(iter(sides)))
        elif len(sides) == 2 and sides & {"left", "right"} and sides & {"top", "bottom"} and lv <= 1: c.append("tile_corner")
    return c


def point_classes(case):
    """-> per point, the list of (level, class) of its trace entries: what a failing device comparison reports"""
    (_, status, _), tr = traced(case)
    l0 = {e["k"]: e["exit"] for e in tr if e["level"] == 0}
    out = [[] for _ in range(len(case["pts"]))]
    for e in tr:
        cl = entry_classes(e, int(status[e["k"], 0]), l0[e["k"]])
        out[e["k"]].append((e["level"], e["exit"], tuple(cl)))
    return out


def membership(case):
    """-> {class: member (point, level) entries} of one case (an entry with two reloads in one direction counts once)"""
    (_, status, _), tr = traced(case)
    l0 = {e["k"]: e["exit"] for e in tr if e["level"] == 0}
    m = dict.fromkeys(CLASSES, 0)
    for e in tr:
        for c in set(entry_classes(e, int(status[e["k"], 0]), l0[e["k"]])):
            m[c] += 1
    return m


def margins(case):
    """-> dict: per quantity of M.SUM_NAMES the largest row-group sum over the case ("group_" + name; the diff sums exist only where a
    window passed minEig), and the largest whole-window |diff * Ix| and |diff * Iy| sums among the points that end with status 1"""
    (_, status, _), tr = traced(case)
    out = {"group_" + n: max((e["group"][n] for e in tr), default=0) for n in M.SUM_NAMES}
    out["whole_dIx"] = max((e["whole"]["dIx"] for e in tr if status[e["k"], 0]), default=0)
    out["whole_dIy"] = max((e["whole"]["dIy"] for e in tr if status[e["k"], 0]), default=0)
    return out
