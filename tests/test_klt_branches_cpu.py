"""CPU (-m "not gpu"): the cases of tests/klt_branch_cases.py reach the branches of klt_kernel they are made for - asserted with the
traced model (tests/klt_flow_model.py) and the oracle alone, both of which sum in int64 - and the inputs reach the magnitudes at
which the kernel's 24-bit products, 32-bit row sums and 64-bit scalar sums would show an error.  The device is compared on the same
cases in tests/test_gpu_klt_branches.py."""
import numpy as np
import pytest

import klt_branch_cases as B
import klt_flow_model as M
import oracle

F = np.float32
PIXEL_MAX = 8160 * 4080                 # |diff| <= 255 << 5, |Ix|, |Iy| <= 4080: the largest product of one window pixel
MIN_MEMBERS = 3


@pytest.fixture(scope="module")
def totals():
    per_case = {c["name"]: B.membership(c) for c in B.cases()}
    print("members per class, all cases:", {k: sum(m[k] for m in per_case.values()) for k in B.CLASSES})
    return per_case


def test_model_equals_oracle_on_every_unseeded_case():
    """next, status and err bit for bit; the trace changes no result; a seed equal to the points is no seed"""
    tracked = 0
    for c in B.unseeded():
        want = oracle.calcOpticalFlowPyrLK(c["prev"], c["next"], c["pts"])
        got, _ = B.traced(c)
        for g, w, what in zip(got, want, ("next", "status", "err")):
            assert np.array_equal(g, w), (c["name"], what, np.nonzero((g != w).any(axis=1))[0][:5])
        for x, y in zip(M.build_pyramid(c["prev"]) + M.build_pyramid(c["next"]), oracle.build_pyramid(c["prev"], 3) + oracle.build_pyramid(c["next"], 3)):
            assert np.array_equal(x, y), c["name"]
        tracked += int(want[1].sum())
    assert tracked >= 1000
    for c in B.unseeded()[:4] + B.seeded()[:2]:
        plain = M.track_on_pyramids(M.build_pyramid(c["prev"]), M.build_pyramid(c["next"]), c["pts"], c["init"])
        assert all(np.array_equal(x, y) for x, y in zip(plain, B.traced(c)[0])), c["name"]
    c = next(x for x in B.seeded() if x["name"] == "seed_same")
    assert all(np.array_equal(x, y) for x, y in zip(B.traced(c)[0], oracle.calcOpticalFlowPyrLK(c["prev"], c["next"], c["pts"])))


def test_case_rules():
    shapes = set()
    for c in B.cases():
        assert c["prev"].dtype == np.uint8 and c["next"].dtype == np.uint8 and c["prev"].shape == c["next"].shape
        shapes.add(c["prev"].shape)
        assert 1 <= len(c["pts"]) <= (200 if c["init"] is None else 64), c["name"]
        if c["init"] is not None:
            assert np.isfinite(c["init"]).all() and float(np.abs(c["init"]).max()) <= B.MAX_GUESS
    assert shapes == {B.HW, B.HW_T}
    assert any(float(np.abs(c["init"]).max()) == B.MAX_GUESS for c in B.seeded())


# classes every (point, level) entry of which is counted over the unseeded cases: what the device is held to the ORACLE on
REQUIRED = tuple(n for n in B.CLASSES if n not in ("d_only", "prev_outside_upper_l0_inside", "start_outside"))


@pytest.mark.parametrize("name", REQUIRED)
def test_class_has_members(totals, name):
    n = sum(totals[c["name"]][name] for c in B.unseeded())
    assert n >= MIN_MEMBERS, (name, n)


def test_seeded_cases_reach_their_branches(totals):
    """the starts the seeded entry adds: outside the image at the top level, 30 px from the truth (ten iterations at the top level,
    which the same pair seeded with the points never needs), and the walk of the top level in each direction"""
    s = {c["name"]: totals[c["name"]] for c in B.seeded()}
    assert s["seed_outside_top_level"]["start_outside"] >= 64 and s["seed_huge"]["start_outside"] >= 64
    assert s["seed_30_from_truth"]["maxiter_l3"] >= MIN_MEMBERS and s["seed_same"]["maxiter_l3"] == 0
    for d in ("+x", "-x", "+y", "-y"):
        assert sum(m["reload_" + d] for m in s.values()) >= MIN_MEMBERS, d
    for name in ("eps_j0", "eps_j1", "left_l0", "left_upper", "mineig_l0", "reloads_2", "err_reload", "tile_corner", "tile_interior"):
        assert sum(m[name] for m in s.values()) >= MIN_MEMBERS, name
    st = np.concatenate([B.traced(c)[0][1].ravel() for c in B.seeded()])
    assert 100 <= int(st.sum()) < len(st) - 100


def test_no_window_is_outside_above_level_0_and_inside_at_level_0(totals):
    """Previous window outside the level image at level 3, 2 or 1 with level 0 inside: empty by geometry, for every image size.
    Level l is inside when -15 <= floor(x 2^-l - 7) < w_l with w_l >= w 2^-l.  Level 0 inside means -8 <= x < w + 7; then
    x 2^-l - 7 >= -8 2^-l - 7 >= -15 and x 2^-l - 7 < (w + 7) 2^-l - 7 <= w_l (x 2^-l is exact in float32, and rounding the
    difference is monotone, so the comparisons survive it).  The converse exists and is a required class
    (prev_outside_l0_upper_inside: -8 2^l <= x < -8)."""
    assert sum(m["prev_outside_upper_l0_inside"] for m in totals.values()) == 0
    for w in (128, 160, 129, 15, 1000, 2024):
        x = np.arange(-200 * 64, (w + 200) * 64, dtype=np.float64) / 64
        edges = F([-8, w + 7, -64, -32, -16])
        x = np.unique(np.concatenate([x.astype(F), edges, np.nextafter(edges, F(-np.inf)), np.nextafter(edges, F(np.inf))]))
        wl, inside = w, []
        for l in range(4):
            ip = np.floor(x * F(1.0 / (1 << l)) - F(7.0))
            inside.append((ip >= -M.WIN) & (ip < wl))
            wl = (wl + 1) // 2
        assert inside[0].any() and not inside[0].all()
        for l in (1, 2, 3):
            assert not (inside[0] & ~inside[l]).any(), (w, l)
            assert (inside[l] & ~inside[0]).any()


def _window_matrices(img):
    """A11, A12, A22 (float32, as the tracker forms them) of every whole-pixel window that lies inside the image"""
    dx, dy = M._scharr(img)                         # whole-pixel position: weights (2^14, 0, 0, 0), Ix = dx and Iy = dy exactly

    def wsum(p):
        c = np.zeros((p.shape[0] + 1, p.shape[1] + 1), np.int64)
        c[1:, 1:] = p.cumsum(0).cumsum(1)
        n = M.WIN
        return (c[n:, n:] - c[:-n, n:] - c[n:, :-n] + c[:-n, :-n]).ravel()

    s = F(1.0 / (1 << 20))
    return [wsum(p).astype(F) * s for p in (dx * dx, dx * dy, dy * dy)]


def test_d_only_failure_search():
    """minEig passes and D < FLT_EPSILON: searched on 466 032 windows whose matrices are nearly rank one with large entries (0 / 255
    diagonal stripes of five periods, one of the other diagonal and one step edge, each as it is and with up to 1, 4 and 16 grey
    levels of noise added to one in 50 pixels; every whole-pixel window inside the 128 x 160 image), none found; the class is unpopulated, and cannot be populated:
    minEig = 2 lambda_min / 450 >= 1e-4 means lambda_min >= 0.0225 less the rounding of its seven operations, each relative 2^-24 on a
    result that counts for at most 7144 (2 * 225 * 4080^2 / 2^20) in 2 lambda_min: < 3e-3, so lambda_min >= 0.02 and the exact D = lambda_min lambda_max >= 0.02 lambda_max;
    the float32 D differs from it by the rounding of the three sums (2^-24 each) and of two products and a difference of numbers
    <= lambda_max^2, together < 1e-6 lambda_max^2 <= 7.2e-3 lambda_max.  So D >= 0.0128 lambda_max >= 2.5e-4 > FLT_EPSILON: after the
    minEig test the D test never decides (asserted on every window here as D >= 0.0064 (A11 + A22))."""
    rng = np.random.default_rng(70)
    h, w = B.HW
    y, x = np.mgrid[0:h, 0:w]
    bases = [np.where((x + y) % p < p // 2, 255, 0) for p in (4, 6, 8, 12, 16)] + [np.where((x - y) % 6 < 3, 255, 0), B.step_edge().astype(np.int64)]
    windows = d_only = near = 0
    for base in bases:
        for amp in (0, 1, 4, 16):
            img = base.copy()
            if amp:
                m = rng.random(base.shape) < 0.02
                img[m] = np.clip(img[m] + rng.integers(-amp, amp + 1, int(m.sum())), 0, 255)
            A11, A12, A22 = _window_matrices(img.astype(np.uint8))
            D = A11 * A22 - A12 * A12
            dA = A11 - A22
            minEig = (A22 + A11 - np.sqrt(dA * dA + F(4.0) * A12 * A12)) / F(2 * M.WIN * M.WIN)
            windows += D.size
            d_only += int(((minEig >= M.MIN_EIG) & (D < F(1.1920929e-07))).sum())
            near += int(((minEig < M.MIN_EIG) & (A11 + A22 > F(1000.0))).sum())
            ok = minEig >= M.MIN_EIG
            assert not ok.any() or float((D[ok] / (A11 + A22)[ok]).min()) >= 0.0064         # lambda_max >= trace / 2
    print("D-only search: windows", windows, "found", d_only, "rank-one windows with a trace above 1000 that fail minEig:", near)
    assert windows >= 100000 and near >= 10000
    assert d_only == 0
    assert sum(B.membership(c)["d_only"] for c in B.cases()) == 0


def test_margins():
    """the inputs reach the limits the kernel's comments rely on, each quantity on its own.
    In x (stripes_*): the 16-lane row sum of diff * Ix holds 32 pixels at the per-pixel maximum, 1 065 369 600 >= 1.0e9 (the 32-bit DPP
    sum); the window's diff * Ix sum is 3 945 196 800 >= 2^31 on a point that ends with status 1 (the 64-bit scalar sum, __ll2float_rn).
    Transposed, in y: the window's diff * Iy sum is the same 3 945 196 800, but the row-group sum of diff * Iy is 986 299 200, not 1.0e9,
    and cannot reach it: diff and Iy are both at their maximum in a pixel only if I[y] = I[y + 1] != I[y - 1] there, so in no two
    consecutive rows, 2 rows x 15 pixels = 998 784 000 at most; and a window in which all 15 pixels of a row have |Iy| = 4080 has
    rows that are uniform across it, Ix = 0 everywhere, and fails minEig before any mismatch is formed.  In the stripe cases the
    rank comes from the window's last column, beside the other stripes, where Iy is 13 / 16 of 4080: 2 x (14 + 13 / 16) pixels.
    The row-group sum of Iy^2 (formed before the minEig test) is 60 x 4080^2 = 998 784 000, as Ix^2 is in x."""
    m = {c["name"]: B.margins(c) for c in B.cases() if c["name"].startswith("stripes_")}
    for name, v in m.items():
        print("margins", name, v)
    t = {k: v for k, v in m.items() if k.endswith("_T")}
    x = {k: v for k, v in m.items() if not k.endswith("_T")}
    assert len(t) == len(x) == 2

    def top(d, key):
        return max(v[key] for v in d.values())

    assert top(x, "group_dIx") == 32 * PIXEL_MAX == 1065369600 >= 1.0e9
    assert top(x, "group_IxIx") == 60 * 4080 ** 2 == 998784000
    assert top(x, "whole_dIx") == 3945196800 >= 2 ** 31
    assert top(t, "group_dIy") == 2 * (14 * PIXEL_MAX + PIXEL_MAX * 13 // 16) == 986299200 < 30 * PIXEL_MAX
    assert top(t, "group_IyIy") == 60 * 4080 ** 2 == 998784000 == 30 * PIXEL_MAX
    assert top(t, "whole_dIy") == 3945196800 >= 2 ** 31
    assert all(v < 2 ** 31 for d in m.values() for k, v in d.items() if k.startswith("group_"))
    # the bound the kernel's comment states for a row of 16 lanes, and what the 60 pixels of it can really reach
    assert 60 * PIXEL_MAX < 64 * PIXEL_MAX < 2 ** 31


@pytest.mark.parametrize("which", ("b", "A"))
def test_window_sums_kept_in_32_bits_would_be_noticed(monkeypatch, which):
    """the model with its whole-window sums wrapped to int32 - the mismatch sums b1, b2, or the matrix sums A11, A12, A22 - differs
    from the oracle on points of every stripe case (39 ... 45 of 75, printed): the margins above are reached where they change a
    result"""
    exact = M._wsum

    def wsum(p, what):
        v = exact(p, what)
        return ((v + 2 ** 31) % 2 ** 32) - 2 ** 31 if what == which else v

    monkeypatch.setattr(M, "_wsum", wsum)
    for c in B.cases():
        if not c["name"].startswith("stripes_"):
            continue
        got = M.track_on_pyramids(M.build_pyramid(c["prev"]), M.build_pyramid(c["next"]), c["pts"])
        want = oracle.calcOpticalFlowPyrLK(c["prev"], c["next"], c["pts"])
        differ = int(((got[0] != want[0]).any(axis=1) | (got[1] != want[1]).ravel() | (got[2] != want[2]).ravel()).sum())
        print("32-bit", which, "sums:", c["name"], "points that differ", differ, "of", len(c["pts"]))
        assert differ > 0, c["name"]


def test_float_entry_sees_the_same_bytes():
    """image / 255 as float32 is what the GPU test gives the float32 entry; its truth is oracle.quantize_u8 of that image, which here
    is the byte it came from, for every byte: both entries are held to the same results, the float32 one through the quantisation"""
    v = np.arange(256, dtype=np.uint8).reshape(1, -1)
    assert np.array_equal(oracle.quantize_u8(v.astype(np.float32) / np.float32(255.)), v)


def test_tile_rule_of_the_trace():
    """the model's restatement of the tile rule on hand-made walks: kept 0 ... 15 from the origin, reloaded at -1 and 16 with origin
    (ix - 8, iy - 8); the sides a tile leaves the image on"""
    e = dict(tiles=[])
    tile, dirs = M._tile_step(e, None, 40, 50, 160, 128)
    assert tile == (32, 42) and dirs == () and e["tiles"] == [frozenset()]
    for ix, iy in ((32, 42), (47, 57), (32, 57)):
        assert M._tile_step(e, tile, ix, iy, 160, 128) == (tile, None)
    for (ix, iy), want in (((48, 50), ("+x",)), ((31, 50), ("-x",)), ((40, 58), ("+y",)), ((40, 41), ("-y",)), ((48, 41), ("+x", "-y"))):
        t2, dirs = M._tile_step(e, tile, ix, iy, 160, 128)
        assert t2 == (ix - 8, iy - 8) and dirs == want
    assert M._tile_sides(0, 0, 160, 128) == frozenset() and M._tile_sides(128, 96, 160, 128) == frozenset()
    assert M._tile_sides(-1, 0, 160, 128) == {"left"} and M._tile_sides(129, 97, 160, 128) == {"right", "bottom"}
    assert M._tile_sides(5, -23, 160, 128) == {"top"} and M._tile_sides(0, 0, 20, 16) == {"right", "bottom"}
