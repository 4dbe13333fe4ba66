"""CPU (-m "not gpu"): the seeded tracker's model (tests/klt_flow_model.py) tied to the oracle, the known answers of the seed, the
defining property of FMT.flowPriorFromFMT on the CPU models, and the large-rotation pair that a motion prior is for.  The device is
compared with the model in tests/test_gpu_klt_flow.py."""
import math

import numpy as np
import pytest

import klt_flow_cases as C
import klt_flow_model as M
import oracle
import warp_affine_model as wam


@pytest.mark.parametrize("hw", C.SHAPES, ids=lambda s: "%dx%d" % s)
def test_unseeded_model_equals_oracle(hw):
    """every line of the model but the seed: points, status and err bit for bit, points on, inside and outside every border"""
    a, b = C.image_pair(hw)
    pts = C.points(hw, 65)
    want_n, want_s, want_e = oracle.calcOpticalFlowPyrLK(a, b, pts)
    got_n, got_s, got_e = M.track(a, b, pts)
    assert np.array_equal(got_s, want_s) and np.array_equal(got_n, want_n) and np.array_equal(got_e, want_e)
    for x, y in zip(M.build_pyramid(a), oracle.build_pyramid(a, 3)):
        assert np.array_equal(x, y)
    assert 10 <= int(want_s.sum()) < 65          # points that track and border points that do not
    # a seed equal to the points is no seed
    sn, ss, se = M.track(a, b, pts, pts.copy())
    assert np.array_equal(sn, want_n) and np.array_equal(ss, want_s) and np.array_equal(se, want_e)


def test_identity_affine_is_exact():
    pts = np.concatenate([C.points(hw, 65) for hw in C.SHAPES] + [np.float32([[1e-3, 2047.99], [-0.0, 1e6]])])
    got = M.apply_affine([1, 0, 0, 0, 1, 0], pts)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), pts.view(np.uint32) & np.where(pts == 0, 0x7fffffff, 0xffffffff).astype(np.uint32))
    # (x * 1 + y * 0) + 0 turns -0.0 into +0.0 and nothing else: the same position


def test_seed_known_answer():
    """a seed of pts + g finds what the unseeded tracker finds in the image moved back by g, plus g"""
    a, _ = C.image_pair(C.SHIFT_HW)
    pts = C.interior_points(C.SHIFT_HW, 65, 200)
    fx, fy = C.SHIFT_FLOW
    worst = 0.0
    for gx, gy in C.SHIFT_GS:
        nxt = np.roll(a, (fy + gy, fx + gx), axis=(0, 1))
        back = np.roll(nxt, (-gy, -gx), axis=(0, 1))
        want_n, want_s, _ = oracle.calcOpticalFlowPyrLK(a, back, pts)
        g = np.float32([gx, gy])
        got_n, got_s, _ = M.track(a, nxt, pts, (pts + g).astype(np.float32))
        assert np.array_equal(got_s, want_s) and want_s.all()
        d = float(np.abs(got_n.astype(np.float64) - (want_n.astype(np.float64) + g)).max())
        print("seed known answer: g", (gx, gy), "max |difference| px", d)
        worst = max(worst, d)
    assert worst <= C.SHIFT_TOL_PX, worst


def test_flow_prior_defining_property():
    """a smooth texture turned by a known angle and moved by whole pixels on the registration's 202-px grid; the prior made from
    the known angle and the oracle's phase correlation maps interior points of the tracker's 2024-px grid to their true positions
    within one registration pixel (10.02 tracker pixels); either sign flipped misses that bound"""
    from scipy.ndimage import gaussian_filter
    from radarslampy_amd import FMT
    tex = gaussian_filter(np.random.default_rng(3).random((202, 202)), 2.0).astype(np.float32)
    tex = (tex - tex.min()) / (tex.max() - tex.min())
    deg, sx, sy = 7.0, 5, -3
    ang = math.radians(deg)
    rot = wam.rotateImg(tex, deg)
    tgt = np.roll(rot, (sy, sx), axis=(0, 1))
    (dx, dy), _ = oracle.phaseCorrelate(rot, tgt)
    s = 1012 / 101
    Mreg = wam.rotation_matrix_2d((101.0, 101.0), deg, 1.0)
    pts = np.array([[x, y] for x in (500., 800., 1012., 1300., 1500.) for y in (520., 1012., 1480.)], np.float32)
    true = s * ((pts.astype(np.float64) / s) @ Mreg[:, :2].T + Mreg[:, 2] + np.array([sx, sy]))

    def worst(a, d):
        A = FMT.flowPriorFromFMT(a, d)
        assert A.shape == (2, 3) and A.dtype == np.float32
        return float(np.abs(M.apply_affine(A, pts) - true).max())

    e = worst(ang, (dx, dy))
    print("flow prior: max error px", e, "bound", s)
    assert e <= s
    assert worst(-ang, (dx, dy)) > s and worst(ang, (-dx, -dy)) > s
    # the batched form is the single one per pair; another pair of factors gives another scale
    Ab = FMT.flowPriorFromFMT(np.array([ang, -ang]), np.array([[dx, dy], [dy, dx]]))
    assert Ab.shape == (2, 2, 3) and np.array_equal(Ab[0], FMT.flowPriorFromFMT(ang, (dx, dy)))
    assert np.array_equal(Ab[1], FMT.flowPriorFromFMT(-ang, (dy, dx)))
    A1 = FMT.flowPriorFromFMT(0.0, (1.0, 2.0), 5, 5, 497)
    assert np.array_equal(A1, np.float32([[1, 0, 1], [0, 1, 2]]))
    with pytest.raises(ValueError):
        FMT.flowPriorFromFMT(np.zeros(3), np.zeros((2, 2)))
    with pytest.raises(ValueError):
        FMT.flowPriorFromFMT(float("nan"), (0.0, 0.0))


def test_large_rotation_pair_needs_the_prior():
    """8 degrees of yaw between two scans of one world: the unseeded oracle keeps fewer than half of its features, the model seeded
    with the generator's motion keeps more"""
    r = C.rotation_pair()
    unseeded, seeded = C.rotation_counts()
    K = len(r["feats"])
    print("large rotation: features", K, "unseeded good", unseeded, "seeded good", seeded)
    assert unseeded < K / 2 and seeded > unseeded
    assert (unseeded, seeded) == (C.ROT_UNSEEDED_GOOD, C.ROT_SEEDED_GOOD)


def test_cpu_chain_yaw():
    """the use case on the CPU: oracle registration -> flowPriorFromFMT -> model tracker -> oracle rejection and Kabsch; its yaw
    error is what the engine test's bound is twice of"""
    import fmt_register_cases as frc
    from radarslampy_amd import FMT
    r = C.rotation_pair()
    out6 = frc.cpu_chain(C.polar(r["recs"][0]), C.polar(r["recs"][1]), 1012, 10, 20)["out6"]
    A = FMT.flowPriorFromFMT(out6[0], out6[3:5])
    n, s, e = M.track(r["prev"], r["next"], r["feats"], M.apply_affine(A, r["feats"]))
    good = (s.ravel() != 0) & (e.ravel() < M.ERR_THRESHOLD)
    old, new, _ = oracle.rejectOutliers(r["feats"][good], n[good])
    R, _ = oracle.calculateTransformSVD(old, new)
    err = abs(math.atan2(R[1, 0], R[0, 0]) - r["yaw"])
    print("cpu chain: registration", out6, "good", int(good.sum()), "inliers", len(old), "yaw error rad", err)
    assert err <= C.CHAIN_YAW_ERR_RAD
