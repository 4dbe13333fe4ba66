"""CPU (-m "not gpu"): the batched 2-D ICP without a device - the argument checks of _ffi.icp2d_args and of the raw ABI, the model
tests/icp_model.py against the ground truth of the revisit world, the separation of true and wrong places, the tolerance the GPU test
compares with (measured here from the model's variants), and the host glue of radarslampy_amd/LoopClosure.py on a patched aligner.

Measured (this file prints them): the model against the truth at every 4th point, 0.038 / 0.071 / 0.072 m and 0.0038 / 0.0022 / 0.0228
rad, so the truth bound is 0.108 m and 0.0341 rad; inlier fractions at every 2nd point, true 0.357 / 0.400 / 0.326 against wrong at
most 0.138; the model and its variants differ by at most 4.4e-15 m and 0 rad over the cases, so the floor 1e-9 is the tolerance."""
import ctypes
import types

import numpy as np
import pytest

import icp_cases as cases
import icp_model as model


# ---------------------------------------------------------------------------------------------------------------- argument errors
def _ok_pair():
    return [(np.zeros((4, 2)), np.ones((5, 2)))]


@pytest.mark.parametrize("what, make", [
    ("no pair", lambda: ([], None, None)),
    ("src not (k, 2)", lambda: ([(np.zeros((4, 3)), np.ones((5, 2)))], None, None)),
    ("dst not (k, 2)", lambda: ([(np.zeros((4, 2)), np.ones(5))], None, None)),
    ("a pair of three", lambda: ([(np.zeros((4, 2)), np.ones((5, 2)), 1)], None, None)),
    ("src NaN", lambda: ([(np.full((4, 2), np.nan), np.ones((5, 2)))], None, None)),
    ("dst inf", lambda: ([(np.zeros((4, 2)), np.full((5, 2), np.inf))], None, None)),
    ("src beyond 1e6 m", lambda: ([(np.full((4, 2), 2e6), np.ones((5, 2)))], None, None)),
    ("src over the limit", lambda: ([(np.zeros((8193, 2)), np.ones((5, 2)))], None, None)),
    ("dst over the limit", lambda: ([(np.zeros((4, 2)), np.ones((8193, 2)))], None, None)),
    ("text", lambda: ([(np.array([["a", "b"]]), np.ones((5, 2)))], None, None)),
    ("init shape", lambda: (_ok_pair(), np.zeros((2, 3)), None)),
    ("init NaN", lambda: (_ok_pair(), (np.nan, 0, 0), None)),
    ("init inf", lambda: (_ok_pair(), (0, np.inf, 0), None)),
    ("gate_end 0", lambda: (_ok_pair(), None, dict(gate_end=0.0))),
    ("gate_end above gate_start", lambda: (_ok_pair(), None, dict(gate_start=0.4, gate_end=0.5))),
    ("gate NaN", lambda: (_ok_pair(), None, dict(gate_start=np.nan))),
    ("gate inf", lambda: (_ok_pair(), None, dict(gate_start=np.inf))),
    ("decay 0", lambda: (_ok_pair(), None, dict(gate_decay=0.0))),
    ("decay above 1", lambda: (_ok_pair(), None, dict(gate_decay=1.01))),
    ("decay NaN", lambda: (_ok_pair(), None, dict(gate_decay=np.nan))),
    ("max_iterations 0", lambda: (_ok_pair(), None, dict(max_iterations=0))),
    ("max_iterations 2.5", lambda: (_ok_pair(), None, dict(max_iterations=2.5))),
    ("min_pairs 1", lambda: (_ok_pair(), None, dict(min_pairs=1))),
    ("eps negative", lambda: (_ok_pair(), None, dict(eps_trans=-1.0))),
    ("eps NaN", lambda: (_ok_pair(), None, dict(eps_rot=np.nan))),
    ("unknown option", lambda: (_ok_pair(), None, dict(gate=1.0))),
])
def test_icp2d_args_raises_before_a_device_is_asked_for(what, make, monkeypatch):
    from radarslampy_amd import _ffi
    from radarslampy_amd import LoopClosure

    def no_device(*a, **k):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(_ffi, "default_context", no_device)
    pairs, init, opts = make()
    with pytest.raises(ValueError, match="icp2d"):
        _ffi.icp2d_args(pairs, init, opts)
    if pairs and what != "a pair of three":
        with pytest.raises(ValueError, match="icp2d"):
            LoopClosure.alignPointClouds([p[0] for p in pairs], [p[1] for p in pairs], (0, 0, 0) if init is None else init, **(opts or {}))


def test_too_many_pairs():
    from radarslampy_amd import _ffi
    e = np.zeros((0, 2))
    with pytest.raises(ValueError, match="65535"):
        _ffi.icp2d_args([(e, e)] * 65536)


def test_icp2d_args_packs_the_pairs():
    from radarslampy_amd import _ffi
    a, b, c = np.arange(8.0).reshape(4, 2), np.arange(6.0).reshape(3, 2), np.zeros((0, 2))
    so, s, do, d, x0, o = _ffi.icp2d_args([(a, b), (c, a), (b, [])], (0.5, 1, 2), dict(max_iterations=7))
    assert so.dtype == np.int32 and so.tolist() == [0, 4, 4, 7] and do.tolist() == [0, 3, 7, 7]
    assert np.array_equal(s, np.concatenate([a, b])) and np.array_equal(d, np.concatenate([b, a])) and s.flags.c_contiguous
    assert x0.shape == (3, 3) and np.array_equal(x0[2], [0.5, 1, 2])
    assert (o.gate_start, o.gate_end, o.gate_decay, o.max_iterations, o.eps_trans, o.eps_rot, o.min_pairs) == (3.0, 0.5, 0.8, 7, 1e-4, 1e-5, 3)
    assert ctypes.sizeof(_ffi.IcpOpts) == 56 and _ffi.ICP_STATS.itemsize == 24       # roam_icp_opts / roam_icp_stats of roam_abi.h


def test_raw_abi_null_context():
    from radarslampy_amd import _ffi
    lib = _ffi.load_library()
    assert lib.roam_icp2d_batch(None, 1, None, None, None, None, None, None, None, None) == _ffi.ROAM_E_ARG
    ms = ctypes.c_float()
    assert lib.roam_time_icp2d_batch(None, 1, None, None, None, None, None, None, 1, ctypes.byref(ms)) == _ffi.ROAM_E_ARG


# ---------------------------------------------------------------------------------------------------------------- the model
def test_model_exact_cases():
    p, s = cases.case_model("identical_64")
    assert np.array_equal(p, np.zeros(3)) and s["rms"] == 0.0 and s["status"] == model.OK
    p, s = cases.case_model("rigid_64")
    assert np.abs(p - [0.3, 0.4 * np.cos(1.0), 0.4 * np.sin(1.0)]).max() <= 1e-12 and s["status"] == model.OK and s["n_inliers"] == 64
    low, high = cases.case_model("dup_low_first")[0], cases.case_model("dup_high_first")[0]
    assert abs(high[0] - low[0]) <= 1e-12 and np.abs(high[1:] - low[1:] - cases.DUP_DELTA).max() <= 1e-12     # the choice changes the sums
    for name in ("n0", "m0", "gated_out", "n1_m1", "n2_m2"):
        p, s = cases.case_model(name)
        assert s["status"] == model.FEW_PAIRS and s["iterations"] == 0 and np.array_equal(p, cases.case(name)[2]), name
    assert cases.case_model("n3_m1")[0][0] == 0.3                    # both sums exactly zero: theta stays
    assert cases.case_model("max_iterations_1")[1]["status"] == model.MAX_ITERATIONS
    for name in (f"m{cases.TILE - 1}", f"m{cases.TILE + 1}"):        # the last two dst points are partners
        trace = []
        src, dst, init, opts = cases.case(name)
        model.icp(src, dst, init, trace=trace, **opts)
        part = trace[-1][0][trace[-1][1]]
        assert part[0] == len(dst) - 1 and part[1] == len(dst) - 2 and part.min() < cases.TILE // 2, name


def test_lowest_index_on_exact_ties():
    """four dst points at one distance of the src point: np.argmin, and so the model, takes the first"""
    src = np.array([[0.0, 0.0]])
    dst32 = np.array([[0.0, 1.0], [1.0, 0.0], [0.0, -1.0], [-1.0, 0.0]], np.float32)
    for roll in range(4):
        part, kept = model.search(src, np.roll(dst32, roll, axis=0), 0.0, 0.0, 0.0, np.float32(4.0))
        assert part[0] == 0 and kept[0]


def test_search_without_fused_multiply_add_differs_from_a_fused_one_somewhere():
    """the two forms of d2 are different functions: the contract names the un-fused one"""
    rng = np.random.default_rng(3)
    a = rng.uniform(-50, 50, (2000, 2)).astype(np.float32)
    dx, dy = a[:, 0], a[:, 1]
    plain = dx * dx + dy * dy
    fused = (dx.astype(np.float64) * dx.astype(np.float64) + (dy * dy).astype(np.float64)).astype(np.float32)
    assert plain.dtype == np.float32 and np.any(plain != fused)


def test_model_against_truth_on_the_revisit_world():
    errs = []
    for t, (pose, stats) in enumerate(cases.revisit_model(4)):
        e = cases.pose_error(pose, cases.revisit_truth(t))
        print(f"revisit {t}, every 4th point: {e[0]:.4f} m, {e[1]:.5f} rad off the truth; {stats}")
        assert stats["status"] == model.OK
        errs.append(e)
    bound = cases.truth_bound()
    print(f"truth bound {bound[0]:.4f} m, {bound[1]:.5f} rad")
    assert max(e[0] for e in errs) <= bound[0] and max(e[1] for e in errs) <= bound[1]
    # the caps are a condition: 1.5 times the largest error stays under them
    assert 1.5 * max(e[0] for e in errs) <= cases.TRUTH_CAP_M and 1.5 * max(e[1] for e in errs) <= cases.TRUTH_CAP_RAD


def test_true_places_separate_from_wrong_places():
    true, wrong = cases.revisit_fractions(2)
    print(f"every 2nd point: true-place fractions {true}, wrong-place fractions {wrong.tolist()}")
    assert true.min() >= 2.0 * wrong.max()


def test_device_tolerance_is_measured_and_its_caps_hold():
    t = cases.tolerance_measured()
    for name, (dm, dr) in t.items():
        print(f"{name}: the variants move the pose or the rms by {dm:.3e} m, the angle by {dr:.3e} rad")
    tol_m, tol_rad = cases.tolerance()
    print(f"tolerance {tol_m:.3e} m, {tol_rad:.3e} rad")
    assert set(t) == set(cases.CASES)
    assert cases.TOL_FLOOR <= tol_m <= cases.TOL_CAP_M and cases.TOL_FLOOR <= tol_rad <= cases.TOL_CAP_RAD


# ---------------------------------------------------------------------------------------------------------------- glue
def test_polar_ind_to_local_metres():
    from radarslampy_amd.LoopClosure import polarIndToLocalMetres
    pc = np.array([[0, 100], [100, 100], [200, 50], [300, 1000], [50, 0]])
    got = polarIndToLocalMetres(pc, 400)
    want = np.array([[4.32, 0.0], [0.0, 4.32], [-2.16, 0.0], [0.0, -43.2], [0.0, 0.0]])
    assert got.dtype == np.float64 and got.shape == (5, 2) and np.abs(got - want).max() <= 1e-12
    assert np.abs(polarIndToLocalMetres(np.array([[50, 10]]), 400, 1.0)[0] - 10 * np.sqrt(0.5)).max() <= 1e-12
    assert polarIndToLocalMetres(np.zeros((0, 2), np.int64), 400).shape == (0, 2)
    assert np.allclose(got, cases.cloud_from_peaks(pc.astype(np.float64)), atol=1e-12)
    with pytest.raises(ValueError):
        polarIndToLocalMetres(np.zeros((3, 3)), 400)
    with pytest.raises(ValueError):
        polarIndToLocalMetres(pc, 0)


def _se2(p):
    c, s = np.cos(p[2]), np.sin(p[2])
    return np.array([[c, -s, p[0]], [s, c, p[1]], [0, 0, 1.0]])


def _exact_aligner(poses_of_cloud, fraction_ok=None, key=lambda cloud: int(cloud[0, 0])):
    """an aligner that knows every cloud's pose (key: the keyframe number a cloud's first row carries): the pose of src = query onto
    dst = candidate is x_candidate^-1 x_query, as a perfect ICP would return it"""
    from radarslampy_amd import _ffi
    calls = []

    def align(pairs, init, opts):
        calls.append((pairs, np.array(init, float)))
        n = len(pairs)
        poses, stats = np.zeros((n, 3)), np.zeros(n, _ffi.ICP_STATS)
        for k, (src, dst) in enumerate(pairs):
            qi, cj = key(src), key(dst)
            z = model.relative_pose(poses_of_cloud[cj], poses_of_cloud[qi])
            poses[k] = [z[2], z[0], z[1]]
            good = fraction_ok is None or fraction_ok(qi, cj)
            stats[k] = (_ffi.ICP_OK, 5, len(src), len(src) if good else 1, 0.1)
        return poses, stats
    return align, calls


def test_verify_candidates_edge_direction_and_selection(monkeypatch):
    from radarslampy_amd import LoopClosure, _ffi
    rng = np.random.default_rng(0)
    kposes = np.column_stack([rng.uniform(-2, 2, (6, 2)), rng.uniform(-3, 3, 6)])
    clouds = [np.full((10, 2), float(k)) for k in range(6)]
    align, calls = _exact_aligner(kposes, fraction_ok=lambda qi, cj: (qi, cj) != (5, 2))
    monkeypatch.setattr(LoopClosure, "_align_batch", align)
    q = np.array([4, 5], np.int32)
    ci = np.array([[0, 1, -1], [2, 3, -1]], np.int32)
    yaw = np.array([[0.1, 0.2, 0.0], [0.3, 0.4, 0.0]])
    edges, table = LoopClosure.verifyCandidates(clouds, q, ci, yaw, minInlierFraction=0.5, maxRmsM=0.5)
    assert len(calls) == 1 and len(calls[0][0]) == 4                 # one call, the empty slots skipped
    assert np.array_equal(calls[0][1], [[0.1, 0, 0], [0.2, 0, 0], [0.3, 0, 0], [0.4, 0, 0]])
    assert table["query"].tolist() == [4, 4, 5, 5] and table["candidate"].tolist() == [0, 1, 2, 3] and table["slot"].tolist() == [0, 1, 0, 1]
    assert table["accepted"].tolist() == [True, True, False, True] and np.allclose(table["fraction"], [1, 1, 0.1, 1])
    assert [(e[0], e[1]) for e in edges] == [(0, 4), (3, 5)]          # the best per query; the lowest slot on a tie
    for i, j, z in edges:                                             # (candidate, query, x_candidate^-1 x_query) as (tx, ty, theta)
        T = np.linalg.inv(_se2(kposes[i])) @ _se2(kposes[j])
        assert np.allclose(z[:2], T[:2, 2], atol=1e-12) and abs(model.normalize_angle(z[2] - np.arctan2(T[1, 0], T[0, 0]))) <= 1e-12
    edges_all, _ = LoopClosure.verifyCandidates(clouds, q, ci, yaw, minInlierFraction=0.5, maxRmsM=0.5, allPerQuery=True)
    assert [(e[0], e[1]) for e in edges_all] == [(0, 4), (1, 4), (3, 5)]
    # the other three conditions
    assert LoopClosure.verifyCandidates(clouds, q, ci, yaw, maxRmsM=0.05)[0] == []
    far = np.hypot(table["tx"], table["ty"])
    edges_t, table_t = LoopClosure.verifyCandidates(clouds, q, ci, yaw, maxTranslationM=float(far[table["accepted"]].min()) + 1e-9, allPerQuery=True)
    assert table_t["accepted"].sum() == 1 and len(edges_t) == 1

    def few(pairs, init, opts):
        poses, stats = align(pairs, init, opts)
        stats["status"] = _ffi.ICP_FEW_PAIRS
        return poses, stats
    monkeypatch.setattr(LoopClosure, "_align_batch", few)
    assert LoopClosure.verifyCandidates(clouds, q, ci, yaw)[0] == []
    # the default rms bound is gate_end
    monkeypatch.setattr(LoopClosure, "_align_batch", align)
    assert LoopClosure.verifyCandidates(clouds, q, ci, yaw, gate_end=0.05, gate_start=1.0)[0] == []
    assert len(LoopClosure.verifyCandidates(clouds, q, ci, yaw, gate_end=0.2, gate_start=1.0)[0]) == 2
    # nothing to try: no call
    n_calls = len(calls)
    e0, t0 = LoopClosure.verifyCandidates(clouds, q, np.full((2, 3), -1, np.int32), yaw)
    assert e0 == [] and len(t0) == 0 and len(calls) == n_calls


def test_the_edge_feeds_the_pose_graph_in_its_own_convention():
    """graphFromKeyframes measures its odometry edges as x_k^-1 x_{k+1}; an edge of verifyCandidates is x_candidate^-1 x_query, the
    same form with (i, j) = (candidate, query)"""
    from radarslampy_amd import PoseGraphLib
    a, b = np.array([1.0, 2.0, 0.5]), np.array([-0.5, 1.0, -1.2])
    assert np.allclose(PoseGraphLib.odometryEdges(np.stack([a, b]))[0], model.relative_pose(a, b), atol=1e-15)


def test_close_loops_builds_the_expected_graph(monkeypatch):
    from radarslampy_amd import LoopClosure, PoseGraphLib
    rng = np.random.default_rng(1)
    n = 6
    true = np.column_stack([rng.uniform(-5, 5, (n, 2)), rng.uniform(-3, 3, n)])
    true[5, :2] = true[1, :2] + [0.5, -0.3]                          # keyframe 5 revisits keyframe 1
    kfs = [types.SimpleNamespace(pose=true[k] + 0.1 * k, pointCloud=np.full((10, 2), k), radarPolarImg=np.zeros((400, 8), np.float32))
           for k in range(n)]
    by_range = lambda cloud: int(round(np.hypot(*cloud[0]) / 0.0432))      # polar indices [k, k] -> a point k range bins out
    align, calls = _exact_aligner(true, fraction_ok=lambda qi, cj: (qi, cj) == (5, 1), key=by_range)
    monkeypatch.setattr(LoopClosure, "_align_batch", align)
    seen = {}

    class Detector:
        def __len__(self):
            return n

        def query(self, idx):
            seen["idx"] = np.array(idx)
            ci = np.full((n, 2), -1, np.int32)
            ci[5] = [0, 1]
            ci[3] = [2, -1]
            return ci, np.zeros((n, 2)), np.zeros((n, 2))
    optimised = []
    monkeypatch.setattr(PoseGraphLib.PoseGraphOptimization, "optimize", lambda self, it=20: optimised.append(it))
    graph, edges, table = LoopClosure.closeLoops(kfs, Detector(), loopInformation=7.0 * np.eye(3), huber=1.5, max_iterations=9)
    assert seen["idx"].tolist() == list(range(n)) and len(calls) == 1 and len(table) == 3 and optimised == [9]
    # the clouds were converted with the rows of the polar image: thetaInd = rInd = k -> r = k res at phi = 2 pi k / 400
    src3 = calls[0][0][0][0]                                         # the first pair tried is query 3 against candidate 2
    assert np.allclose(src3[0], 3 * 0.0432 * np.array([np.cos(2 * np.pi * 3 / 400), np.sin(2 * np.pi * 3 / 400)]), atol=1e-12)
    assert [(e[0], e[1]) for e in edges] == [(1, 5)]
    poses, fixed, ij, meas, info, huber = graph.graph()
    assert np.array_equal(poses, np.array([k.pose for k in kfs])) and fixed.tolist() == [True] + [False] * (n - 1)
    assert ij.tolist() == [[k, k + 1] for k in range(n - 1)] + [[1, 5]]
    assert np.allclose(meas[-1], edges[0][2]) and np.array_equal(info[-1], 7.0 * np.eye(3)) and np.array_equal(info[0], np.eye(3))
    assert huber.tolist() == [0.0] * (n - 1) + [1.5]
    assert np.allclose(meas[:-1], PoseGraphLib.odometryEdges(poses))
    # no accepted edge: the graph comes back un-optimised
    align2, _ = _exact_aligner(true, fraction_ok=lambda qi, cj: False, key=by_range)
    monkeypatch.setattr(LoopClosure, "_align_batch", align2)
    graph, edges, _ = LoopClosure.closeLoops(kfs, Detector())
    assert edges == [] and optimised == [9] and len(graph.graph()[2]) == n - 1
    with pytest.raises(ValueError):
        LoopClosure.closeLoops(kfs[:-1], Detector())
