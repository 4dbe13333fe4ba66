"""CPU (-m "not gpu") half of the back-end edge tests (the inputs, the references and the comparisons are in backend_edge_cases.py;
the GPU half is test_gpu_backend_edges.py):

  * the oracle against the reference's answers in tests/golden/backend_edges.npz (make_backend_edges.py) on the SSC and Kabsch
    cases the reference can run, so that the oracle can carry the cases it cannot;
  * the tolerances of the GPU test are MEASURED here: the deviation of two CPU float64 orders from an exact reference, in
    condition units, and the records in backend_edge_cases.py (KABSCH_CPU_WORST, UNDISTORT_CPU_WORST) must bracket them;
  * every comparison the GPU test makes is handed a wrong result of the kind it is there to catch, and must refuse it."""
import collections
import math

import numpy as np
import pytest

import oracle
import backend_edge_cases as bc


@pytest.fixture(scope="module")
def edges(golden):
    return golden("backend_edges")


# ------------------------------------------------------------------ SSC
def test_ssc_case_set_is_the_covering_set():
    cases = bc.ssc_cases()
    assert len(cases) >= 150
    seen = collections.Counter()
    cross = collections.Counter()
    for name, kp, num_ret, tol, cols, rows in cases:
        assert kp.shape[1] == 3 and (kp[:, :2] >= 0).all() and (kp[:, 0] <= rows).all() and (kp[:, 1] <= cols).all(), name
        seen["size", rows, cols] += 1; seen["num_ret", num_ret] += 1; seen["tol", tol] += 1; seen["dist", name.split("-")[-1]] += 1
        for i, b in enumerate(bc.ssc_b_values(num_ret)):
            seen["B", i] += b == len(kp)
        widths, sel, how = bc.ssc_trace(kp, num_ret, tol, cols, rows)
        # a third statement of the algorithm (covered cells as a set) beside the oracle's pairwise form
        assert bc.compare_ssc(sel, bc.oracle_ssc_indices(kp, num_ret, tol, cols, rows)), name
        for which in ("stage", "batch"):
            cross[which] += bc.ssc_crosses(widths, cols, rows, which)
        cross[how] += 1
        if bc.ssc_reference_pinned((name, kp, num_ret, tol, cols, rows)):
            assert min(widths) >= 1 and max(bc.ssc_cells(w, cols, rows) for w in widths) < 5e6, name
    for key in ([("size",) + s for s in bc.SSC_SIZES] + [("num_ret", k) for k in bc.SSC_NUM_RET] + [("tol", t) for t in bc.SSC_TOL]
                + [("dist", d) for d in bc.SSC_DISTS] + [("B", i) for i in range(14)]):
        assert seen[key] >= 2, key
    assert cross["stage"] >= 10 and cross["batch"] >= 10, cross       # one call on both sides of the grid / pairwise switch
    assert cross["found"] >= 20 and cross["empty-range"] >= 20 and cross["zero-width"] >= 1, cross


def test_ssc_oracle_equals_the_reference_off_the_golden_point(edges):
    pinned = [c for c in bc.ssc_cases() if bc.ssc_reference_pinned(c)]
    assert len(pinned) >= 60 and [c[0] for c in pinned] == edges["ssc_names"].tolist()
    off, sel = edges["ssc_off"], edges["ssc_sel"]
    for i, (name, kp, num_ret, tol, cols, rows) in enumerate(pinned):
        assert bytes.fromhex(bc.sha(kp)) == edges["ssc_sha"][i].tobytes(), name
        assert bc.compare_ssc(bc.oracle_ssc_indices(kp, num_ret, tol, cols, rows), sel[off[i]:off[i + 1]]), name


# ------------------------------------------------------------------ Kabsch
def test_kabsch_oracle_forms_equal_the_reference(edges):
    cases = [c for c in bc.kabsch_cases()[0] if len(c[1]) <= 4097]
    assert [c[0] for c in cases] == edges["kabsch_names"].tolist()
    for i, case in enumerate(cases):
        name, s, t = case
        assert bytes.fromhex(bc.sha(s, t)) == edges["kabsch_sha"][i].tobytes(), name
        Rw, hw = edges["kabsch_R"][i], edges["kabsch_h"][i]
        for form in (oracle.calculateTransformSVD, oracle.kabsch_closed_form):
            R, h = form(s, t)
            dth = abs(bc.wrap_angle(math.atan2(R[1, 0], R[0, 0]) - math.atan2(Rw[1, 0], Rw[0, 0])))
            dh = np.abs(h - hw).max()
            if s.dtype == np.float32:           # the reference ran these two in float32: its own rounding, 2^-24 of the coordinates
                assert dth <= 1e-5 and dh <= 2.0 ** -24 * 64 * max(np.abs(s).max(), np.abs(t).max()), (name, dth, dh)
            else:                               # two float64 evaluations, each within the CPU orders' worst deviation from the exact fit
                ua, uh = bc.kabsch_units(bc.kabsch_exact_of(case)[2])
                assert dth <= 2 * bc.KABSCH_CPU_WORST[0] * ua and dh <= 2 * bc.KABSCH_CPU_WORST[1] * uh, (name, dth / ua, dh / uh)


def test_kabsch_tolerance_is_measured_and_sees_a_lost_lane():
    cases, degenerate = bc.kabsch_cases()
    assert {len(c[1]) for c in cases} | {1} == set(bc.KABSCH_N) and any(len(c[1]) == 1 for c in degenerate)
    worst_a = worst_h = 0.0
    for case in cases:
        name, s, t = case
        ex = bc.kabsch_exact_of(case)
        for form in (oracle.kabsch_closed_form, bc.kabsch_sequential):
            da, dh = bc.kabsch_deviation(*form(s, t), ex)
            worst_a, worst_h = max(worst_a, da), max(worst_h, dh)
    print(f"Kabsch, two CPU float64 orders against the exact fit: angle {worst_a:.3g}, h {worst_h:.3g} condition units")
    assert bc.KABSCH_CPU_WORST[0] / 2 <= worst_a <= 1.25 * bc.KABSCH_CPU_WORST[0], worst_a
    assert bc.KABSCH_CPU_WORST[1] / 2 <= worst_h <= 1.25 * bc.KABSCH_CPU_WORST[1], worst_h
    # the condition that makes the bar see a lost lane: on every noisy case the absolute tolerance is at most a tenth of what
    # removing the last correspondence changes
    noisy = [c for c in cases if "noise1.5" in c[0]]
    assert len(noisy) >= 10
    for case in noisy:
        name, s, t = case
        th, h, cond = bc.kabsch_exact_of(case)
        ua, uh = bc.kabsch_units(cond)
        th1, h1, _ = bc.kabsch_exact(s[:-1], t[:-1])
        assert 10 * bc.KABSCH_K[0] * ua <= abs(bc.wrap_angle(th1 - th)), name
        assert 10 * bc.KABSCH_K[1] * uh <= np.abs(h1 - h).max(), name


# ------------------------------------------------------------------ undistort
def test_undistort_tolerance_is_measured():
    cases = bc.undistort_cases()
    assert {len(c[2]) for c in cases} >= set(bc.UNDISTORT_N)
    assert {c[1][2] for c in cases} == set(bc.UNDISTORT_OMEGA) and {c[3] for c in cases} == set(bc.UNDISTORT_PERIOD)
    worst_xy = worst_dT = 0.0
    for case in cases:
        name, v3, pts, period = case
        ref = bc.undistort_reference(case)
        M = oracle.MotionDistortionSolver
        fx, fd = bc.undistort_deviation(M.undistort(v3, pts, period), M.compute_time_deltas(period, pts), ref)
        worst_xy, worst_dT = max(worst_xy, fx), max(worst_dT, fd)
    print(f"undistort, the oracle's libm evaluation against mpmath at 50 digits: xy {worst_xy:.3g}, dT {worst_dT:.3g} tolerance units")
    assert bc.UNDISTORT_CPU_WORST[0] / 2 <= worst_xy <= 1.25 * bc.UNDISTORT_CPU_WORST[0], worst_xy
    assert bc.UNDISTORT_CPU_WORST[1] / 2 <= worst_dT <= 1.25 * bc.UNDISTORT_CPU_WORST[1], worst_dT


def test_undistort_reference_follows_the_signed_zeros():
    case = next(c for c in bc.undistort_cases() if c[0].startswith("undistort-axes-omega0-"))
    _, dT, _, _ = bc.undistort_reference(case)
    pts, period = case[2], case[3]
    got = {(float(x), math.copysign(1.0, y)): d for (x, y), d in zip(pts.tolist(), dT.tolist()) if y == 0 and x == 1.0}
    assert got[(1.0, 1.0)] == -period / 2 and got[(1.0, -1.0)] == period / 2            # atan2(-0, -1) = -pi, atan2(+0, -1) = +pi
    origin = {(math.copysign(1.0, x), math.copysign(1.0, y)): d for (x, y), d in zip(pts.tolist(), dT.tolist()) if x == 0 and y == 0}
    assert origin == {(1.0, 1.0): -period / 2, (-1.0, 1.0): -0.0, (1.0, -1.0): period / 2, (-1.0, -1.0): 0.0}


# ------------------------------------------------------------------ consistency graph
def test_graph_oracle_equals_live_scipy_and_holds_the_equality_pairs():
    cases, equality = bc.graph_cases()
    assert {len(c[1]) for c in cases} == set(bc.GRAPH_K) and len(equality) >= 4
    for name, p, n, thr in cases:
        adj = oracle.consistency_graph(p, n, thr)
        assert bc.compare_graph(adj, bc.pack_adjacency(bc.graph_scipy(p, n, thr)), equality.get(name)), name
        K = len(p)
        dense = oracle.adjacency_dense(adj, K)
        if "thr0-" in name or "thr1e9" in name:
            assert dense.sum() == K * (K - 1), name
        if "thr-1-" in name:
            assert dense.sum() == 0, name
        if "nan" in name:
            assert dense[K // 2].sum() == 0 and dense[:, K // 2].sum() == 0 and dense.sum() > 0, name


# ------------------------------------------------------------------ the comparisons can fail
def test_every_comparison_refuses_the_mistake_it_is_there_for():
    # Kabsch of all but one point, on every noisy case
    for case in bc.kabsch_cases()[0]:
        name, s, t = case
        ex = bc.kabsch_exact_of(case)
        assert bc.compare_kabsch(*oracle.kabsch_closed_form(s, t), ex, *bc.KABSCH_K), name
        if "noise1.5" in name:
            assert not bc.compare_kabsch(*oracle.kabsch_closed_form(s[:-1], t[:-1]), ex, *bc.KABSCH_K), name
    # SSC with rows and cols exchanged at the entry, on the non-square cases.  The two enter the search only through its upper bound
    # (exp2 is symmetric in them but for its 4 * cols term), so the exchange moves the first width by a pixel or two and most
    # searches still end on the same selection: the comparison must refuse the ones where they do not (7 of 97 when written)
    refused = tried = 0
    for name, kp, num_ret, tol, cols, rows in bc.ssc_cases():
        if rows != cols:
            tried += 1
            refused += not bc.compare_ssc(bc.oracle_ssc_indices(kp, num_ret, tol, rows, cols), bc.oracle_ssc_indices(kp, num_ret, tol, cols, rows))
    assert tried >= 60 and refused >= 5, (tried, refused)
    # ... and exchanged in the (r, q) cell index of the clamped grid, the form the kernel's bitmap has.  The right index gives the
    # oracle's selection on every case; with the grid's two sizes exchanged in it, cells of a non-square image alias
    wrong = tried = 0
    for name, kp, num_ret, tol, cols, rows in bc.ssc_cases():
        want = bc.oracle_ssc_indices(kp, num_ret, tol, cols, rows)
        assert bc.compare_ssc(bc.ssc_trace(kp, num_ret, tol, cols, rows, grid="device")[1], want), name
        if rows != cols and len(kp) >= 63 and "identical" not in name:
            tried += 1
            wrong += not bc.compare_ssc(bc.ssc_trace(kp, num_ret, tol, cols, rows, grid="exchanged")[1], want)
    print(f"SSC, grid sizes exchanged in the cell index: refused on {wrong} of {tried} non-square cases of 63 keypoints or more")
    assert tried >= 40 and wrong >= tried // 2, (tried, wrong)
    # a graph built with "<"
    from scipy.spatial.distance import cdist
    cases, equality = bc.graph_cases()
    for name, pairs in equality.items():
        _, p, n, thr = next(c for c in cases if c[0] == name)
        strict = np.abs(cdist(p, p) - cdist(n, n)) < thr
        np.fill_diagonal(strict, False)
        assert not bc.compare_graph(bc.pack_adjacency(strict), oracle.consistency_graph(p, n, thr), pairs), name
    # a set high bit in the last word
    name, p, n, thr = next(c for c in cases if c[0] == "graph-random-K65")
    adj = oracle.consistency_graph(p, n, thr)
    dirty = adj.copy()
    dirty[3, 1] |= np.uint64(1) << np.uint64(63)
    assert not bc.compare_graph(dirty, adj)
    # dT from atan2(y, x)
    for case in bc.undistort_cases():
        name, v3, pts, period = case
        ref = bc.undistort_reference(case)
        M = oracle.MotionDistortionSolver
        xy = M.undistort(v3, pts, period)
        assert bc.compare_undistort(xy, M.compute_time_deltas(period, pts), ref, *bc.UNDISTORT_K), name
        assert not bc.compare_undistort(xy, period * np.arctan2(pts[:, 1], pts[:, 0]) / (2 * np.pi), ref, *bc.UNDISTORT_K), name
