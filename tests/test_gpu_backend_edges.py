"""GPU (-m gpu): the small back-end kernels away from the golden shapes - ssc_kernel, ssc_batch_kernel (through
roam_debug_ssc_batch), kabsch_kernel, mds_undistort_kernel and consistency_graph_kernel on the inputs of backend_edge_cases.py.

Bars.  SSC selections, adjacency words and clique masks: exact.  Kabsch and undistort: measured, not chosen -

  Kabsch     the result is compared with the fit in exact rational arithmetic (backend_edge_cases.kabsch_exact), the deviation
             expressed in condition units: angle |dtheta| / (u S / |z|), h |dh| / (unit(theta) |mt| + u max|coord|), u = 2^-53.
             Two CPU float64 orders (numpy's sums in oracle.kabsch_closed_form, a plain left-to-right loop) deviate by at most
             2.46 (angle) and 68.3 (h) units over all cases (tests/test_backend_edges_cpu.py measures it; the h figure is the
             left-to-right mean of 100 000 coordinates).  The device sums in a third order, so its bar is ten times that: 24.6 and
             683 units - on the largest case (N = 100 000, centroid 1e6 px) 1.1e-14 rad and 5.0e-7 px; on the golden-sized noisy
             N = 256 case 4.6e-15 rad and 1.0e-10 px, where losing one correspondence moves the fit by 1.8e-6 rad and 1.2e-3 px.
  undistort  against mpmath at 50 digits, in units of u period / 2 (dT) and u (|p| (1 + |a|) + |v| |dT|) (xy), a = v3[2] dT.  The
             oracle's libm evaluation deviates by at most 3.14 (xy) and 1.57 (dT) units; the bar is ten times that.

Every test prints the worst figure the device showed before it asserts."""
import math

import numpy as np
import pytest

import oracle
import backend_edge_cases as bc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from radarslampy_amd import _ffi
    c = _ffi.Context(0)
    assert "gfx950" in c.device_info()["arch"]
    yield c
    c.close()


@pytest.fixture(scope="module")
def ssc_want():
    """the oracle's selection of every SSC case, computed once"""
    return {c[0]: bc.oracle_ssc_indices(*c[1:]) for c in bc.ssc_cases()}


@pytest.fixture(scope="module")
def ssc_stage(ctx):
    """the stage kernel's selection of every SSC case, computed once"""
    return {name: ctx.ssc(kp, num_ret, tol, cols, rows).copy() for name, kp, num_ret, tol, cols, rows in bc.ssc_cases()}


# ------------------------------------------------------------------ SSC
def test_ssc_stage_kernel_equals_the_oracle_on_every_case(ssc_stage, ssc_want):
    bad = [name for name in ssc_want if not bc.compare_ssc(ssc_stage[name], ssc_want[name])]
    assert not bad, bad


def test_ssc_dropin_equals_the_stage_call(ctx, ssc_stage):
    from radarslampy_amd import ANMS
    cases = bc.ssc_cases()
    for name, kp, num_ret, tol, cols, rows in (cases[1], cases[len(cases) // 2], cases[-3]):
        assert np.array_equal(ANMS.ssc(kp, num_ret, tol, cols, rows), kp[ssc_stage[name]]), name


def test_ssc_batch_kernel_equals_the_stage_kernel_and_the_oracle(ctx, ssc_stage, ssc_want):
    batches = bc.ssc_batches(bc.ssc_cases())
    assert sum(len(b[1]) for b in batches) == len(ssc_want) and max(len(b[1]) for b in batches) >= 4
    bad = []
    for (num_ret, tol, cols, rows), names, kp, count in batches:
        sel, n_sel = ctx.debug_ssc_batch(kp, count, num_ret, tol, cols, rows)
        for p, name in enumerate(names):
            got = sel[p, :max(n_sel[p], 0)]
            if not (bc.compare_ssc(got, ssc_want[name]) and bc.compare_ssc(got, ssc_stage[name]) and (sel[p, len(got):] == -1).all()):
                bad.append(name)
    assert not bad, bad


def test_ssc_batch_count_clamp_empty_problems_skips_and_position(ctx, ssc_want):
    (num_ret, tol, cols, rows), names, kp, count = max(bc.ssc_batches(bc.ssc_cases()), key=lambda b: len(b[1]))
    P, cap, _ = kp.shape
    base_sel, base_n = ctx.debug_ssc_batch(kp, count, num_ret, tol, cols, rows)
    # a count above kp_cap is clamped to it: the same selection as count = kp_cap
    big = count.copy(); big[0] = cap + 1000
    capped = count.copy(); capped[0] = cap
    s1, n1 = ctx.debug_ssc_batch(kp, big, num_ret, tol, cols, rows)
    s2, n2 = ctx.debug_ssc_batch(kp, capped, num_ret, tol, cols, rows)
    assert np.array_equal(s1, s2) and np.array_equal(n1, n2)
    assert bc.compare_ssc(s1[0, :n1[0]], bc.oracle_ssc_indices(kp[0], num_ret, tol, cols, rows))
    # count = 0 (and below) gives 0 and leaves the selection alone
    zero = count.copy(); zero[1] = 0; zero[2] = -3
    s, n = ctx.debug_ssc_batch(kp, zero, num_ret, tol, cols, rows)
    assert n[1] == 0 and n[2] == 0 and (s[1] == -1).all() and (s[2] == -1).all()
    assert np.array_equal(s[0], base_sel[0]) and np.array_equal(s[3:], base_sel[3:]) and np.array_equal(n[3:], base_n[3:])
    # problems at or beyond n_active - first keep the sentinel, the others are unchanged
    for n_active, first in ((2, 0), (P, 1), (3, 2), (0, 0), (1, 5)):
        s, n = ctx.debug_ssc_batch(kp, count, num_ret, tol, cols, rows, n_active=n_active, first=first)
        live = max(0, min(P, n_active - first))
        assert (n[live:] == -1).all() and (s[live:] == -1).all(), (n_active, first)
        assert np.array_equal(n[:live], base_n[:live]) and np.array_equal(s[:live], base_sel[:live]), (n_active, first)
    # a problem's result depends neither on its neighbours nor on its position
    perm = np.roll(np.arange(P), 1)[::-1].copy()
    s, n = ctx.debug_ssc_batch(kp[perm], count[perm], num_ret, tol, cols, rows)
    assert np.array_equal(n, base_n[perm]) and np.array_equal(s, base_sel[perm])
    for p in range(P):
        s, n = ctx.debug_ssc_batch(kp[p:p + 1], count[p:p + 1], num_ret, tol, cols, rows)
        assert n[0] == base_n[p] and np.array_equal(s[0], base_sel[p]) and bc.compare_ssc(s[0, :n[0]], ssc_want[names[p]]), names[p]


# ------------------------------------------------------------------ Kabsch
def test_kabsch_within_the_measured_tolerance_of_the_exact_fit(ctx):
    worst = [0.0, 0.0, "", ""]
    bad = []
    for case in bc.kabsch_cases()[0]:
        name, s, t = case
        R, h = ctx.kabsch2d(s, t)
        R2, h2 = ctx.kabsch2d(s, t)
        assert np.array_equal(R, R2) and np.array_equal(h, h2), name              # the same result twice
        ex = bc.kabsch_exact_of(case)
        da, dh = bc.kabsch_deviation(R, h, ex)
        if da > worst[0]:
            worst[0], worst[2] = da, name
        if dh > worst[1]:
            worst[1], worst[3] = dh, name
        if not bc.compare_kabsch(R, h, ex, *bc.KABSCH_K):
            bad.append((name, da, dh, abs(np.linalg.det(R) - 1)))
    print(f"Kabsch on the device against the exact fit: angle {worst[0]:.3g} units ({worst[2]}), h {worst[1]:.3g} units ({worst[3]}); "
          f"bars {bc.KABSCH_K[0]:.3g} / {bc.KABSCH_K[1]:.3g}")
    assert not bad, bad


def test_kabsch_degenerate_sets_give_a_proper_rotation(ctx):
    for name, s, t in bc.kabsch_cases()[1]:
        R, h = ctx.kabsch2d(s, t)
        assert np.isfinite(R).all() and np.isfinite(h).all(), name
        assert np.abs(R @ R.T - np.eye(2)).max() <= 1e-12 and abs(np.linalg.det(R) - 1) <= 1e-12, (name, R)
        ms, mt = s.mean(axis=0), t.mean(axis=0)
        assert np.abs(h.reshape(2) - (ms - R @ mt)).max() <= 1e-9, (name, h)
        if len(s) == 1:
            assert np.array_equal(R, np.eye(2)), R
        R2, h2 = ctx.kabsch2d(s, t)
        assert np.array_equal(R, R2) and np.array_equal(h, h2), name


# ------------------------------------------------------------------ undistort
def test_undistort_within_the_scaled_tolerance_of_mpmath(ctx):
    worst = [0.0, 0.0, "", ""]
    bad = []
    for case in bc.undistort_cases():
        name, v3, pts, period = case
        xy, dT = ctx.mds_undistort(v3, pts, period)
        fx, fd = bc.undistort_deviation(xy, dT, bc.undistort_reference(case))
        if fx > worst[0]:
            worst[0], worst[2] = fx, name
        if fd > worst[1]:
            worst[1], worst[3] = fd, name
        if not bc.compare_undistort(xy, dT, bc.undistort_reference(case), *bc.UNDISTORT_K):
            bad.append((name, fx, fd))
    print(f"undistort on the device against mpmath: xy {worst[0]:.3g} units ({worst[2]}), dT {worst[1]:.3g} units ({worst[3]}); "
          f"bars {bc.UNDISTORT_K[0]:.3g} / {bc.UNDISTORT_K[1]:.3g}")
    assert not bad, bad


def test_undistort_dropin_equals_the_stage_call(ctx):
    from radarslampy_amd.motionDistortion import MotionDistortionSolver as M
    cases = bc.undistort_cases()
    for name, v3, pts, period in (cases[2], cases[7], cases[-4]):
        xy, dT = ctx.mds_undistort(v3, pts, period)
        assert np.array_equal(M.compute_time_deltas(period, pts), dT), name
        out = M.undistort(v3, pts, period)
        assert out.shape == (len(pts), 3) and np.array_equal(out[:, :2], xy) and (out[:, 2] == 1).all(), name


# ------------------------------------------------------------------ consistency graph
def test_graph_equals_the_oracle_word_for_word_and_holds_equality(ctx):
    cases, equality = bc.graph_cases()
    for name, p, n, thr in cases:
        K = len(p)
        mask, n_in, flags, adj = ctx.reject_outliers(p, n, thr, want_adj=True)
        want = oracle.consistency_graph(p, n, thr)
        assert bc.compare_graph(adj, want, equality.get(name)), name
        dense = oracle.adjacency_dense(want, K)
        complete, empty = dense.sum() == K * (K - 1), dense.sum() == 0
        if "thr0-" in name or "thr1e9" in name:
            assert complete, name
        if "thr-1-" in name:
            assert empty, name
        if K <= 513 or empty:                   # (an empty graph's walk is one vertex at any size)
            size, omask, _ = oracle.max_clique_nx(want)
            assert flags & 1 and n_in == size == mask.sum() and np.array_equal(mask, omask), name
        if empty:
            assert flags & 1 and n_in == 1 and mask.sum() == 1, name              # max_clique_nx's single vertex
        if K == 1:
            assert n_in == 1 and mask.all()
        if complete:
            assert flags & 1 and mask.all() and n_in == K, name
