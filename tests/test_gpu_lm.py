"""GPU (-m gpu): the motion-distortion LM solver where the pose bars are blind - nfev, info, lmpar on its own, the batched launch.

mds_lm_wave_kernel<1..4> (csrc/lm_wave.inc) and mds_lm_kernel (csrc/kabsch_mds.hip) against the float64 model tests/lm_model.py on
the cases of tests/lm_cases.py (tests/test_lm_cpu.py holds the model to the oracle and the case list to its rules):
  counts tier   nfev and info equal the model's; x within ten times the spread the model shows against itself with every cos / sin /
                log / atan2 moved by +-4 ulp and the row sums reordered (lm_cases.SPREAD), or within the bars the suite already had
                (1e-3, 1e-4 m, 1e-5 rad) where those are smaller - then on every case whose own spread is at most a tenth of the bar
                (all but the 7 of lm_cases.WIDE)
  info tier     info equal, outputs finite, nfev <= 4200, the model's cost at the device's x at most lm_cases.cost_bound()
  batch         roam_debug_mds_solve_batch: 64 problems of both kernel forms in one launch as the engine makes it - count per
                problem, count clamped to nmax, counts 0 and 1, the list of large problems and its two alternating slots - each
                problem bit for bit what it gives alone, three consecutive solves bit for bit alike, the list's slots read back
  lmpar alone   roam_debug_lm_lmpar, both copies: the same par == 0 exits as the model, MINPACK's exit contract, par / x / sdiag
                within ten times what one ulp on every sqrt and quotient moves them in the model (per input, lm_cases.lmpar_reference)

Measured (model against itself): SPREAD = velocity 1.54e-4, position 3.41e-5 m, angle 6.91e-7 rad; cost 5.7e5 relative (the
degenerate classes end at costs of 1e-28 ... 1e-20); lmpar under +-1 ulp: par 3.7e-9, x 2.1e-9, sdiag 8.8e-13 at the worst input.
Measured (MI355X against the model): counts tier - all 73 (nfev, info) equal, worst asserted differences velocity 2.83e-5, position
4.35e-6 m, angle 2.19e-7 rad; info tier - info equal, nfev 102 ... 190 against the model's 116 ... 169, costs 2.5e-28 ... 4.0e-18
against bounds of 5.4e-22 ... 9.0e-14, the two tight priors at the model's nfev and cost; batch - every comparison bit for bit, the list's last slot holds the 11 large problems once each and the other is 0
after 1 ... 4 solves;
lmpar alone - all 1 440 results (720 inputs, two forms) bit-equal to the model."""
import numpy as np
import pytest

import lm_cases as cases
import lm_model as model

pytestmark = pytest.mark.gpu
NSTRIDE = 320


@pytest.fixture(scope="module")
def ctx():
    from radarslampy_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


def _check_counts(case, x, nfev, info, tag=""):
    """-> list of what fails; prints every figure first"""
    ref = cases.reference(case)
    d = cases.difference(ref.x, x)
    b = cases.x_bounds(case)
    print(f"{tag}{cases.name(case)}: nfev {nfev} (model {ref.nfev})  info {info} (model {ref.info})  "
          + "  ".join(f"{g} {d[q]:.3g} (<= {b[q] if b[q] is not None else 'own spread too wide'})" for q, g in enumerate(("vel", "pos", "ang"))))
    bad = []
    if (nfev, info) != ref.counts:
        bad.append((cases.name(case), "counts", (nfev, info), ref.counts))
    for q in range(3):
        if b[q] is not None and not d[q] <= b[q]:
            bad.append((cases.name(case), "vpa"[q], d[q], b[q]))
    return bad


def test_counts_tier(ctx):
    bad, worst = [], np.zeros(3)
    for c in cases.COUNTS:
        T0, p_w, p_jt, Ti, sg = cases.make(*c)
        x, nfev, info, _, _ = ctx.mds_solve(T0, p_w, p_jt, Ti, sg)
        bad += _check_counts(c, x, nfev, info)
        b = cases.x_bounds(c)
        worst = np.maximum(worst, [t if b[q] is not None else 0.0 for q, t in enumerate(cases.difference(cases.reference(c).x, x))])
    print("worst asserted differences (vel, pos, ang):", worst)
    assert not bad, bad


def test_info_tier(ctx):
    bad = []
    for c in cases.INFO:
        T0, p_w, p_jt, Ti, sg = cases.make(*c)
        ref = cases.reference(c)
        x, nfev, info, _, _ = ctx.mds_solve(T0, p_w, p_jt, Ti, sg)
        cost = ref.prob.cost(x) if np.isfinite(x).all() else np.inf
        print(f"{cases.name(c)}: nfev {nfev} (model {ref.nfev})  info {info} (model {ref.info})  cost {cost:.3g} (model {ref.cost:.3g}, "
              f"<= {cases.cost_bound(c):.3g})")
        if info != ref.info or not np.isfinite(x).all() or not 7 <= nfev <= model.MAXFEV or not cost <= cases.cost_bound(c):
            bad.append(cases.name(c))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ batch
def _batch():
    """64 problems with one sigma5, nstride 320, in a seeded order: every case of both tiers that keeps the default weights, up to 300
    points (both kernel forms, every slot count of the wave form); eight more problems at the slot boundaries that are on neither list
    (only compared with themselves alone); and two problems with count 0 and 1"""
    pick = [c for c in cases.COUNTS + cases.INFO if c[0] not in ("tight", "loose") and c[1] <= 300]
    pick += [("far1", N, 4242) for N in (62, 63, 64, 126, 127, 190, 191, 253)]
    rng = np.random.default_rng(64)
    pick = [pick[i] for i in rng.permutation(len(pick))]
    assert len(pick) == 62 and sum(1 for c in pick if c[1] >= 255) >= 8
    B = 64
    T0 = np.tile(np.eye(3), (B, 1, 1))
    Ti = T0.copy()
    pw, pj = np.zeros((B, NSTRIDE, 2)), np.zeros((B, NSTRIDE, 2))
    count = np.zeros(B, np.int32)
    slots = [b for b in range(B) if b not in (5, 40)]               # problems 5 and 40: count 0 and 1
    names = [None] * B
    for b, c in zip(slots, pick):
        t0, p_w, p_jt, ti, sg = cases.make(*c)
        assert np.array_equal(sg, model.SIGMA5)
        T0[b], Ti[b], count[b], names[b] = t0, ti, c[1], c
        pw[b, :c[1]], pj[b, :c[1]] = p_w, p_jt
        pw[b, c[1]:], pj[b, c[1]:] = 1e6, -1e6                      # what lies past count must not be read
    count[40] = 1
    pw[40], pj[40] = 3.0, 4.0
    return T0, pw, pj, count, Ti, names


@pytest.fixture(scope="module")
def batch():
    return _batch()


@pytest.mark.parametrize("nmax", [320, 200])
def test_batch_is_every_problem_alone(ctx, batch, nmax):
    T0, pw, pj, count, Ti, names = batch
    B = len(count)
    runs = {big: ctx.debug_mds_solve_batch(T0, pw, pj, count, nmax, Ti, model.SIGMA5, big=big, repeat=3) for big in (False, True)}
    for big, (out, nfev, info) in runs.items():
        # three consecutive solves alike (with the list: slot 0, slot 1, slot 0 again - each reset by the solve before)
        for r in (1, 2):
            assert out[r].tobytes() == out[0].tobytes() and np.array_equal(nfev[r], nfev[0]) and np.array_equal(info[r], info[0]), (big, r)
        for b in (5, 40):
            assert info[0, b] == -1 and nfev[0, b] == 0 and out[0, b].tobytes() == np.zeros(6).tobytes(), (b, out[0, b], nfev[0, b], info[0, b])
        assert (info[0, [b for b in range(B) if names[b]]] >= 1).all() and np.isfinite(out[0]).all()
    # with the list and without it: the same bits
    assert runs[True][0].tobytes() == runs[False][0].tobytes() and np.array_equal(runs[True][1], runs[False][1])
    out, nfev, info = runs[True]
    # every problem alone (B = 1, the same nmax and stride), with the list and without: first, middle and last among them
    n_clamped = 0
    for b in range(B):
        for big in (False, True):
            o1, n1, i1 = ctx.debug_mds_solve_batch(T0[b:b + 1], pw[b:b + 1], pj[b:b + 1], count[b:b + 1], nmax, Ti[b:b + 1], model.SIGMA5, big=big)
            assert o1[0, 0].tobytes() == out[0, b].tobytes() and n1[0, 0] == nfev[0, b] and i1[0, 0] == info[0, b], \
                (b, names[b], big, o1[0, 0], out[0, b], n1[0, 0], nfev[0, b])
        n_clamped += count[b] > nmax
    assert n_clamped >= (8 if nmax == 200 else 0)
    if nmax == 320:
        # the unclamped batch holds the counts-tier bars too
        bad = []
        for b in range(B):
            if names[b] in cases.COUNTS:
                bad += _check_counts(names[b], out[0, b], int(nfev[0, b]), int(info[0, b]), tag=f"batch[{b}] ")
        assert not bad, bad


def test_list_slots_after_consecutive_solves(ctx, batch):
    """the list itself after 1 ... 4 consecutive solves: the slot of the last solve holds every problem of 255 or more points exactly
    once, and the other slot has been reset for the solve to come (equal results alone would notice a missing reset only through a
    problem solved twice at once).  With nmax = 200 every problem is the wave kernel's and both slots stay empty."""
    T0, pw, pj, count, Ti, names = batch
    large = sorted(int(b) for b in np.flatnonzero(count >= 255))
    assert len(large) >= 8
    for repeat in (1, 2, 3, 4):
        out, nfev, info, lists = ctx.debug_mds_solve_batch(T0, pw, pj, count, 320, Ti, model.SIGMA5, big=True, repeat=repeat, want_list=True)
        last = (repeat - 1) & 1
        print(f"repeat {repeat}: slot {last} holds {lists[last, 0]} ids, slot {last ^ 1} {lists[last ^ 1, 0]}")
        assert lists[last, 0] == len(large) and sorted(lists[last, 1:1 + len(large)].tolist()) == large, (repeat, lists[last])
        assert lists[last ^ 1, 0] == 0, (repeat, lists[last ^ 1])
        assert out[-1].tobytes() == out[0].tobytes()
    lists = ctx.debug_mds_solve_batch(T0, pw, pj, count, 200, Ti, model.SIGMA5, big=True, repeat=2, want_list=True)[3]
    assert lists[0, 0] == 0 and lists[1, 0] == 0


def test_clamped_count_solves_the_first_nmax_points(ctx, batch):
    """count above nmax: the problem of the first nmax points, bit for bit"""
    T0, pw, pj, count, Ti, names = batch
    b = next(b for b in range(len(count)) if count[b] >= 255)
    o1, n1, i1 = ctx.debug_mds_solve_batch(T0[b:b + 1], pw[b:b + 1], pj[b:b + 1], count[b:b + 1], 200, Ti[b:b + 1], model.SIGMA5)
    o2, n2, i2 = ctx.debug_mds_solve_batch(T0[b:b + 1], pw[b:b + 1, :200], pj[b:b + 1, :200], np.array([200], np.int32), 200, Ti[b:b + 1],
                                           model.SIGMA5)
    assert o1.tobytes() == o2.tobytes() and n1[0, 0] == n2[0, 0] and i1[0, 0] == i2[0, 0] and i1[0, 0] >= 1


def test_single_problem_at_its_own_bound(ctx):
    """B = 1, nmax = nstride = N, through the count path: the counts-tier check, and the bits of roam_mds_solve (no count, no list)"""
    bad = []
    for c in cases.COUNTS:
        T0, p_w, p_jt, Ti, sg = cases.make(*c)
        N = c[1]
        for big in (False, True):
            out, nfev, info = ctx.debug_mds_solve_batch(T0[None], p_w[None], p_jt[None], np.array([N], np.int32), N, Ti[None], sg, big=big)
            x, nf, inf, _, _ = ctx.mds_solve(T0, p_w, p_jt, Ti, sg)
            assert out[0, 0].tobytes() == x.tobytes() and nfev[0, 0] == nf and info[0, 0] == inf, (c, big)
        bad += _check_counts(c, out[0, 0], int(nfev[0, 0]), int(info[0, 0]), tag="alone ")
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ lmpar alone
def _contract(par, x, delta, singular):
    """MINPACK's exit contract of lmpar, on the device's own numbers: par = 0 with |x| - delta <= 0.1 delta, or | |x| - delta | <= 0.1
    delta; with a zero pivot (parl = 0) also the exit `fp <= fp_previous < 0`, seen from outside as fp < 0.  (The tenth iteration
    cannot be seen from outside: the model reaches at most 7 on these inputs, the CPU test says so, and par is held to the model's.)"""
    fp = model.enorm6([float(t) for t in x]) - delta
    return fp <= 0.1 * delta if par == 0 else (abs(fp) <= 0.1 * delta or (singular and fp < 0))


def test_lmpar_alone(ctx):
    keep, spread = cases.lmpar_reference()
    assert len(keep) >= 200
    bad, worst, equal = [], np.zeros(3), 0
    for nm, R, ipvt, qtb, delta, par_in, ref, own in keep:
        for form in (0, 1):
            par, x, sd = ctx.debug_lm_lmpar(R, ipvt, qtb, delta, par_in, form)
            if form == 1 and not (par[0].tobytes() == par[1].tobytes() and x[0].tobytes() == x[1].tobytes() and sd[0].tobytes() == sd[1].tobytes()):
                bad.append((nm, form, "lanes 0 and 63 differ"))
            d = cases.lmpar_difference((par[0], x[0], sd[0]), ref)
            bound = [max(10 * t, cases.LMPAR_FLOOR) for t in own]
            worst = np.maximum(worst, d)
            equal += d == (0.0, 0.0, 0.0)
            if (par[0] == 0) != (ref[0] == 0):
                bad.append((nm, form, "par == 0 exit", par[0], ref[0]))
            elif not all(np.isfinite(t).all() for t in (par, x, sd)) or not all(d[q] <= bound[q] for q in range(3)):
                bad.append((nm, form, d, bound))
            elif not _contract(par[0], x[0], delta, bool((np.diag(R) == 0).any())):
                bad.append((nm, form, "contract", par[0], delta))
    print(f"lmpar alone: {len(keep)} inputs x 2 forms, {equal} results bit-equal to the model, worst (par, x, sdiag) {worst}, "
          f"model's own spread under +-1 ulp {spread}")
    assert not bad, bad[:10]
