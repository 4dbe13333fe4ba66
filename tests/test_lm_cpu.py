"""CPU: the LM model (tests/lm_model.py) against the oracle, and the committed case list (tests/lm_cases.py) against its own rules.

What stands behind tests/test_gpu_lm.py: the device is held to the model's nfev and info on the counts tier, so the model must be
the oracle's lmdif (same nfev, same info, x within the model's own spread), every committed case must still pass its admission, and
the list must reach the branches the pose bars are blind to - three or more lmpar iterations, five or more rejected trials,
info == 2 - at every size at which the device changes its code path.  The seven whole-solve mutants of lm_model.SOLVE_MUTANTS each
change (nfev, info) of a counts-tier case, so a like slip in either device copy fails the GPU test.

Of the three lmpar-only mutants, two change lmpar's (par, x) on isolated inputs (lm_cases.lmpar_inputs): the paru update inside the
loop (reached with a zero pivot: parl = 0 lets the iteration come from the right) and the clamp of the incoming par to paru.  No input
was found for the third, `parl_not_updated` (40 000 random matrices, scalings, qtb, delta and par besides the 720 committed ones), and
none should exist short of rounding: phi(par) = |D x(par)| - delta is convex and decreasing, so Newton's step from the left of the root
(fp > 0, the only place parl is raised) stays left of it and moves right; par + parc then exceeds the raised parl anyway.  The bound
only catches a step from the right (fp < 0) that jumps over the root, and after such a jump every later step is from the left again."""
import numpy as np
import pytest

import lm_cases as cases
import lm_model as model
import oracle


def _oracle(case):
    T0, p_w, p_jt, Ti, sg = cases.make(*case)
    s = oracle.MotionDistortionSolver(np.diag(sg[:2]), np.diag(sg[2:]))
    s.update_problem(T0, p_w, p_jt, Ti)
    out, x0, r0 = s._solve(want_r0=True)
    return out, s.nfev, s.info, x0, r0


@pytest.mark.parametrize("tier", ["counts", "info"])
def test_committed_cases_pass_their_admission(tier):
    for c in cases.COUNTS if tier == "counts" else cases.INFO:
        assert cases.admit(c) == tier, (c, cases.reference(c).counts, sorted({r.counts for r in cases.perturbed(c)}))


def test_model_is_the_oracles_lmdif():
    """nfev and info equal on every admitted case; the start vector and first residual to rounding; x within measure_spread(), and
    within three times the case's own spread between the plain and the perturbed model (the largest of 16 samples understates a
    range; measured: the oracle comes to 0.7 of it at most.  The oracle differs from the plain model by libm against NumPy's cos /
    sin / log and by MINPACK's scaled norm, both inside what the perturbation covers) - on the info tier nfev is free and the cost is
    compared"""
    for c in cases.COUNTS + cases.INFO:
        ref = cases.reference(c)
        x, nfev, info, x0, r0 = _oracle(c)
        assert np.abs(ref.x0 - x0).max() <= 1e-12 * max(1.0, np.abs(x0).max()), c
        assert np.abs(ref.r0 - r0).max() <= 1e-9 * max(1.0, np.abs(r0).max()), c
        assert info == ref.info, (c, info, ref.info)
        if c in cases.COUNTS:
            assert nfev == ref.nfev, (c, nfev, ref.nfev)
            dv, dp, da = cases.difference(ref.x, x)
            own, top = cases.case_spread(c), cases.measure_spread()
            for q, d in enumerate((dv, dp, da)):
                assert d <= min(top[q], max(3 * own[q], 1e-12)), (c, q, d, own[q], top[q])
        else:
            assert np.isfinite(x).all() and nfev <= model.MAXFEV
            assert ref.prob.cost(x) <= cases.cost_bound(c), (c, ref.prob.cost(x), ref.cost)


def test_list_reaches_what_the_pose_bars_miss():
    assert len(cases.COUNTS) >= 60 and len(set(cases.COUNTS)) == len(cases.COUNTS) and not set(cases.COUNTS) & set(cases.INFO)
    for N in cases.SIZES:
        assert sum(1 for c in cases.COUNTS if c[1] == N) >= 2, N
    refs = [cases.reference(c) for c in cases.COUNTS]
    assert sum(1 for r in refs if r.lmpar_max >= 3) >= 10
    assert sum(1 for r in refs if r.rejected >= 5) >= 10
    assert sum(1 for c in cases.INFO if cases.reference(c).info == 2) >= 6
    # the log is what it says: one entry per trial, nfev = 1 + 6 Jacobians + trials
    for r in refs:
        assert (r.nfev - 1 - len(r.log)) % 6 == 0 and r.info in (1, 2, 3, 4)
    # every class of the issue is on one of the two lists
    assert {c[0] for c in cases.COUNTS + cases.INFO} == set(cases.CLASSES)


def test_recorded_spread_is_the_measured_one():
    got = cases.measure_spread()
    print("measure_spread():", got, "recorded:", cases.SPREAD)
    for q in range(4):
        assert cases.SPREAD[q] / 2 <= got[q] <= cases.SPREAD[q] * 2, (q, got[q], cases.SPREAD[q])
    for c in cases.COUNTS:
        own = cases.case_spread(c)
        for q, g in enumerate("vp"):
            if g in cases.WIDE.get(c, ""):
                assert own[q] > cases.BARS[q] / 10 / 2, (c, g, own[q])          # left out of the device's bar: really wide
            else:
                assert own[q] <= cases.BARS[q] / 10 * 2, (c, g, own[q])
    assert set(cases.WIDE) <= set(cases.COUNTS) and all(set(g) <= set("vp") for g in cases.WIDE.values())
    assert 10 * cases.SPREAD[2] <= cases.BARS[2]                               # the angle needs no such list


@pytest.mark.parametrize("mutant", model.SOLVE_MUTANTS)
def test_whole_solve_mutant_changes_counts(mutant):
    hit = []
    for c in cases.COUNTS:
        T0, p_w, p_jt, Ti, sg = cases.make(*c)
        if model.solve(T0, p_w, p_jt, Ti, sg, mutant=mutant).counts != cases.reference(c).counts:
            hit.append(c)
            break
    assert hit, mutant


def test_lmpar_inputs_and_their_mutants():
    keep, spread = cases.lmpar_reference()
    assert len(keep) >= 200
    d1 = [1.0] * 6
    its = [k[6][3] for k in keep]
    assert its.count(0) >= 20 and max(its) >= 6 and sum(1 for k in keep if k[1][5, 5] == 0) >= 20
    for nm, R, ipvt, qtb, delta, par_in, ref, own in keep:
        v = np.concatenate([np.triu(R).ravel(), qtb, [delta, par_in]])
        v = np.abs(v[v != 0])
        assert v.min() >= 1e-150 and v.max() <= 1e150, nm
        _contract(ref, delta, nm, bool((np.diag(R) == 0).any()))
    hits = {m: sum(1 for k in keep if _changed(model.lmpar(k[1], k[2], d1, k[3], k[4], k[5], mutant=m), k[6])) for m in model.LMPAR_MUTANTS}
    assert hits["paru_not_updated"] >= 1 and hits["par_init_no_clamp_hi"] >= 1, hits
    assert hits["parl_not_updated"] == 0, "an input reaches the parl update: name it in the docstring and hold the device to it"


def _changed(a, b):
    return a[0] != b[0] or list(a[1]) != list(b[1])


def _contract(res, delta, nm, singular):
    """MINPACK's contract on exit: par = 0 with |D x| - delta <= 0.1 delta, or | |D x| - delta | <= 0.1 delta, or the tenth iteration
    (which no committed input reaches) - or, only with a zero pivot, the exit `parl == 0 and fp <= fp_previous < 0`"""
    par, x, sdiag, it, dxnorm = res
    fp = dxnorm - delta
    if par == 0:
        assert it == 0 and fp <= 0.1 * delta, nm
    else:
        assert 1 <= it < 10 and (abs(fp) <= 0.1 * delta or (singular and fp < 0)), (nm, fp, delta, it)
