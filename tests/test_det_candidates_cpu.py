"""CPU: the cases of tests/det_candidate_cases.py hold what tests/test_gpu_det_candidates.py relies on, by the oracle alone - the
recorded candidate counts, the cap, the key order, and at least 3 candidates (10 exact ties) per size in every class of the
determinant kernel's special paths that the size can have.  The class table is printed: run with -s."""
import numpy as np
import pytest

import det_candidate_cases as dc

MIN_MEMBERS, MIN_TIES, MIN_PRUNED = 3, 10, 3


def _classes(case):
    pay, rc, val, layers = dc.truth(case)
    clip = case[0]
    return dc.classes(rc, val, layers, 2 * (clip // 2), dc.dark_steps(clip), dc.integral(dc.cartesian(pay)))


@pytest.fixture(scope="module")
def table():
    return {tuple(c[:3]): _classes(c) for c in dc.CASES if not c.overflow}


def test_sizes_are_the_ones_the_geometric_paths_need():
    assert sorted({c.clip for c in dc.CASES if not c.overflow}) == list(dc.CLIPS)
    W = [2 * (c // 2) for c in dc.CLIPS]
    for c in dc.CLIPS:
        assert c >= 32 and (c // 2) % 2 == 0, c                            # what the engine asks of a clip
    assert [w % dc.SD_OUT for w in W] == [8, 2, 0, 2] and [w % dc.SD_T for w in W] == [4, 12, 0, 0]
    assert W[2] // dc.SD_OUT == 8 and W[2] // dc.SD_T == 31                # exactly 8 strips and 31 steps: no partial strip, no partial step
    assert W[3] // dc.SD_T + 1 == 36                                       # steps 32 .. 35: the second word of the dark-step table
    first = dc._edges(dc.dark_steps(560))[1]
    assert ((first[-1] - 1) & ~3) >= 4                                     # the march of 560's last strip (class last_partial_strip) starts at a step >= 4


@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: "%d-%s-%d" % c[:3])
def test_oracle_count_is_the_recorded_one_and_keys_ascend(case):
    clip, family, seed, n_oracle = case[:4]
    pay, rc, val, layers = dc.truth(case)
    assert pay.dtype == np.uint8 and pay.shape == (400, clip)
    assert np.array_equal(pay, dc.payload(family, clip, seed=seed))        # deterministic
    if family in dc.BINARY:
        assert set(np.unique(pay).tolist()) <= {0, 255}
    assert len(rc) == n_oracle, (len(rc), n_oracle)
    if case.overflow:
        assert n_oracle > dc.CAP
    else:
        assert 0 < n_oracle <= dc.CAP
    assert (np.diff(rc.astype(np.int64)) > 0).all()                        # C (row, column, layer) order = strictly ascending keys
    r, c, l = dc.unpack(rc)
    assert np.isin(l, (1, 2)).all() and (val > dc.THRESHOLD).all()
    assert np.array_equal(val, np.where(l == 1, layers[1][r, c], layers[2][r, c]))


@pytest.mark.parametrize("clip", dc.CLIPS)
def test_every_class_the_size_can_have_is_populated(clip, table):
    cases = dc.cases_of(clip)
    names = list(table[tuple(cases[0][:3])])
    total = {k: sum(table[tuple(c[:3])][k] for c in cases) for k in names}
    ties = sum(table[tuple(c[:3])]["ties"] for c in cases if c[1] in dc.BINARY)
    can = dc.possible(clip)
    print("\nclip %d (W %d): candidates per class; * = a class this size can have" % (clip, 2 * (clip // 2)))
    print("%-12s %5s " % ("family", "n") + " ".join("%9.9s" % k for k in names))
    for c in cases:
        print("%-12s %5d " % (c[1], c[3]) + " ".join("%9d" % table[tuple(c[:3])][k] for k in names))
    print("%-12s %5d " % ("together", sum(c[3] for c in cases)) + " ".join("%8d%s" % (total[k], "*" if k in can else " ") for k in names))
    print("positions of edge steps that could hold a candidate: %d, of the steps next to them: %d" %
          (dc.edge_step_positions(clip), dc.edge_step_positions(clip, inward=1)))
    for k in sorted(can):
        assert total[k] >= MIN_MEMBERS, (clip, k, total[k])
    assert ties >= MIN_TIES, (clip, ties)
    if clip == 560:
        r = dc.unpack(np.concatenate([dc.truth(c)[1] for c in cases]))[0]
        assert (r // dc.SD_T >= 32).sum() >= MIN_MEMBERS


def test_pruned_and_failed_positions_exist(table):
    """positions whose bare product dxx * dyy passes the threshold while the determinant does not, next to a candidate: the kernel
    has to evaluate dxy there (3 asked over all sizes; every size has thousands)"""
    n = sum(t["pruned_failed"] for t in table.values())
    print("\npruned-and-failed positions next to a candidate:", {k[0]: sum(t["pruned_failed"] for kk, t in table.items() if kk[0] == k[0]) for k in table})
    assert n >= MIN_PRUNED
    for clip in dc.CLIPS:
        assert sum(t["pruned_failed"] for k, t in table.items() if k[0] == clip) >= MIN_PRUNED, clip


@pytest.mark.parametrize("case", [c for c in dc.CASES if c[:2] in ((132, "blobs"), (497, "bin_squares"))], ids=lambda c: "%d-%s" % c[:2])
def test_hessian_parts_reproduce_the_oracles_layers(case):
    """guards the classifier only: dxx * dyy - 0.81 dxy^2 of the NumPy restatement against the oracle's layers, relative to the
    layer's largest magnitude.  Measured: 0.0 on both cases (the same float64 operations in the same order)."""
    pay, rc, val, layers = dc.truth(case)
    S = dc.integral(dc.cartesian(pay))
    for k in (1, 2):
        dxx, dyy, dxy = dc.hessian_parts(S, dc.SIZES[k])
        err = np.abs(dxx * dyy - 0.81 * (dxy * dxy) - layers[k]).max() / np.abs(layers[k]).max()
        print("\n%s layer %d: largest difference / largest determinant = %.3g" % (case[:2], k, err))
        assert err <= 1e-12, (case, k, err)


@pytest.mark.parametrize("clip", dc.CLIPS + (dc.OVERFLOW_CASE[0],))
def test_dark_steps_hold_nothing_above_the_threshold(clip):
    """the premise of the kernel's skip: in a dark step every determinant of the oracle is at or below the threshold"""
    dark = dc.dark_steps(clip)
    W = 2 * (clip // 2)
    assert dark.shape == (-(-W // dc.SD_OUT), W // dc.SD_T + 1)
    cases = dc.cases_of(clip) or [dc.OVERFLOW_CASE]
    n_dark = 0
    for case in cases:
        layers = dc.truth(case)[3]
        for s, t in zip(*np.nonzero(dark)):
            for k in (1, 2):
                blk = layers[k][dc.SD_T * t:dc.SD_T * t + dc.SD_T, dc.SD_OUT * s:dc.SD_OUT * s + dc.SD_OUT]
                n_dark += blk.size
                assert not (blk > dc.THRESHOLD).any(), (case, s, t, k, blk.max())
    assert n_dark > 0 or clip == 132                                       # (at 132 the range circle reaches every window)
