"""The screen of sd_tile_fast (csrc/retrack_det.hip) on the CPU: the fast path reads the xx-side box of a box size only in the waves
where a bound from the exact dyy and the xx-mid box cannot rule dxx * dyy > threshold out.  tests/det_screen_model.py restates the
six boxes, the bound and its margin in the kernel's operation order; here the one property the kernel relies on is held:

    ruled out  =>  the product, as the kernel rounds it, is at or below the threshold

on every position of every family of tests/det_candidate_cases.py at every size it lists, and on box values chosen against the
margin: side == mid, side == 0, mid == 0 under a side of rounding size, a side above its mid by one ulp and by the largest rounding
of the integral image the margin is derived for, and mids that put the bound, or the product, a few ulp either side of the threshold."""
import numpy as np
import pytest

import det_candidate_cases as dc
import det_screen_model as m

THR = dc.THRESHOLD
DELTA = 1.4e-4                                   # image units: the largest side-over-mid excess SD_SKIP_ABS is derived for


@pytest.mark.parametrize("clip", sorted({c.clip for c in dc.CASES}))
def test_no_passing_product_is_ruled_out(clip):
    n_out = n_pass = 0
    for case in (c for c in dc.CASES if c.clip == clip):
        S = dc.integral(dc.cartesian(dc.payload(case.family, case.clip, seed=case.seed)))
        for size in m.SIZES:
            prod, out = m.screen(S, size, THR)
            dxx, dyy, _ = dc.hessian_parts(S, size)
            passing = prod > THR
            print("clip %d %-11s size %2d: ruled out %5.1f %% of %d positions, product passes at %d, both %d" %
                  (clip, case.family, size, 100.0 * out.mean(), out.size, int(passing.sum()), int((out & passing).sum())))
            assert np.array_equal(prod, dxx * dyy), "the model's product is not the oracle's"      # (the 2^-10 scaling is exact)
            assert not (out & passing).any(), (case, size)
            n_out, n_pass = n_out + int(out.sum()), n_pass + int(passing.sum())
    assert n_out > 0 and n_pass > 0                                          # the size's cases lie on both sides of the rule


def _ulps(x, ks):
    out = []
    for k in ks:
        y = np.float64(x)
        for _ in range(abs(k)):
            y = np.nextafter(y, np.inf if k > 0 else -np.inf)
        out.append(y)
    return out


@pytest.mark.parametrize("size", m.SIZES)
def test_adversarial_box_values(size):
    s3 = size // 3
    top = size * (2 * s3 - 1) * m.SCALE                                      # a mid box full of ones, as the ring holds it
    w, eps = m.w_i(size), DELTA * m.SCALE
    mids = [0.0, 5e-324, 1e-300, 1e-12 * m.SCALE, 1e-6 * m.SCALE, 1e-3 * m.SCALE, m.SCALE, 7 * m.SCALE, 0.25 * top, top]

    def sides(mid):
        return [0.0, mid, mid / 3.0, np.nextafter(mid / 3.0, 0.0), np.nextafter(mid, np.inf), mid + 1e-9 * m.SCALE, mid + eps]

    dyy = np.unique([m.deriv(np.float64(ym), np.float64(ys), size) for ym in mids for ys in sides(ym)])
    assert (dyy > 0).any() and (dyy < 0).any() and (dyy == 0).any() and np.abs(dyy).max() <= 2.0
    n = dict(ruled=0, kept=0, above=0, below=0, near=0)
    for e in dyy:
        xms = list(mids)
        if abs(e) > 1e-200:                                                  # (below that no mid within range reaches the threshold)
            k = 2.0 if e > 0 else 1.0
            xms += _ulps((THR - m.SKIP_ABS) / (abs(e) * k * w * (1.0 + m.SKIP_REL)), range(-4, 5))     # the bound at the threshold it is held against
            xms += _ulps(THR / (abs(e) * k * w), range(-4, 5))                                         # the largest product at the threshold
        for xm in (x for x in xms if x <= top):
            xs = np.array(sides(np.float64(xm)))
            prod = e * m.deriv(np.float64(xm), xs, size)
            out = bool(m.ruled_out(np.float64(e), np.float64(xm), size, THR))
            assert not (out and (prod > THR).any()), (size, e, xm, xs[prod > THR], prod.max())
            n["ruled" if out else "kept"] += 1
            n["above"] += int((prod > THR).sum())
            n["below"] += int(((prod <= THR) & (prod > 0.99 * THR)).sum())
            n["near"] += int((np.abs(prod - THR) <= 16 * np.spacing(THR)).sum())
    print("size %d:" % size, n)
    assert min(n.values()) > 0, n
