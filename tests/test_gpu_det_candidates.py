"""GPU (-m gpu): the candidate lists of rt_det_strip_kernel (csrc/retrack_det.hip) - and, in the 208-lane engines, of the fused kernel
(csrc/retrack_fused.inc) - against oracle.doh_maxima: every key (row << 16 | col << 2 | layer) and every float64 determinant, bit for
bit, through Engine.debug_detect.  The feature tests see what _prune_blobs and SSC keep of a list (~200 of its candidates); here a
missing, an extra or a slightly wrong candidate shows wherever it sits.  The cases and the classes of the kernel's special paths they
populate: tests/det_candidate_cases.py, held by tests/test_det_candidates_cpu.py with the oracle alone.

debug_detect: scratch slot i works on the scan lane i % B saw last; the lanes are stepped once, onto the scan they started on."""
import functools

import numpy as np
import pytest

import det_candidate_cases as dc

pytestmark = pytest.mark.gpu
SWEEP_LANES = 208                                # a chunk of >= 200 detections takes rt_integral_kernel, fewer the two-pass kernels


@functools.lru_cache(maxsize=None)
def _lists(clip, B, fused):
    """the candidate lists of B detections, lane b on case b % T of the size (or on the overflow case alone): a tuple of (n, rc, val)
    per form asked for - the two-kernel form, then the fused kernel"""
    from radarslampy_amd import _ffi
    from radarslampy_amd.engine import Engine
    cases = dc.cases_of(clip) or [dc.OVERFLOW_CASE]
    T = len(cases)
    ctx = _ffi.Context(0)
    eng = Engine(B, T, ctx=ctx, rows=400, stride=clip, payload_off=0, clip=clip, retrack_on_device=True, retrack_slots=B)
    for t, case in enumerate(cases):
        eng.upload_scan(t, dc.truth(case)[0])
    scan = [b % T for b in range(B)]
    eng.init_lanes_detect(0, scan, np.zeros((B, 3)))
    eng.step(scan)
    out = tuple(eng.debug_detect(f, B) for f in ((False, True) if fused else (False,)))
    eng.close()
    ctx.close()
    return out


def _differences(tag, n, rc, val, want_rc, want_val):
    """prints what differs before anything is asserted: which keys are missing / extra tells which path of the kernel broke"""
    got_rc, got_val = rc[:min(n, dc.CAP)], val[:min(n, dc.CAP)]
    missing, extra = np.setdiff1d(want_rc, got_rc), np.setdiff1d(got_rc, want_rc)
    common, iw, ig = np.intersect1d(want_rc, got_rc, return_indices=True)
    dv = np.abs(want_val[iw] - got_val[ig])
    show = lambda k: [tuple(int(x[0]) for x in dc.unpack(np.array([q]))) for q in k[:6]]
    print("%s: n %d (oracle %d), missing %d %s, extra %d %s, common %d with %d values different, largest difference %.3g" %
          (tag, n, len(want_rc), len(missing), show(missing), len(extra), show(extra), len(common), int((dv != 0).sum()), dv.max() if len(dv) else 0.0))


def _same(tag, n, rc, val, case):
    want_rc, want_val = dc.truth(case)[1:3]
    _differences(tag, int(n), rc, val, want_rc, want_val)
    assert n == case[3] == len(want_rc), (tag, int(n), case[3])
    assert np.array_equal(rc[:n], want_rc), tag
    assert val[:n].tobytes() == want_val.tobytes(), tag


@pytest.mark.parametrize("clip", dc.CLIPS)
def test_candidates_equal_the_oracle_two_pass(clip):
    cases = dc.cases_of(clip)
    B = len(cases)
    assert B < 200
    (n, rc, val), = _lists(clip, B, False)
    for b, case in enumerate(cases):
        _same("two-pass clip %d %s slot %d" % (clip, case[1], b), n[b], rc[b], val[b], case)


@pytest.mark.parametrize("clip", [132, 560])
def test_candidates_equal_the_oracle_one_sweep(clip):
    cases = dc.cases_of(clip)
    T, B = len(cases), SWEEP_LANES
    two, fused = _lists(clip, B, True)
    for form, (n, rc, val) in (("one-sweep", two), ("fused", fused)):
        for b in list(range(T)) + [B - 1]:
            case = cases[b % T]
            _same("%s clip %d %s slot %d" % (form, clip, case[1], b), n[b], rc[b], val[b], case)


def test_candidates_are_the_same_for_every_slot_of_a_scan():
    """nothing may depend on the detection's place in the XCD-aware work list"""
    T, B = len(dc.cases_of(132)), SWEEP_LANES
    for form, (n, rc, val) in zip(("one-sweep", "fused"), _lists(132, B, True)):
        for b in range(T, B):
            assert n[b] == n[b % T] and rc[b].tobytes() == rc[b % T].tobytes() and val[b].tobytes() == val[b % T].tobytes(), (form, b)


def test_overflow_counts_every_maximum():
    """beyond 2048 maxima the kernel keeps the first 2048 to arrive and counts them all: the count is the oracle's, the kept keys are
    distinct and each is one of the oracle's with the oracle's value; which 2048 are kept is not asserted"""
    case = dc.OVERFLOW_CASE
    want_rc, want_val = dc.truth(case)[1:3]
    (n, rc, val), = _lists(case[0], 1, False)
    kept = rc[0, :dc.CAP]
    i = np.searchsorted(want_rc, kept)
    inside = (i < len(want_rc)) & (want_rc[np.minimum(i, len(want_rc) - 1)] == kept)
    print("overflow: n %d (oracle %d), kept %d distinct %d, not in the oracle's set %d" %
          (n[0], len(want_rc), len(kept), len(np.unique(kept)), int((~inside).sum())))
    assert n[0] == case[3] == len(want_rc) and n[0] > dc.CAP
    assert len(np.unique(kept)) == dc.CAP
    assert inside.all()
    assert val[0, :dc.CAP].tobytes() == want_val[i].tobytes()
