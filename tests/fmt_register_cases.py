"""Inputs of the Fourier-Mellin registration tests (tests/test_gpu_fmt_register.py on the GPU, tests/test_fmt_register_cpu.py without
one) and the all-CPU chain they are judged by, computed once per process and shared.

The chain (cpu_chain) composes what the device pass composes:
  angle, scale, rot_response = oracle.getRotationUsingFMT(src, tgt, downsample, clip)
  srcCart, tgtCart           = warp_polar_model.convertPolarImageToCartesian(., downsampleFactor=cart_downsample)   (full width)
  srcRot                     = warp_affine_model.rotateImg(srcCart, math.degrees(angle))       (the reference's sign, FMT.py:134-168)
  (dx, dy), trans_response   = oracle.phaseCorrelate(srcRot, tgtCart)
with an optional forced angle in place of the estimate (the GPU test feeds the device's own angle to the two last stages; the
tolerance of the end-to-end comparison comes from forcing angle +- 1e-14 rad, angle_sensitivity).

  case      polar shape                     clip / downsample   cart_downsample  side  DFT plane   what it covers
  live20    400 x 2025                      1012 / 10           20               202   216 x 216   the live shape, padded by the FFT
  live5     400 x 2025                      1012 / 10           5                810   810 x 810   the live shape, no padding, radix 3 and 5
  tex1      64 x 128, random float32        none / 2            1                256   256 x 256   cart_downsample 1, a power of two
  tex3      64 x 128, random float32        none / 2            3                84    90 x 90     128 // 3 = 42: a remainder, padding
  strided7  399 x 497, non-contiguous view  497 / 7             7                142   144 x 144   odd sizes, strides

Four pairs per case, the pattern of tests/fmt_batch_cases.py: (p0, p0), (p0, p1), (p0, roll(p0, k0)), (p1, roll(p0, k1)); live and
strided7 are that file's cases a and c (images and rotation results shared with it), tex its recipe for case b at 64 x 128.

Conventions found (asserted by the CPU test):
  * a scan against itself: angle 0 and (dx, dy) = (0, 0) to 1e-9 px - oracle.phaseCorrelate returns the centre minus the centroid,
    which is zero for identical images, not (Rc, Rc);
  * a target that is the source moved forward comes out with dx < 0: (dx, dy) * 0.0432 * cart_downsample is MINUS the ego motion in
    the source frame, to about one pixel of the downsampled image (EGO_* below)."""
import math

import numpy as np

import fmt_batch_cases as fb
import oracle
import phase_correlate_cases as pc
import warp_affine_model as wam
import warp_polar_model as wpm

CASES = {           # name: (images of, clip_px, downsample, cart_downsample, Rc, M)
    "live20": ("a", 1012, 10, 20, 101, 216),
    "live5": ("a", 1012, 10, 5, 405, 810),
    "tex1": ("t", 0, 2, 1, 128, 256),
    "tex3": ("t", 0, 2, 3, 42, 90),
    "strided7": ("c", 497, 7, 7, 71, 144),
}
T_SEED = 9
ROLLS = {"a": (7, -31), "t": (3, -5), "c": (7, -31)}

# Synthetic ego-motion pairs (known answers of the CPU chain): (seed, frames) of synth.make_sequence, pair 0 -> 1, with and without
# motion distortion, at cart_downsample 20 and 5.  EGO_WORST_M: the largest |(-dx, -dy) * 0.0432 * cart_downsample - true motion in
# the source frame| measured over them per cart_downsample (test_fmt_register_cpu.py prints every figure); the test asserts the sign
# and worst measured + one Cartesian pixel (0.0432 * cart_downsample m).
EGO_SEQUENCES = [(7, 3), (4, 3)]
EGO_WORST_M = {20: 0.1948, 5: 0.2002}

# End-to-end tolerance of the device against this chain (test (d) of the GPU test).  The device's angle differs from the oracle's in
# the last bits (3.2e-15 rad measured, docs/PARITY.md), and a last-bit difference may flip a 1/1024-px rounding of the rotation.  The
# chain was run with the angle forced to the estimate +- 1e-14 rad (three times that difference) on every pair above
# (angle_sensitivity; the CPU test repeats it): no coordinate of any pair flipped, dx, dy and the response did not change in a single
# bit, so ten times the largest change is 0 for all three.  What is left is the arithmetic of the correlation itself on equal
# images: the bounds tests/test_gpu_phase_correlate.py derives for it (6.6e-11 px, 4.0e-12 relative).
ANGLE_EPS = 1e-14
SENS_PX = 0.0               # 10 x the largest |change of dx or dy|, px
SENS_RESPONSE_REL = 0.0     # 10 x the largest relative change of the response
PC_TOL_PX = 6.6e-11
PC_TOL_RESPONSE_REL = 4.0e-12

_cache = {}


def images(case):
    """-> (p0, p1) float32 polar images of the case"""
    base = CASES[case][0]
    if base != "t":
        return fb.images(base)
    if "img-t" not in _cache:
        rng = np.random.default_rng(T_SEED)
        q0 = rng.random((64, 128), dtype=np.float32)
        q1 = (np.float32(0.9) * np.roll(q0, 1, axis=0) + np.float32(0.1) * rng.random((64, 128), dtype=np.float32)).astype(np.float32)
        _cache["img-t"] = (q0, q1)
    return _cache["img-t"]


def pairs(case):
    """-> [(src, tgt)] x 4"""
    p0, p1 = images(case)
    k0, k1 = ROLLS[CASES[case][0]]
    return [(p0, p0), (p0, p1), (p0, np.roll(p0, k0, axis=0)), (p1, np.roll(p0, k1, axis=0))]


def batch(case):
    """-> (src (4, rows, cols), tgt) as 3-D arrays; strided7 as non-contiguous views (row stride 504 floats)"""
    if CASES[case][0] == "c":
        return fb.batch("c")
    ps = pairs(case)
    return np.stack([a for a, _ in ps]), np.stack([b for _, b in ps])


def clip_m(clip_px):
    """the maxRangeClipM that oracle.getRotationUsingFMT turns into clip_px bins (0: no clip)"""
    if clip_px <= 0:
        return 0.0
    m = clip_px * oracle.RANGE_RESOLUTION_CART_M + 1e-9
    assert int(m / oracle.RANGE_RESOLUTION_CART_M) == clip_px
    return m


def cart(img, cart_downsample):
    """warp_polar_model.convertPolarImageToCartesian with the plan of a shape built once"""
    rows, cols = img.shape
    key = ("plan", rows, cols, cart_downsample)
    if key not in _cache:
        _cache[key] = wpm.polar_to_cart_plan(rows, cols, cart_downsample)
    return _cache[key](img)


def translation(src_cart, tgt_cart, angle):
    """the two last stages of the chain for a given angle -> (srcRot, (dx, dy), response)"""
    rot = wam.rotateImg(src_cart, math.degrees(angle))
    (dx, dy), resp = oracle.phaseCorrelate(rot, tgt_cart)
    return rot, (float(dx), float(dy)), float(resp)


def cpu_chain(src, tgt, clip_px, downsample, cart_downsample, angle=None, rotation=None):
    """-> dict(out6, src_cart, tgt_cart, src_rot).  angle: forced in place of the estimate; rotation: (angle, scale, response)
    already known for the pair (the rotation half is then not run again)"""
    if rotation is None:
        rotation = oracle.getRotationUsingFMT(np.ascontiguousarray(src), np.ascontiguousarray(tgt), downsample, clip_m(clip_px))
    a = float(rotation[0]) if angle is None else float(angle)
    sc, tc = cart(src, cart_downsample), cart(tgt, cart_downsample)
    rot, (dx, dy), resp = translation(sc, tc, a)
    return dict(out6=np.array([a, rotation[1], rotation[2], dx, dy, resp], np.float64), src_cart=sc, tgt_cart=tc, src_rot=rot)


def rotations(case):
    """-> (4, 3) oracle.getRotationUsingFMT of the four pairs (cases a and c: tests/fmt_batch_cases.py's)"""
    base, clip_px, ds = CASES[case][:3]
    key = "rot-" + base
    if key not in _cache:
        if base in ("a", "c"):
            assert fb.CASES[base][:2] == (clip_px, ds)
            _cache[key] = fb.oracle_results(base)["out3"]
        else:
            _cache[key] = np.array([oracle.getRotationUsingFMT(a, b, ds, clip_m(clip_px)) for a, b in pairs(case)])
    return _cache[key]


def chain_results(case):
    """-> [cpu_chain(...)] x 4 of the case"""
    key = "chain-" + case
    if key not in _cache:
        _, clip_px, ds, cds, _, _ = CASES[case]
        rot = rotations(case)
        _cache[key] = [cpu_chain(a, b, clip_px, ds, cds, rotation=rot[i]) for i, (a, b) in enumerate(pairs(case))]
    return _cache[key]


def uniqueness(case):
    """-> for each pair, the largest value outside the 5 x 5 box around the maximum as a fraction of the maximum, in the correlation
    plane of the rotation (the oracle's log-polar images) and of the translation (the chain's Cartesian images): (rot, trans)"""
    base = CASES[case][0]
    if base in ("a", "c"):
        rot_u = fb.uniqueness(base)
    else:
        _, clip_px, ds = CASES[case][:3]
        lp = lambda img: oracle.convertPolarImgToLogPolar(oracle._cv_resize_cols_linear(img[:, :clip_px] if clip_px > 0 else img,
                                                                                        img.shape[1] // ds))
        rot_u = [pc.peak_uniqueness(pc.correlate_formula(lp(a), lp(b))[2]) for a, b in pairs(case)]
    trans_u = [pc.peak_uniqueness(pc.correlate_formula(r["src_rot"], r["tgt_cart"])[2]) for r in chain_results(case)]
    return list(zip(rot_u, trans_u))


def angle_sensitivity(case):
    """-> (largest |change of dx or dy| px, largest relative change of the response) over the case's pairs when the chain's angle is
    forced to the estimate +- ANGLE_EPS"""
    dpx = drel = 0.0
    for r in chain_results(case):
        a, dx, dy, resp = r["out6"][0], r["out6"][3], r["out6"][4], r["out6"][5]
        for e in (-ANGLE_EPS, ANGLE_EPS):
            _, (x, y), s = translation(r["src_cart"], r["tgt_cart"], a + e)
            dpx = max(dpx, abs(x - dx), abs(y - dy))
            drel = max(drel, abs(s - resp) / abs(resp))
    return dpx, drel


def ego_pairs():
    """-> [(name, src, tgt, true motion of the target in the source frame (x forward, y, m))]: pair 0 -> 1 of EGO_SEQUENCES, with and
    without motion distortion"""
    if "ego" not in _cache:
        from radarslampy_amd import synth
        out = []
        for seed, frames in EGO_SEQUENCES:
            for distortion in (False, True):
                recs, poses, _ = synth.make_sequence(seed, frames, distortion=distortion)
                p = [r[:, 11:11 + 2025].astype(np.float32) / np.float32(255.) for r in recs[:2]]
                d = np.linalg.inv(synth.se2(*poses[0])) @ synth.se2(*poses[1])
                out.append((f"seed{seed}{'-distorted' if distortion else ''}", p[0], p[1], (float(d[0, 2]), float(d[1, 2]))))
        _cache["ego"] = out
    return _cache["ego"]
