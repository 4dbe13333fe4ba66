"""Inputs of the batched rotation-prior tests (tests/test_gpu_fmt_batch.py on the GPU, tests/test_fmt_batch_cpu.py without one): four
shapes, four pairs each, and the oracle's results for them, computed once per process and shared.

  case  polar shape                     clip / downsample   R    log-polar   DFT plane    what it covers
  a     400 x 2025                      1012 / 10           101  317 x 101   320 x 108    the live shape
  b     16 x 40, random float32         none / 2            20   63 x 20     64 x 20      short rows, repeated angular wrap
  c     399 x 497, non-contiguous view  497 / 7             71   223 x 71    225 x 72     odd sizes, strides
  d     case a's images                 1012 / 2            506  1590 x 506  1600 x 512   a large plane: only the FFT makes it practical

The pairs of a (and d) are those of test_fmt_rotation_matches_oracle: (p0, p0), (p0, p1), (p0, roll(p0, 7)), (p1, roll(p0, -31)) on
synth.make_sequence(3, 2, n_movers=6); b and c follow the same pattern on their own images and row shifts."""
import numpy as np

import oracle
import phase_correlate_cases as pc

CASES = {           # name: (clip_px, downsample, R, (dh, dw), (M, N))
    "a": (1012, 10, 101, (317, 101), (320, 108)),
    "b": (0, 2, 20, (63, 20), (64, 20)),
    "c": (497, 7, 71, (223, 71), (225, 72)),
    "d": (1012, 2, 506, (1590, 506), (1600, 512)),
}
C_LAYOUT = (497, 399, 504, 5)       # gen_inputs.ENGINE_LAYOUTS: (clip, rows, stride, payload_off)
B_SEED = 5

_cache = {}


def _pairs(p0, p1, k0, k1):
    return [(p0, p0), (p0, p1), (p0, np.roll(p0, k0, axis=0)), (p1, np.roll(p0, k1, axis=0))]


def images(case):
    """-> (p0, p1) float32 polar images of the case"""
    key = "img-" + ("a" if case == "d" else case)
    if key not in _cache:
        if case in ("a", "d"):
            from radarslampy_amd import synth
            recs, _, _ = synth.make_sequence(3, 2, n_movers=6)
            _cache[key] = tuple(r[:, 11:11 + 2025].astype(np.float32) / np.float32(255.) for r in recs[:2])
        elif case == "b":
            rng = np.random.default_rng(B_SEED)
            q0 = rng.random((16, 40), dtype=np.float32)
            # the second image: the first one turned by one row, with a tenth of fresh noise on top
            q1 = (np.float32(0.9) * np.roll(q0, 1, axis=0) + np.float32(0.1) * rng.random((16, 40), dtype=np.float32)).astype(np.float32)
            _cache[key] = (q0, q1)
        else:
            from gen_inputs import layout_sequence
            clip, rows, stride, off = C_LAYOUT
            recs, _ = layout_sequence(clip, 2, rows, clip, stride, off, n_movers=6)
            # the whole record as float32: the image is the column slice [off, off + clip) of it, a view with row stride 504
            _cache[key] = tuple((r.astype(np.float32) / np.float32(255.))[:, off:off + clip] for r in recs)
    return _cache[key]


def pairs(case):
    """-> [(src, tgt)] x 4"""
    p0, p1 = images(case)
    k0, k1 = {"a": (7, -31), "d": (7, -31), "b": (3, -5), "c": (7, -31)}[case]
    return _pairs(p0, p1, k0, k1)


def batch(case):
    """-> (src (4, rows, cols), tgt) as 3-D arrays; case c as non-contiguous views (row stride 504 floats)"""
    ps = pairs(case)
    if case != "c":
        return np.stack([a for a, _ in ps]), np.stack([b for _, b in ps])
    clip, rows, stride, off = C_LAYOUT
    A, B = np.zeros((4, rows, stride), np.float32), np.zeros((4, rows, stride), np.float32)
    A[:, :, off:off + clip] = np.stack([a for a, _ in ps])
    B[:, :, off:off + clip] = np.stack([b for _, b in ps])
    return A[:, :, off:off + clip], B[:, :, off:off + clip]


def logpolar(case, img):
    clip_px, ds, R, _, _ = CASES[case]
    clipped = img[:, :clip_px] if clip_px > 0 else img
    return oracle.convertPolarImgToLogPolar(oracle._cv_resize_cols_linear(clipped, R))


def oracle_results(case):
    """-> dict(out3 (4, 3) of oracle.getRotationUsingFMT, lp_src / lp_tgt: the oracle's log-polar images of the four pairs)"""
    key = "res-" + case
    if key not in _cache:
        clip_px, ds, R, _, _ = CASES[case]
        ps = pairs(case)
        clip_m = clip_px * oracle.RANGE_RESOLUTION_CART_M + 1e-9 if clip_px > 0 else 0.0     # int(clip_m / resolution) == clip_px
        assert clip_px <= 0 or int(clip_m / oracle.RANGE_RESOLUTION_CART_M) == clip_px
        out3 = np.array([oracle.getRotationUsingFMT(a, b, ds, clip_m) for a, b in ps])
        _cache[key] = dict(out3=out3, lp_src=[logpolar(case, a) for a, _ in ps], lp_tgt=[logpolar(case, b) for _, b in ps])
    return _cache[key]


def uniqueness(case):
    """-> for each pair, the largest value of the oracle's correlation plane outside the 5 x 5 box around its maximum, as a fraction
    of the maximum (phase_correlate_cases.peak_uniqueness)"""
    r = oracle_results(case)
    return [pc.peak_uniqueness(pc.correlate_formula(a, b)[2]) for a, b in zip(r["lp_src"], r["lp_tgt"])]
