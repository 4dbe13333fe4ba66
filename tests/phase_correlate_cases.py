"""Inputs of the phase-correlation tests (tests/test_gpu_phase_correlate.py on the GPU, tests/test_phase_correlate_cpu.py without
one) and the float64 restatement of the formula they are judged by.

correlate_formula is oracle.phaseCorrelate with two switches the oracle does not have: the window can be left out (hanning=False,
cv2.phaseCorrelate(src, tgt)) and the transforms can run in a second float64 order (order="two_pass": numpy.fft.fft along axis 0,
then along axis 1; numpy's fft2 goes along axis 1 first).  With both switches at their defaults it returns what the oracle returns,
bit for bit (asserted by the CPU test).  The spread between the two orders over all the inputs below is what the tolerances of the
GPU test are derived from (measure_spread; the constants and the procedure are at the top of the GPU test)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# every radix and the padding: 8 = 2^3; 108 x 320: no padding (the rotation prior's size); 317 -> 320, 101 -> 108; 2025 = 3^4 5^2;
# 1012 -> 1024; 2024 -> 2025; 4096 = 4^6 beside the smallest sides; 1000 = 2^3 5^3, 1500 = 2^2 3 5^3
SHAPES = [(8, 8), (108, 320), (317, 101), (400, 2025), (1012, 1012), (2024, 2024), (2, 4096), (4096, 3), (1000, 1500)]
KNOWN_ANSWER_SHAPES = [(108, 320), (2048, 2048)]        # 320 x 108 and 2048 x 2048 as width x height: no padding
FFT_LENGTHS = [1, 2, 3, 4, 5, 6, 8, 9, 15, 16, 25, 27, 30, 45, 64, 81, 108, 125, 243, 320, 625, 1024, 2025, 2048, 3125, 3600, 4050, 4096]
FFT_OTHER_SIDE = 6                                      # the FFT-alone planes are 6 x n and n x 6


def optimal_dft_size(n):
    while True:
        m = n
        for p in (2, 3, 5):
            while m % p == 0:
                m //= p
        if m == 1:
            return n
        n += 1


def _fft2(a, order, inverse=False):
    f = np.fft.ifft if inverse else np.fft.fft
    if order == "fft2":
        return np.fft.ifft2(a) if inverse else np.fft.fft2(a)
    assert order == "two_pass"
    return f(f(a, axis=0), axis=1)


def correlate_formula(src1, src2, hanning=True, order="fft2"):
    """-> ((dx, dy), response, shifted correlation plane)"""
    H, W = src1.shape
    if hanning:
        wc = 0.5 * (1.0 - np.cos(2.0 * np.pi / (W - 1) * np.arange(W)))
        wr = 0.5 * (1.0 - np.cos(2.0 * np.pi / (H - 1) * np.arange(H)))
        win = np.sqrt((wr[:, None] * wc[None, :]).astype(np.float32))
    else:
        win = np.ones((H, W), np.float32)
    M, N = optimal_dft_size(H), optimal_dft_size(W)
    a = np.zeros((M, N), np.float32); b = np.zeros((M, N), np.float32)
    a[:H, :W] = (win * src1).astype(np.float32); b[:H, :W] = (win * src2).astype(np.float32)
    F1, F2 = _fft2(a.astype(np.float64), order), _fft2(b.astype(np.float64), order)
    P = F1 * np.conj(F2)
    mag = np.abs(P)
    eps32 = float(np.finfo(np.float32).eps)
    Cc = np.fft.fftshift(np.real(_fft2(P * mag / (mag * mag + eps32), order, inverse=True)))
    py, px = np.unravel_index(np.argmax(Cc), Cc.shape)
    r0, r1 = max(py - 2, 0), min(py + 2, M - 1)
    c0, c1 = max(px - 2, 0), min(px + 2, N - 1)
    box = Cc[r0:r1 + 1, c0:c1 + 1]
    s = box.sum()
    ys, xs = np.mgrid[r0:r1 + 1, c0:c1 + 1]
    cx, cy = (xs * box).sum() / (s + np.finfo(float).eps), (ys * box).sum() / (s + np.finfo(float).eps)
    return (N / 2.0 - cx, M / 2.0 - cy), s, Cc


def peak_uniqueness(plane):
    """largest value outside the 5 x 5 box around the first maximum, as a fraction of the maximum (0 for a plane of zeros)"""
    py, px = np.unravel_index(np.argmax(plane), plane.shape)
    top = plane[py, px]
    rest = plane.copy()
    rest[max(py - 2, 0):py + 3, max(px - 2, 0):px + 3] = -np.inf
    other = rest.max() if np.isfinite(rest).any() else 0.0
    if top == 0.0:
        return 0.0 if other <= 0.0 else np.inf
    return float(other / top)


def fit(img, shape):
    """crop `img` about its centre to `shape`; where it is too small, continue it by mirror images of itself first (a periodic
    continuation would give the correlation plane one peak per period)"""
    H, W = shape
    h, w = img.shape
    if H > h or W > w:
        img = np.pad(img, ((0, max(H - h, 0)), (0, max(W - w, 0))), mode="symmetric")
        h, w = img.shape
    y0, x0 = (h - H) // 2, (w - W) // 2
    return np.ascontiguousarray(img[y0:y0 + H, x0:x0 + W], np.float32)


def texture(shape, seed):
    """seeded smooth random texture in [0, 1], periodic (so that a circular shift of it is a translation)"""
    from scipy.ndimage import gaussian_filter
    t = gaussian_filter(np.random.default_rng(seed).standard_normal(shape), 2.0, mode="wrap")
    t -= t.min()
    return (t / t.max()).astype(np.float32)


def shift_fraction(img, fy, fx):
    """circular translation by (fy, fx) in [0, 1) pixels down / right, by linear interpolation"""
    t = img.astype(np.float64)
    down, right = np.roll(t, 1, axis=0), np.roll(t, 1, axis=1)
    return ((1 - fy) * (1 - fx) * t + fy * (1 - fx) * down + (1 - fy) * fx * right + fy * fx * np.roll(down, 1, axis=1)).astype(np.float32)


def default_roll(shape):
    """(rows down, columns right) of the circular shifts: (3, -7) where the image is large enough for it"""
    return min(3, shape[0] // 4), -min(7, shape[1] // 4)


_sources = {}


def sources(to_cart):
    """the real and synthetic scans as float32 images: polar (400 x 2025) and Cartesian (2024 x 2024, through `to_cart`: the GPU
    test passes the device warp, the CPU test the oracle's, and the two are equal bit for bit - tests/test_gpu_stages.py)"""
    if to_cart not in _sources:
        from radarslampy_amd import synth
        g = np.load(os.path.join(GOLDEN, "peaks.npz"))
        polar = [g[k].astype(np.float32) / np.float32(255.) for k in ("real0_u8", "real1_u8")]
        recs, poses, _ = synth.make_sequence(4, 2)
        spolar = [r[:, 11:11 + 2025].astype(np.float32) / np.float32(255.) for r in recs]
        _sources[to_cart] = dict(polar=polar, cart=[to_cart(p) for p in polar], synth_polar=spolar,
                                 synth_cart=[to_cart(p) for p in spolar], synth_poses=poses)
    return _sources[to_cart]


def oracle_cases(to_cart):
    """[(name, a, b, hanning)]: the inputs of the comparison with the oracle (hanning True) and with the windowless formula
    (hanning False), the same list on the GPU and on the CPU.

    A 2-row image under the Hanning window is a plane of zeros (both window rows are 0): (2, 4096) with the window on compares two
    exactly defined degenerate results (first maximum = element 0 of a zero plane) and is in the list for the limit itself; the
    windowless entries of that shape carry the arithmetic."""
    s = sources(to_cart)
    out = []
    for shape in SHAPES:
        tag = "%dx%d" % shape
        kind = "polar" if shape[0] <= 400 and shape[1] <= 2025 else "cart"
        r0, r1 = fit(s[kind][0], shape), fit(s[kind][1], shape)
        dy, dx = default_roll(shape)
        tex = texture(shape, 11 + shape[0] + shape[1])
        out += [(f"{tag}-real0-{kind}-self", r0, r0, True),
                (f"{tag}-real0-{kind}-rolled", r0, np.roll(r0, (dy, dx), axis=(0, 1)), True),
                (f"{tag}-real0-real1-{kind}", r0, r1, True),
                (f"{tag}-real1-{kind}-self", r1, r1, True),
                (f"{tag}-real1-{kind}-rolled", r1, np.roll(r1, (dy, dx), axis=(0, 1)), True),
                (f"{tag}-texture-rolled", tex, np.roll(tex, (dy, dx), axis=(0, 1)), True),
                (f"{tag}-texture-fraction", tex, shift_fraction(tex, 0.25 if shape[0] > 2 else 0.0, 0.6 if shape[1] > 3 else 0.0), True),
                (f"{tag}-texture-rolled-nowindow", tex, np.roll(tex, (dy, dx), axis=(0, 1)), False)]
    for shape, kind in (((400, 2025), "synth_polar"), ((2024, 2024), "synth_cart"), ((1012, 1012), "synth_cart")):
        out.append(("%dx%d-%s-ego-motion" % (shape + (kind,)), fit(s[kind][0], shape), fit(s[kind][1], shape), True))
    t2 = texture((2, 4096), 5)
    out += [("2x4096-texture-fraction-nowindow", t2, shift_fraction(t2, 0.0, 0.6), False),
            ("2x4096-real0-polar-rolled-nowindow", fit(s["polar"][0], (2, 4096)), np.roll(fit(s["polar"][0], (2, 4096)), -7, axis=1), False)]
    return out


def known_answer_cases(to_cart):
    """[(name, a, (dy, dx))]: images that need no padding, to be rolled by whole pixels (rows down, columns right)"""
    s = sources(to_cart)
    return [("108x320-real0-polar", fit(s["polar"][0], (108, 320)), (3, -7)),
            ("108x320-texture", texture((108, 320), 3), (-5, 12)),
            ("2048x2048-real0-cart", fit(s["cart"][0], (2048, 2048)), (3, -7)),
            ("2048x2048-texture", texture((2048, 2048), 4), (40, 13))]


def batch_cases(to_cart):
    """five pairs of one shape (317 x 101) for the batch test"""
    s = sources(to_cart)
    pairs = []
    for i in range(5):
        a = np.ascontiguousarray(s["polar"][0][10 * i:10 * i + 317, 300 + 97 * i:401 + 97 * i])
        b = np.ascontiguousarray(s["polar"][i % 2][10 * i + 2:10 * i + 319, 305 + 97 * i:406 + 97 * i])
        pairs.append((a, b))
    return pairs


def large_batch(to_cart):
    """two 4096 x 4096 pairs (the Cartesian scans continued by mirror images): the largest plane, and a batch that does not fit the
    2 GB scratch bound in one chunk -> (A (2, 4096, 4096), B)"""
    s = sources(to_cart)
    a0, a1 = fit(s["cart"][0], (4096, 4096)), fit(s["cart"][1], (4096, 4096))
    return np.stack([a0, a1]), np.stack([np.roll(a0, (3, -7), axis=(0, 1)), a0])


def u8_pair():
    u8 = np.load(os.path.join(GOLDEN, "peaks.npz"))["real0_u8"][:64, :96]
    return u8, np.roll(u8, 2, axis=1)


def all_pairs(to_cart):
    """every (name, a, b, hanning) the GPU tests 1, 2, 4 and 5 put through the device: the uniqueness condition is asserted on each"""
    out = list(oracle_cases(to_cart))
    for name, a, (dy, dx) in known_answer_cases(to_cart):
        b = np.roll(a, (dy, dx), axis=(0, 1))
        out += [(name + "-known-nowindow", a, b, False), (name + "-known-window", a, b, True)]
    for i, (a, b) in enumerate(batch_cases(to_cart)):
        out += [(f"batch-{i}", a, b, True), (f"batch-{i}-nowindow", a, b, False)]
    A, B = large_batch(to_cart)
    out += [(f"4096x4096-pair-{i}", A[i], B[i], True) for i in range(2)]
    u, v = u8_pair()
    out.append(("64x96-u8", u.astype(np.float32), v.astype(np.float32), True))
    return out


def fft_planes():
    """[(name, complex128 plane)]: every length of FFT_LENGTHS as the row length and as the column length"""
    rng = np.random.default_rng(2)
    out = []
    for n in FFT_LENGTHS:
        for shape in ((FFT_OTHER_SIDE, n), (n, FFT_OTHER_SIDE)):
            out.append(("%dx%d" % shape, rng.standard_normal(shape) + 1j * rng.standard_normal(shape)))
    return out


def measure_spread(to_cart, log=print):
    """the largest difference between the two float64 orders over all inputs: (dx px, dy px, response relative) of the correlation
    and the FFT alone relative to max |X| - the procedure behind the GPU test's tolerances"""
    ddx = ddy = dresp = 0.0
    for name, a, b, hanning in all_pairs(to_cart):
        (x0, y0), r0, plane = correlate_formula(a, b, hanning, "fft2")
        (x1, y1), r1, _ = correlate_formula(a, b, hanning, "two_pass")
        rel = abs(r1 - r0) / abs(r0) if r0 != 0 else abs(r1 - r0)
        log(f"{name}: dx {x0:.6f} dy {y0:.6f} response {r0:.6g} | spread dx {abs(x1 - x0):.3g} dy {abs(y1 - y0):.3g} response {rel:.3g} | "
            f"uniqueness {peak_uniqueness(plane):.4f}")
        ddx, ddy, dresp = max(ddx, abs(x1 - x0)), max(ddy, abs(y1 - y0)), max(dresp, rel)
    dfft = 0.0
    for name, z in fft_planes():
        X = np.fft.fft2(z)
        dfft = max(dfft, float(np.abs(_fft2(z, "two_pass") - X).max() / np.abs(X).max()))
        back = np.fft.ifft2(X) * z.size
        dfft = max(dfft, float(np.abs(_fft2(X, "two_pass", inverse=True) * z.size - back).max() / np.abs(back).max()))
    log(f"spread: dx {ddx:.3g} px, dy {ddy:.3g} px, response {dresp:.3g} relative, FFT alone {dfft:.3g} of max |X|")
    return ddx, ddy, dresp, dfft
