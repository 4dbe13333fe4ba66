"""Phase correlation at any image size (roam_phase_correlate_f32, csrc/phasecorr.hip) against the oracle's float64 restatement of
cv2.phaseCorrelate, and the mixed-radix FFT alone against numpy.  The inputs are tests/phase_correlate_cases.py.

Tolerances.  The device and the oracle evaluate one float64 formula in different summation orders, so they agree to the rounding of
the correlation plane, amplified by the centroid's division.  The margin is measured on the CPU, not chosen: the formula is evaluated
in a second float64 order (numpy.fft.fft along axis 0, then axis 1, instead of fft2) over ALL inputs of this file
(phase_correlate_cases.measure_spread), and ten times the largest difference between the two orders is the tolerance.  Measured
(numpy 2.2.6): dx 1.36e-12 px and dy 6.59e-12 px (both on 1012x1012-texture-rolled-nowindow, a weak peak of response 0.0022 because
the roll of a padded image is no circular shift), response 3.99e-13 relative (the same input); the FFT alone 5.02e-16 of max |X|.
Every difference is printed before it is asserted (run with -s).
The cap of 5e-4 px (the rotation prior's 1e-5 rad expressed in pixels) is far above all of them."""
import numpy as np
import pytest

import oracle
import phase_correlate_cases as pc

pytestmark = pytest.mark.gpu

TOL_PX = 6.6e-11            # 10 x 6.59e-12 px: the larger of the dx and dy spreads of the two CPU orders
TOL_RESPONSE_REL = 4.0e-12  # 10 x 3.99e-13
TOL_FFT_REL = 5.1e-15       # 10 x 5.02e-16 of max |X|
assert TOL_PX <= 5e-4


@pytest.fixture(scope="module")
def ctx():
    from radarslampy_amd import _ffi
    c = _ffi.default_context()
    assert "gfx950" in c.device_info()["arch"]
    return c


@pytest.fixture(scope="module")
def to_cart(ctx):
    def warp(polar):
        return ctx.polar_to_cart_f32(polar)[0]
    return warp


def _check(name, got, want):
    (gx, gy), gr = got
    (wx, wy), wr = want
    print(f"{name}: dx {gx:.9f} ({gx - wx:+.3g}) dy {gy:.9f} ({gy - wy:+.3g}) response {gr:.9g} ({(gr - wr) / wr if wr else gr - wr:+.3g} rel)")
    assert abs(gx - wx) <= TOL_PX and abs(gy - wy) <= TOL_PX, (name, gx - wx, gy - wy)
    assert abs(gr - wr) <= TOL_RESPONSE_REL * abs(wr), (name, gr, wr)


@pytest.mark.timeout(1200)
def test_against_oracle(ctx, to_cart):
    """every shape x {real scan against itself, rolled, against the other scan; texture rolled, shifted by a fraction; synthetic
    ego motion}: dx, dy, response against oracle.phaseCorrelate; the windowless entries against the oracle's formula with the
    window replaced by ones"""
    cases = pc.oracle_cases(to_cart)
    assert {a.shape for _, a, _, _ in cases} >= set(pc.SHAPES)
    for name, a, b, hanning in cases:
        if hanning:
            want = oracle.phaseCorrelate(a, b)
        else:
            want = pc.correlate_formula(a, b, hanning=False)[:2]
        _check(name, ctx.phase_correlate(a, b, hanning=hanning), want)


def test_synthetic_pair_sees_the_ego_motion(ctx, to_cart):
    """the synthetic pair moves 1.29 m (14.9 Cartesian pixels) forward and turns by 0.027 rad; a pure translation cannot model the
    turn, so the estimate (14.4 px in the oracle) is held to a quarter of the known motion, no closer"""
    s = pc.sources(to_cart)
    (dx, dy), response = ctx.phase_correlate(s["synth_cart"][0], s["synth_cart"][1])
    d = np.linalg.inv(_se2(s["synth_poses"][0])) @ _se2(s["synth_poses"][1])
    metres = np.hypot(d[0, 2], d[1, 2])
    from radarslampy_amd.parseData import RANGE_RESOLUTION_CART_M
    assert abs(np.hypot(dx, dy) * RANGE_RESOLUTION_CART_M - metres) < 0.25 * metres, (dx, dy, metres)
    assert response > 0.1


def _se2(p):
    c, s = np.cos(p[2]), np.sin(p[2])
    return np.array([[c, -s, p[0]], [s, c, p[1]], [0, 0, 1.0]])


@pytest.mark.timeout(600)
def test_known_answer_whole_pixel_shift(ctx, to_cart):
    """np.roll by whole pixels at sizes that need no padding.  Without the window (dx, dy) rounds to the shift in OpenCV's sign
    convention (b = roll(a, (sy, sx)) -> (dx, dy) = (sx, sy)), and response and centroid agree with the windowless formula; with the
    window the result is compared with the oracle only (the window biases the centroid)."""
    for name, a, (sy, sx) in pc.known_answer_cases(to_cart):
        assert pc.optimal_dft_size(a.shape[0]) == a.shape[0] and pc.optimal_dft_size(a.shape[1]) == a.shape[1]
        b = np.roll(a, (sy, sx), axis=(0, 1))
        got = ctx.phase_correlate(a, b, hanning=False)
        assert (round(got[0][0]), round(got[0][1])) == (sx, sy), (name, got)
        _check(name + "-nowindow", got, pc.correlate_formula(a, b, hanning=False)[:2])
        _check(name + "-window", ctx.phase_correlate(a, b), oracle.phaseCorrelate(a, b))


@pytest.mark.timeout(600)
def test_fft_alone(ctx):
    """forward equals numpy.fft.fft2 and forward-then-inverse returns M N times the input, for every length as the row length and
    as the column length; differences relative to the largest magnitude of the plane compared"""
    worst = 0.0
    for name, z in pc.fft_planes():
        X = ctx.debug_fft2(z)
        want = np.fft.fft2(z)
        e_f = np.abs(X - want).max() / np.abs(want).max()
        back = ctx.debug_fft2(X, inverse=True)
        e_b = np.abs(back - z.size * z).max() / (z.size * np.abs(z).max())
        print(f"fft {name}: forward {e_f:.3g} round trip {e_b:.3g}")
        worst = max(worst, e_f, e_b)
        assert e_f <= TOL_FFT_REL and e_b <= TOL_FFT_REL, (name, e_f, e_b)
    # a real plane (the null imaginary input of the forward row pass)
    r = np.random.default_rng(3).standard_normal((45, 64))
    assert np.abs(ctx.debug_fft2(r) - np.fft.fft2(r)).max() / np.abs(np.fft.fft2(r)).max() <= TOL_FFT_REL
    print("fft worst", worst)


def test_fft_refuses_other_lengths(ctx):
    from radarslampy_amd import _ffi
    for shape in ((7, 8), (8, 11), (4097, 2), (2, 4098)):
        with pytest.raises(_ffi.RoamError):
            ctx.debug_fft2(np.zeros(shape))


@pytest.mark.timeout(600)
def test_batch_and_strides_bit_for_bit(ctx, to_cart):
    pairs = pc.batch_cases(to_cart)
    A, B = np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs])
    for hanning in (True, False):
        dxdy, resp = ctx.phase_correlate(A, B, hanning=hanning)
        assert dxdy.shape == (5, 2) and resp.shape == (5,)
        for i, (a, b) in enumerate(pairs):
            (dx, dy), r = ctx.phase_correlate(a, b, hanning=hanning)
            assert (dx, dy, r) == (dxdy[i, 0], dxdy[i, 1], resp[i]), (i, hanning)
            want = oracle.phaseCorrelate(a, b) if hanning else pc.correlate_formula(a, b, hanning=False)[:2]
            _check(f"batch-{i}-{'window' if hanning else 'nowindow'}", ((dx, dy), r), want)
    a, b = pairs[0]
    single = ctx.phase_correlate(a, b)
    # every second row of a taller array
    tall_a, tall_b = np.zeros((2 * a.shape[0], a.shape[1]), np.float32), np.full((2 * a.shape[0], a.shape[1]), 7, np.float32)
    tall_a[::2], tall_b[::2] = a, b
    assert not tall_a[::2].flags.c_contiguous and ctx.phase_correlate(tall_a[::2], tall_b[::2]) == single
    # a column window of a wider array
    wide_a, wide_b = np.full((a.shape[0], a.shape[1] + 9), 3, np.float32), np.full((a.shape[0], a.shape[1] + 9), 5, np.float32)
    wide_a[:, 4:4 + a.shape[1]], wide_b[:, 4:4 + a.shape[1]] = a, b
    assert ctx.phase_correlate(wide_a[:, 4:4 + a.shape[1]], wide_b[:, 4:4 + a.shape[1]]) == single
    # a strided batch (every second image of a longer stack, rows inside a wider frame) and other dtypes
    frame_a, frame_b = np.zeros((10,) + (a.shape[0], a.shape[1] + 3), np.float32), np.ones((10,) + (a.shape[0], a.shape[1] + 3), np.float32)
    frame_a[::2, :, :a.shape[1]], frame_b[::2, :, :a.shape[1]] = A, B
    d2, r2 = ctx.phase_correlate(frame_a[::2, :, :a.shape[1]], frame_b[::2, :, :a.shape[1]])
    d1, r1 = ctx.phase_correlate(A, B)
    assert np.array_equal(d1, d2) and np.array_equal(r1, r2)
    assert ctx.phase_correlate(a.astype(np.float64), b.astype(np.float64)) == single
    u, v = pc.u8_pair()
    assert ctx.phase_correlate(u, v) == ctx.phase_correlate(u.astype(np.float32), v.astype(np.float32))


@pytest.mark.timeout(600)
def test_large_batch_is_chunked_bit_for_bit(ctx, to_cart):
    """two 4096 x 4096 pairs do not fit the 2 GB scratch bound together: the chunked batch equals the single calls, and the
    largest plane of the two-stage peak search agrees with the oracle"""
    A, B = pc.large_batch(to_cart)
    dxdy, resp = ctx.phase_correlate(A, B)
    for i in range(2):
        (dx, dy), r = ctx.phase_correlate(A[i], B[i])
        assert (dx, dy, r) == (dxdy[i, 0], dxdy[i, 1], resp[i]), i
        _check(f"4096x4096-pair-{i}", ((dx, dy), r), oracle.phaseCorrelate(A[i], B[i]))


@pytest.mark.timeout(600)
def test_fft_is_not_slower_than_the_direct_dft(ctx):
    """the five 2-D transforms of one phase correlation at the rotation prior's size (320 x 108: 108 rows of 320) through the FFT and
    through the direct DFTs the single-pair path used until this change, HIP events after warm runs, best of three; and the figures docs/KERNELS.md records at
    2025 x 2025 and 2048 x 2048 (printed, not asserted: there is no earlier number to hold them to)"""
    from radarslampy_amd import _ffi
    modes = (("five transforms", _ffi.TIME_FFT_FIVE), ("row pass", _ffi.TIME_FFT_ROWS), ("transpose", _ffi.TIME_FFT_TRANSPOSE),
             ("column pass", _ffi.TIME_FFT_COLS))
    fft = [ctx.time_fft2(108, 320, _ffi.TIME_FFT_FIVE, 50) for _ in range(3)]
    dft = [ctx.time_fft2(108, 320, _ffi.TIME_DFT_FIVE, 50) for _ in range(3)]
    print(f"108x320 five transforms: FFT {fft} ms, direct DFT {dft} ms")
    for label, what in modes[1:]:
        print(f"108x320 {label}: {[ctx.time_fft2(108, 320, what, 50) for _ in range(3)]} ms")
    for n in (2025, 2048):
        for label, what in modes:
            ms = [ctx.time_fft2(n, n, what, 20) for _ in range(3)]
            gbps = "" if what == _ffi.TIME_FFT_FIVE else f", {32.0 * n * n / (min(ms) * 1e-3) / 1e9:.0f} GB/s (two float64 planes read and written)"
            print(f"{n}x{n} {label}: {ms} ms{gbps}")
        side = 2024 if n == 2025 else n
        a = np.random.default_rng(0).random((side, side), dtype=np.float32)
        b = np.roll(a, (3, -7), axis=(0, 1))
        ctx.phase_correlate(a, b)
        import time
        ts = []
        for _ in range(5):
            t = time.perf_counter()
            ctx.phase_correlate(a, b)
            ts.append((time.perf_counter() - t) * 1e3)
        print(f"{side}x{side} one phase_correlate call (host to host, images in pageable memory): {ts} ms")
    assert min(fft) <= min(dft), (fft, dft)
    with pytest.raises(_ffi.RoamError):
        ctx.time_fft2(2048, 2048, _ffi.TIME_DFT_FIVE, 1)        # the direct form is refused above 131072 bins


def test_drop_in(ctx, to_cart):
    from radarslampy_amd import FMT
    cases = [c for c in pc.oracle_cases(to_cart) if c[1].shape == (108, 320) and c[3]]
    assert len(cases) >= 5
    for name, a, b, hanning in cases:
        got = FMT.getTranslationUsingPhaseCorrelation(a, b)
        deltas, response = got
        assert isinstance(got, tuple) and isinstance(deltas, tuple) and len(deltas) == 2
        assert all(type(v) is float for v in deltas) and type(response) is float
        assert got == ctx.phase_correlate(a, b), name


def test_argument_errors_on_the_device_side(ctx):
    """the C entry's own refusals (the Python wrapper checks the same things first)"""
    import ctypes as C
    from radarslampy_amd import _ffi
    a = np.zeros((8, 8), np.float32)
    out = np.zeros(2)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    call = lambda *args: ctx.lib.roam_phase_correlate_f32(ctx.h, *args)
    assert call(p(a), p(a), 1, 8, 8, 8, 64, 1, p(out), None) == _ffi.ROAM_OK
    assert call(None, p(a), 1, 8, 8, 8, 64, 1, p(out), None) == _ffi.ROAM_E_ARG
    assert call(p(a), None, 1, 8, 8, 8, 64, 1, p(out), None) == _ffi.ROAM_E_ARG
    assert call(p(a), p(a), 1, 8, 8, 8, 64, 1, None, None) == _ffi.ROAM_E_ARG
    assert call(p(a), p(a), 0, 8, 8, 8, 64, 1, p(out), None) == _ffi.ROAM_E_ARG
    assert call(p(a), p(a), 1, 1, 8, 8, 64, 1, p(out), None) == _ffi.ROAM_E_ARG
    assert call(p(a), p(a), 1, 8, 4097, 4097, 64, 1, p(out), None) == _ffi.ROAM_E_ARG
    assert call(p(a), p(a), 1, 8, 8, 7, 64, 1, p(out), None) == _ffi.ROAM_E_ARG
    assert call(p(a), p(a), 2, 4, 8, 8, 31, 1, p(out), None) == _ffi.ROAM_E_ARG
