"""GPU (-m gpu): the batched Fourier-Mellin rotation prior (roam_fmt_rotation_batch_f32, roam_engine_fmt_rotation; csrc/fmt_batch.hip
and the correlation of csrc/phasecorr.hip, driven by csrc/fmt.hip) against the oracle's restatement of FMT.getRotationUsingFMT.  The inputs and the oracle's
results are tests/fmt_batch_cases.py (four shapes, four pairs each; the CPU test asserts a unique correlation peak for every pair).

Bounds: the angle to 1e-5 rad, the scale to 1e-5 and the response to 1e-4 max(1, |response|) - the bounds of
test_fmt_rotation_matches_oracle for the same quantities; the log-polar images before the window bit for bit, as roam_warp_polar_f32
gives them (docs/PARITY.md); the results of one pair in batches of different size and in different chunks bit for bit; the
engine's results on resident u8 records bit for bit equal to the batch call on the host-decoded float32 images."""
import numpy as np
import pytest

import fmt_batch_cases as cases
import oracle
from gen_inputs import ENGINE_LAYOUTS, layout_sequence

pytestmark = pytest.mark.gpu

ANG_TOL, SCALE_TOL, RESP_TOL = 1e-5, 1e-5, 1e-4


@pytest.fixture(scope="module")
def ctx():
    from radarslampy_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


def _check(tag, got, want):
    print(f"{tag}: got {tuple(got)}, oracle {tuple(want)}, differences {tuple(np.abs(np.asarray(got) - np.asarray(want)))}")
    assert abs(got[0] - want[0]) <= ANG_TOL, (tag, got, want)
    assert abs(got[1] - want[1]) <= SCALE_TOL, (tag, got, want)
    assert abs(got[2] - want[2]) <= RESP_TOL * max(1.0, abs(want[2])), (tag, got, want)


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_batch_matches_oracle_and_logpolar_is_exact(ctx, case):
    clip_px, ds, R, (dh, dw), _ = cases.CASES[case]
    A, B = cases.batch(case)
    want = cases.oracle_results(case)
    out, lp = ctx.fmt_rotation_batch(A, B, clip_px=clip_px, downsample=ds, want_logpolar=True)
    assert out.shape == (4, 3) and lp.shape == (8, dh, dw) and lp.dtype == np.float32
    for i in range(4):
        assert np.array_equal(lp[i], want["lp_src"][i]), (case, "source", i, np.abs(lp[i] - want["lp_src"][i]).max())
        assert np.array_equal(lp[4 + i], want["lp_tgt"][i]), (case, "target", i, np.abs(lp[4 + i] - want["lp_tgt"][i]).max())
    for i in range(4):
        _check(f"case {case} pair {i}", out[i], want["out3"][i])
    assert np.array_equal(ctx.fmt_rotation_batch(A, B, clip_px=clip_px, downsample=ds), out)     # the images are optional
    if case == "a":
        for i in range(4):                                                    # the single-pair entry: n = 1 of the same pass
            assert np.array_equal(out[i], ctx.fmt_rotation(A[i], B[i], clip_px=clip_px, downsample=ds))
        # known answer: the scan turned by k azimuth rows
        assert abs(out[2, 0] + 7 * 2 * np.pi / 400) < 5e-3
    if case == "c":                                                           # the strided view and its contiguous copy
        assert np.array_equal(ctx.fmt_rotation_batch(np.ascontiguousarray(A), np.ascontiguousarray(B), clip_px=clip_px, downsample=ds), out)


def test_large_plane_through_the_fft(ctx):
    """case d: 1012 / 2 -> a 1600 x 512 plane, a size only the FFT makes practical"""
    clip_px, ds, R, _, _ = cases.CASES["d"]
    A, B = cases.batch("d")
    out = ctx.fmt_rotation_batch(A, B, clip_px=clip_px, downsample=ds)
    for i in range(4):
        _check(f"case d pair {i}", out[i], cases.oracle_results("d")["out3"][i])
    assert abs(out[2, 0] + 7 * 2 * np.pi / 400) < 5e-3


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_result_does_not_depend_on_the_batch(ctx, case):
    clip_px, ds, _, _, _ = cases.CASES[case]
    A, B = cases.batch(case)
    out, lp = ctx.fmt_rotation_batch(A, B, clip_px=clip_px, downsample=ds, want_logpolar=True)
    for i in range(4):
        o1, l1 = ctx.fmt_rotation_batch(A[i], B[i], clip_px=clip_px, downsample=ds, want_logpolar=True)
        assert o1.shape == (1, 3) and np.array_equal(o1[0], out[i]), (case, i, o1, out[i])
        assert np.array_equal(l1[0], lp[i]) and np.array_equal(l1[1], lp[4 + i])


def _single_vs_batch_pairs():
    rng = np.random.default_rng(11)
    yield "b", cases.batch("b"), cases.CASES["b"][:2]
    yield "c, contiguous", tuple(np.ascontiguousarray(x) for x in cases.batch("c")), cases.CASES["c"][:2]
    # R = 4 = ROAM_FMT_MIN_R, rows at their minimum; no oracle here: nobody has checked that this pair's correlation peak is unique
    yield "8 x 8", (rng.random((1, 8, 8), dtype=np.float32), rng.random((1, 8, 8), dtype=np.float32)), (0, 2)


def test_single_pair_entry_is_the_batch_of_one(ctx):
    """roam_fmt_rotation against roam_fmt_rotation_batch_f32 at n = 1 on the same pair, bit for bit (case a: above)"""
    for tag, (A, B), (clip_px, ds) in _single_vs_batch_pairs():
        i = min(1, len(A) - 1)
        want = ctx.fmt_rotation_batch(A[i], B[i], clip_px=clip_px, downsample=ds)
        got = ctx.fmt_rotation(A[i], B[i], clip_px=clip_px, downsample=ds)
        print(f"{tag}: single {got}, batch of one {tuple(want[0])}")
        assert want.shape == (1, 3) and np.array_equal(want[0], got), (tag, got, want)


def test_single_pair_entry_argument_errors_on_the_device_side(ctx):
    """the C entry's own refusals, before any device call; scale and response are optional"""
    import ctypes as C
    from radarslampy_amd import _ffi
    a = np.random.default_rng(12).random((8, 8), dtype=np.float32)
    ang = C.c_double(0)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    call = lambda *args: ctx.lib.roam_fmt_rotation(ctx.h, *args)
    assert call(p(a), p(a), 8, 8, 0, 2, C.byref(ang), None, None) == _ffi.ROAM_OK
    assert call(None, p(a), 8, 8, 0, 2, C.byref(ang), None, None) == _ffi.ROAM_E_ARG
    assert call(p(a), None, 8, 8, 0, 2, C.byref(ang), None, None) == _ffi.ROAM_E_ARG
    assert call(p(a), p(a), 8, 8, 0, 2, None, None, None) == _ffi.ROAM_E_ARG
    assert call(p(a), p(a), 7, 8, 0, 2, C.byref(ang), None, None) == _ffi.ROAM_E_ARG
    assert call(p(a), p(a), 8, 1, 0, 1, C.byref(ang), None, None) == _ffi.ROAM_E_ARG
    assert call(p(a), p(a), 8, 8, 0, 0, C.byref(ang), None, None) == _ffi.ROAM_E_ARG
    assert call(p(a), p(a), 8, 8, 6, 2, C.byref(ang), None, None) == _ffi.ROAM_E_ARG            # R = 3
    assert call(p(a), p(a), 8, 1304, 0, 1, C.byref(ang), None, None) == _ffi.ROAM_E_ARG         # R = 1304: refused before a is read
    assert b"bad argument" in ctx.lib.roam_last_error(ctx.h)


def test_chunked_batch_equals_its_originals(ctx, monkeypatch):
    """37 repeats of 3 distinct pairs with the chunk forced to 16 pairs (three chunks, the last of 5)"""
    clip_px, ds, _, _, _ = cases.CASES["b"]
    A, B = cases.batch("b")
    sel = np.arange(37) % 3 + 1
    orig, lp0 = ctx.fmt_rotation_batch(A, B, clip_px=clip_px, downsample=ds, want_logpolar=True)
    monkeypatch.setenv("ROAM_FMT_BATCH_CHUNK", "16")
    out, lp = ctx.fmt_rotation_batch(A[sel], B[sel], clip_px=clip_px, downsample=ds, want_logpolar=True)
    assert out.shape == (37, 3) and np.array_equal(out, orig[sel])
    assert np.array_equal(lp[:37], lp0[sel]) and np.array_equal(lp[37:], lp0[4 + sel])
    monkeypatch.setenv("ROAM_FMT_BATCH_CHUNK", "1")
    assert np.array_equal(ctx.fmt_rotation_batch(A, B, clip_px=clip_px, downsample=ds), orig)
    monkeypatch.delenv("ROAM_FMT_BATCH_CHUNK")
    assert np.array_equal(ctx.fmt_rotation_batch(A[sel], B[sel], clip_px=clip_px, downsample=ds), orig[sel])
    # the live shape in chunks of 3
    clip_px, ds, _, _, _ = cases.CASES["a"]
    A, B = cases.batch("a")
    orig = ctx.fmt_rotation_batch(A, B, clip_px=clip_px, downsample=ds)
    monkeypatch.setenv("ROAM_FMT_BATCH_CHUNK", "3")
    sel = np.arange(8) % 3 + 1
    assert np.array_equal(ctx.fmt_rotation_batch(A[sel], B[sel], clip_px=clip_px, downsample=ds), orig[sel])


def test_drop_in_name(ctx):
    from radarslampy_amd import _ffi
    from radarslampy_amd.FMT import getRotationUsingFMT
    A, B = cases.batch("a")
    ang, sc, resp = getRotationUsingFMT(A, B)
    out = _ffi.default_context().fmt_rotation_batch(A, B)
    assert ang.shape == sc.shape == resp.shape == (4,)
    assert np.array_equal(ang, out[:, 0]) and np.array_equal(sc, out[:, 1]) and np.array_equal(resp, out[:, 2])
    assert np.array_equal(out, ctx.fmt_rotation_batch(A, B))
    assert getRotationUsingFMT(A[1], B[1]) == ctx.fmt_rotation(A[1], B[1])    # 2-D input: the single-pair entry, as before


ENGINE_CASES = [((2025, 400, 3779, 11), 1012, 10), ((497, 399, 504, 5), 497, 7)]


@pytest.mark.parametrize("layout,clip_px,ds", ENGINE_CASES, ids=["oxford", "clip497_rows399"])
def test_engine_on_resident_records(ctx, layout, clip_px, ds):
    """roam_engine_fmt_rotation on pool records against the batch call on the host-decoded images, before a step and right after one
    is enqueued; the step's results equal those of an engine that never made the call.  The small layout uploads its records
    asynchronously and calls at once: the call waits for the uploads itself."""
    from radarslampy_amd import _ffi
    from radarslampy_amd.engine import Engine
    assert layout in ENGINE_LAYOUTS
    clip, rows, stride, off = layout
    recs, poses = layout_sequence(clip + 1, 4, rows, clip, stride, off, n_movers=6)
    polar = np.stack([r[:, off:off + clip].astype(np.float32) / np.float32(255.) for r in recs])
    prev, curr = [0, 0, 2], [1, 0, 3]
    want = ctx.fmt_rotation_batch(polar[prev], polar[curr], clip_px=clip_px, downsample=ds)
    cart = oracle.convertPolarImageToCartesian(polar[0])
    ys, xs = np.unravel_index(np.argsort(cart, axis=None)[-3600:][::30], cart.shape)
    feat = np.stack([xs, ys], axis=1).astype(np.float32)                      # 120 of the brightest pixels: any trackable points do
    asynchronous = clip != 2025
    results = []
    for call in (True, False):
        c = _ffi.Context(0)
        eng = Engine(1, 4, ctx=c, rows=rows, stride=stride, payload_off=off, clip=clip, retrack_on_device=False)
        if asynchronous:
            pinned = c.host_alloc((4, rows, stride))
            for t in range(4):
                pinned[t] = recs[t]
            eng.upload_scans_async(0, pinned, n=4)
        else:
            for t in range(4):
                eng.upload_scan(t, recs[t])
        if call:
            got = eng.fmt_rotation(prev, curr, clip_px=clip_px, downsample=ds)
            assert got.shape == (3, 3) and np.array_equal(got, want), (got, want)
        eng.init_lane(0, 0, feat, poses[0])
        eng.step([1])
        if call:
            got = eng.fmt_rotation(prev, curr, clip_px=clip_px, downsample=ds)
            assert np.array_equal(got, want), (got, want)
            assert np.array_equal(eng.fmt_rotation([3], [2], clip_px=0, downsample=ds),
                                  ctx.fmt_rotation_batch(polar[3], polar[2], clip_px=0, downsample=ds))      # clip_px <= 0: the engine's clip
            with pytest.raises(_ffi.RoamError):
                c.check(c.lib.roam_engine_fmt_rotation(c.h, 1, _ffi._ptr(np.array([4], np.int32)), _ffi._ptr(np.array([0], np.int32)),
                                                       clip_px, ds, _ffi._ptr(np.empty(3))))
        results.append((eng.results_array().tobytes(), eng.lane_features(0)))
        eng.synchronize()
        if asynchronous:
            c.host_free(pinned)
        eng.close()
        c.close()
    assert results[0][0] == results[1][0] and np.array_equal(results[0][1], results[1][1])
