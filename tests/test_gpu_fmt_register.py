"""GPU (-m gpu): the Fourier-Mellin registration in one device pass (roam_fmt_register_batch_f32, roam_engine_fmt_register;
csrc/fmt_register.hip and the correlations of csrc/phasecorr.hip, driven by csrc/fmt.hip) against its parts and against the all-CPU chain of
tests/fmt_register_cases.py (five shapes, four pairs each; the CPU test asserts a unique peak in both correlations of every pair).

  (a) columns 0-2 are fmt_rotation_batch's on the same input, bit for bit;
  (b) the target Cartesian images equal warp_polar_model's bit for bit, the turned sources warp_affine_model.rotateImg of the model's
      Cartesian image at degrees(the DEVICE's angle) bit for bit (a last-bit difference in the angle may legitimately flip a
      1/1024-px rounding, so the model is given the angle the device used);
  (c) dx, dy, trans_response against oracle.phaseCorrelate of those two images within the bounds of
      tests/test_gpu_phase_correlate.py (6.6e-11 px, 4.0e-12 relative; docs/PARITY.md);
  (d) end to end against the chain with the oracle's own angle: fmt_register_cases.SENS_* (ten times the effect of +- 1e-14 rad on the
      chain: measured 0) plus the bounds of (c);
  (e) one pair's six numbers are the same bits in any batch, position and chunk;
  (f) the engine on resident u8 records equals the batch call on the decoded float32 images, bit for bit, and leaves a step's results
      alone;
  (g) FMT.getTransformUsingFMT is the stage call."""
import math

import numpy as np
import pytest

import fmt_register_cases as cases
import oracle
import warp_affine_model as wam
from gen_inputs import ENGINE_LAYOUTS, layout_sequence

pytestmark = pytest.mark.gpu

TOL_PX = cases.SENS_PX + cases.PC_TOL_PX
TOL_RESPONSE_REL = cases.SENS_RESPONSE_REL + cases.PC_TOL_RESPONSE_REL


@pytest.fixture(scope="module")
def ctx():
    from radarslampy_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


_device = {}


def device(ctx, case):
    """the case's four pairs through the device once -> (out (4, 6), images (8, S, S))"""
    if case not in _device:
        _, clip_px, ds, cds, Rc, _ = cases.CASES[case]
        A, B = cases.batch(case)
        _device[case] = ctx.fmt_register_batch(A, B, clip_px=clip_px, downsample=ds, cart_downsample=cds, want_images=True)
    return _device[case]


@pytest.mark.parametrize("case", sorted(cases.CASES))
def test_parts_and_chain(ctx, case):
    _, clip_px, ds, cds, Rc, _ = cases.CASES[case]
    A, B = cases.batch(case)
    out, imgs = device(ctx, case)
    assert out.shape == (4, 6) and out.dtype == np.float64 and imgs.shape == (8, 2 * Rc, 2 * Rc) and imgs.dtype == np.float32
    # (a)
    rot = ctx.fmt_rotation_batch(A, B, clip_px=clip_px, downsample=ds)
    assert np.array_equal(out[:, :3], rot), (case, out[:, :3], rot)
    want = cases.chain_results(case)
    for i in range(4):
        w = want[i]
        # (b)
        assert np.array_equal(imgs[4 + i], w["tgt_cart"]), (case, "target", i, np.abs(imgs[4 + i] - w["tgt_cart"]).max())
        model_rot = wam.rotateImg(w["src_cart"], math.degrees(out[i, 0]))
        assert np.array_equal(imgs[i], model_rot), (case, "turned source", i, np.abs(imgs[i] - model_rot).max())
        # (c)
        (dx, dy), resp = oracle.phaseCorrelate(imgs[i], imgs[4 + i])
        print(f"case {case} pair {i}: device {tuple(out[i])}; phaseCorrelate of its images ({dx}, {dy}), {resp}: differences "
              f"{abs(out[i, 3] - dx):.3g} px, {abs(out[i, 4] - dy):.3g} px, {abs(out[i, 5] - resp) / abs(resp):.3g} relative")
        assert abs(out[i, 3] - dx) <= cases.PC_TOL_PX and abs(out[i, 4] - dy) <= cases.PC_TOL_PX, (case, i, out[i], dx, dy)
        assert abs(out[i, 5] - resp) <= cases.PC_TOL_RESPONSE_REL * abs(resp), (case, i, out[i], resp)
        # (d)
        o = w["out6"]
        print(f"case {case} pair {i}: chain {tuple(o)}: differences angle {abs(out[i, 0] - o[0]):.3g} rad, {abs(out[i, 3] - o[3]):.3g} px, "
              f"{abs(out[i, 4] - o[4]):.3g} px, {abs(out[i, 5] - o[5]) / abs(o[5]):.3g} relative")
        assert abs(out[i, 0] - o[0]) <= 1e-5 and abs(out[i, 1] - o[1]) <= 1e-5 and abs(out[i, 2] - o[2]) <= 1e-4 * max(1.0, abs(o[2]))
        assert abs(out[i, 3] - o[3]) <= TOL_PX and abs(out[i, 4] - o[4]) <= TOL_PX, (case, i, out[i], o)
        assert abs(out[i, 5] - o[5]) <= TOL_RESPONSE_REL * abs(o[5]), (case, i, out[i], o)
    assert np.array_equal(ctx.fmt_register_batch(A, B, clip_px=clip_px, downsample=ds, cart_downsample=cds), out)    # the images are optional
    if case == "strided7":                                                    # the strided view and its contiguous copy
        assert np.array_equal(ctx.fmt_register_batch(np.ascontiguousarray(A), np.ascontiguousarray(B), clip_px=clip_px, downsample=ds,
                                                     cart_downsample=cds), out)


def test_cart_downsample_2_is_the_live_warp(ctx):
    """at downsampleFactor 2 parseData.convertPolarImageToCartesian runs warp.hip's kernel, not warppolar.hip's: the same image"""
    from radarslampy_amd import parseData
    A, B = cases.batch("tex1")
    _, imgs = ctx.fmt_register_batch(A[1], B[1], clip_px=0, downsample=2, cart_downsample=2, want_images=True)
    assert np.array_equal(imgs[1], parseData.convertPolarImageToCartesian(B[1], downsampleFactor=2))
    assert np.array_equal(imgs[1], cases.cart(B[1], 2))


@pytest.mark.parametrize("case", ["live20", "tex3"])
def test_result_does_not_depend_on_batch_position_or_chunk(ctx, case, monkeypatch):
    """(e): n = 7 with the chunk forced to 3 pairs (chunks of 3, 3, 1) against one call per pair"""
    _, clip_px, ds, cds, Rc, _ = cases.CASES[case]
    A, B = cases.batch(case)
    kw = dict(clip_px=clip_px, downsample=ds, cart_downsample=cds)
    out, imgs = device(ctx, case)
    for i in range(4):
        o1, i1 = ctx.fmt_register_batch(A[i], B[i], want_images=True, **kw)
        assert o1.shape == (1, 6) and np.array_equal(o1[0], out[i]), (case, i, o1, out[i])
        assert np.array_equal(i1[0], imgs[i]) and np.array_equal(i1[1], imgs[4 + i])
    sel = np.array([3, 1, 2, 0, 2, 3, 1])
    monkeypatch.setenv("ROAM_FMT_BATCH_CHUNK", "3")
    o7, i7 = ctx.fmt_register_batch(A[sel], B[sel], want_images=True, **kw)
    assert o7.shape == (7, 6) and np.array_equal(o7, out[sel]), (o7, out[sel])
    assert np.array_equal(i7[:7], imgs[sel]) and np.array_equal(i7[7:], imgs[4 + sel])
    monkeypatch.setenv("ROAM_FMT_BATCH_CHUNK", "1")
    assert np.array_equal(ctx.fmt_register_batch(A, B, **kw), out)
    monkeypatch.delenv("ROAM_FMT_BATCH_CHUNK")
    assert np.array_equal(ctx.fmt_register_batch(A[sel], B[sel], **kw), out[sel])
    assert np.array_equal(ctx.fmt_rotation_batch(A, B, clip_px=clip_px, downsample=ds), out[:, :3])     # the rotation pass after this one


def test_drop_in_name(ctx):
    """(g)"""
    from radarslampy_amd import _ffi
    from radarslampy_amd.FMT import getTransformUsingFMT
    A, B = cases.batch("live20")
    out = _ffi.default_context().fmt_register_batch(A, B)
    assert np.array_equal(out, device(ctx, "live20")[0])
    ang, dxdy, sc, rr, tr = getTransformUsingFMT(A, B)
    assert ang.shape == sc.shape == rr.shape == tr.shape == (4,) and dxdy.shape == (4, 2)
    assert np.array_equal(np.column_stack([ang, sc, rr, dxdy, tr]), out)
    one = getTransformUsingFMT(A[1], B[1])
    assert one == (out[1, 0], (out[1, 3], out[1, 4]), out[1, 1], out[1, 2], out[1, 5]) and all(isinstance(v, float) for v in one[2:])
    o5 = getTransformUsingFMT(A[1], B[1], cartDownsampleFactor=5)
    assert np.array_equal([o5[0], o5[2], o5[3], o5[1][0], o5[1][1], o5[4]], device(ctx, "live5")[0][1])


ENGINE_CASES = [((2025, 400, 3779, 11), 1012, 10, 20), ((497, 399, 504, 5), 497, 7, 7)]


@pytest.mark.parametrize("layout,clip_px,ds,cds", ENGINE_CASES, ids=["oxford", "clip497_rows399"])
def test_engine_on_resident_records(ctx, layout, clip_px, ds, cds):
    """(f): roam_engine_fmt_register on pool records against the batch call on the host-decoded images
    (extractDataFromRadarImage's arithmetic: float32(u8) / 255), before a step and right after one is enqueued; the step's results
    equal those of an engine that never made the call.  The small layout uploads its records asynchronously and calls at once."""
    from radarslampy_amd import _ffi
    from radarslampy_amd.engine import Engine
    assert layout in ENGINE_LAYOUTS
    clip, rows, stride, off = layout
    recs, poses = layout_sequence(clip + 1, 4, rows, clip, stride, off, n_movers=6)
    polar = np.stack([r[:, off:off + clip].astype(np.float32) / np.float32(255.) for r in recs])
    if clip == 2025:
        assert np.array_equal(polar[0], oracle.extractDataFromRadarImage(recs[0])[0])
    prev, curr = [0, 0, 2], [1, 0, 3]
    kw = dict(clip_px=clip_px, downsample=ds, cart_downsample=cds)
    want = ctx.fmt_register_batch(polar[prev], polar[curr], **kw)
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
            got = eng.fmt_register(prev, curr, **kw)
            assert got.shape == (3, 6) and np.array_equal(got, want), (got, want)
        eng.init_lane(0, 0, feat, poses[0])
        eng.step([1])
        if call:
            got = eng.fmt_register(prev, curr, **kw)
            assert np.array_equal(got, want), (got, want)
            assert np.array_equal(got[:, :3], eng.fmt_rotation(prev, curr, clip_px=clip_px, downsample=ds))
            with pytest.raises(_ffi.RoamError):
                c.check(c.lib.roam_engine_fmt_register(c.h, 1, _ffi._ptr(np.array([4], np.int32)), _ffi._ptr(np.array([0], np.int32)),
                                                       clip_px, ds, cds, _ffi._ptr(np.empty(6))))
        results.append((eng.results_array().tobytes(), eng.lane_features(0)))
        eng.synchronize()
        if asynchronous:
            c.host_free(pinned)
        eng.close()
        c.close()
    assert results[0][0] == results[1][0] and np.array_equal(results[0][1], results[1][1])
