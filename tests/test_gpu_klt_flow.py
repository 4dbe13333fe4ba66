"""GPU (-m gpu): the standalone tracker with an initial flow (roam_klt_track_u8_flow / _f32_flow) against the NumPy model of
tests/klt_flow_model.py, bit for bit: points, status and err, through both entries, for every kind of guess, at the block sizes around
one wavefront of features; and the large-rotation pair, where the seed is what keeps the features."""
import numpy as np
import pytest

import klt_flow_cases as C
import klt_flow_model as M
import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from radarslampy_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("hw", C.SHAPES, ids=lambda s: "%dx%d" % s)
def test_seeded_tracker_equals_model(ctx, hw):
    a8, b8 = C.image_pair(hw)
    af, bf = ((x.astype(np.float32) + np.float32(0.5)) / np.float32(255.) for x in (a8, b8))    # (img * 255).astype(u8) gives the bytes back
    assert np.array_equal(oracle.quantize_u8(af), a8) and np.array_equal(oracle.quantize_u8(bf), b8)    # the f32 entry sees the same bytes
    pp, npyr = M.build_pyramid(a8), M.build_pyramid(b8)
    moved = lost_outside = 0
    for K in C.KS:
        pts = C.points(hw, K)
        old = [ctx.klt_track(a, b, pts) for a, b in ((a8, b8), (af, bf))]
        for name, g in C.guesses(hw, pts).items():
            want = M.track_on_pyramids(pp, npyr, pts, g)
            for (a, b), unseeded in zip(((a8, b8), (af, bf)), old):
                got = ctx.klt_track(a, b, pts, g)
                tag = (hw, K, name, a.dtype)
                assert np.array_equal(got[1], want[1]), (tag, int((got[1] != want[1]).sum()))
                assert np.array_equal(got[0], want[0]), (tag, float(np.abs(got[0] - want[0]).max()))
                assert np.array_equal(got[2], want[2]), tag
                if name == "same":          # a seed equal to the points is the unseeded entry
                    assert all(np.array_equal(x, y) for x, y in zip(got, unseeded)), tag
            if K == 65 and name == "fraction":
                moved = int((want[0] != old[0][0]).any(axis=1).sum())
            if K == 65 and name == "outside":
                lost_outside = int((want[1] == 0).sum()) - int((old[0][1] == 0).sum())
    # not vacuous: the seed changes results, and guesses outside the image lose features the unseeded call keeps
    assert moved >= 10 and lost_outside >= 5, (moved, lost_outside)


@pytest.mark.parametrize("hw", C.SHAPES, ids=lambda s: "%dx%d" % s)
def test_null_seed_through_new_entries_is_the_old_entry(ctx, hw):
    from radarslampy_amd import _ffi
    a8, b8 = C.image_pair(hw)
    af, bf = ((x.astype(np.float32) + np.float32(0.5)) / np.float32(255.) for x in (a8, b8))    # (img * 255).astype(u8) gives the bytes back
    h, w = hw
    for K in C.KS:
        pts = C.points(hw, K)
        for a, b, fn in ((a8, b8, ctx.lib.roam_klt_track_u8_flow), (af, bf, ctx.lib.roam_klt_track_f32_flow)):
            want = ctx.klt_track(a, b, pts)
            nxt, st, err = np.zeros((K, 2), np.float32), np.zeros(K, np.uint8), np.zeros(K, np.float32)
            ctx.check(fn(ctx.h, _ffi._ptr(a), _ffi._ptr(b), w, h, _ffi._ptr(pts), None, K, _ffi._ptr(nxt), _ffi._ptr(st), _ffi._ptr(err)))
            assert np.array_equal(nxt, want[0]) and np.array_equal(st, want[1].ravel()) and np.array_equal(err, want[2].ravel()), (hw, K, a.dtype)
            # what the Python wrapper refuses, the library refuses too
            bad = pts.copy()
            bad[K // 2, 0] = np.inf
            assert fn(ctx.h, _ffi._ptr(a), _ffi._ptr(b), w, h, _ffi._ptr(pts), _ffi._ptr(bad), K, _ffi._ptr(nxt), _ffi._ptr(st),
                      _ffi._ptr(err)) == _ffi.ROAM_E_ARG
            bad[K // 2, 0] = -2.0 ** 21
            assert fn(ctx.h, _ffi._ptr(a), _ffi._ptr(b), w, h, _ffi._ptr(pts), _ffi._ptr(bad), K, _ffi._ptr(nxt), _ffi._ptr(st),
                      _ffi._ptr(err)) == _ffi.ROAM_E_ARG


def test_large_rotation_pair_counts_equal_the_model(ctx):
    r = C.rotation_pair()
    want_unseeded, want_seeded = C.rotation_counts()
    _, s0, e0 = ctx.klt_track(r["prev"], r["next"], r["feats"])
    _, s1, e1 = ctx.klt_track(r["prev"], r["next"], r["feats"], M.apply_affine(r["affine"], r["feats"]))
    got = (M.count_good(s0, e0), M.count_good(s1, e1))
    print("large rotation on the device: unseeded", got[0], "seeded", got[1], "of", len(r["feats"]))
    assert got == (want_unseeded, want_seeded)
    assert got[0] < len(r["feats"]) / 2 < got[1]
