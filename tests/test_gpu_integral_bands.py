"""GPU (-m gpu): the one-sweep integral kernel (csrc/retrack_integral.hip, rt_integral_kernel: phases of 64 rows x 64 columns, four
stacked column waves of 16 rows each and one row wave) against NumPy: the float64 scratch image of a detection equals
cumsum(cumsum(cart, 0), 1) of the oracle's Cartesian image bit for bit at every pixel inside the maximum range (tiles the determinant
kernel never reads are not written), and the features detected from it are the oracle's.  The image sizes are those at which the
band / quarter / tile geometry takes another path:
   132   two bands + 4 rows: only column wave 0 has live rows in the last band; the last tile has 4 columns (the chain's scalar tail)
   300   44 rows / 44 columns left over: a partly live third quarter
   336   the remainder is exactly one quarter
   384   no partial band, no partial tile
   497   W = 496: remainder 48
   2025  the live shape (W = 2024, remainder 40), synthetic Oxford records of three sequences
208 lanes: a chunk needs at least 200 detections for the one-sweep kernel (fewer take the two-pass kernels)."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu
P = 208


def _cart(payload):
    return oracle.convertPolarImageToCartesian(payload.astype(np.float32) / np.float32(255.))


def _inside(rows, clip):
    """pixels that sample the scan at all: the warp of an all-ones scan is non-zero there"""
    return oracle.convertPolarImageToCartesian(np.ones((rows, clip), np.float32)) > 0


def _check(eng, payloads, scan_of_lane, next_of_lane, lanes):
    """payloads[t]: the (rows, clip) u8 payload of pool scan t; lane b is initialised on scan_of_lane[b] and steps to next_of_lane[b]"""
    rows, clip = payloads[0].shape
    carts = {}

    def cart(t):
        if t not in carts:
            carts[t] = _cart(payloads[t])
        return carts[t]

    eng.init_lanes_detect(0, scan_of_lane, np.zeros((P, 3)))
    feats = {}
    for b in lanes:
        t = scan_of_lane[b]
        if t not in feats:
            feats[t] = oracle.append_dedupe(np.empty((0, 2)), oracle.getFeatures(cart(t))[0])
        assert len(feats[t]) > 0 and np.array_equal(eng.lane_features(b), feats[t]), b
    eng.step(next_of_lane)
    inside = _inside(rows, clip)
    assert inside.any()
    for s in lanes:
        S = eng.debug_detect(False, P, s_slot=s)[3]
        x = cart(next_of_lane[s]).astype(np.float64)
        want = np.cumsum(np.cumsum(x, 0), 1)
        bad = (S != want) & inside
        assert not bad.any(), (s, int(bad.sum()), np.argwhere(bad)[:4].tolist())


@pytest.mark.parametrize("clip", [132, 300, 336, 384, 497])
def test_scratch_image_and_features_on_sizes_that_cut_bands_quarters_and_tiles(clip):
    from radarslampy_amd import _ffi
    from radarslampy_amd.engine import Engine
    rng = np.random.default_rng(clip)
    pay = (rng.random((400, clip)) * 12).astype(np.uint8)
    for _ in range(80):
        a, r = int(rng.integers(0, 400)), int(rng.integers(20, clip - 5))
        pay[max(0, a - 3):a + 3, max(0, r - 3):r + 3] = rng.integers(150, 255)
    pays = [pay, np.ascontiguousarray(pay[::-1])]
    ctx = _ffi.Context(0)
    eng = Engine(P, 2, ctx=ctx, rows=400, stride=clip, payload_off=0, clip=clip, retrack_on_device=True, retrack_slots=P)
    for t in range(2):
        eng.upload_scan(t, pays[t])
    _check(eng, pays, [b % 2 for b in range(P)], [(b + 1) % 2 for b in range(P)], (0, 1, P - 1))
    eng.close()
    ctx.close()


def test_scratch_image_and_features_on_the_live_shape():
    from radarslampy_amd import _ffi, synth
    from radarslampy_amd.engine import Engine
    recs = []
    for seed in (41, 42, 43):
        recs += list(synth.make_sequence(seed, 2, n_movers=6, distortion=True)[0])
    pays = [np.ascontiguousarray(r[:, 11:11 + 2025]) for r in recs]
    ctx = _ffi.Context(0)
    eng = Engine(P, 6, ctx=ctx, retrack_on_device=True, retrack_slots=P)
    for t in range(6):
        eng.upload_scan(t, recs[t])
    _check(eng, pays, [2 * (b % 3) for b in range(P)], [2 * (b % 3) + 1 for b in range(P)], (0, P - 1))
    eng.close()
    ctx.close()
