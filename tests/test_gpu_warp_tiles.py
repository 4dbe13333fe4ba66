"""GPU (-m gpu): warp_gather_kernel (radarslampy_amd/csrc/warp.hip) against the oracle's warp on EVERY lane of a batch, at the small
geometries of tests/warp_tile_cases.py that between them reach every tile class of the kernel (dark / direct / box, the clamp columns
past the last range bin, boxes wider than 64 columns and taller than 16 rows, wrapped rows, every pass size and fill unit, partial lane
groups, the one-lane launch of init_lane and the batched launch with a lane -> scan table; tests/test_warp_tiles_cpu.py holds the proof
that they do).  Lanes carry no features: the step's tracker has nothing to do and the test reads level 0 of every lane's pyramid.  A
mismatch is reported with the lane, its record and the tile class of the first differing pixel."""
import time

import numpy as np
import pytest

import oracle
import warp_tile_cases as wt
from gen_inputs import layout_sequence

pytestmark = pytest.mark.gpu

_T0 = time.perf_counter()


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    yield
    print("\ntests/test_gpu_warp_tiles.py: %.1f s wall" % (time.perf_counter() - _T0))


def _engine(ctx, B, geometry, **kw):
    from radarslampy_amd.engine import Engine
    rows, clip, stride, off = geometry
    return Engine(B, 6, ctx=ctx, rows=rows, stride=stride, payload_off=off, clip=clip, motion_distortion=False,
                  peaks_cap=rows * clip, **kw)


def _check_lanes(eng, geometry, lanes, lane_record, images, what, names=wt.RECORD_NAMES):
    """level 0 of every listed lane equals the image of its record"""
    for b in lanes:
        got, want = eng.lane_image(b, 0), images[lane_record[b]]
        if not np.array_equal(got, want):
            ys, xs = np.nonzero(got != want)
            y, x = int(ys[0]), int(xs[0])
            also = [names[k] for k in range(len(images)) if np.array_equal(got, images[k])]
            pytest.fail("%s, %s: lane %d (group %d, lane %d of it), record %d (%s): %d pixels differ, first at (y=%d, x=%d): got %d, want %d; %s%s"
                        % (wt.geometry_id(geometry), what, b, b // wt.WG_LB, b % wt.WG_LB, lane_record[b],
                           names[lane_record[b]], len(ys), y, x, got[y, x], want[y, x],
                           wt.describe_pixel(geometry, y, x), "; the lane holds the image of " + "/".join(also) if also else ""))


def _run_batch(geometry, B):
    """init_lane (the one-lane launch: no lane table, lane stride 0, every destination offset) with the first map, a step to the
    second map, a step back to the first: every lane, every time"""
    from radarslampy_amd import _ffi
    images = wt.expected_images(geometry)
    first, second = wt.lane_maps(B)
    ctx = _ffi.Context(0)
    eng = _engine(ctx, B, geometry)
    try:
        for k, rec in enumerate(wt.records(geometry)):
            eng.upload_scan(k, rec)
        none = np.empty((0, 2), np.float32)
        for b in range(B):
            eng.init_lane(b, int(first[b]), none, np.zeros(3))
        _check_lanes(eng, geometry, range(B), first, images, "after init_lane")
        eng.step(second)
        _check_lanes(eng, geometry, range(B), second, images, "after the step to the second map")
        eng.step(first)                 # nothing stale, and the dark tiles of this pyramid buffer are still zero
        _check_lanes(eng, geometry, range(B), first, images, "after the step back to the first map")
        res = eng.results()
        assert all(r["n_tracked"] == 0 and r["n_inliers"] == 0 for r in res)
    finally:
        eng.close()
        ctx.close()


@pytest.mark.parametrize("geometry", wt.GEOMETRIES, ids=wt.geometry_id)
def test_every_lane_of_a_batch(geometry):
    _run_batch(geometry, wt.BATCH)


@pytest.mark.parametrize("geometry", wt.PARTIAL_GEOMETRIES, ids=wt.geometry_id)
@pytest.mark.parametrize("B", wt.PARTIAL_BATCHES)
def test_partial_groups(B, geometry):
    _run_batch(geometry, B)


def test_batched_first_detection_offsets():
    """roam_engine_init_lanes_detect warps n lanes from lane0 on in one launch (lane i of the launch reads record pool_idx[i] and writes
    lane lane0 + i): lanes 5 ... 44 of 70 take their records' images, the lanes before and after keep what they had"""
    from radarslampy_amd import _ffi
    from radarslampy_amd.engine import Engine
    geometry = wt.GEOMETRIES[3]
    rows, clip, stride, off = geometry
    B, lane0, n = wt.BATCH, 5, 40
    recs, poses = layout_sequence(7, 6, rows, clip, stride, off, n_movers=4, scintillation=0.3)
    images = [oracle.convertPolarImageToCartesian(r[:, off:off + clip].astype(np.float32) / np.float32(255.), want_u8=True)[1] for r in recs]
    for i in range(6):
        for j in range(i):
            assert not np.array_equal(images[i], images[j])
    idx = wt.lane_maps(B)[0][lane0:lane0 + n].copy()
    idx[idx == 0] = 3                   # no lane of the launch reads record 0: a lane it skipped cannot pass for one it served
    assert len(set(idx.tolist())) == 5 and (np.diff(idx) < 0).any() and (np.diff(idx) > 0).any()
    ctx = _ffi.Context(0)
    eng = Engine(B, 6, ctx=ctx, rows=rows, stride=stride, payload_off=off, clip=clip, motion_distortion=False, peaks_cap=rows * clip,
                 retrack_on_device=True, retrack_slots=8)
    try:
        for k, rec in enumerate(recs):
            eng.upload_scan(k, rec)
        for b in range(B):
            eng.init_lane(b, 0, np.empty((0, 2), np.float32), poses[0])
        eng.init_lanes_detect(lane0, idx, np.tile(poses[0], (n, 1)))
        want = np.zeros(B, np.int32)
        want[lane0:lane0 + n] = idx
        _check_lanes(eng, geometry, range(B), want, images, "after init_lanes_detect(5, 40 lanes)", ["frame %d" % t for t in range(6)])
        assert all(len(eng.lane_features(b)) > 0 for b in (lane0, lane0 + n - 1))
        assert all(len(eng.lane_features(b)) == 0 for b in (0, lane0 - 1, lane0 + n, B - 1))
    finally:
        eng.close()
        ctx.close()


def test_one_row_radar_is_refused():
    """rows == 1: the zero-weight tap row rows + 1 wraps to polar row 1, which a one-row scan does not have (the next record, or past
    the pool) - roam_engine_create refuses it before anything is allocated"""
    from radarslampy_amd import _ffi
    from radarslampy_amd.engine import Engine
    ctx = _ffi.Context(0)
    try:
        with pytest.raises(_ffi.RoamError) as err:
            Engine(2, 2, ctx=ctx, rows=1, stride=132, payload_off=0, clip=132)
        assert err.value.code == -1             # ROAM_E_ARG
        eng = Engine(2, 2, ctx=ctx, rows=2, stride=132, payload_off=0, clip=132)      # the smallest scan it takes
        eng.close()
    finally:
        ctx.close()
