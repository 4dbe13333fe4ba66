"""GPU (-m gpu): loop-closure candidates by scan context (csrc/loop_describe.hip, csrc/loop_query.hip, radarslampy_amd/LoopClosure.py) against the model
tests/scan_context_model.py on the inputs of tests/scan_context_cases.py.  Parity is unpinned: nothing in the reference computes this.

Descriptors: the u8 record form (engine pool, the Oxford layout and the 399 x 504 layout) bit for bit the integer model; the float32
form within 1 float32 ulp; a call repeated, an image alone or in a batch of 65, a batch added at once or one by one: the same bits.
Distances: within cases.tolerance() of the model on every pair of every case - ten times the largest difference between the model's
summation order and the kernel's, both float64, measured in test_scan_context_cpu.py (8.7e-14).  The best shift equals the model's on
the pairs the model decides by more than twice the tolerance (at least 95 % of every case, asserted on the CPU); on every pair the
model's d at the device's shift is within twice the tolerance of the model's minimum.  Degenerate entries give exactly 1 / 0; one
descriptor at three indices gives equal bits and ascending indices; a pair's bits do not depend on the database size, the
position, the number of queries or a forced small chunk.  Top-k: indices and shifts equal the model's, distances within tolerance,
unused slots -1, +inf, 0.  The revisit world runs through LoopDetector and Engine.loop_db_add, and the engine's step results equal
those of a twin engine that never made the call.  Every measured difference is printed; the largest are copied to docs/PARITY.md
as records."""
import numpy as np
import pytest

import scan_context_cases as cases
import scan_context_model as model
from gen_inputs import ENGINE_LAYOUTS, layout_sequence

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from radarslampy_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


def _ulps(a, b):
    """float32 arrays of non-negative values -> the largest distance in units in the last place"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert np.all(a >= 0) and np.all(b >= 0)
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())


def _db(ctx, D, capacity=None):
    from radarslampy_amd import _ffi
    db = _ffi.LoopDb(ctx, capacity or len(D), D.shape[1], D.shape[2])
    assert db.add_desc(D) == 0 and len(db) == len(D)
    return db


# ---------------------------------------------------------------------------------------------------------------- descriptors
@pytest.mark.parametrize("name", list(cases.DESCRIBE_CASES))
def test_f32_descriptors_within_one_ulp_and_repeatable(ctx, name):
    S, R, clip_px = cases.DESCRIBE_CASES[name]
    imgs = cases.describe_images(name)
    for floor in cases.FLOORS:
        got = ctx.scan_context(imgs, S, R, clip_px, floor)
        want = np.stack([model.describe_f32(im, S, R, clip_px, floor) for im in imgs])
        assert got.shape == want.shape and got.dtype == np.float32
        u = _ulps(got, want)
        print(f"{name}, floor {floor:.4f}: float32 descriptor against the model, largest difference {u} ulp")
        assert u <= 1
        assert np.array_equal(ctx.scan_context(imgs, S, R, clip_px, floor), got)                   # a call repeated
        for i in sorted({0, len(imgs) - 1}):                                                        # an image alone
            assert np.array_equal(ctx.scan_context(imgs[i], S, R, clip_px, floor)[0], got[i])
        if name.startswith("strided"):
            assert np.array_equal(ctx.scan_context(np.ascontiguousarray(imgs), S, R, clip_px, floor), got)


def test_add_get_and_capacity(ctx):
    from radarslampy_amd import _ffi
    S, R, clip_px = cases.DESCRIBE_CASES["batch65_16x8"]
    imgs = cases.describe_images("batch65_16x8")
    want = ctx.scan_context(imgs, S, R, clip_px, 0.25)
    a, b = _ffi.LoopDb(ctx, 65, S, R), _ffi.LoopDb(ctx, 66, S, R)
    assert a.add_f32(imgs, clip_px, 0.25) == 0 and len(a) == 65
    for i in range(65):
        assert b.add_f32(imgs[i], clip_px, 0.25) == i
    assert np.array_equal(a.get(), want) and np.array_equal(b.get(), want)
    assert np.array_equal(a.get(7, 3), want[7:10])
    # the stored normalised columns are the same too: the distances of both databases are the same bits
    q = np.arange(65, dtype=np.int32)
    ra, rb = a.query(q, q, k=4, want_full=True), b.query(q, q, k=4, want_full=True)
    for x, y in zip(ra, rb):
        assert np.array_equal(x, y)
    # ready-made descriptors store the same bits as the describing kernel
    c = _ffi.LoopDb(ctx, 65, S, R)
    c.add_desc(want)
    for x, y in zip(ra, c.query(q, q, k=4, want_full=True)):
        assert np.array_equal(x, y)
    for db, room in ((a, 0), (b, 1)):
        with pytest.raises(_ffi.RoamError) as e:
            db.add_f32(imgs[:room + 1], clip_px, 0.25)
        assert e.value.code == _ffi.ROAM_E_CAPACITY and len(db) == 65
        with pytest.raises(_ffi.RoamError) as e:
            db.add_desc(want[:room + 1])
        assert e.value.code == _ffi.ROAM_E_CAPACITY and len(db) == 65
    assert np.array_equal(a.get(), want)
    # the library's own refusals, before any device call
    assert ctx.lib.roam_loop_db_get(ctx.h, a.h, 60, 6, _ffi._ptr(np.empty((6, S, R), np.float32))) == _ffi.ROAM_E_ARG
    assert ctx.lib.roam_loop_db_add_f32(ctx.h, a.h, _ffi._ptr(imgs), 1, 64, 128, 127, 64 * 128, 100, 0.0, None) == _ffi.ROAM_E_ARG
    assert b"row_stride" in ctx.lib.roam_last_error(ctx.h)
    assert ctx.lib.roam_loop_db_add_f32(ctx.h, a.h, _ffi._ptr(imgs), 1, 64, 128, 128, 64 * 128, 100, -1.0, None) == _ffi.ROAM_E_ARG
    assert b"floor" in ctx.lib.roam_last_error(ctx.h)
    one = np.zeros(1, np.int32)
    out = (_ffi._ptr(np.empty(1, np.int32)), _ffi._ptr(np.empty(1)), _ffi._ptr(np.empty(1, np.int32)))
    assert ctx.lib.roam_loop_db_query(ctx.h, a.h, 1, _ffi._ptr(one), _ffi._ptr(one), 33, 1.0, *out, None, None) == _ffi.ROAM_E_ARG
    assert ctx.lib.roam_loop_db_query(ctx.h, a.h, 1, _ffi._ptr(one + 65), _ffi._ptr(one), 1, 1.0, *out, None, None) == _ffi.ROAM_E_ARG
    assert b"query_index" in ctx.lib.roam_last_error(ctx.h)
    for db in (a, b, c):
        db.close()


U8_CASES = [((497, 399, 504, 5), 60, 20, 400, 30), ((497, 399, 504, 5), 7, 3, 0, 0), ((497, 399, 504, 5), 64, 128, 0, 254)]


@pytest.mark.parametrize("layout,S,R,clip_px,floor_code", U8_CASES)
def test_u8_records_of_the_engine_pool_are_the_integer_model(ctx, layout, S, R, clip_px, floor_code):
    """the 399 x 504 layout of the FMT tests (the Oxford layout: test_revisit_world below); the records are uploaded asynchronously
    and described at once - the call waits for the uploads itself"""
    from radarslampy_amd import _ffi
    from radarslampy_amd.engine import Engine
    assert layout in ENGINE_LAYOUTS
    clip, rows, stride, off = layout
    recs, _ = layout_sequence(clip + 1, 4, rows, clip, stride, off, n_movers=6)
    c = _ffi.Context(0)
    eng = Engine(1, 4, ctx=c, rows=rows, stride=stride, payload_off=off, clip=clip, retrack_on_device=False)
    pinned = c.host_alloc((4, rows, stride))
    for t in range(4):
        pinned[t] = recs[t]
    eng.upload_scans_async(0, pinned, n=4)
    db = _ffi.LoopDb(c, 8, S, R)
    order = [2, 0, 3, 3, 1]
    assert eng.loop_db_add(db, order, clip_px=clip_px, floor_code=floor_code) == 0
    assert eng.loop_db_add(db, [1], clip_px=clip_px, floor_code=floor_code) == 5 and len(db) == 6
    want = np.stack([model.describe_u8(recs[t][:, off:off + clip], S, R, clip_px, floor_code) for t in order + [1]])
    assert np.array_equal(db.get(), want)
    with pytest.raises(_ffi.RoamError) as e:
        eng.loop_db_add(db, [0, 1, 2], clip_px=clip_px, floor_code=floor_code)
    assert e.value.code == _ffi.ROAM_E_CAPACITY and len(db) == 6
    rc = c.lib.roam_engine_loop_db_add(c.h, db.h, 1, _ffi._ptr(np.array([4], np.int32)), clip_px, floor_code, None)
    assert rc == _ffi.ROAM_E_ARG
    rc = c.lib.roam_engine_loop_db_add(c.h, db.h, 1, _ffi._ptr(np.array([0], np.int32)), clip_px, 255, None)
    assert rc == _ffi.ROAM_E_ARG and b"floor_code" in c.lib.roam_last_error(c.h)
    eng.synchronize()
    c.host_free(pinned)
    db.close()
    eng.close()
    c.close()


# ---------------------------------------------------------------------------------------------------------------- distances
@pytest.mark.parametrize("name", list(cases.DISTANCE_CASES))
def test_distances_and_shifts_against_the_model(ctx, name):
    S, R, n, _, _ = cases.DISTANCE_CASES[name]
    D, q = cases.distance_case(name)
    want_d, want_s, _ = cases.distance_model(name)
    tol = cases.tolerance()
    db = _db(ctx, D)
    ci, cd, cs, got_d, got_s = db.query(q, np.zeros(len(q), np.int32), k=3, max_distance=np.inf, want_full=True)
    assert np.all(ci == -1) and np.all(np.isinf(cd)) and np.all(cs == 0)              # max_index 0: no candidates
    err = np.abs(got_d - want_d).max()
    dec = cases.decided(name)
    prep = model.prepare(D)
    at_shift = np.stack([model.shift_distances(D[i], D, prep)[np.arange(n), got_s[r]] for r, i in enumerate(q)])
    excess = (at_shift - want_d).max()
    print(f"{name}: distance against the model, largest difference {err:.3g} (tolerance {tol:.3g}); shift compared on {dec.sum()} of "
          f"{dec.size} pairs, {np.count_nonzero(got_s != want_s)} shifts differ in all; model d at the device's shift above the minimum by "
          f"at most {excess:.3g}")
    assert err <= tol
    assert np.array_equal(got_s[dec], want_s[dec])
    assert excess <= 2 * tol
    # self-distance: an entry with a valid sector is at <= tolerance from itself, at shift 0
    valid = np.array([np.any(D[i] != 0) for i in q])
    rows = np.arange(len(q))
    assert np.all(got_d[rows, q][valid] <= tol) and np.all(got_s[rows, q][valid] == 0)
    if n >= 8:
        assert np.all(got_d[:, cases.ALL_ZERO] == 1.0) and np.all(got_s[:, cases.ALL_ZERO] == 0)
        assert np.all(got_s[:, cases.SECTOR_CONSTANT] == 0)
        # as queries too (not among the case's queries where they would thin the shift comparison out)
        _, _, _, dd, ss = db.query([cases.ALL_ZERO, cases.SECTOR_CONSTANT], [0, 0], k=1, want_full=True)
        assert np.all(dd[0] == 1.0) and np.all(ss[0] == 0)
        sc = model.distances(D[[cases.SECTOR_CONSTANT]], D)[0][0]
        assert np.abs(dd[1] - sc).max() <= tol
        a, b, c = cases.triple(n)
        for x in (got_d, got_s):
            assert np.array_equal(x[:, a], x[:, b]) and np.array_equal(x[:, a], x[:, c])
        if S > 2:                     # (at S = 2 every entry with the same empty sector is at exactly 0 from the query)
            r = int(np.flatnonzero(q == cases.TRIPLE_FIRST)[0])
            ci, cd, _ = db.query([cases.TRIPLE_FIRST], [n], k=3, max_distance=np.inf)
            assert list(ci[0]) == [a, b, c] and cd[0, 0] == cd[0, 1] == cd[0, 2] == got_d[r, a]
    db.close()


@pytest.mark.parametrize("name", ["60x20_n65", "7x3_n200", "256x128_n65"])
def test_pair_bits_do_not_depend_on_the_batch(ctx, name, monkeypatch):
    S, R, n, _, _ = cases.DISTANCE_CASES[name]
    D, q = cases.distance_case(name)
    q = q[:24]
    zero = np.zeros(len(q), np.int32)
    db = _db(ctx, D, capacity=n + 3)
    _, _, _, ref_d, ref_s = db.query(q, zero, k=1, want_full=True)
    # the number of queries: one at a time, and a batch that is no multiple of a workgroup's sixteen
    for r in (0, len(q) - 1):
        _, _, _, d1, s1 = db.query(q[r:r + 1], zero[:1], k=1, want_full=True)
        assert np.array_equal(d1[0], ref_d[r]) and np.array_equal(s1[0], ref_s[r])
    _, _, _, d5, s5 = db.query(q[2:7], zero[:len(q[2:7])], k=1, want_full=True)
    assert np.array_equal(d5, ref_d[2:7]) and np.array_equal(s5, ref_s[2:7])
    # a forced small chunk: three queries per launch
    monkeypatch.setenv("ROAM_LOOP_CHUNK_BYTES", str(3 * 12 * n))
    _, _, _, dc, sc = db.query(q, zero, k=1, want_full=True)
    monkeypatch.delenv("ROAM_LOOP_CHUNK_BYTES")
    assert np.array_equal(dc, ref_d) and np.array_equal(sc, ref_s)
    # the candidates' masked path (no full output) selects from the same bits
    ci, cd, cs = db.query(q, np.full(len(q), n, np.int32), k=5, max_distance=np.inf)
    wi, wd, ws = model.candidates(ref_d, ref_s, np.full(len(q), n), np.inf, 5)
    assert np.array_equal(ci, wi) and np.array_equal(cd, wd) and np.array_equal(cs, ws)
    # the database size: three more entries behind
    db.add_desc(D[:3])
    _, _, _, dg, sg = db.query(q, zero, k=1, want_full=True)
    assert np.array_equal(dg[:, :n], ref_d) and np.array_equal(sg[:, :n], ref_s)
    db.close()
    # the position: the same entries in reverse order, and a database of the first ten only
    rev = _db(ctx, D[::-1])
    _, _, _, dr, sr = rev.query(n - 1 - q, zero, k=1, want_full=True)
    assert np.array_equal(dr[:, ::-1], ref_d) and np.array_equal(sr[:, ::-1], ref_s)
    rev.close()
    small = _db(ctx, D[:10])
    qs = q[q < 10]
    _, _, _, dsm, ssm = small.query(qs, np.zeros(len(qs), np.int32), k=1, want_full=True)
    assert np.array_equal(dsm, ref_d[q < 10][:, :10]) and np.array_equal(ssm, ref_s[q < 10][:, :10])
    small.close()


# ---------------------------------------------------------------------------------------------------------------- top-k
def test_topk_against_the_model(ctx):
    D, q, slots, shifts = cases.topk_case()
    want_d, want_s, _ = cases.topk_model()
    tol = cases.tolerance()
    db = _db(ctx, D)
    for tag, max_index, k, max_distance in cases.topk_queries():
        ci, cd, cs = db.query(q, max_index, k=k, max_distance=max_distance)
        wi, wd, ws = model.candidates(want_d, want_s, max_index, max_distance, k)
        used = wi >= 0
        err = np.abs(cd[used] - wd[used]).max() if used.any() else 0.0
        print(f"top-k {tag}: {used.sum()} candidates, largest distance difference {err:.3g}")
        assert np.array_equal(ci, wi) and np.array_equal(cs, ws) and err <= tol
        assert np.all(np.isinf(cd[~used])) and np.all(cd[~used] > 0)
        if tag in ("k1", "k3", "k8"):
            assert np.array_equal(ci, slots[:, :k]) and np.array_equal(cs, shifts[:, :k])
        if tag == "k32":
            assert np.array_equal(ci[:, :8], slots) and np.all(ci[:, 8:] == -1) and np.all(cs[:, 8:] == 0)
        if tag == "max_index_0":
            assert not used.any()
    db.close()
    # k larger than the database
    E = cases.small_db_case()
    db = _db(ctx, E)
    idx = np.arange(5, dtype=np.int32)
    ci, cd, cs = db.query(idx, np.full(5, 99, np.int32), k=32, max_distance=np.inf)
    d, s, _ = model.distances(E, E)
    wi, wd, ws = model.candidates(d, s, np.full(5, 99), np.inf, 32)
    assert np.array_equal(ci, wi) and np.array_equal(cs, ws) and np.abs(cd[:, :5] - wd[:, :5]).max() <= tol
    assert np.all(ci[:, 5:] == -1) and np.all(np.isinf(cd[:, 5:])) and np.all(cs[:, 5:] == 0)
    db.close()


def test_scan_context_distance_wrapper(ctx):
    from radarslampy_amd import LoopClosure as lc
    D, _ = cases.distance_case("60x20_n63")
    d, k, yaw = lc.scanContextDistance(D[0], np.roll(D[0], 7, axis=0))
    assert d <= cases.tolerance() and k == 7 and abs(yaw - 2 * np.pi * 7 / 60) < 1e-12
    d, k, yaw = lc.scanContextDistance(D[0], D[4])
    wd, wk = model.distance(D[0], D[4])
    assert abs(d - wd) <= cases.tolerance() and k == wk and abs(yaw - float(model.shift_to_yaw(wk, 60))) < 1e-12
    got = lc.scanContext(cases.describe_images("rand_16x8")[0], 16, 8)
    assert got.shape == (16, 8) and _ulps(got, model.describe_f32(cases.describe_images("rand_16x8")[0], 16, 8)) <= 1


# ---------------------------------------------------------------------------------------------------------------- revisits
@pytest.mark.parametrize("floor_code", cases.REVISIT_FLOOR_CODES)
def test_revisit_world_through_detector_and_engine(floor_code):
    """eight places and three revisits as Oxford records in an engine's pool: Engine.loop_db_add stores the integer model's
    descriptors bit for bit, LoopDetector.query returns the model's candidates, and the engine's step gives what a twin engine
    that never made the call gives"""
    import oracle
    from radarslampy_amd import _ffi, synth
    from radarslampy_amd.engine import Engine
    from radarslampy_amd.LoopClosure import LoopDetector
    recs = cases.revisit_records()
    D = cases.revisit_descriptors(floor_code)
    n, n_places = len(recs), len(cases.PLACES)
    tol = cases.tolerance()
    polar0 = recs[0][:, synth.META:synth.META + synth.CLIP].astype(np.float32) / np.float32(255.0)
    cart = oracle.convertPolarImageToCartesian(polar0)
    ys, xs = np.unravel_index(np.argsort(cart, axis=None)[-3600:][::30], cart.shape)
    feat = np.stack([xs, ys], axis=1).astype(np.float32)
    results = []
    for call in (True, False):
        c = _ffi.Context(0)
        eng = Engine(1, n + 1, ctx=c, retrack_on_device=False)
        for t in range(n):
            eng.upload_scan(t, recs[t])
        eng.upload_scan(n, cases.next_record_after_place_0())
        if call:
            det = LoopDetector(16, cases.REVISIT_S, cases.REVISIT_R, clip_px=cases.REVISIT_CLIP, floor=floor_code / 255.0, min_gap=1,
                               max_distance=np.inf, k=n_places, ctx=c)
            assert eng.loop_db_add(det, np.arange(n_places)) == 0
        eng.init_lane(0, 0, feat, np.zeros(3))
        eng.step([n])
        if call:
            assert eng.loop_db_add(det, np.arange(n_places, n)) == n_places and len(det) == n
            assert np.array_equal(det.descriptors(), D)
            idx = np.arange(n_places, n)
            ci, cd, yaw = det.query(idx)
            want_d, want_s, _ = model.distances(D[idx], D)
            wi, wd, ws = model.candidates(want_d, want_s, idx, np.inf, n_places)
            err = np.abs(cd[wi >= 0] - wd[wi >= 0]).max()
            print(f"floor {floor_code}: candidates {ci[:, :2].tolist()}, distances {np.round(cd[:, :2], 4).tolist()}, "
                  f"largest difference to the model {err:.3g}")
            assert np.array_equal(ci, wi) and err <= tol
            assert np.allclose(yaw, model.shift_to_yaw(ws, cases.REVISIT_S), atol=1e-12)
            for t, (place, _) in enumerate(cases.REVISITS):
                assert ci[t, 0] == place and cd[t, 0] <= 0.5 * cd[t, 1]
                off = abs((ws[t, 0] - cases.revisit_true_shift(t) + 30) % 60 - 30)
                assert off <= 1.0
            # the float32 path on the decoded scans recognises the same places
            det2 = LoopDetector(16, cases.REVISIT_S, cases.REVISIT_R, clip_px=cases.REVISIT_CLIP, floor=floor_code / 255.0, min_gap=1,
                                max_distance=np.inf, k=2, ctx=c)
            imgs = np.stack([r[:, synth.META:synth.META + synth.CLIP] for r in recs]).astype(np.float32) / np.float32(255.0)
            assert det2.add(imgs[:n_places]) == 0
            for t, (place, _) in enumerate(cases.REVISITS):
                i, ci2, cd2, _ = det2.addAndQuery(imgs[n_places + t])
                assert i == n_places + t and ci2[0] == place and abs(cd2[0] - want_d[t, place]) <= 1e-5
            det.close()
            det2.close()
        results.append((eng.results_array().tobytes(), eng.lane_features(0)))
        eng.synchronize()
        eng.close()
        c.close()
    assert results[0][0] == results[1][0] and np.array_equal(results[0][1], results[1][1])
