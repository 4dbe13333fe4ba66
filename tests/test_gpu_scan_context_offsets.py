"""GPU (-m gpu): origin-shifted scan contexts (csrc/loop_offset.hip, the variant entries of csrc/loop_query.hip and csrc/loop_verify.hip,
LoopClosure.LoopDetector(originOffsetsM=...)) against the model tests/scan_context_offset_model.py on the inputs of
tests/scan_context_offset_cases.py and tests/scan_context_cases.py.  Parity is unpinned: nothing in the reference computes this.

Variants of u8 records (Engine.loop_db_add): bit for bit the model's, with an origin exactly on a sample centre and one 200 m away.
Variants of float32 images (add_f32 and the stateless entry): within 1 float32 ulp of the model - a float64 sum of at most 10^6
non-negative terms is within 1e-10 relative of any other order, so the bound follows from the arithmetic - and the same bits from
run to run, alone or in a batch, under a forced small chunk.  The minimum over the variants on crafted descriptors: indices, shifts
and variants equal the model's, distances within scan_context_cases.tolerance().  End to end: two revisits 5 m off their place are
accepted edges with origin offsets and are not without."""
import numpy as np
import pytest

import icp_cases
import scan_context_cases as sc
import scan_context_model as base
import scan_context_offset_cases as cases
import scan_context_offset_model as model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from radarslampy_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


def _ulps(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert np.all(a >= 0) and np.all(b >= 0)
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())


def _centre_offset(rows, S, a, res):
    """-> (c, an offset in metres whose quotient by res is exactly the centre of sample (a, c) in range bins): the first c >= 40 for
    which such float64 metre values exist (the quotients of neighbouring float64 values skip some targets)"""
    from radarslampy_amd import _ffi
    C, Sn, _, _ = _ffi.scan_context_offset_table(rows, S)
    for c in range(40, 400):
        out = []
        for want in ((c + 0.5) * C[a], (c + 0.5) * Sn[a]):
            v = np.nextafter(np.float64(want) * np.float64(res), -np.inf, dtype=np.float64)
            for _ in range(3):
                if v / np.float64(res) == want:
                    out.append(float(v))
                    break
                v = np.nextafter(v, np.inf)
        if len(out) == 2:
            return c, tuple(out)
    raise AssertionError("no sample centre is the quotient of float64 metre values")


# ---------------------------------------------------------------------------------------------------------------- u8 records
def test_u8_variants_of_resident_records_are_the_model(monkeypatch):
    from radarslampy_amd import _ffi, synth
    from radarslampy_amd.engine import Engine
    from radarslampy_amd.LoopClosure import LoopDetector
    recs = sc.revisit_records()[:2]
    rows = recs[0].shape[0]
    cc, centre = _centre_offset(rows, cases.S, 37, cases.RES)
    offsets = np.array([(2.5, 0.0), (-5.0, 3.1), centre, (200.0, 0.0)])
    ob = model.offsets_bins(offsets, cases.RES)
    tab = _ffi.scan_context_offset_table(rows, cases.S)
    # the centre offset really is on sample (37, cc): the model drops exactly that sample
    x, y, _ = model.sample_xyq(rows, cases.CLIP, ob[2], tab)
    assert x[37, cc] == 0.0 and y[37, cc] == 0.0
    assert model.bin_keys(rows, synth.CLIP, cases.CLIP, cases.S, cases.R, ob[2], tab)[37, cc] == -1
    c = _ffi.Context(0)
    eng = Engine(1, 2, ctx=c, retrack_on_device=False)
    for t in range(2):
        eng.upload_scan(t, recs[t])
    for floor_code in (0, 30):
        want = [model.describe_offsets_u8(cases.payload(r), cases.S, cases.R, cases.CLIP, floor_code, ob, tab) for r in recs]
        det = LoopDetector(4, cases.S, cases.R, clip_px=cases.CLIP, floor=floor_code / 255.0, min_gap=1, max_distance=np.inf, k=1, ctx=c,
                           originOffsetsM=offsets)
        assert eng.loop_db_add(det, [0, 1]) == 0
        monkeypatch.setenv("ROAM_LOOP_CHUNK_BYTES", "1")                      # one record per launch of the variants
        assert eng.loop_db_add(det, [1, 0]) == 2 and len(det) == 4
        monkeypatch.delenv("ROAM_LOOP_CHUNK_BYTES")
        assert np.array_equal(det.descriptors()[:2], sc.revisit_descriptors(floor_code)[:2])      # the plain entries are untouched
        for e, t in enumerate([0, 1, 1, 0]):
            got, valid = det.db.get_variants(e)
            assert got.dtype == np.float32 and got.shape == (4, cases.S, cases.R)
            for a in range(4):
                assert np.array_equal(got[a], want[t][a]), (floor_code, e, a)
            assert np.array_equal(valid, (np.square(got.astype(np.float64)).sum(axis=2) > 0).astype(np.int32))
            assert not got[3].any() and not valid[3].any()                    # 200 m away: every sample is dropped
            assert got[0].any() and not np.array_equal(got[0], det.descriptors()[e])
        det.close()
    eng.close()
    c.close()


def test_zero_variants_are_at_distance_one(ctx):
    """what roam_loop_db_add_desc leaves (and what an origin 200 m away gives): invalid variants, distance 1, the plain result wins"""
    from radarslampy_amd import _ffi
    D, _ = sc.distance_case("60x20_n63")
    db = _ffi.LoopDb(ctx, 3, 60, 20)
    db.keep_offsets([(200.0, 0.0), (0.0, 2.5)])
    db.add_desc(np.stack([D[0], np.zeros_like(D[0]), D[4]]))
    got, valid = db.get_variants(2)
    assert not got.any() and not valid.any()
    ci, cd, cs, cv, df, sf, vf = db.query_offsets([1, 2], [1, 2], k=1, want_full=True)
    assert np.all(df[0] == 1.0) and np.all(sf[0] == 0) and np.all(vf == 0)              # an all-zero query with all-zero variants
    pi, pd, ps, pdf, psf = db.query([1, 2], [1, 2], k=1, want_full=True)
    assert np.array_equal(df, pdf) and np.array_equal(sf, psf) and np.array_equal(ci, pi) and np.array_equal(cd, pd) and np.array_equal(cs, ps)
    db.close()


# ---------------------------------------------------------------------------------------------------------------- float32 images
F32_OFFSETS_M = np.array([(1.25, 0.0), (-2.5, 1.55), (5.5, -10.25)])          # at 0.5 m per bin: (2.5, 0), (-5, 3.1), (11, -20.5) bins
F32_RES = 0.5
F32_CASES = ["rand_7x3", "rand_16x8", "rand_64x128_one_pixel_bins", "rows256_256x128", "strided_399x497_clip400", "batch65_16x8"]


def _f32_case(name):
    if name == "rows256_256x128":                         # beyond one tile of the LDS histogram
        return 256, 128, None, np.random.default_rng(256).random((1, 256, 128), dtype=np.float32)
    S, R, clip_px = sc.DESCRIBE_CASES[name]
    return S, R, clip_px, sc.describe_images(name)


@pytest.mark.parametrize("name", F32_CASES)
def test_f32_variants_within_one_ulp_and_repeatable(ctx, name, monkeypatch):
    from radarslampy_amd import _ffi
    S, R, clip_px, imgs = _f32_case(name)
    floor = sc.FLOORS[1]
    ob = model.offsets_bins(F32_OFFSETS_M, F32_RES)
    tab = _ffi.scan_context_offset_table(imgs.shape[1], S)
    got = ctx.scan_context_offsets(imgs, F32_OFFSETS_M, F32_RES, S, R, clip_px, floor)
    assert got.shape == (len(imgs), 4, S, R) and got.dtype == np.float32
    assert np.array_equal(got[:, 0], ctx.scan_context(imgs, S, R, clip_px, floor))         # variant 0 is the plain kernel's
    check = range(len(imgs)) if len(imgs) <= 3 else (0, 31, 64)
    for i in check:
        want = model.describe_offsets_f32(imgs[i], S, R, clip_px, floor, ob, tab)
        u = _ulps(got[i, 1:], want)
        empty = int((want == 0).sum())
        print(f"{name}, image {i}: float32 variants against the model, largest difference {u} ulp; {empty} of {want.size} bins are zero")
        assert u <= 1
    if name == "rand_64x128_one_pixel_bins":
        assert (got[:, 1:] == 0).any()                   # one-pixel bins: a shifted origin leaves some without a sample
    assert np.array_equal(ctx.scan_context_offsets(imgs, F32_OFFSETS_M, F32_RES, S, R, clip_px, floor), got)       # a call repeated
    for i in sorted({0, len(imgs) - 1}):                                                                            # an image alone
        assert np.array_equal(ctx.scan_context_offsets(imgs[i], F32_OFFSETS_M, F32_RES, S, R, clip_px, floor)[0], got[i])
    # through a database, added at once and under a cut of one image per launch: the stored variants are the same bits
    db = _ffi.LoopDb(ctx, len(imgs), S, R)
    db.keep_offsets(F32_OFFSETS_M, F32_RES)
    if len(imgs) > 1:
        monkeypatch.setenv("ROAM_LOOP_CHUNK_BYTES", "1")
    assert db.add_f32(imgs, clip_px, floor) == 0
    monkeypatch.delenv("ROAM_LOOP_CHUNK_BYTES", raising=False)
    assert np.array_equal(db.get(), got[:, 0])
    for i in sorted({0, len(imgs) // 2, len(imgs) - 1}):
        v, valid = db.get_variants(i)
        assert np.array_equal(v, got[i, 1:])
        assert np.array_equal(valid, (np.square(v.astype(np.float64)).sum(axis=2) > 0).astype(np.int32))
    db.close()


# ---------------------------------------------------------------------------------------------------------------- the minimum over variants
def _variant_db(ctx, D, variants, n_off=2):
    """a database of the descriptors D whose entries `variants` ({index: (n_off, S, R)}) carry crafted variants; the rest keep zeros"""
    from radarslampy_amd import _ffi
    db = _ffi.LoopDb(ctx, len(D), D.shape[1], D.shape[2])
    db.keep_offsets([(0.0, 2.5 * (a + 1)) for a in range(n_off)])
    assert db.add_desc(D) == 0
    for i, v in variants.items():
        db.set_variants(i, v)
    return db


def test_rolled_copy_wins_and_a_tie_reports_variant_zero(ctx):
    D, _ = sc.distance_case("60x20_n65")
    D = D.copy()
    rng = np.random.default_rng(11)
    q = 60                                               # neither degenerate nor one of the three equal entries
    crafted = np.stack([rng.random(D[0].shape, dtype=np.float32), np.roll(D[10], 7, axis=0)])
    db = _variant_db(ctx, D, {q: crafted, q - 1: np.stack([D[q - 1], D[q - 1]])})
    ci, cd, cs, cv, df, sf, vf = db.query_offsets([q, q - 1], [q, q - 1], k=1, want_full=True)
    wd, ws, wv = model.distances_variants(np.stack([np.concatenate([D[q][None], crafted]), np.stack([D[q - 1]] * 3)]), D)
    tol = sc.tolerance()
    assert ci[0, 0] == 10 and cv[0, 0] == 2 and cs[0, 0] == ws[0, 10] == 53 and cd[0, 0] <= tol
    assert np.abs(df - wd).max() <= tol
    # variants equal to the plain descriptor tie with it exactly: variant 0 everywhere, and the plain query's bits
    _, _, _, pdf, psf = db.query([q - 1], [q - 1], k=1, want_full=True)
    assert np.all(vf[1] == 0) and np.array_equal(df[1], pdf[0]) and np.array_equal(sf[1], psf[0])
    assert np.array_equal(db.variant_offsets(cv[0]), [[0.0, 5.0]])
    db.close()


@pytest.mark.parametrize("n", [63, 64, 65])
def test_candidates_over_variants_against_the_model(ctx, n, monkeypatch):
    rng = np.random.default_rng(n)
    D = rng.random((n, 60, 20), dtype=np.float32)        # no degenerate entries: every best shift is decided
    queries = np.array([n - 1, n - 2, n - 3, 0], np.int32)
    crafted = {}
    for i in queries[:3]:                                # each variant near an older entry, rolled and noisy
        crafted[int(i)] = np.stack([np.maximum(np.roll(D[int(rng.integers(4, n - 4))], int(rng.integers(0, 60)), axis=0) +
                                               np.float32(0.2) * (2 * rng.random(D[0].shape, dtype=np.float32) - 1), 0) for _ in range(2)])
    db = _variant_db(ctx, D, crafted)
    V = np.stack([np.concatenate([D[i][None], crafted.get(int(i), np.zeros((2,) + D[0].shape, np.float32))]) for i in queries])
    wd, ws, wv = model.distances_variants(V, D)
    tol = sc.tolerance()
    full = db.query_offsets(queries, np.zeros(len(queries), np.int32), k=1, want_full=True)
    assert np.abs(full[4] - wd).max() <= tol and np.array_equal(full[6], wv)
    assert (wv[:3] > 0).any() and np.all(wv[3] == 0)
    for k in (1, 8, 32):
        ci, cd, cs, cv = db.query_offsets(queries, queries, k=k, max_distance=np.inf)
        wi, wdd, wss = base.candidates(wd, ws, queries, np.inf, k)
        wvv = np.where(wi >= 0, np.take_along_axis(wv, np.maximum(wi, 0), axis=1), 0)
        used = wi >= 0
        assert np.array_equal(ci, wi) and np.array_equal(cs, wss) and np.array_equal(cv, wvv)
        assert np.abs(cd[used] - wdd[used]).max() <= tol and np.all(np.isinf(cd[~used]))
        # a forced small chunk (one query per launch: a query takes 12 bytes per entry and variant, and 4 per entry) gives the same bits
        monkeypatch.setenv("ROAM_LOOP_CHUNK_BYTES", str(12 * n * 3 + 4 * n))
        cut = db.query_offsets(queries, queries, k=k, max_distance=np.inf)
        monkeypatch.delenv("ROAM_LOOP_CHUNK_BYTES")
        for x, y in zip((ci, cd, cs, cv), cut):
            assert np.array_equal(x, y)
    db.close()


def test_a_database_without_offsets_answers_as_before(ctx):
    from radarslampy_amd import _ffi
    D, q = sc.distance_case("60x20_n65")
    db = _ffi.LoopDb(ctx, len(D), 60, 20)
    db.add_desc(D)
    a = db.query(q, q, k=8, want_full=True)
    b = db.query_offsets(q, q, k=8, want_full=True)
    for x, y in zip(a, (b[0], b[1], b[2], b[4], b[5])):
        assert np.array_equal(x, y)
    assert not b[3].any() and not b[6].any()
    with pytest.raises(ValueError):
        db.get_variants(0)
    assert ctx.lib.roam_loop_db_get_variants(ctx.h, db.h, 0, _ffi._ptr(np.empty((1, 60, 20), np.float32)), None) == _ffi.ROAM_E_STATE
    # the library's own refusals, before any device call
    off = np.array([[1.0, 0.0], [0.0, 0.0]])
    assert ctx.lib.roam_loop_db_keep_offsets(ctx.h, db.h, 1, _ffi._ptr(off), 0.0432) == _ffi.ROAM_E_ARG            # not empty
    e = _ffi.LoopDb(ctx, 4, 60, 20)
    assert ctx.lib.roam_loop_db_keep_offsets(ctx.h, e.h, 2, _ffi._ptr(off), 0.0432) == _ffi.ROAM_E_ARG and b"(0, 0)" in ctx.lib.roam_last_error(ctx.h)
    assert ctx.lib.roam_loop_db_keep_offsets(ctx.h, e.h, 49, _ffi._ptr(np.ones((49, 2))), 0.0432) == _ffi.ROAM_E_ARG
    assert ctx.lib.roam_loop_db_keep_offsets(ctx.h, e.h, 1, _ffi._ptr(np.array([[np.inf, 0.0]])), 0.0432) == _ffi.ROAM_E_ARG
    assert ctx.lib.roam_loop_db_keep_offsets(ctx.h, e.h, 1, _ffi._ptr(off), 0.0) == _ffi.ROAM_E_ARG
    assert ctx.lib.roam_loop_db_keep_offsets(ctx.h, e.h, 1, _ffi._ptr(off), 0.0432) == _ffi.ROAM_OK
    assert ctx.lib.roam_loop_db_keep_offsets(ctx.h, e.h, 1, _ffi._ptr(off), 0.0432) == _ffi.ROAM_E_ARG            # a second call
    e.close()
    db.close()


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_far_revisits_end_to_end():
    """the eight places and two revisits 5 m off as Oxford records in an engine's pool: with origin offsets each revisit gives one
    accepted edge at the model's pose, without them none"""
    from radarslampy_amd import _ffi
    from radarslampy_amd.engine import Engine
    from radarslampy_amd.LoopClosure import VERIFY_TABLE, VERIFY_TABLE_OFFSETS, LoopDetector, offsetGrid
    n_places = len(sc.PLACES)
    recs = sc.revisit_records()[:n_places] + [cases.far_records()[t] for t in cases.FAR_ICP]
    n = len(recs)
    assert np.array_equal(offsetGrid(5.0, 2.5), cases.GRID)
    tol_m, tol_rad = icp_cases.tolerance()
    bound_m, bound_rad = icp_cases.truth_bound()
    golden = cases.far_icp_golden()
    c = _ffi.Context(0)
    eng = Engine(1, n, ctx=c, retrack_on_device=False)
    for t in range(n):
        eng.upload_scan(t, recs[t])
    q = np.arange(n_places, n, dtype=np.int32)
    for grid in (cases.GRID, None):
        det = LoopDetector(16, cases.S, cases.R, clip_px=cases.CLIP, min_gap=1, max_distance=np.inf, k=3, ctx=c, keepClouds=True,
                           rows=recs[0].shape[0], originOffsetsM=grid)
        assert eng.loop_db_add(det, np.arange(n)) == 0 and len(det) == n
        edges, tab = det.queryAndVerify(q, maxTranslationM=10.0)
        for row in tab:
            print(f"{'offsets' if grid is not None else 'plain'}: query {row['query']} candidate {row['candidate']}: seed yaw {row['yaw']:.4f}"
                  + (f", origin ({row['ox']}, {row['oy']})" if grid is not None else "")
                  + f", pose ({row['theta']:.4f}, {row['tx']:.4f}, {row['ty']:.4f}), fraction {row['fraction']:.4f}, rms {row['rms']:.4f} m, "
                  f"accepted {row['accepted']}")
        if grid is None:
            assert tab.dtype == VERIFY_TABLE and edges == [] and not tab["accepted"].any()
            det.close()
            continue
        assert tab.dtype == VERIFY_TABLE_OFFSETS and len(tab) == 6
        assert [(e[0], e[1]) for e in edges] == [(cases.FAR_REVISITS[t][0], n_places + i) for i, t in enumerate(cases.FAR_ICP)]
        assert tab["accepted"].sum() == 2
        ci, cd, yaw, off = det.query(q, withOffsets=True)
        for i, t in enumerate(cases.FAR_ICP):
            place = cases.FAR_REVISITS[t][0]
            (wd, ws, wv), _ = cases.far_model(t)
            assert ci[i, 0] == place and abs(cd[i, 0] - wd[place]) <= sc.tolerance()
            assert np.array_equal(off[i, 0], model.variant_offsets(wv[place], cases.GRID)) and yaw[i, 0] == base.shift_to_yaw(ws[place], cases.S)
            row = tab[(tab["query"] == n_places + i) & (tab["candidate"] == place)][0]
            assert (row["ox"], row["oy"]) == tuple(off[i, 0])
            pose, n_in, rms = golden[t]
            z = edges[i][2]
            got = np.array([z[2], z[0], z[1]])
            d_m, d_rad = icp_cases.pose_error(got, pose)
            e_m, e_rad = icp_cases.pose_error(got, cases.far_truth(t))
            print(f"far revisit {t}: edge against the model {d_m:.3g} m, {d_rad:.3g} rad (tolerance {tol_m:.3g} m, {tol_rad:.3g} rad); against "
                  f"the truth {e_m:.4f} m, {e_rad:.5f} rad (bound {bound_m:.4f} m, {bound_rad:.5f} rad)")
            assert d_m <= tol_m and d_rad <= tol_rad and abs(row["rms"] - rms) <= tol_m
            assert e_m <= bound_m and e_rad <= bound_rad
        # LoopDetector.verify on query's own output: the same table
        edges2, tab2 = det.verify(q, ci, yaw, candOffset=off, maxTranslationM=10.0)
        assert [(e[0], e[1]) for e in edges2] == [(e[0], e[1]) for e in edges]
        for name in ("query", "candidate", "slot", "yaw", "ox", "oy", "accepted"):
            assert np.array_equal(tab2[name], tab[name]), name
        assert np.abs(tab2["tx"] - tab["tx"]).max() <= tol_m and np.abs(tab2["theta"] - tab["theta"]).max() <= tol_rad
        det.close()
    eng.close()
    c.close()
