"""GPU (-m gpu): the loop database's resident peak clouds and the verification that runs from them (csrc/loop_cloud.hip, csrc/loop_verify.hip, csrc/icp.hip,
radarslampy_amd/LoopClosure.py) against tests/loop_cloud_model.py, the oracle's peak extraction and the existing ICP entry.  Parity is
unpinned: nothing in the reference computes this.

Everything here is compared bit for bit.  A stored cloud is the model applied to the oracle's peaks with the table of
_ffi.polar_cloud_table (two float64 multiplies per coordinate, nothing to round differently); a verification from the store is
Context.icp2d_batch on the same clouds (one device function runs both); query_verify is query followed by verify.  The one metric bound,
on the revisit world's edges, is icp_cases.truth_bound() - the bound of test_gpu_icp.py, not re-derived here."""
import types

import numpy as np
import pytest

import icp_cases
import icp_model
import loop_cloud_model as model
import scan_context_cases as sc
from gen_inputs import ENGINE_LAYOUTS, layout_sequence

pytestmark = pytest.mark.gpu

RES = 0.0432
LAYOUTS = {(497, 399, 504, 5): (60, 20, 400), (1000, 64, 1000, 0): (16, 8, 0)}      # layout -> (S, R, clip_px) of the descriptor
SETTINGS = [(8192, 1), (512, 1), (2048, 4)]
ORDER = [2, 0, 3, 3, 1]
PAIR_BYTES = 4 * 8192 + 8 + 48 + 24          # device scratch of one stored pair at max_points = 8192 (loop_verify.hip sc_pair_bytes)


@pytest.fixture(scope="module")
def ctx():
    from radarslampy_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


_SEQ = {}


def _records(layout):
    """four records of a layout and the oracle's peaks of each (computed once)"""
    import oracle
    if layout not in _SEQ:
        clip, rows, stride, off = layout
        recs, _ = layout_sequence(clip + 1, 4, rows, clip, stride, off, n_movers=6)
        _SEQ[layout] = (recs, [oracle.peaks_from_record_u8(r, off, clip) for r in recs])
    return _SEQ[layout]


def _same(got, want):
    """(xy, n_peaks) of LoopDb.get_cloud against the model's, bit for bit"""
    return got[1] == want[1] and got[0].shape == want[0].shape and got[0].tobytes() == want[0].tobytes()


# ---------------------------------------------------------------------------------------------------------------- 1: resident records
@pytest.mark.parametrize("max_points,stride", SETTINGS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_stored_clouds_from_resident_records(layout, max_points, stride, monkeypatch):
    from radarslampy_amd import _ffi
    from radarslampy_amd.engine import Engine
    assert layout in ENGINE_LAYOUTS
    clip, rows, stride_b, off = layout
    S, R, clip_px = LAYOUTS[layout]
    recs, peaks = _records(layout)
    counts = [len(p) for p in peaks]
    steps = {model.step(n, max_points, stride) for n in counts}
    print(f"{layout}: {counts} peaks per record, max_points {max_points}, stride {stride}: steps {sorted(steps)}")
    if layout == (497, 399, 504, 5):                      # what the settings are there for
        assert 1407 <= min(counts) and max(counts) <= 1680
        assert steps == {(8192, 1): {1}, (512, 1): {3, 4}, (2048, 4): {4}}[(max_points, stride)]
    table = _ffi.polar_cloud_table(rows)
    c = _ffi.Context(0)
    eng = Engine(1, 4, ctx=c, rows=rows, stride=stride_b, payload_off=off, clip=clip, retrack_on_device=False)
    pinned = c.host_alloc((4, rows, stride_b))
    for t in range(4):
        pinned[t] = recs[t]
    eng.upload_scans_async(0, pinned, n=4)                # the add waits for the uploads itself
    db, plain = _ffi.LoopDb(c, 6, S, R), _ffi.LoopDb(c, 6, S, R)
    db.keep_clouds(rows, max_points, stride, RES)
    assert eng.loop_db_add(db, ORDER, clip_px=clip_px, floor_code=0) == 0 and len(db) == 5
    assert eng.loop_db_add(plain, ORDER, clip_px=clip_px, floor_code=0) == 0
    want = [model.cloud(peaks[t], *table, RES, max_points, stride) for t in ORDER]
    for i in range(5):
        assert _same(db.get_cloud(i), want[i]), (i, ORDER[i])
    n, n_peaks = db.cloud_counts()
    assert n.tolist() == [len(w[0]) for w in want] and n_peaks.tolist() == [counts[t] for t in ORDER]
    assert np.array_equal(db.get(), plain.get())          # the descriptors are those of a database that keeps no clouds
    with pytest.raises(_ffi.RoamError) as e:              # an add that does not fit
        eng.loop_db_add(db, [0, 1], clip_px=clip_px, floor_code=0)
    assert e.value.code == _ffi.ROAM_E_CAPACITY and len(db) == 5
    assert np.array_equal(db.get(), plain.get()) and [x.tolist() for x in db.cloud_counts()] == [n.tolist(), n_peaks.tolist()]
    for i in range(5):
        assert _same(db.get_cloud(i), want[i])
    # the staging cut after every second record: the same bits
    cut = _ffi.LoopDb(c, 6, S, R)
    cut.keep_clouds(rows, max_points, stride, RES)
    monkeypatch.setenv("ROAM_LOOP_CHUNK_BYTES", str(2 * (rows * ((clip + 1) // 2) * 2 + rows * 4) + 1))
    assert eng.loop_db_add(cut, ORDER, clip_px=clip_px, floor_code=0) == 0
    monkeypatch.delenv("ROAM_LOOP_CHUNK_BYTES")
    for i in range(5):
        assert _same(cut.get_cloud(i), want[i]), (i, ORDER[i])
    assert np.array_equal(cut.get(), plain.get())
    cut.close()
    assert eng.loop_db_add(db, [1], clip_px=clip_px, floor_code=0) == 5            # one more fits, behind the others
    assert _same(db.get_cloud(5), model.cloud(peaks[1], *table, RES, max_points, stride)) and _same(db.get_cloud(0), want[0])
    eng.synchronize()
    c.host_free(pinned)
    db.close()
    plain.close()
    eng.close()
    c.close()


# ---------------------------------------------------------------------------------------------------------------- 2: float32 images
def _images():
    """-> [(name, images (n, rows, cols) float32, S, R, clip_px)]: the records' scans decoded, and one real scan"""
    out = []
    for layout, (S, R, clip_px) in LAYOUTS.items():
        clip, rows, _, off = layout
        out.append((str(layout), np.stack([r[:, off:off + clip] for r in _records(layout)[0]]).astype(np.float32) / np.float32(255.0), S, R, clip_px))
    out.append(("real", sc.real_codes()[:1].astype(np.float32) / np.float32(255.0), 60, 20, 1500))
    return out


@pytest.mark.parametrize("max_points,stride", [(8192, 1), (512, 1)])
def test_stored_clouds_from_float32_images(ctx, max_points, stride, monkeypatch):
    import oracle
    from radarslampy_amd import _ffi
    for name, imgs, S, R, clip_px in _images():
        n, rows, cols = imgs.shape
        table = _ffi.polar_cloud_table(rows)
        peaks = [oracle.getPointCloudPolarInd(im) for im in imgs]
        want = [model.cloud(p, *table, RES, max_points, stride) for p in peaks]
        print(f"{name}: {[len(p) for p in peaks]} peaks per image -> {[len(w[0]) for w in want]} points stored")
        batch, single, cut, plain = (_ffi.LoopDb(ctx, n, S, R) for _ in range(4))
        for db in (batch, single, cut):
            db.keep_clouds(rows, max_points, stride, RES)
        assert batch.add_f32(imgs, clip_px) == 0 and plain.add_f32(imgs, clip_px) == 0
        for i in range(n):
            assert single.add_f32(imgs[i], clip_px) == i
        per = 4 * rows * cols + rows * ((cols + 1) // 2) * 2 + rows * 4       # an image's upload and row staging (loop_describe.hip)
        monkeypatch.setenv("ROAM_LOOP_CHUNK_BYTES", str(max(1, n // 2) * per + 1))
        assert cut.add_f32(imgs, clip_px) == 0
        monkeypatch.delenv("ROAM_LOOP_CHUNK_BYTES")
        for db in (batch, single, cut):
            for i in range(n):
                assert _same(db.get_cloud(i), want[i]), (name, i)
            assert np.array_equal(db.get(), plain.get())
            db.close()
        plain.close()


# ---------------------------------------------------------------------------------------------------------------- 3: the engine
def test_the_engine_is_left_alone():
    """the twin-engine check of test_gpu_scan_context.py on the 399 x 504 layout: describing the pool into a cloud-keeping database
    between two steps changes nothing a twin that never made the call returns"""
    import oracle
    from radarslampy_amd import _ffi
    from radarslampy_amd.engine import Engine
    layout = (497, 399, 504, 5)
    clip, rows, stride_b, off = layout
    recs, peaks = _records(layout)
    cart = oracle.convertPolarImageToCartesian(recs[0][:, off:off + clip].astype(np.float32) / np.float32(255.0))
    ys, xs = np.unravel_index(np.argsort(cart, axis=None)[-2400:][::20], cart.shape)
    feat = np.stack([xs, ys], axis=1).astype(np.float32)
    results = []
    for call in (True, False):
        c = _ffi.Context(0)
        eng = Engine(1, 4, ctx=c, rows=rows, stride=stride_b, payload_off=off, clip=clip, retrack_on_device=False, motion_distortion=False)
        for t in range(4):
            eng.upload_scan(t, recs[t])
        eng.init_lane(0, 0, feat, np.zeros(3))
        eng.step([1])
        if call:
            db = _ffi.LoopDb(c, 8, 60, 20)
            db.keep_clouds(rows, 512, 1, RES)
            assert eng.loop_db_add(db, [0, 1, 2, 3], clip_px=400, floor_code=0) == 0       # behind the step that was just enqueued
        eng.step([2])
        if call:
            assert eng.loop_db_add(db, [3, 2], clip_px=400, floor_code=0) == 4
            table = _ffi.polar_cloud_table(rows)
            for i, t in enumerate([0, 1, 2, 3, 3, 2]):
                assert _same(db.get_cloud(i), model.cloud(peaks[t], *table, RES, 512, 1))
            db.close()
        results.append((eng.results_array(0).tobytes(), eng.results_array(1).tobytes(), eng.lane_features(0), eng.lane_peaks(0)))
        eng.synchronize()
        eng.close()
        c.close()
    a, b = results
    assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert len(a[3]) > 0


# ---------------------------------------------------------------------------------------------------------------- 4: verify
@pytest.fixture(scope="module")
def icp_store(ctx):
    """batch130 in a database: source of pair p at entry 2 p, destination at 2 p + 1, ready-made descriptors; and the existing entry's
    results on the same pairs"""
    from radarslampy_amd import _ffi
    names, pairs, init = icp_cases.batch130()
    db = _ffi.LoopDb(ctx, 2 * len(pairs), 7, 3)
    db.keep_clouds(400, 8192, 1, RES)
    assert db.add_desc(np.random.default_rng(1).random((2 * len(pairs), 7, 3), dtype=np.float32)) == 0
    assert db.cloud_counts()[0].tolist() == [0] * (2 * len(pairs))               # ready-made descriptors: empty clouds
    for p, (src, dst) in enumerate(pairs):
        db.set_cloud(2 * p, src)
        db.set_cloud(2 * p + 1, dst)
    want = ctx.icp2d_batch(pairs, init)
    yield db, names, pairs, init, want
    db.close()


def test_verification_from_the_store_is_the_existing_kernel(ctx, icp_store, monkeypatch):
    from radarslampy_amd import _ffi
    db, names, pairs, init, (want_p, want_s) = icp_store
    n = len(pairs)
    si, di = 2 * np.arange(n), 2 * np.arange(n) + 1
    for p in (0, 1, n - 1):                               # the clouds come back as they went in
        xy, n_peaks = db.get_cloud(2 * p + 1)
        assert xy.tobytes() == np.ascontiguousarray(pairs[p][1], np.float64).tobytes() and n_peaks == len(pairs[p][1])
    poses, stats = db.verify(si, di, init)
    assert poses.tobytes() == want_p.tobytes() and stats.tobytes() == want_s.tobytes()
    seen = set()
    for p in list(range(n)):                              # alone: the ends and every case once
        if names[p] in seen and p not in (0, n - 1):
            continue
        seen.add(names[p])
        p1, s1 = db.verify([si[p]], [di[p]], init[p:p + 1])
        assert p1[0].tobytes() == want_p[p].tobytes() and s1[0].tobytes() == want_s[p].tobytes(), names[p]
    rev = db.verify(si[::-1], di[::-1], init[::-1])      # first against last
    assert rev[0][::-1].tobytes() == want_p.tobytes() and rev[1][::-1].tobytes() == want_s.tobytes()
    monkeypatch.setenv("ROAM_LOOP_CHUNK_BYTES", str(7 * PAIR_BYTES))               # seven pairs per launch
    cut = db.verify(si, di, init)
    monkeypatch.delenv("ROAM_LOOP_CHUNK_BYTES")
    assert cut[0].tobytes() == want_p.tobytes() and cut[1].tobytes() == want_s.tobytes()
    # an empty cloud on either side: FEW_PAIRS, the very bits of the seed
    for name in ("n0", "m0"):
        p = names.index(name)
        assert stats[p]["status"] == _ffi.ICP_FEW_PAIRS and stats[p]["iterations"] == 0 and stats[p]["n_inliers"] == 0 and np.isinf(stats[p]["rms"])
        assert poses[p].tobytes() == np.asarray(init[p], np.float64).tobytes()


def test_one_source_against_three_destinations_in_one_call(ctx, icp_store):
    """the partner scratch is per pair: a kernel that keys it by the source's slot lets the three workgroups overwrite each other"""
    db, names, pairs, init, _ = icp_store
    src = names.index("n2049")                            # 2049 points: two sweeps, every lane's partners live in the scratch for long
    others = [names.index("n1100"), names.index("n513")]
    dsts = [2 * src + 1, 2 * others[0] + 1, 2 * others[1] + 1]
    seeds = np.array([init[src], (0.01, 0.2, -0.1), (-0.02, -0.3, 0.1)])
    for rep in range(3):                                  # a race need not show in one launch; three are cheap
        poses, stats = db.verify([2 * src] * 3, dsts, seeds)
        for j in range(3):
            p1, s1 = db.verify([2 * src], [dsts[j]], seeds[j:j + 1])
            assert poses[j].tobytes() == p1[0].tobytes() and stats[j].tobytes() == s1[0].tobytes(), (rep, j)
    want = ctx.icp2d_batch([(pairs[src][0], pairs[src][1]), (pairs[src][0], pairs[others[0]][1]), (pairs[src][0], pairs[others[1]][1])], seeds)
    assert poses.tobytes() == want[0].tobytes() and stats.tobytes() == want[1].tobytes()
    assert stats[0]["n_inliers"] > 0


# ---------------------------------------------------------------------------------------------------------------- 5: query_verify
def _cloud_cycle():
    out = []
    for name in ("n63", "n64", "n0", "n65", "n513", "outliers_400", "far_seed", "n1100", "rigid_64"):
        out += list(icp_cases.case(name)[:2])
    return out


def _query_verify_case(ctx, D, queries, monkeypatch=None, chunk_bytes=None):
    """queries: [(tag, query indices, max_index, k, max_distance)].  chunk_bytes: the launch scratch of query_verify alone (the query and
    the verification it is compared with run uncut)"""
    from radarslampy_amd import _ffi
    from radarslampy_amd.LoopClosure import _yaw
    S = D.shape[1]
    db = _ffi.LoopDb(ctx, len(D), S, D.shape[2])
    db.keep_clouds(400, 8192, 1, RES)
    assert db.add_desc(D) == 0
    clouds = _cloud_cycle()
    for e in range(len(D)):
        db.set_cloud(e, clouds[e % len(clouds)])
    for tag, q, max_index, k, max_distance in queries:
        if chunk_bytes is not None:
            monkeypatch.setenv("ROAM_LOOP_CHUNK_BYTES", str(chunk_bytes))
        ci, cd, cs, poses, stats = db.query_verify(q, max_index, k, max_distance)
        if chunk_bytes is not None:
            monkeypatch.delenv("ROAM_LOOP_CHUNK_BYTES")
        wi, wd, ws = db.query(q, max_index, k, max_distance)
        assert ci.tobytes() == wi.tobytes() and cd.tobytes() == wd.tobytes() and cs.tobytes() == ws.tobytes(), tag
        used = ci >= 0
        print(f"{tag}: {used.sum()} of {used.size} slots hold a candidate")
        if used.any():
            qq = np.repeat(np.asarray(q, np.int32)[:, None], k, axis=1)
            seeds = np.stack([_yaw(cs, S)[used], np.zeros(used.sum()), np.zeros(used.sum())], axis=1)
            wp, wst = db.verify(qq[used], ci[used], seeds)
            assert poses[used].tobytes() == wp.tobytes() and stats[used].tobytes() == wst.tobytes(), tag
        un = ~used
        assert np.all(stats[un]["status"] == _ffi.ICP_FEW_PAIRS) and np.all(poses[un] == 0.0) and np.all(stats[un]["n_inliers"] == 0), tag
        assert np.all(stats[un]["iterations"] == 0) and np.all(np.isinf(stats[un]["rms"]))
    db.close()


def test_query_verify_is_query_then_verify(ctx, monkeypatch):
    E = sc.small_db_case()
    idx = np.arange(5, dtype=np.int32)
    _query_verify_case(ctx, E, [("small k32", idx, np.full(5, 99, np.int32), 32, np.inf), ("small k2 min_gap", idx, idx, 2, np.inf)])
    # the same under a cut: a query takes 12 bytes per entry and k pairs' scratch, so two queries fit a launch and the five go in three
    per = 12 * len(E) + 2 * PAIR_BYTES
    _query_verify_case(ctx, E, [("small k2 min_gap, cut", idx, idx, 2, np.inf)], monkeypatch, 2 * per + 1)
    D, q, _, _ = sc.topk_case()
    _query_verify_case(ctx, D, [(f"topk {tag}", q, mi, k, md) for tag, mi, k, md in sc.topk_queries()])


# ---------------------------------------------------------------------------------------------------------------- 6: the revisit world
def test_revisit_world_end_to_end():
    """the one test at full shape: eleven Oxford records in an engine's pool, described and kept by Engine.loop_db_add"""
    import oracle
    from radarslampy_amd import _ffi
    from radarslampy_amd.engine import Engine
    from radarslampy_amd.LoopClosure import LoopDetector, closeLoops
    recs = sc.revisit_records()
    n, n_places = len(recs), len(sc.PLACES)
    bound_m, bound_rad = icp_cases.truth_bound()
    c = _ffi.Context(0)
    eng = Engine(1, n, ctx=c, retrack_on_device=False)
    for t in range(n):
        eng.upload_scan(t, recs[t])
    det = LoopDetector(16, sc.REVISIT_S, sc.REVISIT_R, clip_px=sc.REVISIT_CLIP, min_gap=1, max_distance=np.inf, k=3, ctx=c, keepClouds=True,
                       rows=recs[0].shape[0])
    assert eng.loop_db_add(det, np.arange(n)) == 0 and len(det) == n
    # the stored clouds: the model on the oracle's peaks
    table = _ffi.polar_cloud_table(recs[0].shape[0])
    clouds = []
    for t in range(n):
        got = det.cloud(t)
        assert _same(got, model.cloud(oracle.peaks_from_record_u8(recs[t]), *table, RES, 8192, 1)), t
        clouds.append(got[0])
    # the three revisits at k = 3
    q = np.arange(n_places, n, dtype=np.int32)
    edges, tab = det.queryAndVerify(q)
    for row in tab:
        print(f"query {row['query']} candidate {row['candidate']}: fraction {row['fraction']:.4f}, rms {row['rms']:.4f} m, status {row['status']}, "
              f"{row['iterations']} iterations, accepted {row['accepted']}")
    assert len(tab) == 9
    assert [(e[0], e[1]) for e in edges] == [(place, n_places + t) for t, (place, _) in enumerate(sc.REVISITS)]
    for t, (place, _) in enumerate(sc.REVISITS):
        z = edges[t][2]
        e_m, e_rad = icp_cases.pose_error(np.array([z[2], z[0], z[1]]), icp_cases.revisit_truth(t))
        print(f"revisit {t}: edge error {e_m:.4f} m, {e_rad:.5f} rad (bound {bound_m:.4f} m, {bound_rad:.5f} rad)")
        assert e_m <= bound_m and e_rad <= bound_rad
    for row in tab:                                       # the six wrong places are rejected at the default threshold
        assert row["accepted"] == (row["candidate"] == sc.REVISITS[row["query"] - n_places][0])
    # every row is the existing entry on the read-back clouds
    wp, ws = c.icp2d_batch([(clouds[r["query"]], clouds[r["candidate"]]) for r in tab], np.stack([tab["yaw"], 0 * tab["yaw"], 0 * tab["yaw"]], axis=1))
    assert np.stack([tab["theta"], tab["tx"], tab["ty"]], axis=1).tobytes() == wp.tobytes()
    for name in ("status", "iterations", "n_pairs_last", "n_inliers", "rms"):
        assert tab[name].tobytes() == ws[name].tobytes(), name
    assert np.array_equal(tab["fraction"], ws["n_inliers"] / np.array([min(len(clouds[r["query"]]), len(clouds[r["candidate"]])) for r in tab]))
    # LoopDetector.verify on query's own output: the same table
    ci, _, yaw = det.query(q)
    edges2, tab2 = det.verify(q, ci, yaw)
    assert tab2.tobytes() == tab.tobytes() and [(e[0], e[1]) for e in edges2] == [(e[0], e[1]) for e in edges]
    # closeLoops from the detector's store: keyframes without a pointCloud, the drift and weights of test_gpu_icp.py
    true = np.array([sc.place_pose(i) for i in range(n_places)] + [p for _, p in sc.REVISITS])
    drift = np.cumsum(np.tile([0.35, -0.25, 0.006], (len(true), 1)), axis=0) - [0.35, -0.25, 0.006]
    kfs = [types.SimpleNamespace(pose=true[k] + drift[k]) for k in range(len(true))]
    det.k = 2
    graph, edges3, _ = closeLoops(kfs, det, loopInformation=1e4 * np.eye(3), odomInformation=np.diag([1e-4, 1e-4, 1.0]), ctx=c)
    assert sorted((e[0], e[1]) for e in edges3) == sorted((place, n_places + t) for t, (place, _) in enumerate(sc.REVISITS))
    for t, (place, _) in enumerate(sc.REVISITS):
        truth = icp_model.relative_pose(true[place], true[n_places + t])
        before = icp_model.relative_pose(kfs[place].pose, kfs[n_places + t].pose) - truth
        after = icp_model.relative_pose(graph.get_pose(place), graph.get_pose(n_places + t)) - truth
        b_m, a_m = np.hypot(*before[:2]), np.hypot(*after[:2])
        b_r, a_r = abs(icp_model.normalize_angle(before[2])), abs(icp_model.normalize_angle(after[2]))
        print(f"revisit {t}: relative pose error {b_m:.3f} m, {b_r:.4f} rad before; {a_m:.4f} m, {a_r:.5f} rad after")
        assert a_m < b_m and a_r < b_r and a_m <= bound_m and a_r <= bound_rad
    det.close()
    eng.close()
    c.close()


# ---------------------------------------------------------------------------------------------------------------- 7: the raw ABI
def test_raw_abi_refuses_bad_calls(ctx):
    from radarslampy_amd import _ffi
    lib = ctx.lib
    err = lambda: lib.roam_last_error(ctx.h)                                      # noqa: E731
    D = sc.small_db_case()
    full = _ffi.LoopDb(ctx, 8, 7, 3)
    full.add_desc(D)
    assert lib.roam_loop_db_keep_clouds(ctx.h, full.h, 64, 8192, 1, RES) == _ffi.ROAM_E_ARG and b"db" in err()      # not empty
    assert lib.roam_loop_db_get_cloud(ctx.h, full.h, 0, None, 0, None, None) == _ffi.ROAM_E_STATE                  # and so it keeps none
    full.close()
    db = _ffi.LoopDb(ctx, 8, 7, 3)
    for mp in (0, 8193):
        assert lib.roam_loop_db_keep_clouds(ctx.h, db.h, 64, mp, 1, RES) == _ffi.ROAM_E_ARG and b"max_points" in err()
    assert lib.roam_loop_db_keep_clouds(ctx.h, db.h, 64, 8, 0, RES) == _ffi.ROAM_E_ARG and b"point_stride" in err()
    assert lib.roam_loop_db_keep_clouds(ctx.h, db.h, 64, 8, 1, float("nan")) == _ffi.ROAM_E_ARG and b"range_resolution_m" in err()
    assert lib.roam_loop_db_keep_clouds(ctx.h, db.h, 65537, 8, 1, RES) == _ffi.ROAM_E_ARG and b"rows" in err()
    assert lib.roam_loop_db_keep_clouds(ctx.h, db.h, 64, 8, 1, RES) == _ffi.ROAM_OK
    assert lib.roam_loop_db_keep_clouds(ctx.h, db.h, 64, 8, 1, RES) == _ffi.ROAM_E_ARG and b"db" in err()          # once
    db.cloud_rows, db.max_points = 64, 8
    # rows not the database's, at add: nothing is stored
    img = np.random.default_rng(3).random((32, 40), dtype=np.float32)
    assert lib.roam_loop_db_add_f32(ctx.h, db.h, _ffi._ptr(img), 1, 32, 40, 40, 32 * 40, 0, 0.0, None) == _ffi.ROAM_E_ARG and b"rows" in err()
    assert len(db) == 0
    db.add_desc(D)
    xy = np.arange(18.0).reshape(9, 2)
    db.set_cloud(1, xy[:8])
    before = db.get_cloud(1)
    assert lib.roam_loop_db_set_cloud(ctx.h, db.h, 1, _ffi._ptr(xy), 9) == _ffi.ROAM_E_ARG and b"max_points" in err()
    bad = xy[:4].copy()
    bad[2, 1] = np.inf
    assert lib.roam_loop_db_set_cloud(ctx.h, db.h, 1, _ffi._ptr(bad), 4) == _ffi.ROAM_E_ARG and b"xy" in err()
    assert lib.roam_loop_db_set_cloud(ctx.h, db.h, 5, _ffi._ptr(xy), 4) == _ffi.ROAM_E_ARG and b"index" in err()
    assert _same(db.get_cloud(1), before) and before[1] == 8 and db.cloud_counts()[0].tolist() == [0, 8, 0, 0, 0]
    pose, stats, init = np.zeros((2, 3)), np.zeros(2, _ffi.ICP_STATS), np.zeros((2, 3))
    for si, di, name in (([0, 5], [1, 1], b"src_index"), ([0, 1], [1, -1], b"dst_index")):
        rc = lib.roam_loop_db_verify(ctx.h, db.h, 2, _ffi._ptr(np.array(si, np.int32)), _ffi._ptr(np.array(di, np.int32)), _ffi._ptr(init), None,
                                     _ffi._ptr(pose), _ffi._ptr(stats))
        assert rc == _ffi.ROAM_E_ARG and name in err()
    assert not pose.any() and not stats["iterations"].any()
    one = np.array([1, 1], np.int32)
    assert lib.roam_loop_db_verify(ctx.h, db.h, 2, _ffi._ptr(one), _ffi._ptr(one), _ffi._ptr(init), None, _ffi._ptr(pose), _ffi._ptr(stats)) == _ffi.ROAM_OK
    assert stats["n_inliers"].tolist() == [8, 8] and not pose.any()                # a cloud onto itself: the identity
    db.close()
