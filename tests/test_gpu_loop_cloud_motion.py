"""GPU (-m gpu): the motion compensation of the loop database's resident peak clouds (cloud_gather_motion_kernel in csrc/loop_cloud.hip,
csrc/cloud_motion.h, the velocity keywords of LoopDb / LoopDetector / Engine) against tests/loop_cloud_motion_model.py, the oracle's
peak extraction and tests/icp_model.py.  Parity is unpinned, as for the clouds themselves.

A stored cloud is compared bit for bit: it is the model applied to the oracle's peaks with the library's own tables
(_ffi.polar_cloud_table, _ffi.cloud_motion_table: the host's libm) - from there on eight float64 operations per point, each rounded
once on both sides.  The metric bounds of the last test are icp_cases.tolerance() (device against model ICP) and the rule of
icp_cases.truth_bound() (1.5 times the model's own error, capped at 0.2 m and 0.04 rad), not re-derived here."""
import numpy as np
import pytest

import global_map_cases as map_cases
import icp_cases
import loop_cloud_model as plain
import loop_cloud_motion_cases as cases
import loop_cloud_motion_model as model
from gen_inputs import ENGINE_LAYOUTS, layout_sequence

pytestmark = pytest.mark.gpu

RES = 0.0432
# layout -> (S, R, clip_px) of the descriptor: odd rows; few rows; 1020 rows, where a lane of the gather owns two
LAYOUTS = {(497, 399, 504, 5): (60, 20, 400), (1000, 64, 1000, 0): (16, 8, 0), (1032, 1020, 1032, 0): (60, 20, 0)}
SETTINGS = [(8192, 1), (512, 1)]
ORDER = [2, 0, 3, 3, 1]
VELOCITIES = [(15.0, 3.0, 0.5), None, (-30.0, 10.0, -1.5), (0.0, 0.0, 0.0), (2.0, -1.0, 0.05)]

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


def _wanted(layout, max_points, stride):
    """the model's stored clouds of ORDER / VELOCITIES from the library's tables -> (compensated, plain)"""
    from radarslampy_amd import _ffi
    rows = layout[1]
    _, peaks = _records(layout)
    trig = _ffi.polar_cloud_table(rows)
    tables = _ffi.cloud_motion_table(rows, VELOCITIES)
    assert np.isnan(tables[1]).all() and not np.isnan(tables[[0, 2, 3, 4]]).any()
    want = [model.cloud(peaks[t], *trig, RES, max_points, stride, None if v is None else tables[i]) for i, (t, v) in enumerate(zip(ORDER, VELOCITIES))]
    raw = [plain.cloud(peaks[t], *trig, RES, max_points, stride) for t in ORDER]
    assert _same(want[1], raw[1])                         # the None entry is loop_cloud_model.cloud
    for i in (0, 2, 4):                                   # ... and the moving ones are metres away from it
        assert np.abs(want[i][0] - raw[i][0]).max() > 0.1
    assert np.array_equal(want[3][0], raw[3][0])          # zero velocity: numerically the plain cloud
    return want, raw


def _engine(c, layout, n=4):
    from radarslampy_amd.engine import Engine
    clip, rows, stride_b, off = layout
    eng = Engine(1, n, ctx=c, rows=rows, stride=stride_b, payload_off=off, clip=clip, retrack_on_device=False)
    recs, _ = _records(layout)
    for t in range(n):
        eng.upload_scan(t, recs[t])
    return eng


def _snapshot(db):
    return [len(db), db.get().tobytes()] + [x.tolist() for x in db.cloud_counts()] + [db.get_cloud(i)[0].tobytes() for i in range(len(db))]


# ---------------------------------------------------------------------------------------------------------------- 1: resident records
@pytest.mark.parametrize("max_points,stride", SETTINGS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_compensated_clouds_from_resident_records(layout, max_points, stride, monkeypatch):
    from radarslampy_amd import _ffi
    assert layout in ENGINE_LAYOUTS
    clip, rows, stride_b, off = layout
    S, R, clip_px = LAYOUTS[layout]
    want, raw = _wanted(layout, max_points, stride)
    print(f"{layout}: {[w[1] for w in want]} peaks -> {[len(w[0]) for w in want]} points stored at max_points {max_points}")
    if rows > 512:
        assert -(-rows // 512) == 2                       # a lane of the gather owns two rows
    c = _ffi.Context(0)
    eng = _engine(c, layout)
    db, nocloud, none = _ffi.LoopDb(c, 6, S, R), _ffi.LoopDb(c, 6, S, R), _ffi.LoopDb(c, 6, S, R)
    db.keep_clouds(rows, max_points, stride, RES)
    none.keep_clouds(rows, max_points, stride, RES)
    assert eng.loop_db_add(db, ORDER, clip_px=clip_px, floor_code=0, velocities=VELOCITIES) == 0 and len(db) == 5
    assert eng.loop_db_add(nocloud, ORDER, clip_px=clip_px, floor_code=0) == 0
    for i in range(5):
        assert _same(db.get_cloud(i), want[i]), (i, ORDER[i], VELOCITIES[i])
    n, n_peaks = db.cloud_counts()
    assert n.tolist() == [len(w[0]) for w in want] and n_peaks.tolist() == [w[1] for w in want]
    assert np.array_equal(db.get(), nocloud.get())        # the descriptors are those of a database that keeps no clouds
    # velocities=None: the parent's add, the plain model
    assert eng.loop_db_add(none, ORDER, clip_px=clip_px, floor_code=0, velocities=None) == 0
    for i in range(5):
        assert _same(none.get_cloud(i), raw[i]), (i, ORDER[i])
    assert np.array_equal(none.get(), nocloud.get())
    # the staging and the table cut after every second record: the same bits
    cut = _ffi.LoopDb(c, 6, S, R)
    cut.keep_clouds(rows, max_points, stride, RES)
    monkeypatch.setenv("ROAM_LOOP_CHUNK_BYTES", str(2 * (rows * ((clip + 1) // 2) * 2 + rows * 4 + rows * 32) + 1))
    assert eng.loop_db_add(cut, ORDER, clip_px=clip_px, floor_code=0, velocities=np.array([v or (np.nan, 0, 0) for v in VELOCITIES])) == 0
    monkeypatch.delenv("ROAM_LOOP_CHUNK_BYTES")
    for i in range(5):
        assert _same(cut.get_cloud(i), want[i]), (i, ORDER[i])
    assert np.array_equal(cut.get(), nocloud.get())
    # one record at a time, behind the others: the scan and its velocity alone decide
    assert eng.loop_db_add(db, [3], clip_px=clip_px, floor_code=0, velocities=VELOCITIES[2], period=0.25) == 5
    assert _same(db.get_cloud(5), want[2]) and _same(db.get_cloud(0), want[0])
    eng.synchronize()
    for d in (db, nocloud, none, cut):
        d.close()
    eng.close()
    c.close()


# ---------------------------------------------------------------------------------------------------------------- 2: float32 images
@pytest.mark.parametrize("max_points,stride", SETTINGS)
def test_compensated_clouds_from_float32_images(max_points, stride, monkeypatch):
    """the same scans decoded, through LoopDetector.add(img, velocity=) as a batch and one by one: the clouds of the records"""
    import oracle
    from radarslampy_amd import _ffi
    from radarslampy_amd.LoopClosure import LoopDetector
    c = _ffi.Context(0)
    for layout, (S, R, clip_px) in LAYOUTS.items():
        clip, rows, _, off = layout
        recs, peaks = _records(layout)
        want, _ = _wanted(layout, max_points, stride)
        imgs = np.stack([recs[t][:, off:off + clip] for t in ORDER]).astype(np.float32) / np.float32(255.0)
        assert np.array_equal(oracle.getPointCloudPolarInd(imgs[0]), peaks[ORDER[0]])
        eng = _engine(c, layout)
        kw = dict(clip_px=clip_px or None, min_gap=1, ctx=c, keepClouds=True, rows=rows, maxPoints=max_points, pointStride=stride, rangeResolutionM=RES)
        rec_det, batch, single, cut = (LoopDetector(5, S, R, **kw) for _ in range(4))
        assert eng.loop_db_add(rec_det, ORDER, velocities=VELOCITIES) == 0
        assert batch.add(imgs, velocity=VELOCITIES) == 0
        for i in range(5):
            assert single.add(imgs[i], velocity=VELOCITIES[i]) == i
        per = 4 * rows * clip + rows * ((clip + 1) // 2) * 2 + rows * 4 + rows * 32      # an image's upload, row staging and table
        monkeypatch.setenv("ROAM_LOOP_CHUNK_BYTES", str(2 * per + 1))
        assert cut.add(imgs, velocity=VELOCITIES) == 0
        monkeypatch.delenv("ROAM_LOOP_CHUNK_BYTES")
        for det in (batch, single, cut):
            for i in range(5):
                got = det.cloud(i)
                assert _same(got, want[i]) and _same(got, rec_det.cloud(i)), (layout, i)
        for det in (rec_det, batch, single, cut):
            det.close()
        eng.close()
    c.close()


# ---------------------------------------------------------------------------------------------------------------- 3: refusals
def test_refused_adds_leave_the_database_as_it_was():
    from radarslampy_amd import _ffi
    layout = (1000, 64, 1000, 0)
    clip, rows, _, off = layout
    S, R, _ = LAYOUTS[layout]
    recs, _ = _records(layout)
    c = _ffi.Context(0)
    lib = c.lib
    err = lambda: lib.roam_last_error(c.h)                                      # noqa: E731
    eng = _engine(c, layout)
    db, nocloud = _ffi.LoopDb(c, 3, S, R), _ffi.LoopDb(c, 3, S, R)
    db.keep_clouds(rows, 512, 1, RES)
    assert eng.loop_db_add(db, [0, 1], floor_code=0, velocities=[VELOCITIES[0], None]) == 0
    assert eng.loop_db_add(nocloud, [0, 1], floor_code=0) == 0
    before, before_nc = _snapshot(db), [len(nocloud), nocloud.get().tobytes()]
    img = np.ascontiguousarray(recs[2][:, off:off + clip]).astype(np.float32) / np.float32(255.0)
    idx = np.array([2], np.int32)

    def add_records(d, vel, period=0.25, n=1, index=idx):
        return lib.roam_engine_loop_db_add_motion(c.h, d.h, n, _ffi._ptr(index), 0, 0, _ffi._ptr(vel), period, None)

    def add_image(d, vel, period=0.25):
        return lib.roam_loop_db_add_f32_motion(c.h, d.h, _ffi._ptr(img), 1, rows, clip, clip, rows * clip, 0, 0.0, _ffi._ptr(vel), period, None)
    v = np.array([[1.0, 2.0, 0.1]])
    for add in (add_records, add_image):
        assert add(nocloud, v) == _ffi.ROAM_E_ARG and b"velocities" in err() and b"no clouds" in err()
        for period in (0.0, -0.25, float("nan"), float("inf")):
            assert add(db, v, period) == _ffi.ROAM_E_ARG and b"period" in err()
        for bad in ([1.0, np.nan, 0.0], [np.inf, 0.0, 0.0], [0.0, 0.0, -np.inf]):
            assert add(db, np.array([bad])) == _ffi.ROAM_E_ARG and b"velocities" in err() and b"finite" in err()
        for bad in ([8.1e6, 0.0, 0.0], [6e6, -6e6, 3.0]):
            assert add(db, np.array([bad])) == _ffi.ROAM_E_ARG and b"velocities" in err() and b"beyond" in err()
    two = np.array([2, 3], np.int32)                      # an add that does not fit: one free entry
    assert add_records(db, np.array([[1.0, 2.0, 0.1], [3.0, 0.0, 0.0]]), n=2, index=two) == _ffi.ROAM_E_CAPACITY
    with pytest.raises(_ffi.RoamError) as e:
        eng.loop_db_add(db, [2, 3], floor_code=0, velocities=[(1, 2, 0.1), None])
    assert e.value.code == _ffi.ROAM_E_CAPACITY
    with pytest.raises(ValueError, match="keeps no clouds"):
        eng.loop_db_add(nocloud, [2], floor_code=0, velocities=[(1, 2, 0.1)])
    assert _snapshot(db) == before and [len(nocloud), nocloud.get().tobytes()] == before_nc
    # the timing entry takes the same velocities and appends nothing
    ms = eng.time_loop_cloud(db, [2], reps=2, velocities=[(1, 2, 0.1)])
    assert len(ms) == 2 and all(np.isfinite(m) and m > 0 for m in ms) and _snapshot(db) == before
    with pytest.raises(_ffi.RoamError) as e:
        eng.time_loop_cloud(nocloud, [2], reps=2)
    assert e.value.code == _ffi.ROAM_E_ARG
    assert add_records(db, np.array([[np.nan, np.inf, 5.0]])) == _ffi.ROAM_OK and len(db) == 3      # the marker: a plain cloud, whatever else the row holds
    trig = _ffi.polar_cloud_table(rows)
    assert _same(db.get_cloud(2), plain.cloud(_records(layout)[1][2], *trig, RES, 512, 1))
    db.close()
    nocloud.close()
    eng.close()
    c.close()


# ---------------------------------------------------------------------------------------------------------------- 4: the map
def test_the_map_reads_the_compensated_store():
    from radarslampy_amd import _ffi
    from radarslampy_amd.LoopClosure import LoopDetector
    layout = (497, 399, 504, 5)
    clip, rows, _, off = layout
    S, R, clip_px = LAYOUTS[layout]
    want, raw = _wanted(layout, 512, 1)
    c = _ffi.Context(0)
    eng = _engine(c, layout)
    det = LoopDetector(2, S, R, clip_px=clip_px, min_gap=1, ctx=c, keepClouds=True, rows=rows, maxPoints=512, rangeResolutionM=RES)
    assert eng.loop_db_add(det, [ORDER[0], ORDER[2]], velocities=[VELOCITIES[0], VELOCITIES[2]]) == 0
    clouds = [want[0][0], want[2][0]]
    kw = dict(poses=np.array([[0.0, 0.0, 0.0], [1.5, -0.7, 0.4]]), use=None, extent=None, res=0.25, min_hits=1, min_views=1)
    extent, _, n, expect = map_cases.expected(clouds, kw, _ffi.map_pose_table(kw["poses"]))
    m = det.renderMap(kw["poses"], cellM=kw["res"])
    assert n == len(clouds[0]) + len(clouds[1]) and m.origin == tuple(extent[:2]) and m.shape == (extent[3], extent[2])
    assert m.hits.tobytes() == expect["hits"].tobytes() and m.views.tobytes() == expect["views"].tobytes()
    assert m.points.tobytes() == expect["points"].tobytes() and m.outside == expect["outside"] == 0
    other = map_cases.expected([raw[0][0], raw[2][0]], kw, _ffi.map_pose_table(kw["poses"]))       # the raw clouds make another map
    assert other[0] != extent or other[3]["hits"].tobytes() != expect["hits"].tobytes()
    det.close()
    eng.close()
    c.close()


# ---------------------------------------------------------------------------------------------------------------- 5: end to end
def test_moving_pairs_end_to_end():
    """one place seen twice at driving speed, three times over (loop_cloud_motion_cases): six Oxford records through an engine's pool
    into a cloud-keeping detector, with the true velocities and without.  The ICP from the store follows the model ICP on the model's
    clouds; from compensated clouds the edge is the true one, from raw clouds it is more than 0.2 m off - and still reported a success"""
    from radarslampy_amd import _ffi
    from radarslampy_amd.engine import Engine
    from radarslampy_amd.LoopClosure import LoopDetector
    recs, vel = cases.records()
    rows = recs[0].shape[0]
    trig, tables = _ffi.polar_cloud_table(rows), _ffi.cloud_motion_table(rows, vel)
    tol_m, tol_rad = icp_cases.tolerance()
    truth = cases.truth()
    c = _ffi.Context(0)
    eng = Engine(1, 6, ctx=c, retrack_on_device=False)
    for t in range(6):
        eng.upload_scan(t, recs[t])
    q, cand, yaw = np.array([1, 3, 5]), np.array([[0], [2], [4]]), np.full((3, 1), cases.SEED[0])
    errors = {}
    for name, velocities, tabs in (("compensated", vel, tables), ("raw", None, None)):
        det = LoopDetector(6, clip_px=2025, min_gap=1, ctx=c, keepClouds=True, rows=rows, pointStride=cases.STRIDE)
        assert eng.loop_db_add(det, np.arange(6), velocities=velocities) == 0
        clouds = cases.model_clouds(trig, tabs)
        for i in range(6):
            assert det.cloud(i)[0].tobytes() == clouds[i].tobytes(), (name, i)
        _, tab = det.verify(q, cand, yaw)
        want = cases.model_edges(clouds)
        assert len(tab) == 3
        for p, row in enumerate(tab):
            pose = np.array([row["theta"], row["tx"], row["ty"]])
            d_m, d_rad = icp_cases.pose_error(pose, want[p][0])
            e_m, e_rad = icp_cases.pose_error(pose, truth)
            m_m, m_rad = icp_cases.pose_error(want[p][0], truth)
            print(f"{name} pair {p}: device against model {d_m:.3g} m, {d_rad:.3g} rad (tolerance {tol_m:.3g}, {tol_rad:.3g}); against the truth "
                  f"{e_m:.4f} m, {e_rad:.5f} rad (model {m_m:.4f} m, {m_rad:.5f} rad); status {row['status']}, rms {row['rms']:.3f} m")
            assert d_m <= tol_m and d_rad <= tol_rad and abs(row["rms"] - want[p][1]["rms"]) <= tol_m
            assert row["status"] == want[p][1]["status"] == _ffi.ICP_OK
            errors[name, p] = (e_m, e_rad, m_m, m_rad)
        det.close()
    for p in range(3):
        e_m, e_rad, m_m, m_rad = errors["compensated", p]
        assert e_m <= min(icp_cases.TRUTH_CAP_M, 1.5 * m_m) and e_rad <= min(icp_cases.TRUTH_CAP_RAD, 1.5 * m_rad)
        assert errors["raw", p][0] > icp_cases.TRUTH_CAP_M
    eng.close()
    c.close()
