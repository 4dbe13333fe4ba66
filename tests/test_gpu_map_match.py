"""GPU (-m gpu): the map matching (csrc/map_match.hip, Mapping.GlobalMap.localizer, MapLocalizer.match, LoopDetector.localize) against
tests/map_match_model.py.  Parity is unpinned: nothing in the reference localises a scan in a map.

Every comparison is bit for bit.  The two tables that need libm are the library's own (host code) and are fed to the model; from there
on a cell is three multiplies, three additions and a division per axis, each rounded once on both sides, and a score is a sum of bytes -
there is nothing left to round differently, so no tolerance appears below.  The model's answers are computed once
(map_match_cases.expected_match) and shared."""
import ctypes

import numpy as np
import pytest

import global_map_model as map_model
import map_match_cases as cases
import map_match_model as model

pytestmark = pytest.mark.gpu

MATCHES = list(cases.matches())
FIELDS = list(cases.fields())


@pytest.fixture(scope="module")
def ctx():
    from radarslampy_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


_LOCALIZERS = {}


@pytest.fixture(scope="module")
def localizer(ctx):
    """name of a field case -> its MapLocalizer, made once through GlobalMap.localizer"""
    from radarslampy_amd.Mapping import GlobalMap

    def make(name):
        if name not in _LOCALIZERS:
            f = cases.fields()[name]
            H, W = f["hits"].shape
            m = GlobalMap(f["origin"], f["res"], (H, W), f["hits"], f["views"], np.zeros((0, 2)), np.zeros(0, np.uint32), np.zeros(0, np.uint32), 0)
            _LOCALIZERS[name] = m.localizer(f["min_hits"], f["min_views"], f["sigma"], f["radius"], ctx=ctx)
        return _LOCALIZERS[name]
    yield make
    for loc in _LOCALIZERS.values():
        loc.close()
    _LOCALIZERS.clear()


def _raw(loc, m, volume=True, clouds=None, priors=None):
    """the raw outputs of a match case: (poses, info, volume)"""
    return loc._field.match_clouds(m["clouds"] if clouds is None else clouds, m["priors"] if priors is None else priors, m["window"], volume)


def _same(got, want):
    """(poses, info, volume) of the device against expected_match's (poses, info, [volume per query]), bit for bit"""
    poses, info, vol = got
    ok = poses.dtype == np.float64 and poses.tobytes() == want[0].tobytes() and info.dtype == np.int32 and np.array_equal(info, want[1])
    if vol is not None:
        ok = ok and vol.dtype == np.uint32 and all(vol[q].shape == want[2][q].shape and vol[q].tobytes() == want[2][q].tobytes() for q in range(len(poses)))
    return ok


# ---------------------------------------------------------------------------------------------------------------- 1: tables, field
def test_tables_against_numpy():
    from radarslampy_amd import _ffi
    for sigma, r in ((1.0, 2), (0.5, 1), (3.0, 8), (1.0, 0)):
        assert np.abs(_ffi.map_field_table(sigma, r).astype(int) - model.field_table(sigma, r).astype(int)).max() <= 1
    priors = np.array([[1.0, 2.0, 0.3], [0.0, 0.0, -3.1]])
    cs = _ffi.map_match_angles(priors, 25, 0.01)
    for q in range(2):
        assert np.abs(cs[q] - model.angles(priors[q], 25, 0.01)).max() <= np.spacing(1.0)


@pytest.mark.parametrize("name", FIELDS)
def test_field_equals_the_model(name, localizer):
    loc = localizer(name)
    table, want = cases.expected_field(name)
    got = loc.field()
    f = cases.fields()[name]
    assert loc.shape == want.shape and loc.cellM == f["res"] and loc.origin == tuple(f["origin"]) and np.array_equal(loc._field.table, table)
    assert got.dtype == np.uint8 and got.shape == want.shape and got.tobytes() == want.tobytes()


# ---------------------------------------------------------------------------------------------------------------- 2: volumes, records
@pytest.mark.parametrize("name", MATCHES)
def test_volumes_and_records_equal_the_model(name, localizer):
    m = cases.matches()[name]
    loc = localizer(m["field"])
    want = cases.expected_match(name)
    got = _raw(loc, m)
    print(f"{name}: info {got[1].tolist()[:3]}")
    assert _same(got, want)
    again = _raw(loc, m)                                  # the same call twice: the same bytes
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes() and again[2].tobytes() == got[2].tobytes()
    assert _same(_raw(loc, m, volume=False), want)        # without the volume: the same records


def test_the_batches_run_at_the_rows_a_workgroup_holds(ctx):
    """the two large batches of the cases (bit-checked above like every case) are cut on THIS device as a realistic batch is: a
    workgroup takes all the rows it holds - 625 candidates in one block (three accumulators per thread), and 65 rows of 65 candidates
    in blocks of 31, 31 and 3 (eight accumulators, a short last block)"""
    from radarslampy_amd import _ffi
    cu = ctx.device_info()["cu_count"]
    small, large = cases.matches()["a batch of 48, window 25 x 25 x 25"], cases.matches()["a batch of 48, window 25 x 65 x 65"]
    assert len(small["clouds"]) * small["window"][0] >= 4 * cu, f"{cu} compute units: the batches of the cases are too small for this device"
    assert _ffi.map_match_plan(cu, len(small["clouds"]), small["window"]) == (25, 1)
    assert _ffi.map_match_plan(cu, len(large["clouds"]), large["window"]) == (31, 3)
    assert _ffi.map_match_plan(cu, 1, large["window"])[0] < 31                    # a single query is cut finer: the other cases' path


@pytest.mark.parametrize("rows", [1, 3, 4, 8, 12, 16, 20, 24, 28, 31, 40])
def test_every_accumulator_count_gives_the_same_bytes(rows, localizer, monkeypatch):
    """ROAM_MATCH_ROWS forces the rows of a workgroup, whatever the device: on a window of 65 rows of 65 candidates that is 1 to 8
    accumulators per thread (ceil(65 rows / 256)), blocks that do and do not divide the 65 rows, and 40 clamped to the 31 a workgroup
    holds.  The cut must not show: every volume entry and record equals the model"""
    from radarslampy_amd import _ffi
    name = "a batch of 48, window 25 x 65 x 65"
    m = cases.matches()[name]
    loc = localizer(m["field"])
    want = cases.expected_match(name)
    pick = [0, 17, 47]
    monkeypatch.setenv("ROAM_MATCH_ROWS", str(rows))
    held = min(rows, 31)
    assert _ffi.map_match_plan(ctx_cu(loc), len(pick), m["window"]) == (held, -(-65 // held))
    nacc = -(-65 * held // 256)
    assert nacc == {1: 1, 3: 1, 4: 2, 8: 3, 12: 4, 16: 5, 20: 6, 24: 7, 28: 8, 31: 8}[held]
    got = _raw(loc, m, clouds=[m["clouds"][q] for q in pick], priors=m["priors"][pick])
    assert _same(got, (want[0][pick], want[1][pick], [want[2][q] for q in pick]))
    assert _same(_raw(loc, m, volume=False, clouds=[m["clouds"][q] for q in pick], priors=m["priors"][pick]), (want[0][pick], want[1][pick], None))


def ctx_cu(loc):
    return loc._field.ctx.device_info()["cu_count"]


def test_match_returns_the_table_and_the_volumes(localizer):
    from radarslampy_amd import _ffi
    name = "a batch of different sizes"
    m = cases.matches()[name]
    loc = localizer(m["field"])
    poses, info, vols = cases.expected_match(name)
    n_theta, step, kx, ky = m["window"]
    kw = dict(reachM=(kx * loc.cellM, ky * loc.cellM), reachRad=(n_theta // 2) * step, stepRad=step)
    assert loc.window(**kw) == m["window"]
    t, got_vols = loc.match(m["clouds"], m["priors"], volume=True, **kw)
    assert t.dtype == _ffi.MATCH_TABLE and len(got_vols) == len(vols) and all(np.array_equal(a, b) for a, b in zip(got_vols, vols))
    assert np.array_equal(np.stack([t["x"], t["y"], t["theta"]], axis=1), poses)
    assert np.array_equal(np.stack([t[k] for k in ("score", "i", "b", "a", "nPoints", "nInside")], axis=1), info)
    assert np.array_equal(t["found"], info[:, 0] > 0) and not t["found"][0] and t["found"][-1] and t["fraction"][0] == 0.0
    assert np.array_equal(t["fraction"][2:], info[2:, 0] / (255.0 * info[2:, 4]))
    t2 = loc.match(m["clouds"], m["priors"], **kw)
    assert t2.tobytes() == t.tobytes()
    one = loc.match(m["clouds"][4], m["priors"][4], **kw)                         # a single (n, 2) cloud with a (3,) prior
    assert len(one) == 1 and one[0].tobytes() == t[4].tobytes()


def test_a_query_gives_the_same_bytes_at_every_batch_position(localizer):
    name = "one query at three positions"
    m = cases.matches()[name]
    poses, info, vol = _raw(localizer(m["field"]), m)
    assert _same((poses, info, vol), cases.expected_match(name))
    for q in (2, 5):
        assert poses[q].tobytes() == poses[0].tobytes() and info[q].tobytes() == info[0].tobytes() and vol[q].tobytes() == vol[0].tobytes()
    alone = _raw(localizer(m["field"]), m, clouds=[m["clouds"][0]], priors=m["priors"][:1])
    assert alone[0][0].tobytes() == poses[0].tobytes() and alone[1][0].tobytes() == info[0].tobytes() and alone[2][0].tobytes() == vol[0].tobytes()


# ---------------------------------------------------------------------------------------------------------------- 3: host and database
def test_host_clouds_and_database_entries_give_the_same_bytes(ctx, localizer):
    from radarslampy_amd.LoopClosure import LoopDetector
    name = "a batch of different sizes"
    m = cases.matches()[name]
    loc = localizer(m["field"])
    want = cases.expected_match(name)
    clouds = m["clouds"]
    det = LoopDetector(len(clouds) + 1, 7, 3, min_gap=1, ctx=ctx, keepClouds=True, rows=400, maxPoints=8192)
    desc = np.random.default_rng(1).random((len(clouds) + 1, 7, 3), dtype=np.float32)
    assert det.addDescriptors(desc, clouds=clouds[::-1] + [clouds[2]]) == 0       # stored in reverse order: entry 4 - q holds cloud q
    idx = [4, 3, 2, 1, 0]
    host = _raw(loc, m)
    db = loc._field.match_db(det.db, idx, m["priors"], m["window"], True)
    assert _same(host, want) and _same(db, want)
    assert all(db[k].tobytes() == host[k].tobytes() for k in range(3))
    n_theta, step, kx, ky = m["window"]
    kw = dict(reachM=(kx * loc.cellM, ky * loc.cellM), reachRad=(n_theta // 2) * step, stepRad=step)
    t, vols = det.localize(loc, idx, m["priors"], volume=True, **kw)
    assert np.array_equal(np.stack([t["x"], t["y"], t["theta"]], axis=1), want[0]) and all(np.array_equal(a, b) for a, b in zip(vols, want[2]))
    newest = det.localize(loc, priors=m["priors"][2], **kw)                       # indices=None: the newest entry, which holds cloud 2
    assert len(newest) == 1 and newest[0].tobytes() == t[2].tobytes()
    det.close()


# ---------------------------------------------------------------------------------------------------------------- 4: the product path
def test_the_product_path_on_the_synthetic_world(ctx):
    """LoopDetector(keepClouds=True).add of the twelve rendered scans, renderMap with a use mask that leaves the four queries out,
    localizer, localize: the result equals the model run on det.cloud(i) and lies within the CPU test's bound of the truth - one
    cell per axis and one angle step"""
    from radarslampy_amd import _ffi, synth
    from radarslampy_amd.LoopClosure import LoopDetector
    recs = cases.world_records()
    rows = recs[0].shape[0]
    det = LoopDetector(16, 60, 20, clip_px=2025, min_gap=1, ctx=ctx, keepClouds=True, rows=rows)
    polar = np.stack([r[:, synth.META:].astype(np.float32) / 255.0 for r in recs])
    assert det.add(polar) == 0 and len(det) == 12
    poses = np.array(cases.WORLD_MAP_POSES + cases.WORLD_QUERY_POSES)
    use = np.array([1] * 8 + [0] * 4, np.int8)
    gmap = det.renderMap(poses, cellM=cases.WORLD_CELL_M, use=use)
    loc = gmap.localizer(radiusCells=cases.WORLD_RADIUS, ctx=ctx)
    idx = np.arange(8, 12)
    priors = cases.world_priors()
    t, vols = det.localize(loc, idx, priors, volume=True, **cases.WORLD_WINDOW)
    window = loc.window(**cases.WORLD_WINDOW)
    assert window == (25, 0.01, 12, 12)
    F = loc.field()
    assert F.tobytes() == model.field(gmap.hits, gmap.views, 1, 1, cases.WORLD_RADIUS, _ffi.map_field_table(1.0, cases.WORLD_RADIUS)).tobytes()
    cs = _ffi.map_match_angles(priors, window[0], window[1])
    for q in range(4):
        cloud = det.cloud(8 + q)[0]
        pose, info, vol = model.match(F, cloud, priors[q], cs[q], window[1], gmap.cellM, gmap.origin[0], gmap.origin[1], window[2], window[3])
        err = np.array([t["x"][q], t["y"][q], t["theta"][q]]) - np.array(cases.WORLD_QUERY_POSES[q])
        print(f"query {q}: {len(cloud)} stored points, error {err[0]:+.4f} m, {err[1]:+.4f} m, {err[2]:+.5f} rad, score {t['score'][q]}, fraction {t['fraction'][q]:.3f}")
        assert np.array([t["x"][q], t["y"][q], t["theta"][q]]).tobytes() == pose.tobytes() and np.array_equal(vols[q], vol)
        assert [t[k][q] for k in ("score", "i", "b", "a", "nPoints", "nInside")] == info.tolist() and t["found"][q]
        assert abs(err[0]) <= gmap.cellM and abs(err[1]) <= gmap.cellM and abs(err[2]) <= window[1]
        assert np.count_nonzero(vol == vol.max()) == 1
    loc.close()
    det.close()


# ---------------------------------------------------------------------------------------------------------------- 5: refusals, timing
def test_raw_abi_refuses_bad_calls_and_a_good_call_still_answers(ctx, localizer):
    from radarslampy_amd import _ffi
    name = "window 3 x 5 x 5"
    m = cases.matches()[name]
    loc = localizer(m["field"])
    want = cases.expected_match(name)
    lib, P = ctx.lib, _ffi._ptr
    err = lambda: lib.roam_last_error(ctx.h)              # noqa: E731
    xy, off = _ffi.map_match_clouds(m["clouds"])
    pri = np.ascontiguousarray(m["priors"])
    pose, info, vol = np.full((1, 3), -7.0), np.full((1, 6), -7, np.int32), np.full((1, 3, 5, 5), 7, np.uint32)
    good = dict(field=loc._field.h, n=1, xy=xy, off=off, pri=pri, n_theta=3, step=0.01, kx=2, ky=2, pose=pose, info=info, vol=vol)

    def call(**kw):
        a = {**good, **kw}
        return lib.roam_map_match_clouds(ctx.h, a["field"], a["n"], P(a["xy"]), P(a["off"]), P(a["pri"]), a["n_theta"], a["step"], a["kx"], a["ky"], P(a["pose"]),
                                         P(a["info"]), P(a["vol"]))
    nan_xy, far_xy, nan_pri, far_pri, inf_th = xy.copy(), xy.copy(), pri.copy(), pri.copy(), pri.copy()
    nan_xy[7, 1], far_xy[3, 0], nan_pri[0, 0], far_pri[0, 1], inf_th[0, 2] = np.nan, 1.5e6, np.nan, -2e6, np.inf
    for kw, text in ((dict(field=None), b"field"), (dict(n=0), b"n_query"), (dict(xy=None), b"xy"), (dict(off=None), b"offsets"), (dict(pri=None), b"priors"),
                     (dict(xy=nan_xy), b"xy of point 7"), (dict(xy=far_xy), b"xy of point 3"), (dict(pri=nan_pri), b"priors of query 0"),
                     (dict(pri=far_pri), b"priors of query 0"), (dict(pri=inf_th), b"priors of query 0"), (dict(off=np.array([1, 300], np.int64)), b"offsets[0]"),
                     (dict(off=np.array([0, -1], np.int64)), b"offsets of query 0"), (dict(off=np.array([0, 8193], np.int64)), b"offsets of query 0"),
                     (dict(n_theta=0), b"n_theta"), (dict(n_theta=4), b"n_theta"), (dict(n_theta=1027), b"n_theta"), (dict(step=-0.01), b"step_rad"),
                     (dict(step=float("nan")), b"step_rad"), (dict(kx=-1), b"kx"), (dict(kx=129), b"kx"), (dict(ky=-1), b"ky"), (dict(ky=129), b"ky"),
                     (dict(n_theta=1025, kx=128, ky=128), b"scores_out"), (dict(pose=None), b"pose_out"), (dict(info=None), b"info_out")):
        assert call(**kw) == _ffi.ROAM_E_ARG and text in err(), (list(kw), err())
    other = _ffi.Context(0)                               # a field of another context
    assert lib.roam_map_match_clouds(other.h, loc._field.h, 1, P(xy), P(off), P(pri), 3, 0.01, 2, 2, P(pose), P(info), None) == _ffi.ROAM_E_ARG
    assert b"another context" in lib.roam_last_error(other.h)
    assert lib.roam_map_field_read(other.h, loc._field.h, P(np.zeros(loc.shape, np.uint8))) == _ffi.ROAM_E_ARG
    # the database entry: no clouds, another context, an index out of range
    plain = _ffi.LoopDb(ctx, 4, 7, 3)
    plain.add_desc(np.random.default_rng(1).random((4, 7, 3), dtype=np.float32))
    idx = np.zeros(1, np.int32)

    def db_call(c, db, index):
        return lib.roam_loop_db_map_match(c.h, db.h if db is not None else None, loc._field.h, 1, P(index), P(pri), 3, 0.01, 2, 2, P(pose), P(info), None)
    assert db_call(ctx, plain, idx) == _ffi.ROAM_E_STATE and b"keeps no clouds" in err()
    with pytest.raises(ValueError, match="keeps no clouds"):
        loc._field.match_db(plain, [0], pri, m["window"])
    plain.close()
    assert db_call(ctx, None, idx) == _ffi.ROAM_E_ARG and b"db" in err()
    kept = _ffi.LoopDb(ctx, 4, 7, 3)
    kept.keep_clouds(400, 512)
    kept.add_desc(np.random.default_rng(1).random((2, 7, 3), dtype=np.float32))
    kept.set_cloud(1, m["clouds"][0])
    for bad in (2, -1):
        assert db_call(ctx, kept, np.array([bad], np.int32)) == _ffi.ROAM_E_ARG and b"index of query 0" in err()
    assert db_call(ctx, kept, None) == _ffi.ROAM_E_ARG and b"index" in err()
    far = _ffi.LoopDb(other, 4, 7, 3)
    far.keep_clouds(400, 512)
    far.add_desc(np.random.default_rng(1).random((1, 7, 3), dtype=np.float32))
    assert db_call(ctx, far, idx) == _ffi.ROAM_E_ARG and b"another context" in err()
    with pytest.raises(ValueError, match="different contexts"):
        loc._field.match_db(far, [0], pri, m["window"])
    far.close()
    other.close()
    # the field's creation
    f = cases.fields()[m["field"]]
    H, W = f["hits"].shape
    table = _ffi.map_field_table(1.0, 2)
    h = ctypes.c_void_p()
    fgood = dict(ox=0.0, oy=0.0, res=0.5, W=W, H=H, hits=f["hits"], views=f["views"], min_hits=1, min_views=1, radius=2, table=table, out=ctypes.byref(h))

    def create(**kw):
        a = {**fgood, **kw}
        return lib.roam_map_field_create(ctx.h, a["ox"], a["oy"], a["res"], a["W"], a["H"], P(a["hits"]), P(a["views"]), a["min_hits"], a["min_views"],
                                         a["radius"], P(a["table"]), a["out"])
    for kw, text in ((dict(res=0.0), b"res"), (dict(res=float("inf")), b"res"), (dict(ox=float("nan")), b"origin"), (dict(W=0), b"W and H"), (dict(H=-1), b"W and H"),
                     (dict(W=8193, H=8192), b"W H"), (dict(min_hits=0), b"min_hits"), (dict(min_views=0), b"min_views"), (dict(radius=-1), b"radius"),
                     (dict(radius=9), b"radius"), (dict(hits=None), b"hits"), (dict(views=None), b"views"), (dict(table=None), b"table"), (dict(out=None), b"field_out")):
        assert create(**kw) == _ffi.ROAM_E_ARG and text in err(), (list(kw), err())
    assert not h.value
    # nothing was written, and a good call still answers: through the raw entry, the database entry and the wrapper
    assert np.all(pose == -7.0) and np.all(info == -7) and np.all(vol == 7)
    assert call() == _ffi.ROAM_OK and _same((pose, info, vol), want)
    db = loc._field.match_db(kept, [1], pri, m["window"], True)
    assert _same(db, want)
    kept.close()


def test_timing_entry_reports_two_parts_and_changes_nothing(localizer):
    name = "window 25 x 25 x 25"
    m = cases.matches()[name]
    loc = localizer(m["field"])
    f = cases.fields()[m["field"]]
    before = loc.field()
    ms = loc._field.time_match(f["hits"], f["views"], m["clouds"], m["priors"], m["window"], f["min_hits"], f["min_views"], reps=2)
    print(f"field build {ms[0]:.4f} ms, match {ms[1]:.4f} ms for {before.shape[1]} x {before.shape[0]} cells, {len(m['clouds'][0])} points, window {m['window']}")
    assert len(ms) == 2 and all(np.isfinite(v) and v > 0.0 for v in ms)
    assert loc.field().tobytes() == before.tobytes() and _same(_raw(loc, m), cases.expected_match(name))
