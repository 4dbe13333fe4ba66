"""GPU (-m gpu): the motion prior as a mode of the engine (roam_engine_set_auto_prior, roam_engine_step_prior).  The engines, records
and comparisons are those of tests/test_gpu_engine_flow.py - three lanes in the (1024, 400, 1027, 1) layout over five frames, lane 0
forward, lane 1 from 40 features, lane 2 backwards, re-detection on the device - registered with clip_px = 0, downsample = 8,
cart_downsample = 8 (R = 128, a Cartesian side of 256); the use case is the 8 degree pair of tests/klt_flow_cases.py in the Oxford
layout with the defaults.  Tolerances: tests/auto_prior_cases.py."""
import math

import numpy as np
import pytest

import auto_prior_cases as cases
import klt_flow_cases as K
import test_gpu_engine_flow as EF

pytestmark = pytest.mark.gpu

FRAMES = EF.FRAMES
SMALL = cases.SMALL
_cache = {}


@pytest.fixture(scope="module")
def ctx():
    from radarslampy_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


def _snapshot(eng):
    return dict(raw=eng.results_array().tobytes(), feats=[eng.lane_features(b) for b in range(3)],
                peaks=[eng.lane_peaks(b) for b in range(3)], pyr=[[eng.lane_image(b, lvl) for lvl in range(4)] for b in range(3)])


def _run(ctx, auto=None, before=None, scans=None, sync=True, register=False):
    """auto: None = the mode is never touched, "off" = switched on and off again before the first step, dict = set_auto_prior(**auto).
    before(eng, t): called ahead of step t.  scans(t): the step's scan list (default: the three lanes' own).  -> per step
    dict(raw, feats, peaks, pyr[, prior][, reg]); sync=False: every step is enqueued before anything is read -> dict(raw[, prior])"""
    eng = EF._engine(ctx)
    if auto == "off":
        eng.set_auto_prior(True, **SMALL)
        eng.set_auto_prior(False)
    elif auto is not None:
        eng.set_auto_prior(True, **auto)
    on = isinstance(auto, dict)
    out = []
    for t, (prev, curr) in zip(range(1, FRAMES), cases.small_steps(FRAMES)):
        if before is not None:
            before(eng, t)
        eng.step(list(curr) if scans is None else scans(t))
        if sync:
            o = _snapshot(eng)
            if on:
                o["prior"] = eng.step_prior()
            if register:
                o["reg"] = eng.fmt_register(prev, curr, **SMALL)
            out.append(o)
    if not sync:
        assert eng.steps_enqueued() == FRAMES - 1
        out = [dict(raw=eng.results_array(step=k).tobytes(), **(dict(prior=eng.step_prior(k)) if on else {})) for k in range(FRAMES - 1)]
    eng.close()
    return out


def _twin(ctx):
    if "twin" not in _cache:
        _cache["twin"] = _run(ctx)
    return _cache["twin"]


def _mode_on(ctx):
    if "on" not in _cache:
        _cache["on"] = _run(ctx, auto=SMALL, register=True)
    return _cache["on"]


def _same(x, y, lanes=(0, 1, 2)):
    return all(EF._same_lane(x, y, b) for b in lanes)


def _seed_from(records):
    """a set_motion_prior hook that replays the affines and sources of a mode-on run's records"""
    def before(eng, t):
        p = records[t - 1]["prior"]
        eng.set_motion_prior(p["affine"], p["source"] == 1)
    return before


def test_mode_off_is_todays_engine(ctx):
    twin = _twin(ctx)
    for k, (x, y) in enumerate(zip(_run(ctx, auto="off"), twin)):
        assert _same(x, y), k
    for k, (x, y) in enumerate(zip(EF._run(ctx, {}), twin)):
        assert _same(x, y), k
    eng = EF._engine(ctx)
    eng.step([1, 1, FRAMES - 2])
    from radarslampy_amd import _ffi
    with pytest.raises(_ffi.RoamError) as e:
        eng.step_prior()
    assert e.value.code == _ffi.ROAM_E_STATE
    eng.close()


def test_in_step_registration_is_the_blocking_one(ctx):
    worst_px = worst_rel = 0.0
    for k, o in enumerate(_mode_on(ctx)):
        got, want = o["prior"]["out6"], o["reg"]
        for b in range(3):
            dpx = float(np.abs(got[b, 3:5] - want[b, 3:5]).max())
            drel = abs(got[b, 5] - want[b, 5]) / abs(want[b, 5])
            print(f"step {k} lane {b}: in-step {got[b]} blocking {want[b]} | dx, dy differ by {dpx} px, translation response by {drel} relative")
            worst_px, worst_rel = max(worst_px, dpx), max(worst_rel, drel)
            assert got[b, :3].tobytes() == want[b, :3].tobytes(), (k, b)         # angle, scale, rotation response: bit for bit
            assert dpx <= cases.TOL_PX and drel <= cases.TOL_RESPONSE_REL, (k, b)
    print(f"largest difference to the blocking pass: {worst_px} px, {worst_rel} relative")


def test_affine_is_flowPriorFromFMT_of_the_record(ctx):
    from radarslampy_amd import FMT
    differ = total = 0
    for k, o in enumerate(_mode_on(ctx)):
        p = o["prior"]
        assert np.array_equal(p["source"], [1, 1, 1]), k                        # every lane has both scans at every step
        want = FMT.flowPriorFromFMT(p["out6"][:, 0], p["out6"][:, 3:5], SMALL["cart_downsample"], 2, EF.LAYOUT[0])
        ulp = np.abs(p["affine"].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        differ, total = differ + int(np.count_nonzero(ulp)), total + ulp.size
        assert ulp.max() <= 1, (k, p["affine"], want)
    print(f"affine entries that differ from flowPriorFromFMT at all: {differ} of {total}")


def test_step_is_the_seeded_tracker_given_the_recorded_affine(ctx):
    on = _mode_on(ctx)
    for k, (x, y) in enumerate(zip(on, _run(ctx, before=_seed_from(on)))):
        assert _same(x, y), k
    assert any(not _same(x, y) for x, y in zip(on, _twin(ctx)))                 # the prior reached the tracker


def test_gate_nobody_passes_is_the_unseeded_engine(ctx):
    got = _run(ctx, auto=dict(SMALL, min_trans_response=2.0))
    for k, (x, y) in enumerate(zip(got, _twin(ctx))):
        assert np.array_equal(x["prior"]["source"], [0, 0, 0]) and np.isfinite(x["prior"]["out6"]).all(), k
        assert _same(x, y), k
    for k, (x, y) in enumerate(zip(got, _mode_on(ctx))):
        assert x["prior"]["out6"].tobytes() == y["prior"]["out6"].tobytes(), k


def test_new_sequence_lane_runs_unseeded_once(ctx):
    from radarslampy_amd import _ffi
    steps = cases.small_steps(FRAMES)

    def scans(t):
        s = list(steps[t - 1][1])
        if t == 3:
            s[1] |= _ffi.STEP_NEW_SEQUENCE
        return s
    got, on = _run(ctx, auto=SMALL, scans=scans), _mode_on(ctx)
    assert [int(o["prior"]["source"][1]) for o in got] == [1, 1, 0, 1]
    assert np.isnan(got[2]["prior"]["out6"][1]).all()
    for k, (x, y) in enumerate(zip(got, on)):
        assert _same(x, y, lanes=(0, 2)), k
        assert x["prior"][[0, 2]].tobytes() == y["prior"][[0, 2]].tobytes(), k


@pytest.mark.parametrize("chunk", [None, 2])
def test_back_to_back_steps_and_chunks(ctx, monkeypatch, chunk):
    if chunk is not None:
        monkeypatch.setenv("ROAM_FMT_BATCH_CHUNK", str(chunk))                  # two chunks for three lanes
    got, on = _run(ctx, auto=SMALL, sync=False), _mode_on(ctx)
    for k, (x, y) in enumerate(zip(got, on)):
        assert x["prior"].tobytes() == y["prior"].tobytes(), k
        assert x["raw"] == y["raw"], k


def test_manual_prior_wins_for_its_step(ctx):
    on = _mode_on(ctx)
    A, use = np.stack([EF.WRONG, EF.WRONG, EF.IDENTITY]), [1, 0, 1]

    def manual(eng, t):
        if t == 2:
            eng.set_motion_prior(A, use)
    got = _run(ctx, auto=SMALL, before=manual)
    assert np.array_equal(got[1]["prior"]["source"], [2, 0, 2]) and np.isnan(got[1]["prior"]["out6"]).all()
    assert np.array_equal(got[1]["prior"]["affine"], A)
    assert np.array_equal(got[2]["prior"]["source"], [1, 1, 1]) and np.isfinite(got[2]["prior"]["out6"]).all()
    assert got[2]["prior"]["out6"].tobytes() == on[2]["prior"]["out6"].tobytes()       # the registration reads the records only

    def twin(eng, t):
        if t == 2:
            eng.set_motion_prior(A, use)
        else:
            eng.set_motion_prior(got[t - 1]["prior"]["affine"], got[t - 1]["prior"]["source"] == 1)
    for k, (x, y) in enumerate(zip(got, _run(ctx, before=twin))):
        assert _same(x, y), k


def test_overwritten_previous_record_is_refused(ctx):
    from radarslampy_amd import _ffi
    recs = EF._inputs()[0]
    on = _mode_on(ctx)
    eng = EF._engine(ctx)
    eng.set_auto_prior(True, **SMALL)
    eng.step([1, 1, FRAMES - 2])
    eng.upload_scan(1, recs[0])                                              # the previous record of lanes 0 and 1
    with pytest.raises(_ffi.RoamError, match="slot 1.*lane 0") as e:
        eng.step([2, 2, FRAMES - 3])
    assert e.value.code == _ffi.ROAM_E_STATE and eng.steps_enqueued() == 1
    eng.upload_scan(1, recs[1])
    eng.step([2, 2, FRAMES - 3])
    assert _same(_snapshot(eng), on[1])
    assert eng.step_prior().tobytes() == on[1]["prior"].tobytes()
    eng.close()


def test_use_case_large_rotation(ctx):
    from radarslampy_amd.engine import Engine
    r = K.rotation_pair()

    def run(mode):
        eng = Engine(3, 2, ctx=ctx)
        for t in range(2):
            eng.upload_scan(t, r["recs"][t])
        for b in range(3):
            eng.init_lane(b, 0, r["feats"], r["poses"][0])
        if mode:
            eng.set_auto_prior()
        eng.step([1, 1, 1])
        res = eng.results()
        src = eng.step_prior()["source"] if mode else None
        eng.close()
        return res, src

    (seeded, src), (plain, _) = run(True), run(False)
    assert np.array_equal(src, [1, 1, 1])
    for b in range(3):
        yaw = math.atan2(seeded[b]["R"][1, 0], seeded[b]["R"][0, 0])
        print("lane", b, "inliers with the mode", seeded[b]["n_inliers"], "twin", plain[b]["n_inliers"], "yaw", yaw, "error", abs(yaw - r["yaw"]))
        assert seeded[b]["n_inliers"] > plain[b]["n_inliers"]
        assert abs(yaw - r["yaw"]) <= K.CHAIN_YAW_TOL_RAD


def test_streaming_driver_flag(ctx):
    from radarslampy_amd import synth
    from radarslampy_amd.RawROAMSystem import RING, stream_records
    from radarslampy_amd.engine import Engine
    recs, poses, _ = synth.make_sequence(7, 5)
    n = len(recs)

    def by_hand(mode):
        eng = Engine(1, RING, ctx=ctx, retrack_on_device=True, stage_events=False)
        for t in range(n):
            eng.upload_scan(t, recs[t])
        eng.init_lane_detect(0, 0, poses[0])
        if mode:
            eng.set_auto_prior(True)
        out = []
        for t in range(1, n):
            eng.step([t])
            out.append(eng.results()[0]["pose"])
        eng.close()
        return np.array(out)

    sources = []
    collect = lambda eng: sources.extend(int(eng.step_prior(k)["source"][0]) for k in range(n - 1))
    off = stream_records(iter(recs), n, poses[0], {}, ctx)[0]
    on = stream_records(iter(recs), n, poses[0], {"fmtPrior": True}, ctx, before_close=collect)[0]
    assert off.tobytes() == by_hand(False).tobytes()
    assert on.tobytes() == by_hand(True).tobytes()
    assert sources == [1] * (n - 1)
