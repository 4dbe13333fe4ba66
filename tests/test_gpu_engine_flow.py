"""GPU (-m gpu): the engine's one-step motion prior (roam_engine_set_motion_prior).  Three lanes in the (1024, 400, 1027, 1) layout of
gen_inputs.ENGINE_LAYOUTS, run as tests/test_gpu_engine_shapes.py runs it (lane 0 forward, lane 1 from 40 features, lane 2
backwards, re-detection on the device), beside a twin engine that never gets a prior; and the use case on the large-rotation pair
of tests/klt_flow_cases.py in the Oxford layout, the prior made from the engine's own registration.

Left out: the issue's assertion that set_motion_prior returns before the enqueued steps have completed.  The existing streaming
tests have no event or query for "not completed yet" to borrow; test (g) checks what can be checked without one - steps enqueued
back to back behind set_motion_prior, nothing read in between, give the records of the synchronised run."""
import math

import numpy as np
import pytest

import klt_flow_cases as C
import klt_flow_model as M
import oracle
from gen_inputs import ENGINE_LAYOUTS, layout_sequence

pytestmark = pytest.mark.gpu

LAYOUT = (1024, 400, 1027, 1)
assert LAYOUT in ENGINE_LAYOUTS
FRAMES = 5
IDENTITY = np.float32([[1, 0, 0], [0, 1, 0]])
_cache = {}


def _rot_shift(deg, tx, ty, centre):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.float32([[c, s, centre - c * centre - s * centre + tx], [-s, c, centre + s * centre - c * centre + ty]])


# a prior that is wrong on purpose (3 degrees and (40, -24) px on a sequence that moves a few pixels): the seeded tracker keeps other
# features than the unseeded one
WRONG = _rot_shift(3.0, 40.0, -24.0, 512.0)


def _inputs():
    if "in" not in _cache:
        clip, rows, stride, off = LAYOUT
        recs, poses = layout_sequence(clip, FRAMES, rows, clip, stride, off, n_movers=12, scintillation=0.3)
        feats = []
        for rec in (recs[0], recs[-1]):
            cart = oracle.convertPolarImageToCartesian(rec[:, off:off + clip].astype(np.float32) / np.float32(255.))
            feats.append(oracle.append_dedupe(np.empty((0, 2)), oracle.getFeatures(cart)[0]).astype(np.float32))
        _cache["in"] = (recs, poses, feats[0], feats[1])
    return _cache["in"]


def _engine(ctx):
    from radarslampy_amd.engine import Engine
    clip, rows, stride, off = LAYOUT
    recs, poses, f_first, f_last = _inputs()
    T = len(recs)
    eng = Engine(3, T, ctx=ctx, rows=rows, stride=stride, payload_off=off, clip=clip, retrack_on_device=True)
    for t in range(T):
        eng.upload_scan(t, recs[t])
    for b, (t0, f) in enumerate([(0, f_first), (0, f_first[:40]), (T - 1, f_last)]):
        eng.init_lane(b, t0, f, poses[t0])
    return eng


def _run(ctx, priors, sync=True):
    """priors: step (1-based) -> list of set_motion_prior argument pairs issued before that step.  -> per step dict(raw, feats, peaks, pyr);
    sync=False: every step is enqueued before anything is read, -> per step raw records only"""
    eng = _engine(ctx)
    out = []
    for t in range(1, FRAMES):
        for affine, use in priors.get(t, []):
            eng.set_motion_prior(affine, use)
        eng.step([t, t, FRAMES - 1 - t])
        if sync:
            out.append(dict(raw=eng.results_array().tobytes(), feats=[eng.lane_features(b) for b in range(3)],
                            peaks=[eng.lane_peaks(b) for b in range(3)],
                            pyr=[[eng.lane_image(b, lvl) for lvl in range(4)] for b in range(3)]))
    if not sync:
        assert eng.steps_enqueued() == FRAMES - 1
        out = [dict(raw=eng.results_array(step=k).tobytes()) for k in range(FRAMES - 1)]
    eng.close()
    return out


@pytest.fixture(scope="module")
def ctx():
    from radarslampy_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def twin(ctx):
    return _run(ctx, {})


def _lane_records(raw):
    from radarslampy_amd import _ffi
    import ctypes
    n = ctypes.sizeof(_ffi.LaneResult)
    return [raw[i * n:(i + 1) * n] for i in range(3)]


def _same_lane(x, y, b):
    return (_lane_records(x["raw"])[b] == _lane_records(y["raw"])[b] and np.array_equal(x["feats"][b], y["feats"][b])
            and np.array_equal(x["peaks"][b], y["peaks"][b]) and all(np.array_equal(p, q) for p, q in zip(x["pyr"][b], y["pyr"][b])))


def test_identity_prior_is_no_prior(ctx, twin):
    eye = np.tile(IDENTITY, (3, 1, 1))
    got = _run(ctx, {1: [(eye, None)], 2: [(eye.reshape(3, 6), [1, 1, 1])]})
    for k, (x, y) in enumerate(zip(got, twin)):
        for b in range(3):
            assert _same_lane(x, y, b), (k, b)


def test_use_mask_leaves_other_lanes_alone(ctx, twin):
    A = np.stack([WRONG, WRONG, WRONG])
    got = _run(ctx, {1: [(A, [0, 1, 0])], 2: [(A, [0, 1, 0])]})
    for k, (x, y) in enumerate(zip(got, twin)):
        for b in (0, 2):
            assert _same_lane(x, y, b), (k, b)
    assert not _same_lane(got[0], twin[0], 1)          # the prior reached lane 1


def test_withdrawn_prior_is_gone(ctx, twin):
    A = np.stack([WRONG, WRONG, WRONG])
    got = _run(ctx, {1: [(A, None), (None, None)], 3: [(A, [1, 0, 1]), (None, None)]})
    for k, (x, y) in enumerate(zip(got, twin)):
        for b in range(3):
            assert _same_lane(x, y, b), (k, b)


def test_seeded_step_is_the_standalone_seeded_call_and_lasts_one_step(ctx):
    """(d) and (e): the lane's features and level-0 image before a step, the image after it, through the standalone tracker"""
    eng = _engine(ctx)
    eng.step([1, 1, FRAMES - 2])
    lane = 0
    A = np.stack([WRONG, IDENTITY, IDENTITY])

    def one_step(t, prior):
        feats, prev = eng.lane_features(lane), eng.lane_image(lane, 0)
        if prior:
            eng.set_motion_prior(A, [1, 0, 0])
        eng.step([t, t, FRAMES - 1 - t])
        rec = eng.results()[lane]
        nxt = eng.lane_image(lane, 0)
        _, s, e = ctx.klt_track(prev, nxt, feats, M.apply_affine(WRONG, feats))
        _, s0, e0 = ctx.klt_track(prev, nxt, feats)
        return rec, len(feats), M.count_good(s, e), M.count_good(s0, e0)

    rec, K, seeded, unseeded = one_step(2, True)
    print("seeded step: tracked", rec["n_tracked"], "good", rec["n_good"], "| standalone seeded", seeded, "unseeded", unseeded)
    assert K >= 60 and rec["n_tracked"] == K and rec["n_good"] == seeded and seeded != unseeded
    rec, K, seeded, unseeded = one_step(3, False)
    print("next step: tracked", rec["n_tracked"], "good", rec["n_good"], "| standalone seeded", seeded, "unseeded", unseeded)
    assert rec["n_tracked"] == K and rec["n_good"] == unseeded and seeded != unseeded
    eng.close()


def test_back_to_back_steps_behind_set_motion_prior(ctx):
    A = np.stack([WRONG, _rot_shift(-2.0, -8.0, 16.0, 512.0), IDENTITY])
    priors = {t: [(A, [t % 2, 1, 1])] for t in range(1, FRAMES)}
    a, b = _run(ctx, priors, sync=True), _run(ctx, priors, sync=False)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x["raw"] == y["raw"], k


def test_argument_errors(ctx):
    from radarslampy_amd import _ffi
    assert ctx.lib.roam_engine_set_motion_prior(ctx.h, _ffi._ptr(np.zeros(18, np.float32)), None) == _ffi.ROAM_E_STATE      # no engine
    eng = _engine(ctx)
    bad = np.tile(IDENTITY, (3, 1, 1)).reshape(3, 6).copy()
    for i, v in ((2, np.nan), (7, 65.0), (17, 2.0 ** 21)):
        m = bad.copy()
        m.reshape(-1)[i] = v
        assert ctx.lib.roam_engine_set_motion_prior(ctx.h, _ffi._ptr(m), None) == _ffi.ROAM_E_ARG
        with pytest.raises(ValueError):
            eng.set_motion_prior(m)
    eng.close()


def test_registration_as_prior_keeps_a_large_rotation(ctx):
    """(f) the use case, Oxford layout: three lanes fed the large-rotation pair; the prior is Engine.fmt_register through
    FMT.flowPriorFromFMT.  The yaw bound is twice the error of the same chain on the CPU (klt_flow_cases.CHAIN_YAW_ERR_RAD)"""
    from radarslampy_amd import FMT
    from radarslampy_amd.engine import Engine
    r = C.rotation_pair()

    def run(seed):
        eng = Engine(3, 2, ctx=ctx)
        for t in range(2):
            eng.upload_scan(t, r["recs"][t])
        for b in range(3):
            eng.init_lane(b, 0, r["feats"], r["poses"][0])
        if seed:
            reg = eng.fmt_register([0, 0, 0], [1, 1, 1])
            eng.set_motion_prior(FMT.flowPriorFromFMT(reg[:, 0], reg[:, 3:5]))
        eng.step([1, 1, 1])
        res = eng.results()
        eng.close()
        return res

    seeded, plain = run(True), run(False)
    for b in range(3):
        yaw = math.atan2(seeded[b]["R"][1, 0], seeded[b]["R"][0, 0])
        print("lane", b, "inliers seeded", seeded[b]["n_inliers"], "twin", plain[b]["n_inliers"], "good", seeded[b]["n_good"], plain[b]["n_good"],
              "yaw", yaw, "error", abs(yaw - r["yaw"]))
        assert seeded[b]["n_inliers"] > plain[b]["n_inliers"]
        assert abs(yaw - r["yaw"]) <= C.CHAIN_YAW_TOL_RAD
