"""GPU (-m gpu): the batched engine and the standalone tracker against the oracle at record layouts and image sizes other than the
Oxford one.  W = 2 * (clip // 2) chooses the pyramid kernel of every level (fused two-level, wave with the dark table, rows, tiled:
tests/test_pyramid_dispatch_model.py holds which layout reaches which), the dark table's geometry, the detection strips and the
peak staging; rows, stride and payload offset change the ingest.  Each layout runs a few lanes over several steps, once with
re-detection when a lane runs out of features (inside the step; through retrack_lane above W = 2048, where the engine refuses the
device retrack) and once without, compared step by step with oracle.OdometryPipeline in the same layout: the
counts, features, peaks and all four pyramid levels bit for bit, R / h / pose to 1e-4 m and 1e-5 rad, the keyframe and retrack
flags.  The tracker is compared bit for bit with oracle.calcOpticalFlowPyrLK on square and non-square images, points on and
outside every border of every level included.  (Poses are compared engine against oracle only: both keep the reference's fixed
Cartesian centre of 1012 px, so they are not the generator's ground truth at W != 2024.)"""
import numpy as np
import pytest

import oracle
from gen_inputs import ENGINE_LAYOUTS, KLT_SIZES, layout_sequence

pytestmark = pytest.mark.gpu

POS_TOL = 1e-4   # m
ANG_TOL = 1e-5   # rad


def _detect(cart):
    return oracle.getFeatures(cart)[0]


def _frames(clip):
    return 4 if clip > 2048 else 6          # the oracle's detection at 3768^2 dominates the run time


_SEQ = {}


def _sequence(layout):
    if layout not in _SEQ:
        clip, rows, stride, off = layout
        _SEQ[layout] = layout_sequence(clip, _frames(clip), rows, clip, stride, off, n_movers=12, scintillation=0.3)
    return _SEQ[layout]


def _first_features(rec, off, clip):
    cart = oracle.convertPolarImageToCartesian(rec[:, off:off + clip].astype(np.float32) / np.float32(255.))
    return oracle.append_dedupe(np.empty((0, 2)), _detect(cart)).astype(np.float32)


def _motion_distortion(clip):
    """the motion-distortion solve is off below W = 1000: with the fixed Cartesian centre of 1012 px every feature of a small image
    lies 60 m or more off the sensor in one quadrant, and the solve is no longer determined to 1e-4 m by its inputs - the oracle's
    own pose moves by 3.6 mm when its starting translation moves by 1e-10 m (W = 496, 36 points), so a rounding difference decides
    it.  These layouts compare the Kabsch pose chain instead; every other stage is the same."""
    return 2 * (clip // 2) >= 1000


def _device_retrack(clip):
    return 2 * (clip // 2) <= 2048          # roam_engine_create refuses the device retrack above (engine.hip)


def _run_layout(layout, retrack, upload_async=False):
    """lane 0 tracks forward from the features detected on frame 0, lane 1 from 40 of them (it retracks at once), lane 2 tracks the
    sequence backwards from the features of the last frame -> (per-step results, lane images at every step, features, peaks).
    retrack: re-detect when a lane runs out of features - in the step where the engine allows it, else through retrack_lane
    (device DoH, host bookkeeping) after the step; retrack=False leaves the lanes to the features they keep"""
    from radarslampy_amd import _ffi
    from radarslampy_amd.engine import Engine
    clip, rows, stride, off = layout
    recs, poses = _sequence(layout)
    T = len(recs)
    ctx = _ffi.Context(0)
    on_device = retrack and _device_retrack(clip)
    if retrack and not on_device:
        with pytest.raises(_ffi.RoamError):
            Engine(3, T, ctx=ctx, rows=rows, stride=stride, payload_off=off, clip=clip, retrack_on_device=True)
    eng = Engine(3, T, ctx=ctx, rows=rows, stride=stride, payload_off=off, clip=clip, retrack_on_device=on_device,
                 motion_distortion=_motion_distortion(clip))
    if upload_async:
        pinned = ctx.host_alloc((T, rows, stride))
        for t in range(T):
            pinned[t] = recs[t]
        eng.upload_scans_async(0, pinned, n=T)
        eng.synchronize()
        eng.fence()
    else:
        for t in range(T):
            eng.upload_scan(t, recs[t])
    f_first, f_last = _first_features(recs[0], off, clip), _first_features(recs[-1], off, clip)
    starts = [(0, f_first), (0, f_first[:40]), (T - 1, f_last)]
    for b, (t0, f) in enumerate(starts):
        eng.init_lane(b, t0, f, poses[t0])
    out = []
    for t in range(1, T):
        scans = [t, t, T - 1 - t]
        eng.step(scans)
        res = eng.results()
        if retrack and not on_device:
            for b in range(3):
                if res[b]["retrack"]:
                    eng.retrack_lane(b, scans[b])
        out.append(dict(res=res, raw=eng.results_array().tobytes(),
                        feats=[eng.lane_features(b) for b in range(3)], peaks=[eng.lane_peaks(b) for b in range(3)],
                        pyr=[[eng.lane_image(b, lvl) for lvl in range(4)] for b in range(3)]))
    if upload_async:
        eng.synchronize()
        ctx.host_free(pinned)
    eng.close()
    ctx.close()
    return out, starts


@pytest.mark.parametrize("retrack", [True, False], ids=["retrack", "no_retrack"])
@pytest.mark.parametrize("layout", ENGINE_LAYOUTS, ids=lambda l: "clip%d_rows%d_stride%d_off%d" % l)
def test_engine_layout_matches_oracle_pipeline(layout, retrack):
    clip, rows, stride, off = layout
    recs, poses = _sequence(layout)
    T = len(recs)
    got_steps, starts = _run_layout(layout, retrack)
    on_device = retrack and _device_retrack(clip)
    pipes = []
    for b, (t0, f) in enumerate(starts):
        pipes.append(oracle.OdometryPipeline(recs[t0], f, poses[t0], detect=_detect if retrack else None, payload_off=off, clip=clip,
                                            motion_distortion=_motion_distortion(clip)))
    n_feat0 = min(len(starts[0][1]), len(starts[2][1]))
    n_rejected = n_retrack = n_kf = 0
    for t in range(1, T):
        g = got_steps[t - 1]
        for b in range(3):
            want = pipes[b].step(recs[t if b < 2 else T - 1 - t])
            got = g["res"][b]
            tag = (layout, retrack, t, b)
            assert got["n_tracked"] == want["n_tracked"], tag
            assert got["n_good"] == want["n_good"], tag
            assert got["n_inliers"] == want["n_inliers"], tag
            assert got["n_peaks"] == want["n_peaks"], tag
            assert got["clique_proven"], tag
            assert np.array_equal(g["feats"][b], pipes[b].blobCoord), tag
            for lvl in range(4):
                assert np.array_equal(g["pyr"][b][lvl], pipes[b].prevPyr[lvl]), (tag, lvl)
            assert np.array_equal(g["peaks"][b], want["peaks"]), tag
            if "R" in want:
                assert np.abs(got["h"] - want["h"]).max() <= POS_TOL, tag
                assert abs(np.arctan2(got["R"][1, 0], got["R"][0, 0]) - np.arctan2(want["R"][1, 0], want["R"][0, 0])) <= ANG_TOL, tag
            assert np.abs(got["pose"][:2] - want["pose"][:2]).max() <= POS_TOL, (tag, got["pose"], want["pose"])
            assert abs(got["pose"][2] - want["pose"][2]) <= ANG_TOL, (tag, got["pose"], want["pose"])
            assert got["new_keyframe"] == bool(want["new_keyframe"]), tag
            assert got["retrack"] == bool(want["retrack"]), tag
            assert got["retracked_on_device"] == (on_device and bool(want["retrack"])), tag
            n_rejected += want["n_good"] - want["n_inliers"]
            n_retrack += bool(want["retrack"])
            n_kf += bool(want["new_keyframe"])
    print("layout", layout, "retrack", retrack, "on device", on_device, "| first features", n_feat0, "rejected outliers", n_rejected,
          "retracks", n_retrack, "keyframes", n_kf)
    # not vacuous: features to track, outliers the clique removed, the retrack and keyframe branches taken
    assert n_feat0 >= 25 and n_rejected >= 1 and n_retrack >= 1 and n_kf >= 1, (n_feat0, n_rejected, n_retrack, n_kf)


@pytest.mark.parametrize("layout", [l for l in ENGINE_LAYOUTS if l[2] % 4 or l[3] % 4], ids=lambda l: "clip%d_stride%d_off%d" % (l[0], l[2], l[3]))
def test_async_pinned_upload_matches_sync_upload_in_unaligned_layouts(layout):
    """records of an odd stride / payload offset streamed from pinned host memory give exactly the results of upload_scan"""
    a, _ = _run_layout(layout, True)
    b, _ = _run_layout(layout, True, upload_async=True)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x["raw"] == y["raw"], k
        for lane in range(3):
            assert np.array_equal(x["feats"][lane], y["feats"][lane]) and np.array_equal(x["peaks"][lane], y["peaks"][lane]), (k, lane)
            for lvl in range(4):
                assert np.array_equal(x["pyr"][lane][lvl], y["pyr"][lane][lvl]), (k, lane, lvl)


# ------------------------------------------------------------------ standalone tracker
def _textured_pair(h, w, seed):
    """a smooth random texture with bright blobs, and the same texture moved by a sub-pixel shift plus a small rotation (f32 in
    [0, 1]) - most points track"""
    rng = np.random.default_rng(seed)
    g = 6.0
    base = rng.random((int(h / g) + 8, int(w / g) + 8))
    for _ in range(max(8, h * w // 6000)):
        base[rng.integers(0, base.shape[0]), rng.integers(0, base.shape[1])] += rng.uniform(1.0, 3.0)
    base /= base.max()
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)

    def sample(dx, dy, th):
        cx, cy = w / 2.0, h / 2.0
        c, s = np.cos(th), np.sin(th)
        X = ((c * (xx - cx) - s * (yy - cy) + cx + dx) / g) + 2.0
        Y = ((s * (xx - cx) + c * (yy - cy) + cy + dy) / g) + 2.0
        X = np.clip(X, 0, base.shape[1] - 2.001)
        Y = np.clip(Y, 0, base.shape[0] - 2.001)
        x0, y0 = np.floor(X).astype(int), np.floor(Y).astype(int)
        fx, fy = X - x0, Y - y0
        v = (base[y0, x0] * (1 - fx) * (1 - fy) + base[y0, x0 + 1] * fx * (1 - fy) +
             base[y0 + 1, x0] * (1 - fx) * fy + base[y0 + 1, x0 + 1] * fx * fy)
        return v.astype(np.float32)

    return sample(0, 0, 0), sample(-2.7, 1.3, 0.004)


def _border_points(h, w, seed):
    """for every pyramid level, points on each border of that level's image (in level-0 coordinates), just inside and just outside
    it, in the corners, and where the level-3 window is partly outside the image"""
    def edge(n):
        return [-1.0, -0.25, 0.0, 0.5, 1.0, 7.0, n - 8.0, n - 1.5, n - 1.0, n - 0.5, float(n), n + 0.25]
    pts = []
    for lvl in range(4):
        lw, lh = w, h
        for _ in range(lvl):
            lw, lh = (lw + 1) // 2, (lh + 1) // 2
        s = float(1 << lvl)
        xs, ys = edge(lw), edge(lh)
        pts += [(x * s, y * s) for x in xs for y in ys + [lh / 3.0, 2 * lh / 3.0]]
        pts += [(x * s, y * s) for x in (lw / 3.0, 2 * lw / 3.0) for y in ys]
    pts = np.unique(np.array(pts, np.float32), axis=0)
    np.random.default_rng(seed).shuffle(pts)
    return pts


def _edge_heavy(h, w, K, seed):
    """K points: border points of every level (a quarter of them for small K), the rest spread over the image and a little
    beyond it"""
    rng = np.random.default_rng(seed)
    edge = _border_points(h, w, seed)
    ne = min(len(edge), max(1, K // 4) if K < 1000 else len(edge))
    inner = np.column_stack((rng.uniform(-4, w + 4, K - ne), rng.uniform(-4, h + 4, K - ne))).astype(np.float32)
    pts = np.vstack((edge[:ne], inner))
    rng.shuffle(pts)
    return pts


@pytest.fixture(scope="module")
def ctx():
    from radarslampy_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("hw", KLT_SIZES, ids=lambda s: "%dx%d" % s)
def test_klt_matches_oracle_at_other_sizes(ctx, hw):
    h, w = hw
    assert min(h, w) >= 128                 # below that, OpenCV's pyramid depth is an open question (docs/PARITY.md)
    af, bf = _textured_pair(h, w, h * 7919 + w)
    au, bu = oracle.quantize_u8(af), oracle.quantize_u8(bf)
    pp, npyr = oracle.build_pyramid(au, 3), oracle.build_pyramid(bu, 3)
    for lvl in range(1, 4):                 # the device pyramid levels, through launch_pyr_down (level by level)
        assert np.array_equal(ctx.pyr_down_u8(pp[lvl - 1]), pp[lvl]), (hw, lvl)
    tracked = 0
    for K in (1, 63, 64, 65, 3000):
        pts = _edge_heavy(h, w, K, K + h + w)
        want_n, want_s, want_e = oracle.klt_on_pyramids(pp, npyr, pts)
        for a, b in ((au, bu), (af, bf)):   # the u8 and the f32 entry points (the latter quantises on the device)
            got_n, got_s, got_e = ctx.klt_track(a, b, pts)
            tag = (hw, K, a.dtype)
            assert np.array_equal(got_s, want_s), (tag, int((got_s != want_s).sum()))
            assert np.array_equal(got_n, want_n), (tag, float(np.abs(got_n - want_n).max()))
            assert np.array_equal(got_e, want_e), tag
        if K == 3000:
            tracked = int(want_s.sum())
    assert tracked >= 1500, tracked         # not vacuous: most points track
