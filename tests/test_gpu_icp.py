"""GPU (-m gpu): loop-closure verification by batched 2-D ICP (csrc/icp.hip, radarslampy_amd/LoopClosure.py) against the model
tests/icp_model.py on the inputs of tests/icp_cases.py.  Parity is unpinned: nothing in the reference computes this.

Exact cases: identical clouds give exactly (0, 0, 0) and rms 0; an exact rigid motion is recovered to 1e-12; of two dst points with
one float32 rounding the lowest index is the partner (the two orders differ by the 1e-8 m between the points).  Every case of
icp_cases against the model: pose and rms within cases.tolerance() - ten times the largest difference between the model and its
variants, measured in test_icp_cpu.py (the floor 1e-9 holds) - status equal, iterations within one, n_inliers within 1 %.  A call
repeated, a pair alone or in a batch of 130, first or last, in one chunk or many: the same bits.  The stated limit as one pair.  The
revisit world at full density, peaks and clouds from the device: LoopDetector's candidates verified, the three true edges within the
truth bound of the CPU test, every wrong place rejected at the default threshold; closeLoops pulls eleven drifted keyframes back.
Every measured difference is printed; the largest are copied to docs/PARITY.md as records."""
import types

import numpy as np
import pytest

import icp_cases as cases
import icp_model as model
import scan_context_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from radarslampy_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


def _one(ctx, name):
    src, dst, init, opts = cases.case(name)
    poses, stats = ctx.icp2d_batch([(src, dst)], init, opts)
    return poses[0], stats[0]


# ---------------------------------------------------------------------------------------------------------------- exact cases
def test_identical_clouds_give_exactly_the_identity(ctx):
    from radarslampy_amd import _ffi
    pose, st = _one(ctx, "identical_64")
    assert np.array_equal(pose, np.zeros(3)) and st["rms"] == 0.0 and st["status"] == _ffi.ICP_OK and st["n_inliers"] == 64


def test_exact_rigid_motion_is_recovered(ctx):
    from radarslampy_amd import _ffi
    pose, st = _one(ctx, "rigid_64")
    err = np.abs(pose - np.array([0.3, 0.4 * np.cos(1.0), 0.4 * np.sin(1.0)]))
    print(f"rigid_64: |pose - truth| = {err}, rms {st['rms']:.3e}, {st['iterations']} iterations")
    assert err.max() <= 1e-12 and st["status"] == _ffi.ICP_OK and st["n_inliers"] == 64 and st["rms"] <= 1e-12


def test_lowest_index_wins_among_equal_float32_points(ctx):
    low, _ = _one(ctx, "dup_low_first")
    high, _ = _one(ctx, "dup_high_first")
    d = high - low
    print(f"dup: high first - low first = {d}")
    # the partner is the half that comes first, so the translation moves by the 1e-8 m between the halves; were the highest index
    # (or any fixed half) taken, the two results would be equal
    assert abs(d[0]) <= 1e-12 and np.abs(d[1:] - cases.DUP_DELTA).max() <= 1e-12
    for name, got in (("dup_low_first", low), ("dup_high_first", high)):
        assert np.abs(got - cases.case_model(name)[0]).max() <= 1e-12


# ---------------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("name", cases.CASES)
def test_case_against_the_model(ctx, name):
    tol_m, tol_rad = cases.tolerance()
    pose, st = _one(ctx, name)
    want, ws = cases.case_model(name)
    d_rad = abs(model.normalize_angle(pose[0] - want[0]))
    d_m = float(np.abs(pose[1:] - want[1:]).max())
    d_rms = 0.0 if (np.isinf(st["rms"]) and np.isinf(ws["rms"])) else abs(st["rms"] - ws["rms"])
    print(f"{name}: |theta| {d_rad:.3e} rad, |t| {d_m:.3e} m, |rms| {d_rms:.3e} m (tolerance {tol_m:.1e} m, {tol_rad:.1e} rad); status "
          f"{st['status']} / {ws['status']}, iterations {st['iterations']} / {ws['iterations']}, inliers {st['n_inliers']} / {ws['n_inliers']}, "
          f"pairs {st['n_pairs_last']} / {ws['n_pairs_last']}")
    assert st["status"] == ws["status"]
    assert abs(int(st["iterations"]) - ws["iterations"]) <= 1
    assert d_rad <= tol_rad and d_m <= tol_m and d_rms <= tol_m
    assert abs(int(st["n_inliers"]) - ws["n_inliers"]) <= 0.01 * ws["n_inliers"]
    if ws["status"] == model.FEW_PAIRS:             # the pose stays: the very bits of the seed
        assert np.array_equal(pose, np.array(cases.case(name)[2]))


def test_named_outcomes(ctx):
    """the statuses the cases are there for, asserted by name and not only through the model"""
    from radarslampy_amd import _ffi
    for name in ("n0", "m0", "gated_out", "n1_m1", "n2_m2"):
        pose, st = _one(ctx, name)
        assert st["status"] == _ffi.ICP_FEW_PAIRS and st["iterations"] == 0 and np.array_equal(pose, np.array(cases.case(name)[2])), name
    for name in ("n0", "m0", "gated_out"):
        _, st = _one(ctx, name)
        assert st["n_inliers"] == 0 and np.isinf(st["rms"]) and st["rms"] > 0, name
    _, st = _one(ctx, "max_iterations_1")
    assert st["status"] == _ffi.ICP_MAX_ITERATIONS and st["iterations"] == 1


# ---------------------------------------------------------------------------------------------------------------- bits
def test_same_bits_alone_in_a_batch_at_either_end_and_in_any_chunk(ctx, monkeypatch):
    names, pairs, init = cases.batch130()
    assert len(pairs) == 130 and "n0" in names and "m0" in names
    poses, stats = ctx.icp2d_batch(pairs, init)
    again = ctx.icp2d_batch(pairs, init)
    assert poses.tobytes() == again[0].tobytes() and stats.tobytes() == again[1].tobytes()           # a call repeated
    first = {}
    for k, name in enumerate(names):                                                                # one case at several positions
        if name in first:
            assert poses[k].tobytes() == poses[first[name]].tobytes() and stats[k].tobytes() == stats[first[name]].tobytes(), name
        else:
            first[name] = k
            p1, s1 = _one(ctx, name)                                                                # alone
            assert p1.tobytes() == poses[k].tobytes() and s1.tobytes() == stats[k].tobytes(), name
    # the first pair against the last position
    rev = ctx.icp2d_batch(pairs[::-1], init[::-1])
    assert rev[0][::-1].tobytes() == poses.tobytes() and rev[1][::-1].tobytes() == stats.tobytes()
    monkeypatch.setenv("ROAM_ICP_CHUNK_BYTES", "200000")                                            # a few pairs per launch
    cut = ctx.icp2d_batch(pairs, init)
    assert cut[0].tobytes() == poses.tobytes() and cut[1].tobytes() == stats.tobytes()


# ---------------------------------------------------------------------------------------------------------------- the limit
def test_a_pair_at_the_stated_limit(ctx):
    """8192 x 8192 points, an exact motion: both blocks of rows and both LDS tiles are full.  The gate stays at 0.6 m, well under
    half the 2.5 m spacing, so the nearest neighbour is the true partner from the seed on and the motion is recovered in two updates"""
    from radarslampy_amd import _ffi
    rng = np.random.default_rng(8192)
    src, _ = cases._scene(rng, cases.MAX_POINTS, cases.MAX_POINTS, (0, 0, 0))
    truth = (0.2, 0.3, -0.2)
    dst = cases.rigid(src, *truth)[rng.permutation(len(src))]
    poses, stats = ctx.icp2d_batch([(src, dst)], (0.2 - 0.001, 0.25, -0.15), dict(gate_start=0.6, gate_end=0.6, gate_decay=1.0))
    err = np.abs(poses[0] - truth)
    print(f"limit: |pose - truth| = {err}, stats {stats[0]}")
    assert err.max() <= 1e-10 and stats[0]["status"] == _ffi.ICP_OK and stats[0]["n_inliers"] == cases.MAX_POINTS
    assert stats[0]["iterations"] <= 3 and stats[0]["rms"] <= 1e-10


def test_raw_abi_refuses_sizes_and_offsets(ctx):
    from radarslampy_amd import _ffi
    lib = ctx.lib
    xy = np.zeros((cases.MAX_POINTS + 1, 2))
    init, pose, stats = np.zeros(3), np.zeros(3), np.zeros(1, _ffi.ICP_STATS)

    def call(src_off, dst_off):
        so, do = np.asarray(src_off, np.int32), np.asarray(dst_off, np.int32)
        return lib.roam_icp2d_batch(ctx.h, len(so) - 1, _ffi._ptr(so), _ffi._ptr(xy), _ffi._ptr(do), _ffi._ptr(xy), _ffi._ptr(init), None,
                                    _ffi._ptr(pose), _ffi._ptr(stats))
    assert call([0, cases.MAX_POINTS + 1], [0, 4]) == _ffi.ROAM_E_ARG and b"8192" in lib.roam_last_error(ctx.h)
    assert call([0, 4], [0, cases.MAX_POINTS + 1]) == _ffi.ROAM_E_ARG
    assert call([4, 2], [0, 4]) == _ffi.ROAM_E_ARG and b"decreases" in lib.roam_last_error(ctx.h)
    assert call([0, 4], [-1, 4]) == _ffi.ROAM_E_ARG
    assert call([0, 4], [0, 4]) == _ffi.ROAM_OK                      # the same arrays within the limits are taken


# ---------------------------------------------------------------------------------------------------------------- the public interface
def test_polar_axes_agree_with_the_cartesian_image(ctx):
    """one reflector: polarIndToLocalMetres puts it where convertPolarImageToCartesian's image has it, (pixel - centre) resolution with
    x along the columns and y along the rows"""
    from radarslampy_amd import parseData
    from radarslampy_amd.LoopClosure import polarIndToLocalMetres
    rows, cols, th, r = 400, 600, 70, 400            # 63 degrees, 400 bins out
    polar = np.zeros((rows, cols), np.float32)
    polar[th - 1:th + 2, r - 4:r + 5] = 1.0
    cart = parseData.convertPolarImageToCartesian(polar)            # downsample factor 2: 600 x 600, 0.0864 m per pixel
    yy, xx = np.nonzero(cart > 0.5)
    centre = cart.shape[0] / 2.0
    got = np.array([xx.mean() - centre, yy.mean() - centre]) * parseData.RANGE_RESOLUTION_M * 2
    want = polarIndToLocalMetres(np.array([[th, r]]), rows)[0]
    print(f"reflector: the Cartesian image has it at {got} m, polarIndToLocalMetres at {want} m")
    assert np.abs(got - want).max() <= 0.1                           # about one Cartesian pixel; a swapped or mirrored axis is metres off


@pytest.fixture(scope="module")
def revisit_clouds():
    """the eleven full-density clouds: records rendered by radarslampy_amd.synth, peaks by the device"""
    from radarslampy_amd.getPointCloud import getPointCloudFromRecord
    from radarslampy_amd.LoopClosure import polarIndToLocalMetres
    recs = sc.revisit_records()
    peaks = [getPointCloudFromRecord(r) for r in recs]
    return peaks, [polarIndToLocalMetres(p, recs[0].shape[0]) for p in peaks]


def _detector(ctx, k):
    from radarslampy_amd import synth
    from radarslampy_amd.LoopClosure import LoopDetector
    det = LoopDetector(16, sc.REVISIT_S, sc.REVISIT_R, clip_px=sc.REVISIT_CLIP, min_gap=1, max_distance=np.inf, k=k, ctx=ctx)
    imgs = np.stack([r[:, synth.META:synth.META + synth.CLIP] for r in sc.revisit_records()]).astype(np.float32) / np.float32(255.0)
    assert det.add(imgs) == 0
    return det


def test_revisit_world_true_edges_and_wrong_places(ctx, revisit_clouds):
    from radarslampy_amd.LoopClosure import verifyCandidates
    _, clouds = revisit_clouds
    bound_m, bound_rad = cases.truth_bound()
    det = _detector(ctx, 3)
    n_places = len(sc.PLACES)
    q = np.arange(n_places, n_places + len(sc.REVISITS), dtype=np.int32)
    ci, cd, yaw = det.query(q)
    det.close()
    edges, table = verifyCandidates(clouds, q, ci, yaw)
    for row in table:
        print(f"query {row['query']} candidate {row['candidate']}: fraction {row['fraction']:.4f}, rms {row['rms']:.4f} m, status {row['status']}, "
              f"{row['iterations']} iterations, accepted {row['accepted']}")
    assert len(table) == 9
    assert [(e[0], e[1]) for e in edges] == [(place, n_places + t) for t, (place, _) in enumerate(sc.REVISITS)]
    for t, (place, _) in enumerate(sc.REVISITS):
        z = edges[t][2]
        e_m, e_rad = cases.pose_error(np.array([z[2], z[0], z[1]]), cases.revisit_truth(t))
        print(f"revisit {t}: edge error {e_m:.4f} m, {e_rad:.5f} rad (bound {bound_m:.4f} m, {bound_rad:.5f} rad)")
        assert e_m <= bound_m and e_rad <= bound_rad
    for row in table:                                                # every wrong place is rejected at the default threshold
        assert row["accepted"] == (row["candidate"] == sc.REVISITS[row["query"] - n_places][0])


def test_close_loops_pulls_drifted_keyframes_back(ctx, revisit_clouds):
    from radarslampy_amd.LoopClosure import closeLoops
    peaks, _ = revisit_clouds
    bound_m, bound_rad = cases.truth_bound()
    n_places = len(sc.PLACES)
    true = np.array([sc.place_pose(i) for i in range(n_places)] + [p for _, p in sc.REVISITS])
    drift = np.cumsum(np.tile([0.35, -0.25, 0.006], (len(true), 1)), axis=0) - [0.35, -0.25, 0.006]      # none at keyframe 0, 3.5 m at the last
    kfs = [types.SimpleNamespace(pose=true[k] + drift[k], pointCloud=peaks[k]) for k in range(len(true))]
    det = _detector(ctx, 2)
    # the weights.  The keyframes lie up to 1.4 km apart, so a heading error of 0.036 rad at one of them moves its neighbour by 50 m:
    # under unit odometry information (a sigma of 1 m on such a leg) the optimiser keeps the drifted heading of revisit 1 rather than
    # bend a leg, whatever the loop edge says (tests/pose_graph_model.py gives the same 0.0357 rad).  The odometry translation is
    # weighted as sigma = 100 m, the loop edges, good to centimetres, as sigma = 0.01
    graph, edges, table = closeLoops(kfs, det, rows=sc.revisit_records()[0].shape[0], loopInformation=1e4 * np.eye(3),
                                     odomInformation=np.diag([1e-4, 1e-4, 1.0]))
    det.close()
    assert sorted((e[0], e[1]) for e in edges) == sorted((place, n_places + t) for t, (place, _) in enumerate(sc.REVISITS))
    for t, (place, _) in enumerate(sc.REVISITS):
        truth = model.relative_pose(true[place], true[n_places + t])
        before = model.relative_pose(kfs[place].pose, kfs[n_places + t].pose) - truth
        after = model.relative_pose(graph.get_pose(place), graph.get_pose(n_places + t)) - truth
        b_m, a_m = np.hypot(*before[:2]), np.hypot(*after[:2])
        b_r, a_r = abs(model.normalize_angle(before[2])), abs(model.normalize_angle(after[2]))
        print(f"revisit {t}: relative pose error {b_m:.3f} m, {b_r:.4f} rad before; {a_m:.4f} m, {a_r:.5f} rad after")
        assert a_m < b_m and a_r < b_r and a_m <= bound_m and a_r <= bound_rad
