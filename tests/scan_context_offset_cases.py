"""Shared, seeded inputs of the origin-offset scan-context tests (test_scan_context_offsets_cpu.py, test_gpu_scan_context_offsets.py).
The model's results are computed once and cached; nothing here touches a device."""
import functools

import numpy as np

import scan_context_cases as sc
import scan_context_offset_model as model

RES = 0.0432                                        # metres per range bin (parseData.RANGE_RESOLUTION_M)
S, R, CLIP = sc.REVISIT_S, sc.REVISIT_R, sc.REVISIT_CLIP
FAR_M, FAR_YAW = 5.0, 1.0
# (place, direction of the displacement in the world frame): the query is FAR_M metres from the place, its yaw the place's + FAR_YAW
FAR_REVISITS = [(0, 0.4), (0, 2.3), (3, 0.4), (3, 2.3)]
FAR_ICP = (0, 3)                                    # the two pairs that go through the ICP: place 0 / 0.4 rad, place 3 / 2.3 rad
GRID = model.offset_grid(5.0, 2.5)                  # 24 offsets


def far_pose(t):
    place, d = FAR_REVISITS[t]
    x, y, yaw = sc.place_pose(place)
    return (x + FAR_M * np.cos(d), y + FAR_M * np.sin(d), yaw + FAR_YAW)


@functools.lru_cache(maxsize=None)
def far_records():
    """the four far revisits as Oxford records, t_index 30 .. 33"""
    from radarslampy_amd import synth
    w = synth.StreamWorld(5, per_tile=40)
    return [synth.render_stream_record(w, far_pose(t), t_index=30 + t) for t in range(len(FAR_REVISITS))]


def payload(rec):
    from radarslampy_amd import synth
    return rec[:, synth.META:synth.META + CLIP]


@functools.lru_cache(maxsize=None)
def place_descriptors():
    return sc.revisit_descriptors(0)[:len(sc.PLACES)]


@functools.lru_cache(maxsize=None)
def far_variants(t):
    """(25, S, R) float32 of far revisit t: variant 0 the plain descriptor, then GRID's"""
    ob = model.offsets_bins(GRID, RES)
    pl = payload(far_records()[t])
    return np.concatenate([sc.model.describe_u8(pl, S, R, CLIP, 0)[None], model.describe_offsets_u8(pl, S, R, CLIP, 0, ob)])


@functools.lru_cache(maxsize=None)
def far_model(t):
    """far revisit t against the eight places -> (dist (8,), shift (8,), variant (8,)) over the variants, then the plain (dist, shift)"""
    V = far_variants(t)
    d, s, v = model.distances_variants(V[None], place_descriptors())
    pd, ps, _ = sc.model.distances(V[:1], place_descriptors())
    return (d[0], s[0], v[0]), (pd[0], ps[0])


def far_seeds(t):
    """-> (the plain seed (yaw, 0, 0), the offset seed (yaw, -R(yaw) o)) of far revisit t against its true place, from the model"""
    place = FAR_REVISITS[t][0]
    (_, s, v), _ = far_model(t)
    yaw = float(sc.model.shift_to_yaw(s[place], S))
    return np.array([yaw, 0.0, 0.0]), model.seed(yaw, model.variant_offsets(v[place], GRID))


@functools.lru_cache(maxsize=None)
def far_cloud(t):
    """the peak cloud of far revisit t by the oracle's peak extraction, full density, metres"""
    import icp_cases
    import oracle
    rec = far_records()[t]
    return icp_cases.cloud_from_peaks(np.asarray(oracle.peaks_from_record_u8(rec), np.float64), rec.shape[0])


@functools.lru_cache(maxsize=None)
def far_icp_model(t, offset_seed):
    """the ICP model at full density, default options, far revisit t onto its place from one of far_seeds(t) -> (pose, stats)"""
    import icp_cases
    import icp_model
    return icp_model.icp(far_cloud(t), icp_cases.revisit_clouds_oracle()[FAR_REVISITS[t][0]], tuple(far_seeds(t)[1 if offset_seed else 0]))


FAR_ICP_GOLDEN = "far_icp_model.npz"                # tests/golden: far_icp_model(t, True) of t in FAR_ICP, recorded for the GPU test


def far_icp_golden():
    """-> {t: (pose (3,), n_inliers, rms)}: the recorded model results (test_scan_context_offsets_cpu.py holds them to the model)"""
    import os
    g = np.load(os.path.join(sc.GOLDEN, FAR_ICP_GOLDEN))
    return {int(t): (g["pose"][i], int(g["n_inliers"][i]), float(g["rms"][i])) for i, t in enumerate(g["t"])}


def far_truth(t):
    """the true pose (th, tx, ty) that aligns far revisit t to its place: x_place^-1 x_query"""
    import icp_model
    z = icp_model.relative_pose(sc.place_pose(FAR_REVISITS[t][0]), far_pose(t))
    return np.array([z[2], z[0], z[1]])


def true_offset(t):
    """the origin offset (metres, query's sensor frame) that moves the query's origin onto the place: -R(theta)^T t of the truth"""
    th, tx, ty = far_truth(t)
    c, s = np.cos(th), np.sin(th)
    return np.array([-(c * tx + s * ty), -(-s * tx + c * ty)])
