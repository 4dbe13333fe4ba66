"""Shared, seeded inputs of the motion-compensation tests (test_loop_cloud_motion_cpu.py, test_gpu_loop_cloud_motion.py): the moving
pairs of one place seen twice at driving speed, their model clouds and the model ICP's edges.  Everything is computed once and cached;
nothing here touches a device."""
import ctypes
import ctypes.util
import functools

import numpy as np

import icp_cases
import icp_model
import loop_cloud_motion_model as model

RES = icp_cases.RANGE_RESOLUTION_M
PLACE_POSE, REVISIT_POSE = (0.0, 0.0, 0.0), (1.0, -0.5, np.pi / 2)      # t_index 0 and 20 of StreamWorld(5, per_tile=40)
SEED = (np.pi / 2, 0.0, 0.0)
STRIDE = 4                                           # every 4th peak, as icp_cases.truth_bound()
# (velocity at the place, velocity at the revisit): vx, vy in m/s, vtheta in rad/s
MOVING_PAIRS = [((12.0, 0.0, 0.2), (12.0, 0.0, -0.2)), ((15.0, 0.0, 0.0), (-15.0, 0.0, 0.0)), ((8.0, 0.0, 0.4), (8.0, 0.0, 0.4))]


def libm():
    """(cos, sin) of the host's libm on float64 arrays - what the library's tables are made with"""
    m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    out = []
    for name in ("cos", "sin"):
        f = getattr(m, name)
        f.restype, f.argtypes = ctypes.c_double, [ctypes.c_double]
        out.append(lambda a, f=f: np.array([f(float(x)) for x in np.asarray(a, np.float64).ravel()], np.float64).reshape(np.shape(a)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def records():
    """six Oxford records: pair p is records 2 p (the place) and 2 p + 1 (the revisit), each rendered with its velocity -> (records,
    velocities (6, 3))"""
    from radarslampy_amd import synth
    w = synth.StreamWorld(5, per_tile=40)
    recs, vel = [], []
    for v_place, v_revisit in MOVING_PAIRS:
        recs.append(synth.render_stream_record(w, PLACE_POSE, t_index=0, velocity=v_place))
        recs.append(synth.render_stream_record(w, REVISIT_POSE, t_index=20, velocity=v_revisit))
        vel += [v_place, v_revisit]
    return recs, np.array(vel, np.float64)


@functools.lru_cache(maxsize=None)
def peaks():
    import oracle
    return [oracle.peaks_from_record_u8(r) for r in records()[0]]


def truth():
    """the pose (th, tx, ty) that aligns the revisit to the place: x_place^-1 x_revisit"""
    z = icp_model.relative_pose(PLACE_POSE, REVISIT_POSE)
    return np.array([z[2], z[0], z[1]])


def model_clouds(trig, tables):
    """the six stored clouds at every 4th peak from the polar table `trig` = (cos_t, sin_t); tables: one motion table per record, or
    None for the raw clouds"""
    return [model.cloud(p, *trig, RES, 8192, STRIDE, None if tables is None else tables[i])[0] for i, p in enumerate(peaks())]


def model_edges(clouds):
    """the model ICP of the three pairs, revisit onto place from SEED -> [(pose, stats)]"""
    return [icp_model.icp(clouds[2 * p + 1], clouds[2 * p], SEED) for p in range(len(MOVING_PAIRS))]


@functools.lru_cache(maxsize=None)
def numpy_model():
    """the pairs on NumPy's own tables (no library): -> (raw edges, compensated edges), each [(pose, stats)]"""
    rows = records()[0][0].shape[0]
    phi = 2.0 * np.pi * np.arange(rows, dtype=np.float64) / rows
    trig = (np.cos(phi), np.sin(phi))
    tables = [model.table(rows, v) for v in records()[1]]
    return model_edges(model_clouds(trig, None)), model_edges(model_clouds(trig, tables))
