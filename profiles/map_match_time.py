"""Times of the map matching (csrc/map_match.hip: Mapping.MapLocalizer, LoopDetector.localize) on the GPU, each workload in a process of
its own under its own `timeout`; the first that fails ends the run.  The map is synthetic and of a realistic size: about 1000 x 1000
cells of 0.25 m with 3 % of them occupied in streaks (walls), QUERIES queries of POINTS points each (an Oxford scan keeps about 4 500
peaks) scattered over the radar's 87 m around priors inside the map, in a LoopDetector(keepClouds=True) at maxPoints 8192.

  kernels   roam_time_map_match (HIP events, two warm launches first): the field's build from the grids, and the match kernels on the
            window 25 x 25 x 25 (angles x rows x columns) and on the large window 61 x 65 x 65 - with the lookups of each, queries x
            points x candidates, and the rate that makes.  A lookup is one byte gathered from the field, which at 1 MB lives in L2
  localize  the blocking call LoopDetector.localize on the stored clouds: host wall clock, two warm calls first, both windows
  host      what there was before: the NumPy model of the same definition (tests/map_match_model.py, its vectorised form) on ONE query
            of the same shape at the 25 x 25 x 25 window - host wall clock; its record must equal localize's

Records, not bounds (docs/MEASUREMENT.md), from

    python profiles/map_match_time.py
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
LIMITS = {"kernels": 300, "localize": 300, "host": 300}   # seconds per workload
QUERIES, POINTS, CELL_M, SIDE = 64, 4500, 0.25, 1000
WINDOWS = {"25x25x25": dict(reachM=3.0, reachRad=0.12, stepRad=0.01), "61x65x65": dict(reachM=8.0, reachRad=0.30, stepRad=0.01)}


def world():
    """-> (ctx, detector holding QUERIES synthetic clouds, the GlobalMap, its localizer, priors (QUERIES, 3))"""
    from radarslampy_amd import _ffi
    from radarslampy_amd.LoopClosure import LoopDetector
    from radarslampy_amd.Mapping import GlobalMap
    rng = np.random.default_rng(0)
    hits = np.zeros((SIDE, SIDE), np.uint32)
    for _ in range(3000):                                 # streaks of ten cells, along x or along y
        v, u = rng.integers(0, SIDE - 10, 2)
        if rng.random() < 0.5:
            hits[v, u:u + 10] += 3
        else:
            hits[v:v + 10, u] += 3
    views = np.minimum(hits, 2).astype(np.uint32)
    gmap = GlobalMap((-125.0, -125.0), CELL_M, (SIDE, SIDE), hits, views, np.zeros((0, 2)), np.zeros(0, np.uint32), np.zeros(0, np.uint32), 0)
    ctx = _ffi.Context(0)
    loc = gmap.localizer(ctx=ctx)
    det = LoopDetector(QUERIES, 7, 3, min_gap=1, ctx=ctx, keepClouds=True, rows=400, maxPoints=8192)
    det.addDescriptors(rng.random((QUERIES, 7, 3), dtype=np.float32))
    for e in range(QUERIES):
        r, phi = rng.uniform(2.0, 87.0, POINTS), rng.uniform(0.0, 2.0 * np.pi, POINTS)
        det.db.set_cloud(e, np.stack([r * np.cos(phi), r * np.sin(phi)], axis=1))
    priors = np.stack([rng.uniform(-30.0, 30.0, QUERIES), rng.uniform(-30.0, 30.0, QUERIES), rng.uniform(-np.pi, np.pi, QUERIES)], axis=1)
    return ctx, det, gmap, loc, priors


def wall(call, calls, warm=2):
    for _ in range(warm):
        call()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        call()                                            # blocking: ends in a stream synchronise and a read-back
        t.append(1e3 * (time.perf_counter() - t0))
    return dict(calls=calls, ms_mean=float(np.mean(t)), ms_median=float(np.median(t)), ms_min=float(np.min(t)), ms_max=float(np.max(t)))


def run_kernels():
    ctx, det, gmap, loc, priors = world()
    clouds = [det.cloud(e)[0] for e in range(QUERIES)]
    out = dict(workload="kernels", device=ctx.device_info(), queries=QUERIES, points_per_query=POINTS, cells=[SIDE, SIDE],
               occupied=int(np.count_nonzero(gmap.hits)), field_nonzero=int(np.count_nonzero(loc.field())))
    for name, kw in WINDOWS.items():
        w = loc.window(**kw)
        ms = [loc._field.time_match(gmap.hits, gmap.views, clouds, priors, w, reps=5) for _ in range(3)]
        lookups = QUERIES * POINTS * w[0] * (2 * w[2] + 1) * (2 * w[3] + 1)
        out[name] = dict(window=[w[0], 2 * w[3] + 1, 2 * w[2] + 1], field_ms=[m[0] for m in ms], match_ms=[m[1] for m in ms], lookups=lookups,
                         lookups_per_s=lookups / (min(m[1] for m in ms) * 1e-3))
    return out


def run_localize():
    ctx, det, gmap, loc, priors = world()
    idx = np.arange(QUERIES)
    out = dict(workload="localize", queries=QUERIES)
    for name, kw in WINDOWS.items():
        t = det.localize(loc, idx, priors, **kw)
        out[name] = dict(found=int(t["found"].sum()), mean_fraction=float(t["fraction"].mean()), **wall(lambda: det.localize(loc, idx, priors, **kw), 5))
    out["first_record"] = [float(v) if isinstance(v, (float, np.floating)) else int(v) for v in det.localize(loc, [0], priors[:1], **WINDOWS["25x25x25"])[0]]
    return out


def run_host():
    import map_match_model as model
    from radarslampy_amd import _ffi
    ctx, det, gmap, loc, priors = world()
    w = loc.window(**WINDOWS["25x25x25"])
    F, cloud = loc.field(), det.cloud(0)[0]
    cs = _ffi.map_match_angles(priors[:1], w[0], w[1])[0]
    call = lambda: model.match(F, cloud, priors[0], cs, w[1], CELL_M, gmap.origin[0], gmap.origin[1], w[2], w[3])      # noqa: E731
    out = wall(call, 3, warm=1)
    pose, info, _ = call()
    t = det.localize(loc, [0], priors[:1], **WINDOWS["25x25x25"])[0]
    same = bool(pose.tobytes() == np.array([t["x"], t["y"], t["theta"]]).tobytes() and info.tolist() == [int(t[k]) for k in ("score", "i", "b", "a", "nPoints", "nInside")])
    return dict(workload="host", queries=1, window=[w[0], 2 * w[3] + 1, 2 * w[2] + 1], equals_localize=same, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(LIMITS))
    args = ap.parse_args()
    if args.workload:
        run = {"kernels": run_kernels, "localize": run_localize, "host": run_host}
        print(json.dumps(run[args.workload]()))
        return 0
    for w in ("kernels", "localize", "host"):             # a fresh process each; the first one that fails ends the run
        r = subprocess.run(["timeout", "-k", "10", str(LIMITS[w]), sys.executable, os.path.abspath(__file__), "--workload", w])
        if r.returncode != 0:
            print(json.dumps(dict(workload=w, failed=r.returncode)))
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
