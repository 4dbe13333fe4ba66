"""Times of the global map (csrc/loop_map.hip: LoopDetector.renderMap) on the GPU, each workload in a process of its own under its own
`timeout`; the first that fails ends the run.  The database is synthetic and of a realistic size: ENTRIES keyframes 2 m apart on a
lawnmower path over a square kilometre, POINTS points each (an Oxford scan keeps about 4 500 peaks) scattered over the radar's 87 m,
in a LoopDetector(keepClouds=True) at maxPoints 8192; the grid is the planned one at 0.5 m.

  kernels  the three parts of a render apart (roam_time_loop_db_map: HIP events, two warm launches first): the grid's clear, the splat
           and the compaction - with the splat's byte floor, the 16 bytes it must read per point, at the 6 300 GB/s a streaming kernel
           reaches on this part
  render   the blocking call LoopDetector.renderMap: host wall clock, two warm calls first - on the planned extent passed in, with and
           without the two grid read-backs, and with extent=None (bounds, plan, render)
  host     what there was before: LoopDetector.cloud(i) for every entry, then NumPy binning of the same definition (per entry a
           np.unique of the cell keys and two np.bincount sums) - host wall clock, one warm call first; its grids must equal render's

Records, not bounds (docs/MEASUREMENT.md), from

    python profiles/loop_map_time.py
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"kernels": 240, "render": 240, "host": 420}     # seconds per workload
ENTRIES, POINTS, CELL_M = 2000, 4500, 0.5
HBM_ACHIEVABLE_GBS = 6300.0


def world():
    """-> (ctx, detector holding ENTRIES synthetic clouds, poses (ENTRIES, 3), the planned extent)"""
    from radarslampy_amd import _ffi
    from radarslampy_amd.LoopClosure import LoopDetector
    rng = np.random.default_rng(0)
    ctx = _ffi.Context(0)
    det = LoopDetector(ENTRIES, 7, 3, min_gap=1, ctx=ctx, keepClouds=True, rows=400, maxPoints=8192)
    det.addDescriptors(rng.random((ENTRIES, 7, 3), dtype=np.float32))
    for e in range(ENTRIES):
        r, phi = rng.uniform(2.0, 87.0, POINTS), rng.uniform(0.0, 2.0 * np.pi, POINTS)
        det.db.set_cloud(e, np.stack([r * np.cos(phi), r * np.sin(phi)], axis=1))
    k = np.arange(ENTRIES)
    lane, along = np.divmod(k, 500)                       # four lanes of 1 km, 2 m between keyframes, every other lane driven back
    x = np.where(lane % 2 == 0, 2.0 * along, 2.0 * (499 - along))
    poses = np.stack([x, 250.0 * lane, np.where(lane % 2 == 0, 0.0, np.pi) + rng.normal(0.0, 0.05, ENTRIES)], axis=1)
    b, n = det.db.map_bounds(poses)
    assert n == ENTRIES * POINTS
    return ctx, det, poses, _ffi.map_plan(b, CELL_M)


def wall(call, calls, warm=2):
    for _ in range(warm):
        call()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        call()                                            # blocking: ends in a stream synchronise and a read-back
        t.append(1e3 * (time.perf_counter() - t0))
    return dict(calls=calls, ms_mean=float(np.mean(t)), ms_median=float(np.median(t)), ms_min=float(np.min(t)), ms_max=float(np.max(t)))


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def run_kernels():
    ctx, det, poses, extent = world()
    ms = [det.db.time_map(poses, CELL_M, extent, reps=10) for _ in range(3)]
    best = min(m[1] for m in ms)
    read = 16 * ENTRIES * POINTS
    return dict(workload="kernels", device=ctx.device_info(), entries=ENTRIES, points_per_entry=POINTS, cells=[extent[2], extent[3]], clear_ms=[m[0] for m in ms],
                splat_ms=[m[1] for m in ms], compact_ms=[m[2] for m in ms], splat_bytes_read=read, splat_floor_ms=1e3 * read / (HBM_ACHIEVABLE_GBS * 1e9),
                splat_gb_per_s=read / (best * 1e-3) / 1e9)


def run_render():
    ctx, det, poses, extent = world()
    m = det.renderMap(poses, cellM=CELL_M, extent=extent)
    return dict(workload="render", cells=[extent[2], extent[3]], occupied=int(np.count_nonzero(m.hits)), map_points=m.nPoints, outside=m.outside,
                grids=wall(lambda: det.renderMap(poses, cellM=CELL_M, extent=extent), 10),
                no_grids=wall(lambda: det.renderMap(poses, cellM=CELL_M, extent=extent, grids=False), 10),
                planned=wall(lambda: det.renderMap(poses, cellM=CELL_M), 10), grids_sha=sha(m.hits, m.views))


def run_host():
    from radarslampy_amd import _ffi
    ctx, det, poses, extent = world()
    ox, oy, W, H = extent
    cs = _ffi.map_pose_table(poses)
    moved = [0]

    def call():
        hits, views = np.zeros(W * H, np.uint32), np.zeros(W * H, np.uint32)
        sx, sy = np.zeros(W * H, np.uint64), np.zeros(W * H, np.uint64)
        moved[0] = 0
        for e in range(len(det)):
            xy, _ = det.cloud(e)
            moved[0] += xy.nbytes
            c, s = cs[e]
            dx = ((((c * xy[:, 0]) - (s * xy[:, 1])) + poses[e, 0]) - ox) / CELL_M
            dy = ((((s * xy[:, 0]) + (c * xy[:, 1])) + poses[e, 1]) - oy) / CELL_M
            ok = (dx >= 0.0) & (dx < W) & (dy >= 0.0) & (dy < H)
            dx, dy = dx[ok], dy[ok]
            fu, fv = np.floor(dx), np.floor(dy)
            k, inv, cnt = np.unique(fv.astype(np.int64) * W + fu.astype(np.int64), return_inverse=True, return_counts=True)
            hits[k] += cnt.astype(np.uint32)
            views[k] += np.uint32(1)
            sx[k] += np.bincount(inv, weights=np.floor((dx - fu) * 65536.0)).astype(np.uint64)
            sy[k] += np.bincount(inv, weights=np.floor((dy - fv) * 65536.0)).astype(np.uint64)
        return hits.reshape(H, W), views.reshape(H, W)
    out = wall(call, 3, warm=1)
    hits, views = call()
    return dict(workload="host", **out, bytes_over_pcie_per_call=moved[0], grids_sha=sha(hits, views))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(LIMITS))
    args = ap.parse_args()
    if args.workload:
        run = {"kernels": run_kernels, "render": run_render, "host": run_host}
        print(json.dumps(run[args.workload]()))
        return 0
    for w in ("kernels", "render", "host"):               # a fresh process each; the first one that fails ends the run
        r = subprocess.run(["timeout", "-k", "10", str(LIMITS[w]), sys.executable, os.path.abspath(__file__), "--workload", w])
        if r.returncode != 0:
            print(json.dumps(dict(workload=w, failed=r.returncode)))
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
