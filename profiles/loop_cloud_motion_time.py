"""Times of the loop database's cloud build with and without motion compensation (csrc/loop_cloud.hip: cloud_gather_kernel and
cloud_gather_motion_kernel) on the GPU: 64 Oxford records resident in an engine's pool (the eleven scans of the revisit world of
tests/scan_context_cases.py in turn, about 4 500 peaks each, all kept), built into the free entries of an empty
LoopDetector(keepClouds=True) by Engine.time_loop_cloud - HIP events on the context's stream around 50 launches of each kernel, two
warm ones first.  Each workload runs three times in a process of its own under its own `timeout`; the first that fails ends the run.

  plain    velocities=None: the peak row kernel and cloud_gather_kernel (roam_engine_time_loop_cloud)
  motion   a velocity for every record: the same row kernel and cloud_gather_motion_kernel, its table (32 bytes per azimuth row)
           uploaded once before the launches (roam_engine_time_loop_cloud_motion)
  mixed    every second record without a velocity: the motion kernel with both of its paths in one launch

--plain-only runs `plain` alone: with ROAM_LIB pointing at another build of the library (and ROAM_LIB_PARTIAL=1 when that build lacks
newer entries) it is the comparison of the plain kernel between two builds.  Records, not bounds (docs/MEASUREMENT.md), from

    python profiles/loop_cloud_motion_time.py
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
LIMIT = 240                                          # seconds per workload
RECORDS, REPS, RUNS = 64, 50, 3
VELOCITIES = [(12.0, 0.0, 0.2), (-15.0, 0.0, 0.0), (8.0, 0.0, 0.4), (15.0, 3.0, 0.5), (-30.0, 10.0, -1.5)]


def run(workload):
    import scan_context_cases as sc
    from radarslampy_amd import _ffi
    from radarslampy_amd.engine import Engine
    from radarslampy_amd.LoopClosure import LoopDetector
    recs = sc.revisit_records()
    ctx = _ffi.Context(0)
    eng = Engine(1, RECORDS, ctx=ctx, retrack_on_device=False)
    for t in range(RECORDS):
        eng.upload_scan(t, recs[t % len(recs)])
    det = LoopDetector(RECORDS, sc.REVISIT_S, sc.REVISIT_R, clip_px=sc.REVISIT_CLIP, min_gap=1, ctx=ctx, keepClouds=True, rows=recs[0].shape[0])
    vel = None
    if workload != "plain":
        vel = [None if workload == "mixed" and t % 2 else VELOCITIES[t % len(VELOCITIES)] for t in range(RECORDS)]
    ms = [eng.time_loop_cloud(det, np.arange(RECORDS), reps=REPS, velocities=vel) for _ in range(RUNS)]
    assert len(det) == 0
    return dict(workload=workload, library=_ffi.LIB_PATH, records=RECORDS, reps=REPS, rows_kernel_ms=[m[0] for m in ms],
                gather_kernel_ms=[m[1] for m in ms], gather_us_per_record=1e3 * min(m[1] for m in ms) / RECORDS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("plain", "motion", "mixed"))
    ap.add_argument("--plain-only", action="store_true")
    args = ap.parse_args()
    if args.workload:
        print(json.dumps(run(args.workload)))
        return 0
    for w in ("plain",) if args.plain_only else ("plain", "motion", "mixed", "plain", "motion"):      # a fresh process each
        r = subprocess.run(["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--workload", w])
        if r.returncode != 0:
            print(json.dumps(dict(workload=w, failed=r.returncode)))
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
