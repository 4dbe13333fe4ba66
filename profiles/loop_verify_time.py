"""Times of the loop database's resident peak clouds and of the verification that runs from them (csrc/loop_cloud.hip, csrc/loop_verify.hip, csrc/icp.hip) on
the GPU, each workload in a process of its own under its own `timeout`; the first that fails ends the run.  The world is the eleven-scan
revisit world of tests/scan_context_cases.py (eight places, three revisits, Oxford records) in an engine's pool, described into a
LoopDetector(keepClouds=True) by Engine.loop_db_add; 60 x 20 descriptors, every peak kept (about 4 500 per scan), default ICP options.

  build    the cloud build of the eleven resident records into free entries, its two kernels apart (roam_engine_time_loop_cloud: HIP
           events, two warm launches first) - with the bytes the row kernel must read (the clipped payload) as a share of the
           6 300 GB/s a streaming kernel reaches on this part
  verify   the ICP launch on the nine stored pairs (the three revisits' k = 3 candidates; roam_time_loop_db_verify, events likewise)
  qv       the blocking call LoopDetector.queryAndVerify for the three revisits at k = 3: host wall clock, two warm calls first
  parent   the same three queries by the route there was before the store: LoopDetector.query, then verifyCandidates on host
           clouds, which uploads both clouds of every pair - host wall clock, two warm calls first; its table must equal qv's

Records, not bounds (docs/MEASUREMENT.md), from

    python profiles/loop_verify_time.py
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
LIMITS = {"build": 180, "verify": 180, "qv": 180, "parent": 180}      # seconds per workload
CALLS = 20
HBM_ACHIEVABLE_GBS = 6300.0


def world():
    """-> (ctx, engine, detector holding the eleven scans and their clouds, the three query indices)"""
    import scan_context_cases as sc
    from radarslampy_amd import _ffi
    from radarslampy_amd.engine import Engine
    from radarslampy_amd.LoopClosure import LoopDetector
    recs = sc.revisit_records()
    ctx = _ffi.Context(0)
    eng = Engine(1, len(recs), ctx=ctx, retrack_on_device=False)
    for t, r in enumerate(recs):
        eng.upload_scan(t, r)
    det = LoopDetector(32, sc.REVISIT_S, sc.REVISIT_R, clip_px=sc.REVISIT_CLIP, min_gap=1, max_distance=np.inf, k=3, ctx=ctx, keepClouds=True,
                       rows=recs[0].shape[0])
    assert eng.loop_db_add(det, np.arange(len(recs))) == 0
    return ctx, eng, det, np.arange(len(sc.PLACES), len(recs), dtype=np.int32)


def wall(call):
    for _ in range(2):
        call()
    t = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        call()                                      # blocking: ends in a stream synchronise and a read-back
        t.append(1e3 * (time.perf_counter() - t0))
    return dict(calls=CALLS, ms_mean=float(np.mean(t)), ms_median=float(np.median(t)), ms_min=float(np.min(t)), ms_max=float(np.max(t)))


def run_build():
    from radarslampy_amd import synth
    ctx, eng, det, _ = world()
    n = len(det)
    rows_ms, gather_ms = eng.time_loop_cloud(det, np.arange(n), reps=50)
    read = n * synth.ROWS * synth.CLIP
    gbs = read / ((rows_ms + gather_ms) * 1e-3) / 1e9
    peaks = det.db.cloud_counts()[1]
    return dict(workload="build", records=n, peaks_per_record=[int(p) for p in peaks], rows_kernel_ms=rows_ms, gather_kernel_ms=gather_ms,
                us_per_record=1e3 * (rows_ms + gather_ms) / n, bytes_read=read, gb_per_s=gbs, share_of_hbm_roofline=gbs / HBM_ACHIEVABLE_GBS)


def run_verify():
    from radarslampy_amd.LoopClosure import _yaw
    ctx, eng, det, q = world()
    ci, _, cs = det.db.query(q, q - det.min_gap + 1, det.k, det.max_distance)
    assert np.all(ci >= 0)
    src = np.repeat(q, det.k)
    seeds = np.stack([_yaw(cs, det.sectors).ravel(), np.zeros(ci.size), np.zeros(ci.size)], axis=1)
    ms = [det.db.time_verify(src, ci.ravel(), seeds, reps=10) for _ in range(3)]
    _, stats = det.db.verify(src, ci.ravel(), seeds)
    n = det.db.cloud_counts()[0]
    evals = int(sum((int(s["iterations"]) + 1) * int(n[a]) * int(n[b]) for s, a, b in zip(stats, src, ci.ravel())))
    return dict(workload="verify", pairs=int(ci.size), ms=ms, updates=[int(s["iterations"]) for s in stats], distance_evaluations=evals,
                evaluations_per_s=evals / (min(ms) * 1e-3))


def run_qv():
    ctx, eng, det, q = world()
    out = wall(lambda: det.queryAndVerify(q))
    edges, table = det.queryAndVerify(q)
    return dict(workload="qv", **out, rows=len(table), edges=[(e[0], e[1]) for e in edges], table_sha=hash_table(table))


def run_parent():
    from radarslampy_amd.LoopClosure import verifyCandidates
    ctx, eng, det, q = world()
    clouds = [det.cloud(i)[0] for i in range(len(det))]        # host clouds, the points the store holds

    def call():
        ci, _, yaw = det.query(q)
        return verifyCandidates(clouds, q, ci, yaw)
    out = wall(call)
    edges, table = call()
    return dict(workload="parent", **out, rows=len(table), edges=[(e[0], e[1]) for e in edges], table_sha=hash_table(table),
                upload_bytes_per_call=int(sum(16 * (len(clouds[r["query"]]) + len(clouds[r["candidate"]])) for r in table)))


def hash_table(table):
    import hashlib
    return hashlib.sha256(table.tobytes()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(LIMITS))
    args = ap.parse_args()
    if args.workload:
        run = {"build": run_build, "verify": run_verify, "qv": run_qv, "parent": run_parent}
        print(json.dumps(run[args.workload]()))
        return 0
    for w in ("build", "verify", "qv", "parent"):      # a fresh process each; the first one that fails ends the run
        r = subprocess.run(["timeout", "-k", "10", str(LIMITS[w]), sys.executable, os.path.abspath(__file__), "--workload", w])
        if r.returncode != 0:
            print(json.dumps(dict(workload=w, failed=r.returncode)))
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
