"""Times of the loop-closure candidates (csrc/loop_describe.hip, csrc/loop_query.hip) on the GPU, each workload in a process of its own under its own
`timeout`; the first that fails ends the run.  HIP events around repeated launches on the context's stream, two warm launches first
(roam_engine_time_loop_describe, roam_time_loop_db_query):

  describe  the descriptor kernel on 1 024 resident Oxford records (400 x 2025 u8 bins each, 60 x 20, floor 0) of an engine's pool
            - with the bytes it must read (the clipped payload) as a share of the 6 300 GB/s a streaming kernel reaches on this part
  query1    one query against 8 866 entries (the length of full_seq_1), k = 8, min_gap 50: distance and selection kernels
  all       all 8 866 against all, k = 8, min_gap 50 (entry i asks for the entries below i - 49)
  numpy     as context only: tests/scan_context_model.py, one query against 8 866 on the host

There is no earlier version to compare with and no bar: the figures are records (docs/MEASUREMENT.md), from

    python profiles/loop_closure_time.py
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
LIMITS = {"describe": 240, "query1": 120, "all": 240, "numpy": 120}      # seconds per workload
ENTRIES, S, R, K, MIN_GAP = 8866, 60, 20, 8, 50
HBM_ACHIEVABLE_GBS = 6300.0


def database(ctx):
    from radarslampy_amd import _ffi
    db = _ffi.LoopDb(ctx, ENTRIES, S, R)
    db.add_desc(np.random.default_rng(1).random((ENTRIES, S, R), dtype=np.float32))
    return db


def run_describe():
    import ctypes as C
    from radarslampy_amd import _ffi, synth
    from radarslampy_amd.engine import Engine
    n, distinct = 1024, 8
    ctx = _ffi.Context(0)
    eng = Engine(1, n, ctx=ctx, retrack_on_device=False)
    w = synth.StreamWorld(5, per_tile=40)
    for t in range(distinct):
        eng.upload_scan(t, synth.render_stream_record(w, (3.0 * t, 0.0, 0.01 * t), t_index=t))
    for t in range(distinct, n):
        eng.copy_scan(t, t % distinct)
    eng.synchronize()
    db = _ffi.LoopDb(ctx, n, S, R)
    idx = np.arange(n, dtype=np.int32)
    ms = C.c_float(0)
    ctx.check(ctx.lib.roam_engine_time_loop_describe(ctx.h, db.h, n, _ffi._ptr(idx), 0, 0, 20, C.byref(ms)))
    read = n * synth.ROWS * synth.CLIP
    gbs = read / (ms.value * 1e-3) / 1e9
    out = dict(workload="describe", records=n, sectors=S, rings=R, ms=ms.value, bytes_read=read, gb_per_s=gbs,
               share_of_hbm_roofline=gbs / HBM_ACHIEVABLE_GBS, us_per_record=1e3 * ms.value / n)
    db.close()
    eng.close()
    ctx.close()
    return out


def run_query(all_queries):
    from radarslampy_amd import _ffi
    ctx = _ffi.Context(0)
    db = database(ctx)
    q = np.arange(ENTRIES, dtype=np.int32) if all_queries else np.array([ENTRIES - 1], np.int32)
    max_index = q - MIN_GAP + 1
    d_ms, s_ms = db.time_query(q, max_index, K, 0.2, reps=3 if all_queries else 50)
    pairs = int(np.clip(max_index, 0, ENTRIES).sum())
    macs = pairs * S * S * R
    out = dict(workload="all" if all_queries else "query1", entries=ENTRIES, queries=len(q), k=K, min_gap=MIN_GAP, pairs=pairs,
               distance_ms=d_ms, select_ms=s_ms, multiply_adds=macs, multiply_adds_per_s=macs / (d_ms * 1e-3),
               pairs_per_s=pairs / (d_ms * 1e-3))
    db.close()
    ctx.close()
    return out


def run_numpy():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import scan_context_model as model
    D = np.random.default_rng(1).random((ENTRIES, S, R), dtype=np.float32)
    t0 = time.perf_counter()
    d = model.shift_distances(D[-1], D[:ENTRIES - MIN_GAP])
    best = d.min(axis=1)
    order = np.argsort(best, kind="stable")[:K]
    return dict(workload="numpy", context_only=True, entries=ENTRIES, queries=1, seconds=time.perf_counter() - t0, nearest=int(order[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(LIMITS))
    args = ap.parse_args()
    if args.workload:
        run = {"describe": run_describe, "query1": lambda: run_query(False), "all": lambda: run_query(True), "numpy": run_numpy}
        print(json.dumps(run[args.workload]()))
        return 0
    for w in ("describe", "query1", "all", "numpy"):      # a fresh process each; the first one that fails ends the run
        r = subprocess.run(["timeout", "-k", "10", str(LIMITS[w]), sys.executable, os.path.abspath(__file__), "--workload", w])
        if r.returncode != 0:
            print(json.dumps(dict(workload=w, failed=r.returncode)))
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
