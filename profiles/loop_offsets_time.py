"""Times of the origin-shifted scan contexts (csrc/loop_offset.hip and the variant pass of csrc/loop_query.hip) on the GPU, beside the
plain kernels at the same shapes in the same process.  Each workload runs in a process of its own under its own `timeout`; the first
that fails ends the run.  HIP events around repeated launches on the context's stream, two warm launches first
(roam_engine_time_loop_offsets, roam_engine_time_loop_describe, roam_time_loop_db_query_offsets, roam_time_loop_db_query):

  describe  the 24 variants of offsetGrid(5.0, 2.5) of 1 and of 8 resident Oxford records (400 x 2025 u8 bins each, 60 x 20, floor 0) -
            the clear of the sums, the binning kernel and the finishing kernel as one launch - and the plain describing kernel on
            the same records
  query     one entry with its 25 variants against 1 000 entries, k = 8: the plain distance kernel, the variants' distance kernel with
            the fold, the selection kernel; and the plain query (distance, selection) of the same entry

There is no earlier version to compare with and no bar: the figures are records (docs/MEASUREMENT.md), from

    python profiles/loop_offsets_time.py
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"describe": 180, "query": 120}         # seconds per workload
S, R, K, ENTRIES = 60, 20, 8, 1000


def run_describe():
    from radarslampy_amd import _ffi, synth
    from radarslampy_amd.engine import Engine
    from radarslampy_amd.LoopClosure import offsetGrid
    n = 8
    ctx = _ffi.Context(0)
    eng = Engine(1, n, ctx=ctx, retrack_on_device=False)
    w = synth.StreamWorld(5, per_tile=40)
    for t in range(n):
        eng.upload_scan(t, synth.render_stream_record(w, (3.0 * t, 0.0, 0.01 * t), t_index=t))
    eng.synchronize()
    db = _ffi.LoopDb(ctx, n, S, R)
    grid = offsetGrid(5.0, 2.5)
    db.keep_offsets(grid)
    out = dict(workload="describe", sectors=S, rings=R, offsets=len(grid), samples_per_record=synth.ROWS * synth.CLIP)
    ms = C.c_float(0)
    for m in (1, n):
        idx = np.arange(m, dtype=np.int32)
        ctx.check(ctx.lib.roam_engine_time_loop_offsets(ctx.h, db.h, m, _ffi._ptr(idx), 0, 0, 50, C.byref(ms)))
        out[f"variants_ms_{m}_records"] = ms.value
        ctx.check(ctx.lib.roam_engine_time_loop_describe(ctx.h, db.h, m, _ffi._ptr(idx), 0, 0, 50, C.byref(ms)))
        out[f"plain_ms_{m}_records"] = ms.value
    out["variant_samples_per_s_8_records"] = n * len(grid) * synth.ROWS * synth.CLIP / (out[f"variants_ms_{n}_records"] * 1e-3)
    db.close()
    eng.close()
    ctx.close()
    return out


def run_query():
    from radarslampy_amd import _ffi
    from radarslampy_amd.LoopClosure import offsetGrid
    ctx = _ffi.Context(0)
    rng = np.random.default_rng(1)
    db = _ffi.LoopDb(ctx, ENTRIES, S, R)
    grid = offsetGrid(5.0, 2.5)
    db.keep_offsets(grid)
    db.add_desc(rng.random((ENTRIES, S, R), dtype=np.float32))
    q = np.array([ENTRIES - 1], np.int32)
    db.set_variants(int(q[0]), rng.random((len(grid), S, R), dtype=np.float32))
    plain_ms, variants_ms, select_ms = db.time_query_offsets(q, q, K, np.inf, reps=50)
    d_ms, s_ms = db.time_query(q, q, K, np.inf, reps=50)
    out = dict(workload="query", entries=ENTRIES, queries=1, variants=1 + len(grid), k=K, plain_distance_ms=plain_ms,
               variants_distance_and_fold_ms=variants_ms, select_ms=select_ms, query_offsets_ms=plain_ms + variants_ms + select_ms,
               plain_query_distance_ms=d_ms, plain_query_select_ms=s_ms, plain_query_ms=d_ms + s_ms)
    db.close()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(LIMITS))
    args = ap.parse_args()
    if args.workload:
        print(json.dumps({"describe": run_describe, "query": run_query}[args.workload]()))
        return 0
    for w in ("describe", "query"):                  # a fresh process each; the first one that fails ends the run
        r = subprocess.run(["timeout", "-k", "10", str(LIMITS[w]), sys.executable, os.path.abspath(__file__), "--workload", w])
        if r.returncode != 0:
            print(json.dumps(dict(workload=w, failed=r.returncode)))
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
