#!/usr/bin/env python3
"""The three pyramid levels alone (roam_engine_time_kernel("pyramid"): every launch that builds the pyramid of all lanes' next
scans, between one pair of events), at 4096 scans and at 64: ms per launch and TB/s on the algorithmic byte count.
usage: python profiles/time_pyramid.py [repeats [reps per repeat]]   (one line per repeat, then min / median / spread)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from radarslampy_amd import _ffi, synth
from radarslampy_amd.engine import Engine
repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
recs, poses, feat = synth.make_sequence(5, 2, n_movers=16, distortion=True)
ctx = _ffi.Context(0)
for B in (4096, 64):
    eng = Engine(B, 2 * B, ctx=ctx)
    for t in range(2):
        eng.upload_scan(t, recs[t])
    for b in range(1, B):
        for t in range(2):
            eng.copy_scan(b * 2 + t, t)
    eng.synchronize()
    for b in range(B):
        eng.init_lane(b, b * 2, feat, poses[0])
    eng.step(np.arange(B, dtype=np.int32) * 2 + 1)
    eng.synchronize()
    eng.time_kernel("pyramid", 5)                                  # warm-up
    ms = []
    for r in range(repeats):
        m, by = eng.time_kernel("pyramid", reps)
        ms.append(m)
        print(f"pyramid B={B} repeat {r}: {m:.4f} ms = {m * 1e3 / B:.3f} us per scan, {by / m / 1e9:.3f} TB/s algorithmic", flush=True)
    a = np.array(ms)
    print(f"pyramid B={B}: min {a.min():.4f} median {np.median(a):.4f} max {a.max():.4f} ms, spread (max - min) {a.max() - a.min():.4f} ms", flush=True)
    eng.close()
ctx.close()
