#!/usr/bin/env python3
"""cost of find_peaks' distance / prominence conditions (peaks_cond.hip) next to the plain detection (peaks.hip) on the two real
scans of tests/golden/peaks.npz, through the stage API (upload + kernels + download per call).  Under `rocprofv3 --kernel-trace
--stats` the kernel table gives the device times: peaks_rows_u8_wave_kernel / peaks_rows_kernel<false> (plain), peaks_cond_rows_kernel
<true> / <false> (conditioned), peaks_gather_kernel (both).
usage: python profiles/time_peaks_cond.py [reps]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from radarslampy_amd import _ffi
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
g = np.load(os.path.join(ROOT, "tests", "golden", "peaks.npz"))
scans = [g["real0_u8"], g["real1_u8"]]
ctx = _ffi.Context(0)
configs = [("plain", None, None), ("distance 5", 5, None), ("prominence 0.03", None, 0.03), ("distance 10.5 + prominence (0.02, 0.2)", 10.5, (0.02, 0.2)),
           ("distance 1.7 + prominence 0 (no-op)", 1.7, 0)]
for src in ("u8", "f32"):
    for name, d, p in configs:
        imgs = scans if src == "u8" else [s.astype(np.float32) / 255. for s in scans]
        call = (lambda im: ctx.peaks_record_u8(im, payload_off=0, clip=im.shape[1], distance=d, prominence=p)) if src == "u8" else \
               (lambda im: ctx.peaks_polar_f32(im, distance=d, prominence=p))
        n = [len(call(im)) for im in imgs]
        t0 = time.perf_counter()
        for _ in range(reps):
            for im in imgs:
                call(im)
        dt = (time.perf_counter() - t0) / (reps * len(imgs))
        print(f"{src:3s} {name:42s} {dt * 1e6:8.1f} us per scan call (host wall)   peaks {n}")
ctx.close()
