#!/usr/bin/env python3
"""cost of getBlobsFromCart(method="log") (log.hip + the host bookkeeping) on the two real scans of tests/golden/peaks.npz, Cartesian
images from the oracle's warp.  Per parameter set: the stage call (upload + layers + maxima + download, Context.log_maxima) and the
whole getBlobsFromCart (adds the response sort and the host prune).  Under `rocprofv3 --kernel-trace --stats` the kernel table gives
the device times: log_cols_kernel<float> (column pass), log_rows_kernel (row pass), log_maxima_kernel<false> / <true>,
log_row_scan_kernel.
usage: python profiles/time_log_blobs.py [reps]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import oracle
from radarslampy_amd import _ffi
from radarslampy_amd import getFeatures as gf
from radarslampy_amd.gaussian import blob_log_sigmas
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
g = np.load(os.path.join(ROOT, "tests", "golden", "peaks.npz"))
carts = [oracle.convertPolarImageToCartesian(g[f"real{i}_u8"].astype(np.float32) / 255.) for i in (0, 1)]
ctx = _ffi.default_context()
for mn, mx, num, thr in [(0.01, 10, 3, 5e-4), (1, 10, 3, 0.01), (1, 30, 10, 0.01)]:
    sig = blob_log_sigmas(mn, mx, num)
    n = [len(ctx.log_maxima(c, sig, thr)[0]) for c in carts]
    t0 = time.perf_counter()
    for _ in range(reps):
        for c in carts:
            ctx.log_maxima(c, sig, thr)
    stage = (time.perf_counter() - t0) / (reps * len(carts))
    params = dict(min_sigma=mn, max_sigma=mx, num_sigma=num, threshold=thr, method="log")
    nb = [len(gf.getBlobsFromCart(c, **params)) for c in carts]
    t0 = time.perf_counter()
    for _ in range(max(1, reps // 2)):
        for c in carts:
            gf.getBlobsFromCart(c, **params)
    whole = (time.perf_counter() - t0) / (max(1, reps // 2) * len(carts))
    print(f"({mn}, {mx}, {num}, {thr}): stage call {stage * 1e3:8.2f} ms  getBlobsFromCart {whole * 1e3:8.2f} ms per scan (host wall)"
          f"   maxima {n}  blobs {nb}")
