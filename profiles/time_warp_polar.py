#!/usr/bin/env python3
"""cost of roam_warp_polar_f32 (warppolar.hip) in all four modes on the real scans of tests/golden/tiny_track.npz (400 x 2025):
convertPolarImageToCartesian at downsampleFactor 1 / 3 / 20, linear and semilog, and convertCartesianImageToPolar of the 2024 x 2024
live Cartesian image with OpenCV's default size and with shapeHW = (400, 1012), linear and semilog.  Prints the host wall time of
one call (pageable upload, kernel, pageable download).  Under `rocprofv3 --kernel-trace --stats --output-format csv` the kernel table
gives the device times: warp_polar_inverse_kernel<false / true>, warp_polar_forward_kernel.
usage: python profiles/time_warp_polar.py [reps]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from radarslampy_amd import _ffi, parseData
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
scans = np.load(os.path.join(ROOT, "tests", "golden", "tiny_track.npz"))["payload"].astype(np.float32) / np.float32(255.)
ctx = _ffi.default_context()
cart = ctx.polar_to_cart_f32(scans[0])[0]


def timed(label, fn, out_bytes):
    fn()
    t0 = time.perf_counter()
    for i in range(reps):
        fn()
    dt = (time.perf_counter() - t0) / reps
    print(f"{label:52s} {dt * 1e3:8.2f} ms per call (host wall)   output {out_bytes / 1e6:7.1f} MB")


for df in (1, 3, 20):
    R = 2025 // df if df > 1 else 2025
    for log in (False, True):
        timed(f"polar -> Cartesian df={df:2d} {'semilog' if log else 'linear '} ({2 * R} x {2 * R})",
              lambda: parseData.convertPolarImageToCartesian(scans[1], logPolarMode=log, downsampleFactor=df), 4 * (2 * R) ** 2)
for shapeHW in (None, (400, 1012)):
    ds = parseData.warpPolarDsize(1012.0, None if shapeHW is None else (shapeHW[1], shapeHW[0]))
    for log in (False, True):
        timed(f"Cartesian 2024 -> polar {'semilog' if log else 'linear '} ({ds[1]} x {ds[0]})",
              lambda: parseData.convertCartesianImageToPolar(cart, logPolarMode=log, shapeHW=shapeHW), 4 * ds[0] * ds[1])
timed("convertPolarImgToLogPolar (400 x 101)", lambda: parseData.convertPolarImgToLogPolar(scans[2][:, :101]), 0)
