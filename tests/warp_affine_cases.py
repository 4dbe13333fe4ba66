"""Inputs shared by the warpAffine tests (CPU and GPU): the real scan, the reference's perfect-image chain (FMT.py:190-208) on the
project's NumPy models, and the matrices that are no rotation."""
import math
import os

import numpy as np

import warp_affine_model as A
import warp_polar_model as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CHAIN_DOWNSAMPLE = 20                   # FMT.py:191
LOG_POLAR_ROW_RAD = 2 * math.pi / 317   # one row of the estimator's log-polar image: its resolution
# measured on the CPU chain (test_warp_affine_cpu.test_perfect_image_chain prints them): recovered - applied, radians
CHAIN_MEASURED_ERR = {5: 2.750e-3, -5: 1.220e-3, 20: 2.041e-3, -20: -0.909e-3}
CHAIN_BOUND_RAD = max(abs(v) for v in CHAIN_MEASURED_ERR.values()) + LOG_POLAR_ROW_RAD

# shear + scale 0.7 + translation (source -> destination), and its use into a dsize different from the source
GENERAL_M = np.array([[0.7, 0.21, 13.25], [-0.12, 0.7 * 0.9, -4.5]], np.float64)
SINGULAR_M = np.array([[2.0, 4.0, 3.0], [1.0, 2.0, -7.0]], np.float64)


def real_scan0():
    """scan 0 of tests/golden/peaks.npz as extractDataFromRadarImage returns it: (400, 2025) float32"""
    return np.load(os.path.join(GOLDEN, "peaks.npz"))["real0_u8"].astype(np.float32) / np.float32(255.)


_chain = {}


def cpu_chain(deg):
    """-> (cart, rotated cart, polar of the rotated cart) of the perfect-image test for one angle, computed once"""
    if "cart" not in _chain:
        _chain["polar"] = real_scan0()
        _chain["cart"] = P.convertPolarImageToCartesian(_chain["polar"], downsampleFactor=CHAIN_DOWNSAMPLE)
    if deg not in _chain:
        rot = A.rotateImg(_chain["cart"], deg)
        _chain[deg] = (rot, P.convertCartesianImageToPolar(rot, shapeHW=_chain["polar"].shape))
    return (_chain["cart"],) + _chain[deg]


def known_answers(a):
    """rotateImg of a square image by 0, +90, -90 and 180 degrees -> {angle: expected}: with the centre at (n / 2, n / 2) the
    quarter turns land one pixel off the array's own rot90, and the row / column that falls outside reads the zero border"""
    up = np.zeros_like(a); up[1:] = np.rot90(a)[:-1]
    right = np.zeros_like(a); right[:, 1:] = np.rot90(a, -1)[:, :-1]
    both = np.zeros_like(a); both[1:, 1:] = a[::-1, ::-1][:-1, :-1]
    return {0: a, 90: up, -90: right, 180: both}
