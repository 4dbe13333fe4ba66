"""NumPy model of the motion compensation of the loop database's peak clouds (csrc/cloud_motion.h, cloud_gather_motion_kernel in
csrc/loop_cloud.hip, include/roam_abi.h): how a kept peak of a scan with a velocity becomes metres.  PARITY UNPINNED as the clouds
themselves (tests/loop_cloud_model.py); this is the reference's MotionDistortionSolver.undistort(v, cloud, period) with the time of
a point taken from its azimuth row instead of atan2 of its coordinates.

A scan sweeps its `rows` azimuths over `period` seconds; v = (vx, vy, vtheta) in m/s, m/s, rad/s is its velocity in the sensor frame
of the stored points (Keyframe.velocity, the solver's v_j).  Every operation below is one float64 operation, rounded once.

Row time.  tau_t = period * ((2 t - rows) / (2 rows)): -period / 2 at row 0, 0 at mid-scan - compute_time_deltas for a point on row t.
Motion table, per row: a = vtheta * tau_t, C = cos a, S = sin a, DX = vx * tau_t, DY = vy * tau_t.  cos / sin are GIVEN functions, as the
tables of loop_cloud_model are given: a device comparison passes the host's libm, never np.cos.
Stored point.  (x0, y0) = loop_cloud_model.metres; x = ((C * x0) - (S * y0)) + DX, y = ((S * x0) + (C * y0)) + DY.
Selection.  Unchanged: loop_cloud_model.select.  A scan without a velocity (None) is loop_cloud_model.cloud, bit for bit - zeros are
not: a -0.0 coordinate becomes +0.0 under them."""
import numpy as np

import loop_cloud_model as plain

PERIOD = 0.25


def row_times(rows, period=PERIOD):
    """-> (rows,) float64 tau_t"""
    t = np.arange(int(rows), dtype=np.int64)
    return np.float64(period) * ((2 * t - int(rows)).astype(np.float64) / np.float64(2 * int(rows)))


def table(rows, velocity, period=PERIOD, cos=np.cos, sin=np.sin):
    """-> (rows, 4) float64 rows C S DX DY; all NaN for velocity None.  cos, sin: functions of a float64 array"""
    if velocity is None:
        return np.full((int(rows), 4), np.nan)
    vx, vy, vth = (np.float64(c) for c in velocity)
    tau = row_times(rows, period)
    a = vth * tau
    return np.stack([np.asarray(cos(a), np.float64), np.asarray(sin(a), np.float64), vx * tau, vy * tau], axis=1)


def apply(xy0, theta, tab):
    """plain points (K, 2) on the azimuth rows theta (K,) and a scan's table -> the compensated points (K, 2)"""
    xy0 = np.asarray(xy0, np.float64).reshape(-1, 2)
    T = np.asarray(tab, np.float64)[np.asarray(theta, np.int64)]
    C, S, DX, DY = T[:, 0], T[:, 1], T[:, 2], T[:, 3]
    x0, y0 = xy0[:, 0], xy0[:, 1]
    return np.stack([((C * x0) - (S * y0)) + DX, ((S * x0) + (C * y0)) + DY], axis=1)


def metres(peaks, cos_t, sin_t, res, tab):
    """(K, 2) integer rows [theta, r] -> (K, 2) float64 metres, compensated with the scan's table (None: plain)"""
    p = np.asarray(peaks).reshape(-1, 2)
    xy0 = plain.metres(p, cos_t, sin_t, res)
    return xy0 if tab is None else apply(xy0, p[:, 0], tab)


def cloud(peaks, cos_t, sin_t, res, max_points, point_stride, tab=None):
    """a scan's peak list and its motion table (None: no velocity) -> (the stored cloud (n, 2) float64, the full peak count)"""
    p = np.asarray(peaks).reshape(-1, 2)
    return metres(p[plain.select(len(p), max_points, point_stride)], cos_t, sin_t, res, tab), len(p)
