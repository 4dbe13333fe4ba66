"""NumPy model of the loop database's peak-cloud store (csrc/loop_cloud.hip, include/roam_abi.h): which peaks of a scan an entry keeps,
and how a kept peak becomes metres.  PARITY UNPINNED - the reference stores Keyframe.pointCloud and never reads it.

Selection.  A scan has N peaks in azimuth-major order.  step = max(point_stride, ceil(N / max_points)); the entry keeps the peaks
0, step, 2 step, ...: ceil(N / step) of them, never more than max_points, and never only the first azimuths of a dense scan.

Metres.  A peak (theta, r) becomes x = fl64(fl64(r res) cos_t[theta]), y = fl64(fl64(r res) sin_t[theta]): two float64 multiplies each,
every one rounded once.  cos_t / sin_t are a GIVEN table, cos / sin of phi_t = (2 pi t) / rows by the host's libm
(roam_polar_cloud_table, _ffi.polar_cloud_table) - a device comparison uses that table, never np.cos, because NumPy may dispatch another
routine on another machine."""
import numpy as np


def step(n_peaks, max_points, point_stride):
    return max(int(point_stride), -(-int(n_peaks) // int(max_points)))


def select(n_peaks, max_points, point_stride):
    """-> the indices of the peaks an entry keeps"""
    return np.arange(0, int(n_peaks), step(n_peaks, max_points, point_stride))


def metres(peaks, cos_t, sin_t, res):
    """(K, 2) integer rows [theta, r] -> (K, 2) float64 metres from the table"""
    p = np.asarray(peaks).reshape(-1, 2)
    rho = p[:, 1].astype(np.float64) * np.float64(res)
    th = p[:, 0].astype(np.int64)
    return np.stack([rho * np.asarray(cos_t, np.float64)[th], rho * np.asarray(sin_t, np.float64)[th]], axis=1)


def cloud(peaks, cos_t, sin_t, res, max_points, point_stride):
    """a scan's peak list -> (the stored cloud (n, 2) float64, the full peak count)"""
    p = np.asarray(peaks).reshape(-1, 2)
    return metres(p[select(len(p), max_points, point_stride)], cos_t, sin_t, res), len(p)
