"""Polar peak extraction (reference getPointCloud.py:11-54) on the MI355X (peaks.hip; with find_peaks' distance / prominence
conditions: peaks_cond.hip)."""
import numpy as np

from . import _ffi


def getPointCloudPolarInd(polarImage: np.ndarray, peakDistance: float = None, peakProminence: float = None) -> np.ndarray:
    """-> (K, 2) int64 rows [thetaInd, rInd], azimuth-major, range ascending.  peakDistance / peakProminence: find_peaks' distance /
    prominence (ValueError for a distance below 1; NotImplementedError for per-sample prominence bounds)."""
    if peakDistance is None and peakProminence is None:
        return _ffi.default_context().peaks_polar_f32(polarImage).astype(np.int64)
    _ffi.peak_conditions(peakDistance, peakProminence)          # argument errors before any device call
    return _ffi.default_context().peaks_polar_f32(polarImage, distance=peakDistance, prominence=peakProminence).astype(np.int64)


def getPointCloudFromRecord(record_u8: np.ndarray, payload_off: int = 11, clip: int = 2025, peakDistance: float = None,
                            peakProminence: float = None) -> np.ndarray:
    """Fused decode + peaks straight from the raw u8 record (no f32 polar image)."""
    if peakDistance is None and peakProminence is None:
        return _ffi.default_context().peaks_record_u8(record_u8, payload_off, clip).astype(np.int64)
    _ffi.peak_conditions(peakDistance, peakProminence)
    return _ffi.default_context().peaks_record_u8(record_u8, payload_off, clip, distance=peakDistance,
                                                  prominence=peakProminence).astype(np.int64)
