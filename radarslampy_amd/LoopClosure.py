"""Loop-closure candidates on the device: the radar scan context of Kim et al. (the MulRan data set).

The reference stops at a commented-out "import m2dp" (Mapping.py:7) and a Keyframe.pointCloud marked "not sure if needed"
(Mapping.py:61-62); it has no place recognition, so this module has nothing to be pinned against - its contract is
tests/scan_context_model.py.  The polar scan is area-averaged to sectors x rings; two places are compared by the mean cosine distance
of their sector columns, minimised over all circular sector shifts; the best shift is a yaw estimate (yaw of the query minus yaw of
the candidate ~ 2 pi shift / sectors).  The device compares a query with every stored keyframe at every shift exactly: no ring-key
tree, no coarse sector-key alignment.

What comes out are CANDIDATES and a yaw.  The method's reach is short: on the synthetic worlds a revisit 2.5 m off the stored place
still ranks first but at 0.79 of the next place's distance, and at 5 m it is not recognised (the point reflectors move to other
rings).  Verifying a candidate metrically and measuring its edge (FMT.getTransformUsingFMT after a pre-rotation by the yaw is the
obvious route), and feeding edges to PoseGraphLib.PoseGraphOptimization, are not done here."""
import numbers

import numpy as np

from . import _ffi


def _yaw(shift, sectors):
    a = 2.0 * np.pi * np.asarray(shift, np.float64) / sectors
    return np.where(a > np.pi, a - 2.0 * np.pi, a)


def scanContext(polarImg, sectors=60, rings=20, clip_px=None, floor=0.0):
    """The scan-context descriptor of a float32 polar image (azimuth rows x range columns) -> (sectors, rings) float32, or of a 3-D
    batch -> (n, sectors, rings): the mean of max(value - floor, 0) over each bin, sector s = the rows [floor(s rows / sectors),
    floor((s + 1) rows / sectors)), ring r = the columns [floor(r clip / rings), floor((r + 1) clip / rings)), clip = clip_px if
    0 < clip_px < cols else cols.  floor = 0 is the plain area mean.  ValueError before the device is touched for a bad argument."""
    a = np.asarray(polarImg)
    _ffi.scan_context_images(a, clip_px, sectors, rings)          # the argument checks come before a device is asked for
    _ffi.scan_context_floor(floor)
    out = _ffi.default_context().scan_context(a, sectors, rings, clip_px, floor)
    return out[0] if a.ndim == 2 else out


def scanContextDistance(a, b):
    """Two descriptors of one shape -> (distance, shift, yaw): the mean cosine distance of the sector columns of a against those of b
    shifted by `shift` sectors, minimised over the shifts (the lowest shift of the minimum); yaw = 2 pi shift / sectors in (-pi, pi],
    the yaw of a's scan minus the yaw of b's.  Runs on the device through a two-entry database."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.ndim != 2 or a.shape != b.shape:
        raise ValueError(f"scanContextDistance: two descriptors of one (sectors, rings) shape, not {a.shape} and {b.shape}")
    db = _ffi.LoopDb(None, 2, a.shape[0], a.shape[1])
    try:
        db.add_desc(np.stack([b, a]))
        _, cd, cs = db.query([1], [1], k=1)
    finally:
        db.close()
    return float(cd[0, 0]), int(cs[0, 0]), float(_yaw(cs[0, 0], a.shape[0]))


class LoopDetector:
    """Keyframe scans in, loop-closure candidates out.  Every added scan becomes one entry (its index is its order of arrival);
    query(i) returns the k stored entries most like entry i among those at least min_gap entries older, with their distances and
    yaw differences."""

    def __init__(self, capacity, sectors=60, rings=20, clip_px=None, floor=0.0, min_gap=50, max_distance=0.2, k=8, ctx=None):
        if not isinstance(min_gap, numbers.Integral) or isinstance(min_gap, bool) or min_gap < 1:
            raise ValueError(f"LoopDetector: min_gap an integer >= 1, not {min_gap!r}")
        if clip_px is not None and (not isinstance(clip_px, numbers.Integral) or isinstance(clip_px, bool) or clip_px < 0):
            raise ValueError(f"LoopDetector: clip_px a non-negative integer or None, not {clip_px!r}")
        self.floor = _ffi.scan_context_floor(floor)
        _ffi.loop_query_args(1, [0], [0], k, max_distance)
        self.clip_px, self.min_gap, self.max_distance, self.k = clip_px, int(min_gap), float(max_distance), int(k)
        self.db = _ffi.LoopDb(ctx, capacity, sectors, rings)
        self.sectors, self.rings = self.db.sectors, self.db.rings

    def close(self):
        self.db.close()

    def __len__(self):
        return len(self.db)

    def add(self, polarImg):
        """describe a float32 polar image (or a 3-D batch) on the device and store it -> the index of the (first) new entry"""
        return self.db.add_f32(polarImg, self.clip_px, self.floor)

    def addDescriptors(self, desc):
        """store ready-made descriptors, (sectors, rings) or (n, sectors, rings) -> the index of the first new entry"""
        return self.db.add_desc(desc)

    def floorCode(self):
        """the integer floor of the u8 record form that equals this detector's floor (Engine.loop_db_add): floor * 255, which must be
        an integer in [0, 254]"""
        code = int(round(self.floor * 255.0))
        if code > 254 or abs(self.floor * 255.0 - code) > 1e-9:
            raise ValueError(f"LoopDetector: floor {self.floor} is no u8 code / 255 in [0, 254 / 255]")
        return code

    def query(self, indices=None):
        """candidates of the entries `indices` (None: the newest) among the entries j <= i - min_gap -> (index (m, k) int32, distance
        (m, k) float64, yaw (m, k) float64); unused slots hold -1, +inf, 0"""
        idx = np.array([len(self.db) - 1], np.int32) if indices is None else np.ascontiguousarray(indices, np.int32).ravel()
        ci, cd, cs = self.db.query(idx, idx - self.min_gap + 1, self.k, self.max_distance)
        return ci, cd, _yaw(cs, self.sectors)

    def addAndQuery(self, polarImg):
        """add one image and query it -> (index, candidate indices (k,), distances (k,), yaws (k,))"""
        a = np.asarray(polarImg)
        if a.ndim != 2:
            raise ValueError(f"LoopDetector.addAndQuery: one 2-D image, not shape {a.shape}")
        i = self.add(a)
        ci, cd, yaw = self.query([i])
        return i, ci[0], cd[0], yaw[0]

    def descriptors(self):
        """the stored descriptors (n, sectors, rings) float32"""
        return self.db.get() if len(self.db) else np.empty((0, self.sectors, self.rings), np.float32)
