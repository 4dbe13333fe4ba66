"""Keyframe / Map containers (reference Mapping.py:13-174): host-side bookkeeping around the
device stages (polar peaks on every updateInfo, undistortion of the keyframe features)."""
import numpy as np

from .getPointCloud import getPointCloudPolarInd
from .motionDistortion import MotionDistortionSolver

ROT_THRESHOLD = 0.2
TRANS_THRESHOLD = 2.0
TRANS_THRESHOLD_SQ = TRANS_THRESHOLD ** 2
RADAR_CART_CENTER = np.array([1012., 1012.])


def _se2_apply(pose, pts):
    x, y, th = pose
    c, s = np.cos(th), np.sin(th)
    return pts @ np.array([[c, s], [-s, c]]) + np.array([x, y])


class Keyframe():
    """pose [x,y,th] (m, m, rad), features in sensor-centred metres, the scan's polar peaks, velocity."""

    def __init__(self, globalPose, featurePointsLocal, radarPolarImg, velocity) -> None:
        self.updateInfo(globalPose, featurePointsLocal, radarPolarImg, velocity)

    def updateInfo(self, globalPose, featurePointsLocal, radarPolarImg, velocity) -> None:
        self.pose, self.velocity = globalPose, velocity
        self.radarPolarImg = radarPolarImg
        self.featurePointsLocal = self.prunedFeaturePoints = featurePointsLocal
        self.pointCloud = getPointCloudPolarInd(radarPolarImg)                                   # Mapping.py:62
        und = MotionDistortionSolver.undistort(velocity, featurePointsLocal)[:, :2]               # Mapping.py:65
        self.featurePointsLocalUndistorted = self.prunedUndistortedLocals = und

    def getPrunedFeaturesGlobalPosition(self) -> np.ndarray:
        return _se2_apply(self.pose, self.prunedUndistortedLocals)

    def pruneFeaturePoints(self, corrStatus: np.ndarray) -> None:
        keep = np.asarray(corrStatus).reshape(-1) != 0
        self.prunedFeaturePoints = self.prunedFeaturePoints[keep]
        self.prunedUndistortedLocals = self.prunedUndistortedLocals[keep]


class Map():
    def __init__(self, sequenceName=None, estTraj=None, imgPathArr=(), filePaths=None) -> None:
        self.sequenceName, self.estTraj = sequenceName, estTraj
        self.imgPathArr, self.filePaths = imgPathArr, filePaths
        self.mapPoints, self.keyframes = [], []

    def isGoodKeyframe(self, keyframe: Keyframe) -> bool:
        """rotation >= 0.2 rad or squared translation >= 4 m^2 w.r.t. the last keyframe (Mapping.py:149-174)"""
        last, cand = np.asarray(self.keyframes[-1].pose), np.asarray(keyframe.pose)
        if abs(last[2] - cand[2]) >= ROT_THRESHOLD:
            return True
        return bool(np.sum((last[:2] - cand[:2]) ** 2) >= TRANS_THRESHOLD_SQ)

    def addKeyframe(self, keyframe: Keyframe) -> None:
        self.keyframes.append(keyframe)


class GlobalMap():
    """What the reference's Map.mapPoints was meant to become ("a big array of map points in global coordinates", an empty list there):
    the keyframes' polar peaks in one world frame, binned on a grid.  A plain result object, made by LoopDetector.renderMap /
    LoopClosure.mapFromGraph (csrc/loop_map.hip; the definition is include/roam_abi.h's "global map" and tests/global_map_model.py).
    hits, views (H, W) uint32: the points in a cell and the distinct keyframes that put one there (None when rendered with
    grids=False); origin (ox, oy) metres: the corner of cell (0, 0); cellM: the cell size; shape = (H, W); points (M, 2) float64: the
    mean position of the points of every qualifying cell, row-major (v major), with pointHits, pointViews (M,) uint32; outside: the
    points that fell outside the extent."""

    def __init__(self, origin, cellM, shape, hits, views, points, pointHits, pointViews, outside) -> None:
        self.origin, self.cellM, self.shape = (float(origin[0]), float(origin[1])), float(cellM), (int(shape[0]), int(shape[1]))
        self.hits, self.views = hits, views
        self.points, self.pointHits, self.pointViews = points, pointHits, pointViews
        self.outside = int(outside)

    @property
    def nPoints(self) -> int:
        return len(self.points)

    def cellOf(self, xy) -> np.ndarray:
        """world points (n, 2) metres -> (n, 2) int64 rows (u, v) = floor((x - ox) / cellM), floor((y - oy) / cellM), each operation in
        float64: the column and the row of hits / views that a point lands in.  A point outside the extent gives a u outside [0, W) or
        a v outside [0, H) - floor, not truncation, so just below the origin is -1"""
        a = np.asarray(xy, np.float64).reshape(-1, 2)
        return np.floor((a - np.array(self.origin)) / self.cellM).astype(np.int64)

    def localizer(self, minHits=1, minViews=1, sigmaCells=1.0, radiusCells=2, ctx=None) -> "MapLocalizer":
        """The map as something a scan can be placed in -> MapLocalizer: the cells with at least minHits points from at least minViews
        keyframes, smeared over radiusCells cells with a Gaussian of sigmaCells (a maximum, one byte per cell), resident on the device.
        ValueError for a map rendered with grids=False, and before the device is touched for a bad argument"""
        if self.hits is None or self.views is None:
            raise ValueError("GlobalMap.localizer: the map was rendered with grids=False; it needs hits and views")
        return MapLocalizer(self, minHits, minViews, sigmaCells, radiusCells, ctx)


class MapLocalizer():
    """Correlative scan-to-map matching (Olson 2009) against a GlobalMap: an exhaustive search over a window of rotations and
    whole-cell translations around a prior pose, every candidate scored by the sum of the smeared occupancy under the scan's points
    (csrc/map_match.hip; the definition is include/roam_abi.h's "map matching" and tests/map_match_model.py).  The score is a sum of
    bytes, so the result is bit-reproducible.  Made by GlobalMap.localizer; origin, cellM and shape are the map's."""

    def __init__(self, globalMap, minHits=1, minViews=1, sigmaCells=1.0, radiusCells=2, ctx=None) -> None:
        from . import _ffi
        self.origin, self.cellM, self.shape = globalMap.origin, globalMap.cellM, globalMap.shape
        self._field = _ffi.MapField(ctx, globalMap.hits, globalMap.views, globalMap.origin, globalMap.cellM, minHits, minViews, sigmaCells, radiusCells)

    def close(self) -> None:
        self._field.close()

    def field(self) -> np.ndarray:
        """-> (H, W) uint8: 255 on an occupied cell, falling off to 0 beyond radiusCells"""
        return self._field.read()

    def window(self, reachM=3.0, reachRad=0.12, stepRad=0.01):
        """-> (n_theta, step_rad, kx, ky): the angles and the cells of shift to either side that match searches"""
        from . import _ffi
        return _ffi.map_match_window(self.cellM, reachM, reachRad, stepRad)

    def match(self, clouds, priors, reachM=3.0, reachRad=0.12, stepRad=0.01, volume=False):
        """clouds: one (n, 2) cloud or a list of them, metres in the sensor frame (LoopClosure.polarIndToLocalMetres), at most 8192
        points each; priors (3,) or (n, 3) rows x, y, theta in the map's frame.  Searched: the angles theta0 + j stepRad with
        |j| <= floor(reachRad / stepRad + 1e-9) and the shifts of whole cells within reachM (a scalar, or (x, y)) ->
        a structured array of _ffi.MATCH_TABLE rows: x, y, theta (the best candidate), score, fraction = score / (255 nPoints),
        nPoints, nInside (the points inside the grid at the best candidate), i, b, a (its indices in the window) and found
        (score > 0).  Among equal scores the lowest angle, then the lowest y, then the lowest x wins.  volume=True: also the list of
        the queries' score volumes, (n_theta, 2 ky + 1, 2 kx + 1) uint32 each"""
        from . import _ffi
        poses, info, scores = self._field.match_clouds(clouds, priors, self.window(reachM, reachRad, stepRad), volume)
        return (_ffi.match_table(poses, info), list(scores)) if volume else _ffi.match_table(poses, info)


class DeviceMap():
    """the keyframes of one engine lane, resident in HBM (roam_engine_map_*).  Read-only view with the
    reference's attribute names; `keyframes[-1]` is the live keyframe the tracker is pruning."""

    class _KF():
        def __init__(self, d):
            self.pose, self.velocity = d["pose"], d["velocity"]
            self.prunedUndistortedLocals = d["prunedUndistortedLocals"]
            self.scan = d["scan"]

        def getPrunedFeaturesGlobalPosition(self) -> np.ndarray:
            return _se2_apply(self.pose, self.prunedUndistortedLocals)

    def __init__(self, engine, lane: int) -> None:
        self.engine, self.lane = engine, int(lane)

    def __len__(self) -> int:
        return self.engine.map_count(self.lane)

    @property
    def keyframes(self):
        return [DeviceMap._KF(d) for d in self.engine.map_keyframes(self.lane)]

    def isGoodKeyframe(self, pose) -> bool:
        """rotation >= 0.2 rad or squared translation >= 4 m^2 w.r.t. the live keyframe (Mapping.py:149-174)"""
        last = self.engine.map_keyframe(self.lane, len(self) - 1)["pose"]
        pose = np.asarray(pose)
        return bool(abs(last[2] - pose[2]) >= ROT_THRESHOLD or np.sum((last[:2] - pose[:2]) ** 2) >= TRANS_THRESHOLD_SQ)
