"""Drop-in for the reference's Tracker (reference Tracker.py:16-127): same constructor, same
track()/getTransform() signatures, return orders and dtypes; the arithmetic runs on the MI355X.

The Fourier-Mellin rotation estimate that track() computes first and returns in slot 3 (Tracker.py:62-63; the reference
only prints it, RawROAMSystem.py:187-188) runs on the GPU as well (FMT.getRotationUsingFMT: csrc/fmt_batch.hip and the
correlation of csrc/phasecorr.hip, driven by csrc/fmt.hip).
One documented difference: paramFlags["rejectOutliers"]=False returns an all-ones pruning mask where the reference raises
NameError (Tracker.py:93-104).
One addition: paramFlags["fmtPrior"] (default False) makes track() run the whole registration (FMT.getTransformUsingFMT) and start
the tracker's search at the position it predicts for each feature; useFMT stays the no-op it is in the reference."""
import time

import numpy as np

from . import FMT as _fmt
from . import getTransformKLT as _klt
from . import outlierRejection as _orj
from .parseData import RANGE_RESOLUTION_CART_M


def getTrackedPointsKLT(srcImg, targetImg, blobCoordSrc, initialFlow=None):      # module-level hook (tests patch it, like the reference's import)
    if initialFlow is None:
        return _klt.getTrackedPointsKLT(srcImg, targetImg, blobCoordSrc)
    return _klt.getTrackedPointsKLT(srcImg, targetImg, blobCoordSrc, initialFlow=initialFlow)


def flowFromPrior(prior, featureCoord):
    """the (2, 3) float32 prior applied to (K, >= 2) feature positions in the float32 order of the device (roam_engine_set_motion_prior)"""
    p = np.ascontiguousarray(np.asarray(featureCoord)[:, :2]).astype(np.float32)
    a = np.asarray(prior, np.float32).reshape(6)
    x, y = p[:, 0], p[:, 1]
    return np.stack([(a[0] * x + a[1] * y) + a[2], (a[3] * x + a[4] * y) + a[5]], axis=1).astype(np.float32)


class Tracker():
    def __init__(self, sequenceName, imgPathArr, filePaths, paramFlags) -> None:
        self.sequenceName, self.imgPathArr = sequenceName, imgPathArr
        self.sequenceSize = len(imgPathArr)
        self.filePaths, self.paramFlags = filePaths, paramFlags
        self.estTraj = self.gtTraj = None
        self.verbose = False

    def initTraj(self, estTraj, gtTraj=None):
        self.estTraj, self.gtTraj = estTraj, gtTraj

    def track(self, prevImgCart, currImgCart, prevImgPolar, currImgPolar, featureCoord, seqInd):
        """-> (good_old (K',2) f32, good_new (K',2) f32, angleRotRad, corrStatus (K,1) u8)"""
        t0 = time.time()
        angleRotRad = 0.0
        flow = None
        if prevImgPolar is not None and currImgPolar is not None:
            if self.paramFlags.get("fmtPrior", False):
                # the registration as the tracker's motion prior (cv2's OPTFLOW_USE_INITIAL_FLOW): what the reference computes the
                # angle for and never gets to (Tracker.py:66-72).  The Cartesian images are the polar ones at downsample factor
                # 2 R / W of their own width W
                angleRotRad, dxdy, _, _, _ = _fmt.getTransformUsingFMT(prevImgPolar, currImgPolar)
                cols = prevImgPolar.shape[1]
                prior = _fmt.flowPriorFromFMT(angleRotRad, dxdy, _fmt.FMT_CART_DOWNSAMPLE_FACTOR, max(1, round(2 * cols / prevImgCart.shape[1])), cols)
                flow = flowFromPrior(prior, featureCoord)
            else:
                angleRotRad, _, _ = _fmt.getRotationUsingFMT(prevImgPolar, currImgPolar)
        if flow is None:
            new_ok, old_ok, new_bad, _, status = getTrackedPointsKLT(prevImgCart, currImgCart, featureCoord)
        else:
            new_ok, old_ok, new_bad, _, status = getTrackedPointsKLT(prevImgCart, currImgCart, featureCoord, initialFlow=flow)
        n_all = new_ok.shape[0] + new_bad.shape[0]
        if self.verbose:
            print(f"{seqInd} | Num good features: {new_ok.shape[0]} of {n_all} | Time: {time.time() - t0:.2f}s")
        if self.paramFlags.get("rejectOutliers", True):
            old_ok, new_ok, keep = _orj.rejectOutliers(old_ok, new_ok)
        else:
            keep = np.ones(old_ok.shape[0], dtype=bool)
        alive = np.flatnonzero(status.reshape(-1) != 0)            # rows of corrStatus that KLT kept
        status[alive] &= keep.astype(status.dtype)[:, None]
        return old_ok, new_ok, angleRotRad, status

    def getTransform(self, srcCoord, targetCoord, pixel: bool):
        """-> (R (2,2), h (2,1)); h in metres when pixel=False (Tracker.py:108-127)."""
        R, h = _klt.calculateTransformSVD(srcCoord, targetCoord)
        return (R, h) if pixel else (R, h * RANGE_RESOLUTION_CART_M)
