"""Fourier-Mellin registration with the reference's names (reference FMT.py:10-100): the rotation prior (csrc/fmt_batch.hip, one pair
or a batch of pairs in the same pass), the translation by phase correlation (csrc/phasecorr.hip), the rotation of an image (csrc/warpaffine.hip) and the chain of the three in one
device pass (getTransformUsingFMT, csrc/fmt_register.hip);
the computation runs on the MI355X.  SURVEY §8f-f4."""
import math

import numpy as np

from . import _ffi
from .parseData import RANGE_RESOLUTION_CART_M

FMT_DOWNSAMPLE_FACTOR = 10      # FMT.py:10
FMT_RANGE_CLIP_M = 87.5         # FMT.py:11
FMT_CART_DOWNSAMPLE_FACTOR = 20 # FMT.py:191, 213: the Cartesian images of the script


def getTranslationUsingPhaseCorrelation(srcImg, targetImg):
    """FMT.py:13-33 -> ((dx, dy), response): cv2.phaseCorrelate(srcImg, targetImg, Hanning window) on two images of one shape"""
    a, b = _ffi.phase_correlate_args(srcImg, targetImg)
    if a.ndim != 2:
        raise ValueError(f"getTranslationUsingPhaseCorrelation: 2-D images, not {a.ndim}-D")
    return _ffi.default_context().phase_correlate(a, b, hanning=True)


def getRotationUsingFMT(srcPolarImg, targetPolarImg, downsampleFactor: int = FMT_DOWNSAMPLE_FACTOR, maxRangeClipM=FMT_RANGE_CLIP_M):
    """-> (angleRad with R(angleRad) @ src = target, scaling factor, response); polar (not log-polar) float32 images.
    Two 3-D batches of polar images of one shape go through the batched device pass (roam_fmt_rotation_batch_f32) and give three
    arrays with one entry per pair; argument errors are then ValueError before any device call.  Two 2-D images go through
    roam_fmt_rotation, which is n = 1 of that pass and refuses what it refuses (RoamError)."""
    assert srcPolarImg.shape == targetPolarImg.shape, "Images need to have the same shape!"
    clip = int(maxRangeClipM / RANGE_RESOLUTION_CART_M) if maxRangeClipM > 0 else 0
    if np.ndim(srcPolarImg) == 3:
        _ffi.fmt_rotation_batch_args(srcPolarImg, targetPolarImg, clip, int(downsampleFactor))
        out = _ffi.default_context().fmt_rotation_batch(srcPolarImg, targetPolarImg, clip_px=clip, downsample=int(downsampleFactor))
        return out[:, 0].copy(), out[:, 1].copy(), out[:, 2].copy()
    return _ffi.default_context().fmt_rotation(srcPolarImg, targetPolarImg, clip_px=clip, downsample=int(downsampleFactor))


def getTransformUsingFMT(srcPolarImg, targetPolarImg, downsampleFactor: int = FMT_DOWNSAMPLE_FACTOR, maxRangeClipM=FMT_RANGE_CLIP_M,
                         cartDownsampleFactor: int = FMT_CART_DOWNSAMPLE_FACTOR):
    """The whole registration in one device pass (roam_fmt_register_batch_f32) -> (angleRad, (dx, dy), scale, rotResponse,
    transResponse): getRotationUsingFMT's estimate (FMT.py:211-250), then rotateImg(srcCart, degrees(angleRad)) on the Cartesian
    images at cartDownsampleFactor (FMT.py:134-168, 191) and getTranslationUsingPhaseCorrelation(srcRot, targetCart).  (dx, dy) are
    pixels of that Cartesian image (metres: px * RANGE_RESOLUTION_M * cartDownsampleFactor); they come out as minus the ego motion
    in the source frame.  2-D polar images give scalars, 3-D batches arrays with one entry per pair, (dx, dy) of shape (n, 2).
    Different shapes: AssertionError; other argument errors ValueError (TypeError for a cartDownsampleFactor that is no integer)
    before any device call."""
    assert np.shape(srcPolarImg) == np.shape(targetPolarImg), "Images need to have the same shape!"
    clip = int(maxRangeClipM / RANGE_RESOLUTION_CART_M) if maxRangeClipM > 0 else 0
    _ffi.fmt_register_batch_args(srcPolarImg, targetPolarImg, clip, int(downsampleFactor), cartDownsampleFactor)
    out = _ffi.default_context().fmt_register_batch(srcPolarImg, targetPolarImg, clip_px=clip, downsample=int(downsampleFactor),
                                                    cart_downsample=cartDownsampleFactor)
    if np.ndim(srcPolarImg) == 3:
        return out[:, 0].copy(), out[:, 3:5].copy(), out[:, 1].copy(), out[:, 2].copy(), out[:, 5].copy()
    angle, scale, rot_resp, dx, dy, trans_resp = (float(v) for v in out[0])
    return angle, (dx, dy), scale, rot_resp, trans_resp


def getRotationMatrix2D(center, angle, scale):
    """cv2.getRotationMatrix2D -> (2, 3) float64: the centre rounded to float32 (cv::Point2f), the rest in float64; angle in degrees,
    positive = counter-clockwise with the image's y axis pointing down.  Host code only."""
    cx, cy = float(np.float32(center[0])), float(np.float32(center[1]))
    rad = float(angle) * math.pi / 180.0
    a, b = math.cos(rad) * float(scale), math.sin(rad) * float(scale)
    return np.array([[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy]], np.float64)


def rotateImg(image, angle_degrees):
    """FMT.py:93-100: cv2.warpAffine(image, getRotationMatrix2D((w / 2, h / 2), angle_degrees, 1.0), (w, h), INTER_LINEAR)
    (roam_warp_affine_f32, warpaffine.hip).  Unlike cv2, which remaps u8 and f64 natively, any input is converted to float32 first
    and the output is float32.  image may be a 3-D batch of one shape; angle_degrees is then one angle for all images or a 1-D array
    with one angle per image, and the whole batch is one launch.  Argument errors (Context.warp_affine_f32's, a non-finite angle,
    an angle array that does not match the batch) are ValueError before any device call."""
    img = np.asarray(image)
    if img.ndim not in (2, 3):
        raise ValueError(f"rotateImg: a 2-D image or a 3-D batch, not {img.ndim}-D")
    h, w = img.shape[-2:]
    ang = np.asarray(angle_degrees, np.float64)
    if ang.ndim > 1 or (ang.ndim == 1 and (img.ndim != 3 or len(ang) != img.shape[0])):
        raise ValueError(f"rotateImg: one angle, or one per image of a 3-D batch, not angles of shape {ang.shape} for an image of "
                         f"shape {img.shape}")
    if not np.isfinite(ang).all():
        raise ValueError("rotateImg: the angle is not finite")
    center = (w / 2, h / 2)
    M = getRotationMatrix2D(center, ang, 1.0) if ang.ndim == 0 else np.stack([getRotationMatrix2D(center, t, 1.0) for t in ang])
    _ffi.warp_affine_args(img, M, (w, h))
    return _ffi.default_context().warp_affine_f32(img, M, (w, h))


def flowPriorFromFMT(angleRad, dxdy, cartDownsampleFactor: int = FMT_CART_DOWNSAMPLE_FACTOR, trackDownsampleFactor: int = 2,
                     cols: int = 2025):
    """A registration result (getTransformUsingFMT, Engine.fmt_register) as the tracker's motion prior -> float32 (2, 3): the affine
    map from a feature's pixel position in the previous Cartesian image at trackDownsampleFactor to its predicted position in the
    current one (getTrackedPointsKLT's initialFlow through tests' apply_affine order, Engine.set_motion_prior).  Arrays of n angles
    and (n, 2) translations give (n, 2, 3).  Host code only.

    On the registration's grid the chain is: srcRot = warpAffine(src, M), M = getRotationMatrix2D((w / 2, h / 2), degrees(angleRad),
    1) - a feature at p in src lies at M p in srcRot - then phaseCorrelate(srcRot, target) = (dx, dy), which is the shift that
    takes srcRot to target: the feature lies at M p + (dx, dy) in the target.  (PARITY.md's "minus the ego motion": the scene moves
    against the sensor.)  The grids: parseData.convertPolarImageToCartesian at factor f makes a 2 R_f x 2 R_f image, R_f = cols // f,
    centred on (R_f, R_f), in which one pixel spans cols / R_f range bins.  A pixel q of the registration's grid is therefore pixel
    s q of the tracker's, s = R_track / R_reg = (cols // trackDownsampleFactor) / (cols // cartDownsampleFactor) - 1012 / 101 =
    10.0198 for 2025 bins at 2 and 20 (a 2024-px image against a 202-px one), not the integer ratio 10 - and the prior is
    [ M_linear | s (M_translation + (dx, dy)) ]: the same rotation about the tracker image's own centre (R_track, R_track), and
    the translation scaled."""
    ang = np.asarray(angleRad, np.float64)
    d = np.asarray(dxdy, np.float64)
    if ang.ndim > 1 or d.shape != ang.shape + (2,):
        raise ValueError(f"flowPriorFromFMT: one angle and (dx, dy), or n angles and (n, 2) translations, not {ang.shape} and {d.shape}")
    if int(cartDownsampleFactor) < 1 or int(trackDownsampleFactor) < 1 or int(cols) // int(cartDownsampleFactor) < 1 \
            or int(cols) // int(trackDownsampleFactor) < 1:
        raise ValueError("flowPriorFromFMT: downsample factors >= 1 that leave at least one pixel of radius")
    if not (np.isfinite(ang).all() and np.isfinite(d).all()):
        raise ValueError("flowPriorFromFMT: the registration result is not finite")
    r_reg, r_trk = int(cols) // int(cartDownsampleFactor), int(cols) // int(trackDownsampleFactor)
    s = r_trk / r_reg

    def one(a, t):
        M = getRotationMatrix2D((2 * r_reg / 2, 2 * r_reg / 2), math.degrees(float(a)), 1.0)
        M[:, 2] = s * (M[:, 2] + t)
        return M.astype(np.float32)

    if ang.ndim == 0:
        return one(ang, d)
    return np.stack([one(a, t) for a, t in zip(ang, d)]) if len(ang) else np.zeros((0, 2, 3), np.float32)
