"""Fourier-Mellin registration with the reference's names (reference FMT.py:10-90): the rotation prior (csrc/fmt.hip) and the
translation by phase correlation (csrc/fft.hip); the computation runs on the MI355X.  SURVEY §8f-f4."""
from . import _ffi
from .parseData import RANGE_RESOLUTION_CART_M

FMT_DOWNSAMPLE_FACTOR = 10      # FMT.py:10
FMT_RANGE_CLIP_M = 87.5         # FMT.py:11


def getTranslationUsingPhaseCorrelation(srcImg, targetImg):
    """FMT.py:13-33 -> ((dx, dy), response): cv2.phaseCorrelate(srcImg, targetImg, Hanning window) on two images of one shape"""
    a, b = _ffi.phase_correlate_args(srcImg, targetImg)
    if a.ndim != 2:
        raise ValueError(f"getTranslationUsingPhaseCorrelation: 2-D images, not {a.ndim}-D")
    return _ffi.default_context().phase_correlate(a, b, hanning=True)


def getRotationUsingFMT(srcPolarImg, targetPolarImg, downsampleFactor: int = FMT_DOWNSAMPLE_FACTOR, maxRangeClipM=FMT_RANGE_CLIP_M):
    """-> (angleRad with R(angleRad) @ src = target, scaling factor, response); polar (not log-polar) float32 images"""
    assert srcPolarImg.shape == targetPolarImg.shape, "Images need to have the same shape!"
    clip = int(maxRangeClipM / RANGE_RESOLUTION_CART_M) if maxRangeClipM > 0 else 0
    return _ffi.default_context().fmt_rotation(srcPolarImg, targetPolarImg, clip_px=clip, downsample=int(downsampleFactor))
