"""CPU side of the batched rotation prior (no GPU): the ABI declarations against the _ffi table, the argument errors raised before any
library call, the shapes the GPU test relies on, and the uniqueness condition on every pair the GPU test compares with the oracle -
the largest value of the oracle's correlation plane outside the 5 x 5 box around its maximum is at most 0.99 of the maximum (the
condition of tests/test_phase_correlate_cpu.py), so that the pick of the first maximum cannot depend on rounding.  No pair is
skipped; one that failed would be replaced by another seed in tests/fmt_batch_cases.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fmt_batch_cases as cases
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_TYPES = {"roam_ctx *": C.c_void_p, "const float *": C.c_void_p, "float *": C.c_void_p, "double *": C.c_void_p,
           "const int32_t *": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64}
ENTRIES = {
    "roam_fmt_rotation": ["ctx", "src_polar", "tgt_polar", "rows", "cols", "clip_px", "downsample", "angle_rad", "scale", "response"],
    "roam_fmt_rotation_batch_f32": ["ctx", "src", "tgt", "n", "rows", "cols", "row_stride", "image_stride", "clip_px", "downsample", "out3",
                                    "logpolar_out"],
    "roam_engine_fmt_rotation": ["ctx", "n", "prev_pool_idx", "curr_pool_idx", "clip_px", "downsample", "out3"],
}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_header_and_ffi_table_agree(name):
    from radarslampy_amd import _ffi
    txt = open(os.path.join(ROOT, "include", "roam_abi.h")).read()
    m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, txt)
    assert m, f"include/roam_abi.h does not declare {name}"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ENTRIES[name]
    types = [C_TYPES[re.sub(r"\w+$", "", a).strip()] for a in args]
    res, sig = _ffi._SIGS[name]
    assert res is C.c_int32 and sig == types
    assert name in _ffi.ABI_SYMBOLS
    assert (_ffi.FMT_MIN_R, _ffi.FMT_MAX_R) == tuple(int(re.search(r"#define\s+ROAM_FMT_%s_R\s+(\d+)" % k, txt).group(1)) for k in ("MIN", "MAX"))


def test_library_exports_the_entries():
    from radarslampy_amd import _ffi
    lib = C.CDLL(_ffi.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name


def test_argument_errors_come_before_any_library_call(monkeypatch):
    from radarslampy_amd import FMT, _ffi
    from radarslampy_amd.engine import Engine

    def no_device(*a, **k):
        raise AssertionError("a library call was made")
    monkeypatch.setattr(_ffi, "default_context", no_device)
    monkeypatch.setattr(_ffi, "load_library", no_device)
    ctx = object.__new__(_ffi.Context)                                        # no library, no device behind it
    ctx.h = None
    img = np.zeros((3, 16, 2700), np.float32)
    for call in (lambda a, b, **k: ctx.fmt_rotation_batch(a, b, clip_px=0, **k), lambda a, b, **k: FMT.getRotationUsingFMT(a, b, k.get("downsample", 10), 0)):
        with pytest.raises(AssertionError, match="same shape"):
            call(img, img[:, :, :2000])
        with pytest.raises(AssertionError, match="same shape"):
            call(img, img[:2])
        with pytest.raises(ValueError, match="rows"):
            call(img[:, :7], img[:, :7])                                       # rows < 8
        with pytest.raises(ValueError, match="1303"):
            call(img[:, :, :30], img[:, :, :30])                               # R = 30 // 10 = 3
        with pytest.raises(ValueError, match="1303"):
            call(img[:, :, :2608], img[:, :, :2608], downsample=2)             # R = 1304
        with pytest.raises(ValueError):
            call(img[:0], img[:0])                                             # an empty batch
    with pytest.raises(ValueError, match="1303"):
        ctx.fmt_rotation_batch(img, img, clip_px=39, downsample=10)            # the clip decides: R = 3
    with pytest.raises(ValueError, match="1303"):
        ctx.fmt_rotation_batch(img[0], img[0], clip_px=0, downsample=2)        # no clip: R = 1350, 2-D input
    with pytest.raises(ValueError, match="downsample"):
        ctx.fmt_rotation_batch(img, img, downsample=0)
    with pytest.raises(ValueError):
        ctx.fmt_rotation_batch(img[0, 0], img[0, 0])
    with pytest.raises(ValueError):
        ctx.fmt_rotation_batch(img[None], img[None])
    assert _ffi.fmt_rotation_batch_args(img[:, :, :2606], img[:, :, :2606], 0, 2)[2:] == (2606, 1303)      # the limits themselves pass
    assert _ffi.fmt_rotation_batch_args(img[0, :8, :40], img[0, :8, :40], 1012, 10)[2:] == (40, 4)
    eng = object.__new__(Engine)                                              # an engine without a library behind it
    eng.ctx, eng.lib, eng.pool_scans, eng.rows = ctx, None, 4, 400
    eng.cfg = _ffi.EngineCfg(clip=2025)
    for prev, curr, kw in (([0, 1], [1], {}), ([], [], {}), ([0, 4], [1, 2], {}), ([0, -1], [1, 2], {}), ([0], [1], dict(downsample=0)),
                           ([0], [1], dict(clip_px=30)), ([0], [1], dict(clip_px=0, downsample=1))):
        with pytest.raises(ValueError):
            eng.fmt_rotation(prev, curr, **kw)
    eng.rows = 7
    with pytest.raises(ValueError, match="rows"):
        eng.fmt_rotation([0], [1])
    eng.ctx = None


def test_shapes_of_the_cases():
    """the log-polar size and the DFT plane of every case are the ones the GPU test is written for"""
    for case, (clip_px, ds, R, (dh, dw), (M, N)) in cases.CASES.items():
        p0, p1 = cases.images(case)
        assert p0.shape == p1.shape and p0.dtype == p1.dtype == np.float32
        clip = clip_px if 0 < clip_px < p0.shape[1] else p0.shape[1]
        assert clip // ds == R and (int(np.rint(R * np.pi)), R) == (dh, dw)
        assert (oracle._get_optimal_dft_size(dh), oracle._get_optimal_dft_size(dw)) == (M, N)
        assert cases.logpolar(case, p0).shape == (dh, dw)
    assert cases.images("b")[0].shape == (16, 40) and cases.images("c")[0].shape == (399, 497) and cases.images("a")[0].shape == (400, 2025)
    A, B = cases.batch("c")
    assert not A.flags.c_contiguous and A.strides == (399 * 504 * 4, 504 * 4, 4) and A.strides == B.strides
    from radarslampy_amd._ffi import _f32_rows_in_place
    assert _f32_rows_in_place(A) is A                                         # read in place, strides and all


@pytest.mark.parametrize("case", sorted(cases.CASES))
def test_every_pair_has_a_unique_peak(case):
    u = cases.uniqueness(case)
    print(f"case {case}: largest second value / maximum per pair: {u}")
    assert len(u) == 4
    for i, v in enumerate(u):
        assert v <= 0.99, (case, i, v)
