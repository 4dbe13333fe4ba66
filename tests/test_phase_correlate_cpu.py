"""CPU side of phase correlation (no GPU): the drop-in's name and argument errors, raised before any device call; the ABI
declaration; the restatement the GPU test is judged by against the oracle; and the uniqueness condition on every input of the GPU
test - the largest value of the oracle's correlation plane outside the 5 x 5 box around its maximum is at most 0.99 of the maximum,
so that the pick of the first maximum cannot depend on rounding.  No input is skipped or filtered."""
import os
import re

import numpy as np
import pytest

import oracle
import phase_correlate_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pairs():
    return pc.all_pairs(oracle.convertPolarImageToCartesian)


def test_name_imports_with_the_reference_signature():
    import inspect
    from radarslampy_amd import FMT
    assert list(inspect.signature(FMT.getTranslationUsingPhaseCorrelation).parameters) == ["srcImg", "targetImg"]
    from radarslampy_amd import _ffi
    assert callable(_ffi.Context.phase_correlate) and "roam_phase_correlate_f32" in _ffi.ABI_SYMBOLS


def test_header_declares_the_entry():
    txt = open(os.path.join(ROOT, "include", "roam_abi.h")).read()
    m = re.search(r"int32_t\s+roam_phase_correlate_f32\s*\(([^;]*)\)\s*;", txt)
    assert m, "include/roam_abi.h does not declare roam_phase_correlate_f32"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["ctx", "src", "tgt", "batch", "rows", "cols", "row_stride", "image_stride", "hanning",
                                                          "out_dxdy", "out_response"]


def test_argument_errors_come_before_any_device_call(monkeypatch):
    from radarslampy_amd import FMT, _ffi

    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_ffi, "default_context", no_device)
    monkeypatch.setattr(_ffi, "load_library", no_device)
    img = np.zeros((16, 24), np.float32)
    with pytest.raises(AssertionError, match="same shape"):
        FMT.getTranslationUsingPhaseCorrelation(img, img[:, :20])
    with pytest.raises(ValueError):
        FMT.getTranslationUsingPhaseCorrelation(img[0], img[0])
    with pytest.raises(ValueError):
        FMT.getTranslationUsingPhaseCorrelation(img[None], img[None])
    with pytest.raises(ValueError):
        FMT.getTranslationUsingPhaseCorrelation(img[:1], img[:1])              # a 1-wide Hanning window divides by zero
    with pytest.raises(ValueError):
        FMT.getTranslationUsingPhaseCorrelation(np.zeros((2, 4097), np.float32), np.zeros((2, 4097), np.float32))
    ctx = object.__new__(_ffi.Context)                                        # no library, no device behind it
    with pytest.raises(AssertionError, match="same shape"):
        ctx.phase_correlate(img, img.T)
    with pytest.raises(ValueError):
        ctx.phase_correlate(np.zeros((2, 3, 4, 5), np.float32), np.zeros((2, 3, 4, 5), np.float32))
    with pytest.raises(ValueError):
        ctx.phase_correlate(np.zeros((0, 8, 8), np.float32), np.zeros((0, 8, 8), np.float32))
    with pytest.raises(ValueError):
        ctx.phase_correlate(np.zeros((3, 8, 1), np.float32), np.zeros((3, 8, 1), np.float32))
    ctx.h = None


def test_in_place_rule():
    from radarslampy_amd._ffi import _f32_rows_in_place
    a = np.zeros((6, 10, 12), np.float32)
    for v in (a, a[0], a[::2], a[:, ::2], a[:, :, 2:9], a[1, ::3, 1:5]):
        assert _f32_rows_in_place(v) is v
    for v in (a[:, :, ::2], a[::-1], a[:, ::-1], a.astype(np.float64), a[0].T, np.broadcast_to(a[0, 0], (10, 12))):
        w = _f32_rows_in_place(v)
        assert w is not v and w.flags.c_contiguous and w.dtype == np.float32 and np.array_equal(w, v)


def test_restatement_is_the_oracle(pairs):
    done = set()
    for name, a, b, hanning in pairs:
        if hanning and a.shape not in done and a.size <= 1 << 20:
            done.add(a.shape)
            assert pc.correlate_formula(a, b)[:2] == oracle.phaseCorrelate(a, b), name
    assert len(done) >= 6
    assert [pc.optimal_dft_size(n) for n in (1, 2, 7, 101, 317, 1012, 2024, 2025, 4096)] == \
           [oracle._get_optimal_dft_size(n) for n in (1, 2, 7, 101, 317, 1012, 2024, 2025, 4096)]


def test_every_input_has_a_unique_peak(pairs):
    assert {a.shape for _, a, _, _ in pairs} >= set(pc.SHAPES) | {(2048, 2048), (4096, 4096)}
    worst = 0.0
    for name, a, b, hanning in pairs:
        assert a.shape == b.shape and a.dtype == b.dtype == np.float32, name
        u = pc.peak_uniqueness(pc.correlate_formula(a, b, hanning)[2])
        worst = max(worst, u)
        assert u <= 0.99, (name, u)
    print("largest second value / maximum:", worst)
