"""GPU (-m gpu): the device argsort's heapsort fallback (csrc/npsort_wave.h, csrc/blobprune.h) through the public peak extraction,
on the rows of tests/sort_adversary_cases.py - McIlroy's quicksort adversary with ties in pairs and organ pipes, which use up the
depth budget 2 * floor(log2 n) at wave level and inside the segments sorted one lane each, next to controls that do not
(tests/test_sort_adversary_cpu.py proves both, and that the order of equal heights shows in the peak lists).  The truth is live
scipy under NumPy 1.22.3's argsort (peaks_cond_cases.truth); every comparison is exact."""
import numpy as np
import pytest

import peaks_cond_cases as pc
import sort_adversary_cases as sc

pytestmark = pytest.mark.gpu

PROMINENCES = [0, (None, 0.05)]


@pytest.fixture(scope="module")
def ctx():
    from radarslampy_amd import _ffi
    c = _ffi.default_context(0)
    assert "gfx950" in c.device_info()["arch"]
    return c


@pytest.fixture(scope="module")
def truth():
    """truth(image name, distance, prominence) of the image as float32 (the u8 images decoded), computed once"""
    pytest.importorskip("scipy")
    done = {}

    def get(name, d, p=None):
        if (name, d, p) not in done:
            kind, names, img = sc.images()[name]
            done[name, d, p] = pc.truth(img if kind == "f32" else pc.decode(img), d, p)
        return done[name, d, p]
    return get


def _same(got, want, what):
    if not np.array_equal(got, want):
        rows = sorted(set(got[:, 0].tolist()) | set(want[:, 0].tolist()))
        bad = [r for r in rows if not np.array_equal(got[got[:, 0] == r], want[want[:, 0] == r])]
        kind, names, img = sc.images()[what[0]]
        raise AssertionError(f"{what}: rows {[(r, names[r]) for r in bad]} differ")


def test_f32_images_at_every_distance(ctx, truth):
    for name, (kind, names, img) in sc.images().items():
        if kind == "f32":
            for d in sc.DISTANCES:
                _same(ctx.peaks_polar_f32(img, distance=d), truth(name, d), (name, d))


def test_f32_survivors_feed_prominence_and_threshold(ctx, truth):
    for name in ("f32_first", "f32_small"):
        img = sc.images()[name][2]
        for d in sc.DISTANCES:
            for p in PROMINENCES:
                _same(ctx.peaks_polar_f32(img, distance=d, prominence=p), truth(name, d, p), (name, d, p))


def test_u8_record_path(ctx, truth):
    for name, (kind, names, u8) in sc.images().items():
        if kind == "u8":
            cols = u8.shape[1]
            for d in sc.DISTANCES:
                for p in [None] + (PROMINENCES if name == "u8_first" else []):
                    got = ctx.peaks_record_u8(u8, payload_off=0, clip=cols, distance=d, prominence=p)
                    _same(got, truth(name, d, p), (name, d, p))


def test_u8_rows_inside_an_oxford_record(ctx, truth):
    """11 metadata bytes, 3768 power bins of which 2025 are read, random bytes everywhere else"""
    u8 = sc.images()["u8_oxford"][2]
    assert u8.shape[1] == 2025
    rec = np.random.default_rng(3779).integers(0, 256, size=(u8.shape[0], 3779), dtype=np.uint8)
    rec[:, 11:11 + 2025] = u8
    for d in sc.DISTANCES:
        got = ctx.peaks_record_u8(rec, payload_off=11, clip=2025, distance=d)
        _same(got, truth("u8_oxford", d), ("u8_oxford", d, "Oxford layout"))


def test_dropin(ctx, truth):
    from radarslampy_amd.getPointCloud import getPointCloudPolarInd
    got = getPointCloudPolarInd(sc.images()["f32_last"][2], peakDistance=5)
    assert got.dtype == np.int64
    _same(got, truth("f32_last", 5), ("f32_last", 5, "drop-in"))


def test_same_result_every_time_and_whatever_the_neighbours(ctx):
    """one wavefront per row: a row's peaks are the same when the image is run twice, when the row is run alone and when it stands
    first, last or in the middle of a stack"""
    rows, imgs = sc.key_rows(), sc.images()
    for d in (3, 5, 10.5):
        alone = {}
        for name, (kind, names, img) in imgs.items():
            run = (lambda a: ctx.peaks_polar_f32(a, distance=d)) if kind == "f32" else \
                  (lambda a: ctx.peaks_record_u8(a, payload_off=0, clip=a.shape[1], distance=d))
            first = run(img)
            assert np.array_equal(run(img), first), (name, d)
            for i, n in enumerate(names):
                if rows[n].kind == sc.CONTROL:
                    continue
                if (kind, n) not in alone:
                    alone[kind, n] = run(getattr(rows[n], kind)[None])[:, 1]
                assert np.array_equal(first[first[:, 0] == i][:, 1], alone[kind, n]), (name, n, d)
