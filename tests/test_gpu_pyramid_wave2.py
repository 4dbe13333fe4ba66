"""GPU: pyr_down2_wave_kernel (levels 2 and 3 of the pyramid, one wavefront per band) byte for byte against the oracle's pyr_down
applied twice, through the pyramid builder's two-level branch (Context.pyr_down2_u8), at the smallest shapes at which each border can go
wrong; every byte of the pyramid storage outside the two output levels - the gaps after each level's rows among them - is a 0xA5
sentinel that must survive."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def _levels(w, h):
    dw, dh = (w + 1) // 2, (h + 1) // 2
    return [(w, h), (dw, dh), ((dw + 1) // 2, (dh + 1) // 2)]


def _layout(w, h, engine_like):
    """offsets of the three levels inside a lane and the lane stride.  engine_like: as pyr_desc_init lays out the 4-level pyramid whose
    level 1 is w x h (levels 256-B aligned, level 0 in front); otherwise the same rounding plus 64 guard bytes after every level, so
    that there is a sentinel behind each level's last row whatever its size."""
    offs, off = [], 0
    sizes = ([(2 * w) * (2 * h)] if engine_like else []) + [a * b for a, b in _levels(w, h)]
    for n, sz in enumerate(sizes):
        if not (engine_like and n == 0):
            offs.append(off)
        off += ((sz + 255) & ~255) + (0 if engine_like else 64)
    return offs, off


def _inputs(w, h):
    rng = np.random.default_rng(w * 131 + h)
    yield "random", rng.integers(0, 256, (h, w), dtype=np.uint8)
    yield "all255", np.full((h, w), 255, np.uint8)
    yield "all0", np.zeros((h, w), np.uint8)
    yield "checker", (((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1) * 255).astype(np.uint8)
    pts = np.zeros((h, w), np.uint8)
    for y in (0, h // 2, h - 1):
        for x in (0, w // 2, w - 1):
            if (y, x) != (h // 2, w // 2):
                pts[y, x] = 255                         # each corner and each edge midpoint
    yield "corners_edges", pts


@pytest.fixture(scope="module")
def ctx():
    from radarslampy_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


def _run(ctx, w, h, lanes, engine_like, kernel):
    lv = _levels(w, h)
    offs, stride = _layout(w, h, engine_like)
    inputs = list(_inputs(w, h))
    # lanes hold different inputs: input n goes to lane n % lanes of launch n // lanes
    for first in range(0, len(inputs), lanes):
        batch = [inputs[(first + b) % len(inputs)] for b in range(lanes)]
        buf = np.full(lanes * stride, SENTINEL, np.uint8)
        for b, (_, im) in enumerate(batch):
            buf[b * stride + offs[0]: b * stride + offs[0] + w * h] = im.ravel()
        before = buf.copy()
        assert ctx.pyr_down2_u8(buf, w, h, lanes, stride, offs) == kernel
        written = np.zeros(buf.size, bool)
        for b, (name, im) in enumerate(batch):
            want = oracle.build_pyramid(im, 2)
            for l in (1, 2):
                lw, lh = lv[l]
                a = b * stride + offs[l]
                got = buf[a: a + lw * lh].reshape(lh, lw)
                assert np.array_equal(got, want[l]), (w, h, name, "lane", b, "level", l, np.argwhere(got != want[l])[:4])
                written[a: a + lw * lh] = True
        # the inputs, the gaps behind each level's rows and everything else in the storage are as they were
        assert np.array_equal(buf[~written], before[~written]), (w, h, np.flatnonzero((buf != before) & ~written)[:8])


def test_live_shape_three_lanes(ctx):
    # 1012 -> 506 -> 253: the last lane's partial dword, odd dw2, a partial last band; lane stride as pyr_desc_init gives it
    _run(ctx, 1012, 1012, 3, True, "wave")


def test_smallest_width_short_image(ctx):
    # both vertical reflections inside one band
    _run(ctx, 512, 36, 2, False, "wave")


def test_largest_width_odd_heights(ctx):
    # 1024 x 70: dh = 35 is odd (dh2 = 18 is not: the next test has both odd)
    assert _levels(1024, 70)[1][1] % 2 == 1
    _run(ctx, 1024, 70, 2, False, "wave")


def test_largest_width_both_output_heights_odd(ctx):
    # 1024 x 66: dh = 33, dh2 = 17, both odd
    assert _levels(1024, 66)[1][1] % 2 == 1 and _levels(1024, 66)[2][1] % 2 == 1
    _run(ctx, 1024, 66, 2, False, "wave")


def test_fewer_rows_than_one_band(ctx):
    _run(ctx, 1012, 22, 1, False, "wave")


def test_rejected_width_takes_the_row_kernel(ctx):
    # below the wave kernel's smallest width: the LDS kernel, unchanged, through the same entry point
    _run(ctx, 508, 36, 2, False, "rows")
