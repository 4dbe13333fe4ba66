"""The cases of tests/warp_tile_cases.py reach every path of warp_gather_kernel (radarslampy_amd/csrc/warp.hip) that depends on the
geometry or on the batch size.  These are conditions on the cases, asserted on the oracle's exact sampling map, not measurements: if
one fails, tests/test_gpu_warp_tiles.py no longer tests that path and a geometry has to move.  The last test ties the exported map to
the image the GPU test compares against."""
import numpy as np
import pytest

import oracle
from warp_tile_cases import (BATCH, BOX, DARK, DIRECT, GEOMETRIES, PARTIAL_BATCHES, PARTIAL_GEOMETRIES, RECORD_NAMES, WG_LB, class_table,
                             classify, expected_images, fill_units, format_table, geometry_id, grid, group_sizes, lane_maps, records,
                             remap_numpy)


@pytest.fixture(scope="module")
def table():
    t = class_table()
    print()
    print(format_table(t))
    return t


def test_geometries_are_engine_shapes():
    # roam_engine_create: rows 2 ... 1020, clip 32 ... 4094 with clip / 2 even, payload inside the stride; and nothing larger than W = 1000
    for rows, clip, stride, off in GEOMETRIES:
        assert 2 <= rows <= 1020 and 32 <= clip <= 4094 and (clip // 2) % 2 == 0 and off >= 0 and stride >= off + clip
        assert 2 * (clip // 2) <= 1000
    assert all(g in GEOMETRIES for g in PARTIAL_GEOMETRIES)


def test_every_tile_class_occurs(table):
    for col in ("dark", "direct_all_in", "direct_part_out", "box_nochk", "box_chk", "box_part_out", "box_wide", "box_tall", "box_wraps",
                "direct_wraps", "box_iy_top"):
        assert any(t[col] > 0 for t in table), col


def test_pass_sizes(table):
    per = set()
    for t in table:
        per |= set(t["per"])
    assert 1 in per and WG_LB in per, sorted(per)
    assert len([p for p in per if 1 < p < WG_LB]) >= 5, sorted(per)


def _units_over_box_tiles(geometry, B):
    c = classify(geometry[0], geometry[1])
    units, short = set(), False
    for per in sorted(set(int(p) for p in c["per"][c["cls"] == BOX])):
        for n in group_sizes(B):
            for p in fill_units(n, per):
                units |= set(p)
                short |= sum(p) < per
    return units, short


def test_fill_units_model():
    assert group_sizes(70) == [32, 32, 6] and group_sizes(1) == [1] and group_sizes(33) == [32, 1]
    assert fill_units(32, 32) == [(4,) * 8]
    assert fill_units(6, 32) == [(4, 2)]
    assert fill_units(32, 5) == [(4, 1)] * 6 + [(2,)]
    assert fill_units(31, 7) == [(4, 2, 1)] * 4 + [(2, 1)]
    assert fill_units(1, 1) == [(1,)]
    for n in range(1, 33):
        for per in range(1, 33):
            p = fill_units(n, per)
            assert sum(sum(u) for u in p) == n and all(sum(u) <= per for u in p) and all(sum(u) == per for u in p[:-1])


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=geometry_id)
def test_fill_units_of_the_batch(geometry):
    """70 lanes: the fills of the box tiles of every geometry use each of the units 4, 2 and 1, and a pass of fewer than `per` scans"""
    units, short = _units_over_box_tiles(geometry, BATCH)
    assert units == {4, 2, 1} and short, (units, short)


def test_partial_batches_reach_short_passes():
    for g in PARTIAL_GEOMETRIES:
        for B in PARTIAL_BATCHES:
            units, short = _units_over_box_tiles(g, B)
            assert short, (g, B)
            assert units == ({1} if B == 1 else {4, 2, 1}), (g, B, units)


def test_grid_edges():
    totals = [np.prod(grid(g[1], BATCH)) for g in GEOMETRIES]
    assert any(t % 8 for t in totals), totals               # blocks with vid >= total
    assert any((2 * (g[1] // 2)) % 64 and (2 * (g[1] // 2)) % 16 for g in GEOMETRIES)      # xin and sok


def test_lane_maps():
    for B in (BATCH,) + PARTIAL_BATCHES:
        a, b = lane_maps(B)
        assert a.shape == b.shape == (B,) and a.dtype == b.dtype == np.int32
        assert (a != b).all()
        for m in (a, b):
            assert m.min() >= 0 and m.max() < 6
            for l0 in range(0, B - WG_LB + 1, WG_LB):
                assert set(m[l0:l0 + WG_LB].tolist()) == set(range(6))
            if B > 6:
                d = np.diff(m)
                assert (d > 0).any() and (d < 0).any() and len(set(m.tolist())) < B


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=geometry_id)
def test_records(geometry):
    rows, clip, stride, off = geometry
    recs = records(geometry)
    assert len(recs) == len(RECORD_NAMES) == 6
    outside = np.ones(stride, bool)
    outside[off:off + clip] = False
    for name, rec in zip(RECORD_NAMES, recs):
        assert rec.shape == (rows, stride) and rec.dtype == np.uint8
        assert (rec[:, outside] == 255).all(), name
    pay = {n: r[:, off:off + clip] for n, r in zip(RECORD_NAMES, recs)}
    assert (pay["ones"] == 255).all()
    assert (pay["seam"][0] == 255).all() and (pay["seam"][rows - 1] == 128).all() and not pay["seam"][1:rows - 1].any()
    assert (pay["rim"][:, [0, clip - 2, clip - 1]] == 255).all() and not pay["rim"][:, 1:clip - 2].any()
    assert pay["rowcode"][rows - 1, clip - 1] == (37 * (rows - 1) + 11 * (clip - 1)) & 255
    assert not np.array_equal(pay["noise"], pay["noise2"])
    # the six images differ pairwise: a lane that shows another lane's scan is seen
    imgs = expected_images(geometry)
    for i in range(6):
        for j in range(i):
            assert not np.array_equal(imgs[i], imgs[j]), (RECORD_NAMES[i], RECORD_NAMES[j])


@pytest.mark.parametrize("geometry", [GEOMETRIES[1], GEOMETRIES[3]], ids=geometry_id)
def test_map_export_reproduces_the_oracle_warp(geometry):
    rows, clip, stride, off = geometry
    sx, sy = oracle.polar_sampling_map(rows, clip)
    W = 2 * (clip // 2)
    assert sx.shape == sy.shape == (W, W) and sx.dtype == sy.dtype == np.int32
    for name, rec in zip(RECORD_NAMES, records(geometry)):
        polar = rec[:, off:off + clip].astype(np.float32) / np.float32(255.)
        cart, u8 = oracle.convertPolarImageToCartesian(polar, want_u8=True)
        got_f, got_u8 = remap_numpy(polar, rows, clip)
        assert np.array_equal(got_f, cart), name
        assert np.array_equal(got_u8, u8), name


def test_top_tap_row_has_zero_weight():
    """iy == rows + 1 occurs at few azimuths, always with a zero fraction: its second tap row (padded row rows + 2, which the kernel
    stages as polar row 1) never contributes - the reason the engine can take rows >= 2 and must refuse rows == 1"""
    seen = 0
    for rows, clip, _, _ in GEOMETRIES:
        sx, sy = oracle.polar_sampling_map(rows, clip)
        top = ((sy >> 5) >= rows + 1) & ((sx >> 5) < clip)
        assert ((sy[top] >> 5) == rows + 1).all() and ((sy[top] & 31) == 0).all(), (rows, clip)
        seen += int(top.sum())
    assert seen > 0
