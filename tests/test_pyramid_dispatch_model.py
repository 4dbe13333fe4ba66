"""CPU: the kernel choice of csrc/pyrklt.hip's pyramid builders (launch_build_pyramid / launch_pyr_down), restated in Python, and the
coverage it implies for the GPU tests: the engine layouts of tests/test_gpu_engine_shapes.py must reach every branch - the fused
two-level kernel, the wave kernel with the engine's dark table, the row kernel and the tiled kernel - at every level where it can
occur, and the standalone tracker sizes must reach the wave kernel without a dark table.  The condition strings below are the
source's own: when a threshold moves, this test fails and points at the model (and so at the GPU coverage) to update with it."""
import os
import re

from gen_inputs import ENGINE_LAYOUTS, KLT_SIZES

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "radarslampy_amd", "csrc", "pyrklt.hip")
LEVELS = 4

# the conditions this model restates, as they stand in the source (whitespace-normalised)
CONDITIONS = [
    "const bool rows_ok = ((w & 3) == 0) && w >= 16 && w <= PR_MAXW && ((dw & 1) == 0) && ((src_lane_stride & 3) == 0) &&",
    "const bool wave_ok = rows_ok && ((w & 3) == 0) && (w >> 2) > 32 * PW_DPL && (w >> 2) <= 64 * PW_DPL && ((dw & 3) == 0) && h >= 8 &&",
    "((reinterpret_cast<uintptr_t>(dst) & 1) == 0) && h >= 4;",
    "if (l + 2 < ROAM_PYR_LEVELS && (w & 3) == 0 && w >= 64 && w <= PF_MAXW && (dw & 1) == 0 && h >= 16 && dh >= 8 &&",
    "launch_pyr_down(st, pyr + d.off[l], d.lane_stride, w, h, pyr + d.off[l + 1], d.lane_stride, B, l == 0 ? dark_l0 : nullptr);",
    "off += (((int64_t)w * h) + 255) & ~(int64_t)255;",
]


def _norm(s):
    return re.sub(r"\s+", " ", s).strip()


def _source():
    with open(SRC) as f:
        return f.read()


def _define(src, name):
    m = re.search(r"^#define\s+%s\s+(\d+)" % name, src, re.M)
    assert m, name
    return int(m.group(1))


def _consts():
    src = _source()
    return {k: _define(src, k) for k in ("PR_MAXW", "PW_DPL", "PF_MAXW")}


def pyr_down_branch(w, h, dark, c):
    """launch_pyr_down for one level (every buffer 256-B aligned: pyr_desc_init's level offsets, the scratch pyramids)"""
    dw = (w + 1) // 2
    rows_ok = w % 4 == 0 and 16 <= w <= c["PR_MAXW"] and dw % 2 == 0 and h >= 4
    wave_ok = rows_ok and 32 * c["PW_DPL"] < (w >> 2) <= 64 * c["PW_DPL"] and dw % 4 == 0 and h >= 8
    if wave_ok:
        return "wave+dark" if dark else "wave"
    return "rows" if rows_ok else "tiled"


def pyramid_branches(w, h, engine, c=None):
    """launch_build_pyramid on a w x h level 0 -> the kernel that makes each level 1..3, as [(source level, branch)]; engine=True
    passes the engine's dark table (it is only ever given to level 0)"""
    c = c or _consts()
    shapes = [(w, h)]
    for _ in range(LEVELS - 1):
        shapes.append(((shapes[-1][0] + 1) // 2, (shapes[-1][1] + 1) // 2))
    out, l = [], 0
    while l + 1 < LEVELS:
        (lw, lh), (dw, dh) = shapes[l], shapes[l + 1]
        if l + 2 < LEVELS and lw % 4 == 0 and 64 <= lw <= c["PF_MAXW"] and dw % 2 == 0 and lh >= 16 and dh >= 8:
            out += [(l, "fused"), (l + 1, "fused")]
            l += 2
            continue
        out.append((l, pyr_down_branch(lw, lh, engine and l == 0, c)))
        l += 1
    return out


def test_the_model_restates_the_source():
    src = _norm(_source())
    for cond in CONDITIONS:
        assert _norm(cond) in src, "pyrklt.hip changed: update this model and the GPU shape lists with it\n  " + cond
    assert _consts() == {"PR_MAXW": 2048, "PW_DPL": 8, "PF_MAXW": 1024}


def test_model_on_the_oxford_layout():
    # 2024 -> 1012 by the wave kernel with the dark table, then 1012 -> 506 -> 253 in one pass
    assert pyramid_branches(2024, 2024, True) == [(0, "wave+dark"), (1, "fused"), (2, "fused")]


EXPECTED = {        # W: branch making levels 1, 2, 3 (the table of the engine-shape tests)
    2024: ["wave+dark", "fused", "fused"],
    132: ["fused", "fused", "tiled"],
    496: ["fused", "fused", "rows"],
    1000: ["fused", "fused", "tiled"],
    1024: ["fused", "fused", "rows"],
    1028: ["rows", "tiled", "tiled"],
    1032: ["wave+dark", "fused", "fused"],
    2048: ["wave+dark", "fused", "fused"],
    2052: ["tiled", "tiled", "tiled"],
    3768: ["tiled", "rows", "tiled"],
}


def test_engine_layouts_take_the_expected_branches():
    got = {}
    for clip, rows, stride, off in ENGINE_LAYOUTS:
        W = 2 * (clip // 2)
        got[W] = [b for _, b in pyramid_branches(W, W, True)]
    assert got == EXPECTED


def test_engine_layouts_reach_every_branch_at_every_level_it_can_occur():
    """every (level, branch) pair an engine image can produce (W = 2 * (clip // 2), clip 32 ... 4094 with clip / 2 even) is
    reached by one of ENGINE_LAYOUTS - except the wave kernel at level 1 (W 4000 ... 4094), which the standalone tracker sizes
    reach instead"""
    possible = set()
    for clip in range(32, 4095):
        if (clip // 2) % 2 == 0:
            W = 2 * (clip // 2)
            possible |= set(pyramid_branches(W, W, True))
    covered = set()
    for clip, rows, stride, off in ENGINE_LAYOUTS:
        W = 2 * (clip // 2)
        covered |= set(pyramid_branches(W, W, True))
    assert possible - covered == {(1, "wave")}, sorted(possible - covered)
    assert {b for _, b in covered} == {"fused", "wave+dark", "rows", "tiled"}
    klt = set()
    for h, w in KLT_SIZES:
        klt |= set(pyramid_branches(w, h, False))
    assert {(0, "wave"), (1, "wave")} <= klt
    assert {b for _, b in klt} == {"fused", "wave", "rows", "tiled"}
    for lvl in range(3):                                   # the tracker sizes reach the row and tiled kernels at every level
        assert {(lvl, "rows"), (lvl, "tiled")} <= klt, lvl


def test_engine_layouts_are_accepted_by_roam_engine_create():
    # engine.hip roam_engine_create: rows 2 ... 1020, clip 32 ... 4094 with clip / 2 even, payload inside the stride
    for clip, rows, stride, off in ENGINE_LAYOUTS:
        assert 2 <= rows <= 1020 and 32 <= clip <= 4094 and (clip // 2) % 2 == 0 and off >= 0 and stride >= off + clip
    assert any(stride % 4 for _, _, stride, _ in ENGINE_LAYOUTS) and any(off % 4 for _, _, _, off in ENGINE_LAYOUTS)
    assert any(rows != 400 for _, rows, _, _ in ENGINE_LAYOUTS) and max(c for c, _, _, _ in ENGINE_LAYOUTS) > 2048
