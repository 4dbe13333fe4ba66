"""GPU (-m gpu; the scans themselves are held without one): rt_det_strip_kernel's screen (sd_tile_fast, csrc/retrack_det.hip: a wave reads the xx-side box of a box size only if
one of its 128 positions is not ruled out by the bound from dyy and the xx-mid box) on scans crafted for the ways a wave-uniform skip
can go wrong, against oracle.doh_maxima: every candidate key and float64 determinant bit for bit, through Engine.debug_detect, at
clip 132 and 188.  A reflector is a Gaussian spot drawn at a chosen Cartesian pixel on speckle too weak to keep any wave from skipping:

    single_lane   the spot lies just right of strip 0, so that in some waves of strip 0 ONE lane - its last, the halo column the
                  neighbour strip's maxima are compared with - needs the box, and that lane's product passes the threshold
    straddle      the maximum lies on the last output column of strip 0, its neighbourhood half in strip 1
    first_step    the maximum lies in the first row of the first step that takes the fast path (step 1; step 0 clips its box rows)
    last_step     the maximum lies in the last fast step
    speckle       no reflector: nearly every wave skips both boxes and nothing may be found
    saturated     strong noise: the waves read everything, as before the screen

Whether a scan is what its name says is held here with the model of the screen (tests/det_screen_model.py) and the oracle alone,
before the device's list is looked at."""
import functools

import numpy as np
import pytest

import det_candidate_cases as dc
import det_screen_model as m

ROWS = 400
SCANS = ("single_lane", "straddle", "first_step", "last_step", "speckle", "saturated")


def _speckle(clip, hi):
    return np.random.default_rng([clip, hi]).integers(0, hi, size=(ROWS, clip)).astype(np.uint8)


def _reflector(pay, r, c, amp=255.0, sigma=2.0):
    """a Gaussian spot around Cartesian pixel (row r, column c), drawn into the polar samples that the warp reads there"""
    clip = pay.shape[1]
    W = 2 * (clip // 2)
    a, k = np.meshgrid(np.arange(ROWS), np.arange(clip), indexing="ij")
    x = 0.5 * (k + 0.5) * np.cos(2 * np.pi * (a + 0.5) / ROWS) + W / 2 - 1
    y = 0.5 * (k + 0.5) * np.sin(2 * np.pi * (a + 0.5) / ROWS) + W / 2 - 1
    return np.maximum(pay, np.floor(amp * np.exp(-0.5 * ((x - c) ** 2 + (y - r) ** 2) / sigma ** 2))).astype(np.uint8)


def _last_fast_step(W):
    return (W - 1 - m.SD_HR - (m.SD_T - 1)) // m.SD_T


def _payload(name, clip):
    W = 2 * (clip // 2)
    if name == "speckle":
        return _speckle(clip, 32)
    if name == "saturated":
        return np.random.default_rng([clip, 1]).integers(128, 256, size=(ROWS, clip)).astype(np.uint8)
    r, c = {"single_lane": (W // 2 + 9, m.SD_OUT + 5), "straddle": (W // 2 + 9, m.SD_OUT - 1), "first_step": (m.SD_T, W // 2 + 2),
            "last_step": (m.SD_T * _last_fast_step(W) + m.SD_T - 3, W // 2 + 2)}[name]
    return _reflector(_speckle(clip, 4), r, c)


@functools.lru_cache(maxsize=None)
def _truth(clip):
    """per scan (payload, rc, val, figures of the screen's model), computed once, read-only"""
    out = []
    lit = ~dc.dark_steps(clip, ROWS)
    for name in SCANS:
        pay = _payload(name, clip)
        rc, val, _ = dc.want(pay)
        S = dc.integral(dc.cartesian(pay))
        fig = dict(read=[], single_pass=0)
        for size in m.SIZES:
            need, passing, fast = m.waves(S, size, dc.THRESHOLD)
            sel = lit[:, :, None] & fast[None, :, None] & np.ones(8, bool)  # the waves of the fast path
            lanes = need.reshape(need.shape[:3] + (2, m.SD_PC)).any(axis=-2)
            fig["read"].append(float(need.any(axis=-1)[sel].mean()))
            one = sel & (lanes.sum(axis=-1) == 1) & passing.any(axis=-1)     # one lane needs the box, and its product passes
            fig["single_pass"] += int(one.sum())
            fig["single_pass_last_lane"] = fig.get("single_pass_last_lane", 0) + int((one & lanes[..., m.SD_PC - 1]).sum())
        for a in (pay, rc, val):
            a.setflags(write=False)
        out.append((pay, rc, val, fig))
    return out


@functools.lru_cache(maxsize=None)
def _lists(clip):
    from radarslampy_amd import _ffi
    from radarslampy_amd.engine import Engine
    B = len(SCANS)
    ctx = _ffi.Context(0)
    eng = Engine(B, B, ctx=ctx, rows=ROWS, stride=clip, payload_off=0, clip=clip, retrack_on_device=True, retrack_slots=B)
    for t, (pay, _, _, _) in enumerate(_truth(clip)):
        eng.upload_scan(t, pay)
    scan = list(range(B))
    eng.init_lanes_detect(0, scan, np.zeros((B, 3)))
    eng.step(scan)
    out = eng.debug_detect(False, B)
    eng.close()
    ctx.close()
    return out


@pytest.mark.parametrize("clip", [132, 188])
def test_the_scans_are_what_their_names_say(clip):
    W = 2 * (clip // 2)
    T = dict(zip(SCANS, _truth(clip)))
    for name in SCANS:
        r, c, l = dc.unpack(T[name][1])
        print("clip %d %-11s: %d candidates %s, waves that read (15 / 30) %.3f / %.3f, single-lane waves with a passing product %d" %
              ((clip, name, len(r), list(zip(r.tolist(), c.tolist(), l.tolist()))[:3]) + tuple(T[name][3]["read"]) + (T[name][3]["single_pass"],)))
    for name in ("single_lane", "straddle", "first_step", "last_step"):
        assert len(T[name][1]) == 1 and max(T[name][3]["read"]) < 0.25, name       # one maximum, in a scan whose waves mostly skip
    assert T["single_lane"][3]["single_pass_last_lane"] >= 1
    (r,), (c,), _ = dc.unpack(T["straddle"][1])
    assert c == m.SD_OUT - 1
    (r,), _, _ = dc.unpack(T["first_step"][1])
    assert r == m.SD_T
    (r,), _, _ = dc.unpack(T["last_step"][1])
    assert r // m.SD_T == _last_fast_step(W)
    assert len(T["speckle"][1]) == 0 and 0.0 < max(T["speckle"][3]["read"]) < 0.05
    assert len(T["saturated"][1]) > 100 and min(T["saturated"][3]["read"]) > 0.85


@pytest.mark.gpu
@pytest.mark.parametrize("clip", [132, 188])
def test_candidates_equal_the_oracle(clip):
    n, rc, val = _lists(clip)
    for b, (name, (_, want_rc, want_val, _)) in enumerate(zip(SCANS, _truth(clip))):
        k = int(n[b])
        got_rc, got_val = rc[b, :min(k, dc.CAP)], val[b, :min(k, dc.CAP)]
        missing, extra = np.setdiff1d(want_rc, got_rc), np.setdiff1d(got_rc, want_rc)
        print("clip %d %-11s: n %d (oracle %d), missing %d, extra %d" % (clip, name, k, len(want_rc), len(missing), len(extra)))
        assert k == len(want_rc), name
        assert np.array_equal(got_rc, want_rc), name
        assert got_val.tobytes() == want_val.tobytes(), name
