"""GPU (-m gpu): max_clique_kernel when its node budget runs out, held to the model of tests/clique_budget_model.py on the
(case, budget) table of tests/clique_budget_cases.py (tests/test_clique_budget_cpu.py holds the model to the oracle):

    L <  n1        flags bit 0 clear, phase 1's best so far - empty until the first descent reaches a leaf
    n1 <= L < n2   flags bit 0 clear, exactly phase 1's witness
    L >= n2        proven, networkx's clique

through the stage entry in both wavefront forms, the batch of the timing entry and the engine's step.  Everything is compared
exactly; nothing here has a tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import clique_budget_cases as cases
import clique_budget_model as model

pytestmark = pytest.mark.gpu

THR = cases.THR


@pytest.fixture(scope="module")
def ctx():
    from radarslampy_amd import _ffi
    c = _ffi.Context(0)
    assert "gfx950" in c.device_info()["arch"]
    yield c
    c.close()


def _check(c, L, got, tag):
    """one stage answer (mask, n_inliers, flags) against the model's"""
    mask, n_in, flags = got
    want_mask, want_n, want_proven, _, _ = c.run(L)
    assert bool(flags & 1) == want_proven, (tag, c.name, L, flags)
    assert n_in == want_n == int(mask.sum()), (tag, c.name, L, n_in, want_n)
    assert np.array_equal(mask, model.mask_array(want_mask, c.K)), (tag, c.name, L)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_stage_entry_follows_the_budget_table(ctx, name):
    c = cases.case(name)
    for L in c.budgets:
        mask, n_in, flags, adj = ctx.reject_outliers(c.prev, c.new, THR, node_limit=L, want_adj=True)
        assert np.array_equal(adj, c.adj_words), (name, L)
        _check(c, L, (mask, n_in, flags), "stage")


def test_a_call_leaves_nothing_behind(ctx):
    """the same unproven call twice gives the same bits, and the call at the default budget right after it is proven and the oracle's:
    the context's scratch stack, masks and result words carry nothing over"""
    for c in cases.all_cases():
        _, omask, _ = oracle.max_clique_nx(c.adj_words)
        for L in sorted({1, c.first, c.n1 - 1, c.n1, c.n2 - 1} - {0}):
            if L >= c.n2:
                continue
            a = ctx.reject_outliers(c.prev, c.new, THR, node_limit=L)
            b = ctx.reject_outliers(c.prev, c.new, THR, node_limit=L)
            assert not a[2] & 1, (c.name, L)
            assert a[1] == b[1] and a[2] == b[2] and np.array_equal(a[0], b[0]), (c.name, L)
            _check(c, L, b[:3], "again")
            mask, n_in, flags, _ = ctx.reject_outliers(c.prev, c.new, THR)
            assert flags & 1 and n_in == omask.sum() and np.array_equal(mask, omask), (c.name, L)


_CHILD = """
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from radarslampy_amd import _ffi
ctx = _ffi.Context(0)
inp, out = np.load(sys.argv[2]), {}
for name in inp["names"].tolist():
    for L in inp[name + "_budgets"].tolist():
        mask, n_in, flags, adj = ctx.reject_outliers(inp[name + "_prev"], inp[name + "_new"], float(inp["thr"]), node_limit=L, want_adj=True)
        out["%s_%d_mask" % (name, L)], out["%s_%d_res" % (name, L)] = mask, np.array([n_in, flags])
        out["%s_%d_adj" % (name, L)] = adj
np.savez(sys.argv[3], **out)
ctx.close()
print("DONE", len(out) // 3)
"""


def test_one_wavefront_form_follows_the_same_table(tmp_path):
    """ROAM_CLIQUE_TWO_WAVES is read once per process: the table of a third of the cases in a fresh child with the one-wavefront kernel
    (no helper to release, no split degree pass).  The child only runs the device; the comparison with the model is made here."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cs = [cases.case(n) for n in cases.ONE_WAVE_CASES]
    inp = dict(names=np.array([c.name for c in cs]), thr=np.float64(THR))
    for c in cs:
        inp[c.name + "_prev"], inp[c.name + "_new"], inp[c.name + "_budgets"] = c.prev, c.new, np.array(c.budgets)
    np.savez(tmp_path / "in.npz", **inp)
    env = dict(os.environ, ROAM_CLIQUE_TWO_WAVES="0")
    run = subprocess.run([sys.executable, "-c", _CHILD, root, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                         capture_output=True, text=True, timeout=120, env=env)
    n = sum(len(c.budgets) for c in cs)
    assert run.returncode == 0 and "DONE %d" % n in run.stdout, (run.returncode, run.stdout[-500:], run.stderr[-2000:])
    out = np.load(tmp_path / "out.npz")
    for c in cs:
        for L in c.budgets:
            assert np.array_equal(out["%s_%d_adj" % (c.name, L)], c.adj_words), (c.name, L)
            n_in, flags = (int(v) for v in out["%s_%d_res" % (c.name, L)])
            _check(c, L, (out["%s_%d_mask" % (c.name, L)], n_in, flags), "one wavefront")


def test_batch_of_70_copies_reports_the_model(ctx):
    """70 problems beside each other (more than one launch wave of a CU's resident workgroups), one (case, budget) of every row of
    the table (the cut one with a mask that is not empty): the timing entry reports the last copy's count and flag"""
    c = cases.case("tie257")
    assert c.first <= c.n1 - 1 and c.n1 < (c.n1 + c.n2) // 2 < c.n2
    for L, row in ((c.n1 - 1, "cut"), ((c.n1 + c.n2) // 2, "witness"), (c.n2, "proven")):
        assert cases.regime(c.n1, c.n2, L) == row
        _, _, n_in, proven = ctx.time_reject_outliers(c.prev, c.new, THR, copies=70, reps=1, node_limit=L)
        assert (n_in, proven) == c.run(L)[1:3], (L, row, n_in, proven)


# ------------------------------------------------------------------ the engine
def _engine(ctx, limit):
    from radarslampy_amd.engine import Engine
    clip, rows, stride, off = cases.ENGINE_LAYOUT
    recs, poses, starts = cases.engine_inputs()
    eng = Engine(3, len(recs), ctx=ctx, rows=rows, stride=stride, payload_off=off, clip=clip, retrack_on_device=False,
                 clique_node_limit=limit)
    for t, rec in enumerate(recs):
        eng.upload_scan(t, rec)
    for b, (t0, f) in enumerate(starts):
        eng.init_lane(b, t0, f, poses[t0])
    return eng


def _lane_records(raw):
    import ctypes
    from radarslampy_amd import _ffi
    n = ctypes.sizeof(_ffi.LaneResult)
    return [raw[i * n:(i + 1) * n] for i in range(3)]


def test_engine_step_takes_the_unproven_mask(ctx):
    """two engines on the same three lanes, one at the default budget and one at ENGINE_LIMIT.  Per step and lane the expectation is
    recomputed with stage calls on what the lane held: its features and level-0 image before the step, its image after it"""
    L = cases.ENGINE_LIMIT
    poses0 = [cases.engine_inputs()[1][t0] for t0, _ in cases.engine_inputs()[2]]
    twin = _engine(ctx, 0)
    twin_raw = []
    for t in range(1, cases.ENGINE_FRAMES):
        twin.step(cases.engine_scans(t))
        res = twin.results()
        assert all(r["clique_proven"] for r in res), t
        twin_raw.append(_lane_records(twin.results_array().tobytes()))
    twin.close()

    eng = _engine(ctx, L)
    pose = [np.asarray(p, np.float64) for p in poses0]
    always_proven = [True] * 3
    seen = []
    for t in range(1, cases.ENGINE_FRAMES):
        before = [(eng.lane_features(b), eng.lane_image(b, 0)) for b in range(3)]
        eng.step(cases.engine_scans(t))
        res = eng.results()
        raw = _lane_records(eng.results_array().tobytes())
        for b in range(3):
            feats, prev = before[b]
            nxt_img = eng.lane_image(b, 0)
            got = res[b]
            tag = (t, b)
            if len(feats):
                nxt, s, e = ctx.klt_track(prev, nxt_img, feats)
                good = ((s != 0) & (e < oracle.ERR_THRESHOLD)).reshape(-1)
            else:
                nxt, good = np.zeros((0, 2), np.float32), np.zeros(0, bool)
            if good.any():
                mask, n_in, flags, _ = ctx.reject_outliers(feats[good], nxt[good], THR, node_limit=L)
                mmask, mn, mproven, row = cases.reject(feats[good], nxt[good], L)
                assert np.array_equal(mask, mmask) and n_in == mn and bool(flags & 1) == mproven, tag       # the stage call is the model's
            else:
                mask, n_in, flags, row = np.zeros(0, bool), 0, 1, "proven"
            seen.append((t, b, int(good.sum()), n_in, bool(flags & 1), row))
            assert got["n_tracked"] == len(feats) and got["n_good"] == int(good.sum()), tag
            assert got["n_inliers"] == n_in and got["clique_proven"] == bool(flags & 1), tag
            assert np.array_equal(eng.lane_features(b), nxt[good][mask]), tag
            assert np.isfinite(got["pose"]).all() and np.isfinite(got["velocity"]).all(), tag
            if n_in == 0:                                               # nothing to fit: the pose stays, the lane asks for features
                assert np.array_equal(got["pose"], pose[b]) and got["retrack"] and len(eng.lane_features(b)) == 0, tag
            always_proven[b] = always_proven[b] and row == "proven"
            if always_proven[b]:
                assert raw[b] == twin_raw[t - 1][b], tag                 # never short of nodes so far: the twin's lane, byte for byte
            pose[b] = got["pose"]
    eng.close()
    print("engine lane-steps (step, lane, n_good, n_inliers, proven, row) at L =", L, seen)
    rows = {s[5] for s in seen}
    assert {"cut", "witness", "proven"} <= rows, rows
    assert any(s[5] == "cut" and s[3] == 0 for s in seen)               # an empty mask reached the step
    assert any(always_proven), always_proven
    assert seen == cases.engine_lane_steps(L)                           # what the choice of L was made from, on the CPU
