"""GPU (-m gpu): roam_pose_graph_optimize against its NumPy model (tests/pose_graph_model.py) on the cases of
tests/pose_graph_cases.py, at the bounds measure_spread() measures between two float64 orders of the model; batch independence and
repeatability bit for bit; the converged runs against SciPy's optimum; PoseGraphLib end to end; the keyframes of an engine."""
import ctypes

import numpy as np
import pytest

import pose_graph_cases as PC
from test_pose_graph_cpu import SCIPY_CASES, converged  # noqa: F401  (the fixture: model at 50 iterations twice, SciPy's optimum)

pytestmark = pytest.mark.gpu
COUNTS = ("iterations", "trials", "rejected", "stop")


@pytest.fixture(scope="module")
def ctx():
    from radarslampy_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def big_batch(ctx):
    graphs, names = PC.batch(300)
    poses, stats = ctx.pose_graph_optimize(graphs, max_iterations=8)
    return graphs, names, poses, stats


def _same(pa, sa, pb, sb):
    return np.array_equal(pa, pb) and sa.tobytes() == sb.tobytes()


@pytest.mark.parametrize("name", list(PC.cases()))
def test_case_against_the_model(ctx, name):
    c = PC.cases()[name]
    it, tr, lam = c["opts"]
    _, bound = PC.measure_spread()
    start = [a.copy() if a is not None else None for a in c["graph"]]
    poses, stats = ctx.pose_graph_optimize([c["graph"]], it, tr, lam)
    xm, sm, _ = PC.reference(name)
    d = PC.difference(xm, sm, poses[0], stats[0])
    print(f"{name}: position {d[0]:.3g} (<= {bound[0]:.3g})  angle {d[1]:.3g} (<= {bound[1]:.3g})  chi2 {d[2]:.3g} (<= {bound[2]:.3g})  "
          f"lambda {d[3]:.3g} (<= {bound[3]:.3g})  counts {[int(stats[0][k]) for k in COUNTS]} model {[int(sm[k]) for k in COUNTS]}")
    assert [int(stats[0][k]) for k in COUNTS] == [int(sm[k]) for k in COUNTS]
    if c.get("exact"):              # failed factorisations in exact arithmetic: the model's bits
        assert stats[0]["rejected"] == 10 and stats[0]["stop"] == 1
        assert stats[0].tobytes() == sm.tobytes() and np.array_equal(poses[0], xm) and np.array_equal(poses[0], c["poses"])
        return
    assert abs(stats[0]["chi2_initial"] - sm["chi2_initial"]) <= bound[2] * abs(sm["chi2_initial"])
    assert d[0] <= bound[0] and d[1] <= bound[1] and d[2] <= bound[2] and d[3] <= bound[3]
    assert np.array_equal(poses[0][c["fixed"]], c["poses"][c["fixed"]])                # fixed vertices are constants
    assert all(a is None and b is None or np.array_equal(a, b) for a, b in zip(start, c["graph"]))      # the inputs are not modified
    if it == 0:
        assert np.array_equal(poses[0], c["poses"]) and stats[0]["chi2_final"] == stats[0]["chi2_initial"]


def test_one_edge_is_compose(ctx):
    """x_1 = x_0 (+) z within one ulp of the largest coordinate and chi2 = 0 to rounding: an error of that ulp in every component
    under the largest information entry (R^T (t_j - t_i) - z rounds, so an exact 0 is not reachable in general).  Measured on the
    MI355X: 0.5 of that ulp (4.4e-16 m), chi2 4.3e-29 against a bound of 2e-24"""
    c = PC.cases()["n2"]
    poses, stats = ctx.pose_graph_optimize([c["graph"]], max_iterations=20)
    ulp = np.finfo(float).eps * np.abs(c["truth"]).max()
    print("n2 at 20 iterations:", stats[0], "distance to x_0 (+) z", np.abs(poses[0] - c["truth"]).max(), "ulp", ulp)
    assert np.abs(poses[0] - c["truth"]).max() <= ulp
    assert 0.0 <= stats[0]["chi2_final"] <= 9 * np.abs(c["info"]).max() * ulp ** 2
    assert stats[0]["chi2_initial"] > 1e3


def test_graph_alone_and_anywhere_in_a_batch(ctx, big_batch):
    graphs, names, poses, stats = big_batch
    assert "ring1024" in names and len(set(names)) >= 10
    for i in (0, 100, 150, 299):
        alone_p, alone_s = ctx.pose_graph_optimize([graphs[i]], max_iterations=8)
        assert _same(alone_p[0], alone_s[0], poses[i], stats[i]), (i, names[i])
    # one graph first, in the middle and last among others
    g = PC.cases()["ring130"]["graph"]
    want_p, want_s = ctx.pose_graph_optimize([g], max_iterations=8)
    others = graphs[:40]
    for at in (0, 20, 40):
        p, s = ctx.pose_graph_optimize(others[:at] + [g] + others[at:], max_iterations=8)
        assert _same(p[at], s[at], want_p[0], want_s[0]), at
    p3, s3 = ctx.pose_graph_optimize(graphs[5:8], max_iterations=8)
    assert all(_same(p3[k], s3[k], poses[5 + k], stats[5 + k]) for k in range(3))


def test_graph_in_any_chunk(ctx, big_batch, monkeypatch):
    """the same batch cut into many launches (ROAM_POSE_GRAPH_CHUNK_BYTES: 200 kB of scratch per chunk, the 1024-vertex ring in a
    chunk of its own): every graph's bits are those of the one-launch call"""
    from radarslampy_amd import _ffi
    graphs, names, poses, stats = big_batch
    lo, hi = 90, 150
    assert "ring1024" in names[lo:hi]
    monkeypatch.setenv("ROAM_POSE_GRAPH_CHUNK_BYTES", "200000")
    _, cut = _ffi.pose_graph_plan(graphs[lo:hi])
    p, s = ctx.pose_graph_optimize(graphs[lo:hi], max_iterations=8)
    monkeypatch.delenv("ROAM_POSE_GRAPH_CHUNK_BYTES")
    _, whole = _ffi.pose_graph_plan(graphs[lo:hi])
    assert whole > 2 * cut                                      # the call was cut
    assert s.tobytes() == stats[lo:hi].tobytes() and all(np.array_equal(a, b) for a, b in zip(p, poses[lo:hi]))


def test_noise_free_ring_of_1024_recovers_the_truth(ctx):
    """the largest size against a known answer (SciPy's dense LM is not run there)"""
    from test_pose_graph_cpu import noise_free_1024
    r, start = noise_free_1024()
    poses, stats = ctx.pose_graph_optimize([(start, r["fixed"], r["ij"], r["meas"], r["info"], None)], max_iterations=4, lambda_init=1e-6)
    d = np.abs(np.column_stack([poses[0][:, :2] - r["truth"][:, :2], PC.model.normalize(poses[0][:, 2] - r["truth"][:, 2])])).max()
    print("noise-free N = 1024:", stats[0], "distance to the truth", d)
    assert d < 1e-9 and stats[0]["chi2_final"] < 1e-12


def test_same_call_twice(ctx, big_batch):
    graphs, names, poses, stats = big_batch
    p, s = ctx.pose_graph_optimize(graphs, max_iterations=8)
    assert s.tobytes() == stats.tobytes() and all(np.array_equal(a, b) for a, b in zip(p, poses))


def test_converged_runs_against_scipy(ctx, converged):
    """50 iterations on the device against SciPy's optimum, at the CPU test's bounds"""
    names = SCIPY_CASES
    poses, stats = ctx.pose_graph_optimize([PC.cases()[k]["graph"] for k in names], max_iterations=50)
    own = [PC.difference(a[0], a[1], b[0], b[1]) for a, b, _, _ in converged.values()]
    bound = (10 * max(o[0] for o in own), 10 * max(o[1] for o in own))
    for k, p, s in zip(names, poses, stats):
        _, _, xs, chi2 = converged[k]
        d = PC.difference(p, s, xs, dict(chi2_final=chi2, lambda_final=s["lambda_final"]))
        print(f"{k}: chi2 device {float(s['chi2_final'])!r} scipy {chi2!r} rel {d[2]:.3g}; poses {d[0]:.3g} {d[1]:.3g} (<= {bound[0]:.3g} {bound[1]:.3g})")
        if chi2 > 1e-12:
            assert d[2] <= 1e-9, k
        else:
            assert s["chi2_final"] <= 1e-12, k
        assert d[0] <= bound[0] and d[1] <= bound[1], k


def _lib_graph(c, ctx=None):
    from radarslampy_amd.PoseGraphLib import PoseGraphOptimization
    g = PoseGraphOptimization(ctx)
    for v, (p, f) in enumerate(zip(c["poses"], c["fixed"])):
        g.add_vertex(("v", v), p, fixed=bool(f))
    for t, (i, j) in enumerate(c["ij"]):
        g.add_edge((("v", int(i)), ("v", int(j))), c["meas"][t], c["info"][t], None if c["huber"] is None or c["huber"][t] == 0 else c["huber"][t])
    return g


def test_pose_graph_lib_end_to_end(ctx):
    c = PC.cases()["ring65"]
    g = _lib_graph(c, ctx)
    g.optimize(20)
    got = np.array([g.get_pose(("v", v)) for v in range(65)])
    want, stats = ctx.pose_graph_optimize([c["graph"]], max_iterations=20)
    assert np.array_equal(got, want[0]) and g.stats.tobytes() == stats[0].tobytes()
    e0 = np.linalg.norm(c["poses"][:, :2] - c["truth"][:, :2], axis=1).max()
    e1 = np.linalg.norm(got[:, :2] - c["truth"][:, :2], axis=1).max()
    print(f"ring65 through PoseGraphOptimization: worst position error {e0:.2f} -> {e1:.2f} m, chi2 {g.stats['chi2_initial']:.4g} -> {g.stats['chi2_final']:.4g}")
    assert e1 <= e0 / 4 and g.stats["chi2_final"] < g.stats["chi2_initial"]
    # without a context of its own the graph runs on the process-wide one
    h = _lib_graph(PC.cases()["triangle"])
    h.optimize(3)
    want, stats = ctx.pose_graph_optimize([PC.cases()["triangle"]["graph"]], max_iterations=3)
    assert np.array_equal(np.array([h.get_pose(("v", v)) for v in range(3)]), want[0]) and h.stats.tobytes() == stats[0].tobytes()


def test_optimize_graphs_is_separate_calls(ctx):
    from radarslampy_amd.PoseGraphLib import optimizeGraphs
    names = ["ring40", "huber", "triangle", "fixed_two"]
    together = [_lib_graph(PC.cases()[k], ctx) for k in names]
    optimizeGraphs(together, 8)
    for k, g in zip(names, together):
        one = _lib_graph(PC.cases()[k], ctx)
        one.optimize(8)
        n = len(PC.cases()[k]["poses"])
        assert all(np.array_equal(one.get_pose(("v", v)), g.get_pose(("v", v))) for v in range(n)), k
        assert one.stats.tobytes() == g.stats.tobytes(), k


def test_engine_keyframes_come_back_unchanged(ctx):
    """the keyframes of the three-lane engine of tests/test_gpu_engine_flow.py (a keyframe per step) as a pose graph without loop
    edges: the odometry edges are measured from the poses, so the poses are the optimum - chi2 = 0 to rounding, nothing moves"""
    import test_gpu_engine_flow as flow
    from radarslampy_amd.engine import Engine
    from radarslampy_amd.Mapping import DeviceMap
    from radarslampy_amd.PoseGraphLib import graphFromKeyframes, optimizeGraphs
    clip, rows, stride, off = flow.LAYOUT
    recs, poses, f_first, f_last = flow._inputs()
    T = len(recs)
    eng = Engine(3, T, ctx=ctx, rows=rows, stride=stride, payload_off=off, clip=clip, retrack_on_device=True, keyframe_trans_m=1e-9)
    try:
        eng.map_reserve(8)
        for t in range(T):
            eng.upload_scan(t, recs[t])
        for b, (t0, f) in enumerate([(0, f_first), (0, f_first[:40]), (T - 1, f_last)]):
            eng.init_lane(b, t0, f, poses[t0])
        for t in range(1, flow.FRAMES):
            eng.step([t, t, flow.FRAMES - 1 - t])
        kfs = [DeviceMap(eng, b).keyframes for b in range(3)]
    finally:
        eng.close()
    assert all(len(k) >= 2 for k in kfs), [len(k) for k in kfs]
    graphs = [graphFromKeyframes(k, odomInformation=PC.OMEGA, ctx=ctx) for k in kfs]
    optimizeGraphs(graphs, 20)
    for b, (g, k) in enumerate(zip(graphs, kfs)):
        want = np.array([kf.pose for kf in k])
        print(f"lane {b} keyframe poses:", want.tolist())
        assert np.ptp(want[:, :2], axis=0).max() > 0.01            # the lane moved: the odometry edges are not all zero
        got = np.array([g.get_pose(v) for v in range(len(k))])
        scale = np.finfo(float).eps * max(1.0, np.abs(want).max())
        print(f"lane {b}: {len(k)} keyframes, chi2 {g.stats['chi2_initial']!r} -> {g.stats['chi2_final']!r}, moved {np.abs(got - want).max():.3g}")
        # an error of 4 ulp of the largest coordinate per component of each edge under the largest information entry, and a step of
        # that size at most
        assert g.stats["chi2_initial"] <= 9 * len(k) * np.abs(PC.OMEGA).max() * (4 * scale) ** 2
        assert g.stats["chi2_final"] <= g.stats["chi2_initial"]
        assert np.abs(got - want).max() <= 16 * scale


def test_library_refuses_with_graph_and_edge_in_the_text(ctx):
    """the ABI's own checks, behind the Python ones: ROAM_E_ARG, the text names graph and edge"""
    from radarslampy_amd import _ffi
    a, b = PC.cases()["triangle"], PC.cases()["ring40"]
    voff, poses, fixed, eoff, ij, meas, info, hub, opts = _ffi.pose_graph_args([a["graph"], b["graph"]])
    stats = np.zeros(2, _ffi.POSE_GRAPH_STATS)

    def call(**kw):
        arg = dict(poses=poses.copy(), fixed=fixed, ij=ij, meas=meas, info=info, opts=opts)
        arg.update(kw)
        rc = ctx.lib.roam_pose_graph_optimize(ctx.h, 2, _ffi._ptr(voff), _ffi._ptr(arg["poses"]), _ffi._ptr(arg["fixed"]), _ffi._ptr(eoff),
                                              _ffi._ptr(arg["ij"]), _ffi._ptr(arg["meas"]), _ffi._ptr(arg["info"]), None,
                                              ctypes.byref(arg["opts"]), _ffi._ptr(stats))
        return rc, ctx.lib.roam_last_error(ctx.h).decode()

    e = ij.copy()
    e[3 + 5] = (4, 4)
    rc, text = call(ij=e)
    assert rc == _ffi.ROAM_E_ARG and "graph 1" in text and "edge 5" in text, text
    m = meas.copy()
    m[1, 2] = np.nan
    rc, text = call(meas=m)
    assert rc == _ffi.ROAM_E_ARG and "graph 0" in text and "edge 1" in text, text
    f = fixed.copy()
    f[3:] = 0
    rc, text = call(fixed=f)
    assert rc == _ffi.ROAM_E_ARG and "graph 1" in text and "fixed" in text, text
    rc, text = call(opts=_ffi.PoseGraphOpts(1001, 10, 0.0))
    assert rc == _ffi.ROAM_E_ARG and "max_iterations" in text, text
    rc, text = call()
    assert rc == _ffi.ROAM_OK
    # a graph beyond a launch's scratch: its index and its envelope are in the text (32768 vertices that all see vertex 1)
    V = 32768
    big = (np.zeros((V, 3)), np.arange(V) == 0, np.stack([np.ones(V - 2, np.int32), np.arange(2, V, dtype=np.int32)], axis=1),
           np.zeros((V - 2, 3)), np.eye(3), None)
    with pytest.raises(_ffi.RoamError, match=f"graph 1: an envelope of {(V - 1) * V // 2} blocks") as err:
        ctx.pose_graph_optimize([a["graph"], big])
    assert err.value.code == _ffi.ROAM_E_ARG
