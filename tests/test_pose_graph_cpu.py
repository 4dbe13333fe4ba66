"""CPU (-m "not gpu"): the pose-graph optimiser without a device - the ABI table, the argument checks ahead of the library, the host
half (roam_pose_graph_plan) against the envelope computed in Python, the conditions on the cases, the NumPy model
(tests/pose_graph_model.py) against live SciPy and against known answers, measure_spread() (the device's bar), and PoseGraphLib over a
stubbed pose_graph_optimize."""
import ctypes
import os
import re

import numpy as np
import pytest

import pose_graph_cases as PC
import pose_graph_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = ("iterations", "trials", "rejected", "stop")


def test_header_table_and_exports_agree():
    from radarslampy_amd import _ffi
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "roam_abi.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name, nargs in (("roam_pose_graph_plan", 7), ("roam_pose_graph_optimize", 12)):
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*)\)\s*;", txt)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_ffi._SIGS[name][1])
        assert hasattr(lib, name)
    assert ctypes.sizeof(_ffi.PoseGraphOpts) == 16 and _ffi.POSE_GRAPH_STATS.itemsize == 40
    assert _ffi.POSE_GRAPH_STATS == M.STATS
    for field in ("max_iterations", "max_trials", "lambda_init") + COUNTS + ("chi2_initial", "chi2_final", "lambda_final"):
        assert re.search(r"\b" + field + r"\b", txt), field


def test_argument_errors_come_before_the_library():
    from radarslampy_amd import _ffi
    ctx = object.__new__(_ffi.Context)              # no library, no handle: any call into it would raise AttributeError
    g = PC.cases()["ring40"]
    poses, fixed, ij, meas, info, _ = g["graph"]

    def bad(graphs, **kw):
        with pytest.raises(ValueError):
            ctx.pose_graph_optimize(graphs, **kw)

    bad([])
    bad([g["graph"][:5]])
    bad([(poses[:, :2], fixed, ij, meas, info, None)])
    bad([(poses, fixed[:-1], ij, meas, info, None)])
    bad([(poses[:0], fixed[:0], ij[:0], meas[:0], info[:0], None)])
    bad([(np.zeros((32769, 3)), np.arange(32769) == 0, ij, meas, info, None)])
    bad([(poses, fixed, ij[:, :1], meas, info, None)])
    bad([(poses, fixed, ij.astype(float), meas, info, None)])
    bad([(poses, fixed, ij, meas[:-1], info, None)])
    bad([(poses, fixed, ij, meas, info[:-1], None)])
    bad([(poses, fixed, ij, meas, info, np.ones(3))])
    for k, v in ((0, 40), (1, -1)):
        e = ij.copy()
        e[5, k] = v
        bad([(poses, fixed, e, meas, info, None)])
    e = ij.copy()
    e[5] = (7, 7)
    bad([(poses, fixed, e, meas, info, None)])
    for arr, idx in ((poses, (3, 1)), (meas, (4, 2)), (info, (2, 1, 1))):
        for v in (np.nan, np.inf):
            a = arr.copy()
            a[idx] = v
            bad([tuple(a if x is arr else x for x in (poses, fixed, ij, meas, info, None))])
    asym = info.copy()
    asym[3, 0, 1] = np.nextafter(asym[3, 0, 1], 1e9)
    bad([(poses, fixed, ij, meas, asym, None)])
    h = np.zeros(len(ij))
    for v in (-1.0, np.nan, np.inf):
        h[2] = v
        bad([(poses, fixed, ij, meas, info, h)])
    bad([(poses, np.zeros(40, bool), ij, meas, info, None)])
    bad([g["graph"]], max_iterations=-1)
    bad([g["graph"]], max_iterations=1001)
    bad([g["graph"]], max_trials=-1)
    bad([g["graph"]], max_trials=1001)
    bad([g["graph"]], lambda_init=-1.0)
    bad([g["graph"]], lambda_init=np.nan)
    with pytest.raises(AttributeError):             # what is left is a call into the library this context does not have
        ctx.pose_graph_optimize([g["graph"]])
    # a graph without edges may give them as empty lists
    packed = _ffi.pose_graph_args([(poses, fixed, [], [], [], None), (poses[:1], [1], np.zeros((0, 2)), np.zeros((0, 3)), np.eye(3), [])])
    assert packed[3].tolist() == [0, 0, 0] and packed[4].shape == (0, 2) and packed[4].dtype == np.int32
    # a (3, 3) information matrix stands for every edge
    packed = _ffi.pose_graph_args([(poses, fixed, ij, meas, PC.OMEGA, None)])
    assert packed[6].shape == (len(ij), 6) and packed[7] is None
    assert np.array_equal(packed[6][0], PC.OMEGA[[0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]])


def test_plan_is_the_envelope_computed_in_python():
    from radarslampy_amd import _ffi
    names = list(PC.cases())
    env, nbytes = _ffi.pose_graph_plan([PC.cases()[k]["graph"] for k in names])
    for k, got in zip(names, env):
        c = PC.cases()[k]
        first, want = M.envelope(c["fixed"], c["ij"])
        print(k, "envelope", want, "free", len(first))
        assert got == want, k
    # what the cost rule says: the diagonal, the chain below it, and the span of every loop between free vertices (vertex 0 is fixed:
    # the loop (0, 1023) costs nothing)
    assert env[names.index("ring1024")] == 1023 + 1022 + (899 - 99 - 1) + (699 - 299 - 1) + (499 - 49 - 1)
    # compaction: vertex 17 fixed cuts the chain once and renumbers the loop (0, 39) to (0, 38)
    assert env[names.index("fixed_middle")] == 39 + 37 + (38 - 0 - 1)
    # backwards and duplicate edges change nothing: (21, 20) is the chain's edge, (39, 0) ends at the fixed vertex, (12, 30) twice
    # widens row 29 once
    assert env[names.index("backward_duplicate")] == 39 + 38 + (29 - 11 - 1)
    # 144 bytes of matrix and 4 of column list per block, the rest grows with vertices and edges
    rest = 400 * sum(len(PC.cases()[k]["poses"]) + len(PC.cases()[k]["ij"]) + 1 for k in names)
    assert env.sum() * 144 < nbytes < env.sum() * 148 + rest
    alone, _ = _ffi.pose_graph_plan([PC.cases()["ring130"]["graph"]])
    assert alone[0] == env[names.index("ring130")]


def test_plan_cuts_the_batch_where_the_chunk_limit_says(monkeypatch):
    """ROAM_POSE_GRAPH_CHUNK_BYTES lowers where a batch is cut (the GPU test runs such a call): the scratch of the call is then its
    largest chunk, a graph above the figure gets a chunk of its own, and the envelopes do not change"""
    from radarslampy_amd import _ffi
    graphs, names = PC.batch(300)
    env, whole = _ffi.pose_graph_plan(graphs)
    single = [_ffi.pose_graph_plan([g])[1] for g in graphs[:12]]
    monkeypatch.setenv("ROAM_POSE_GRAPH_CHUNK_BYTES", "200000")
    env2, cut = _ffi.pose_graph_plan(graphs)
    assert np.array_equal(env, env2) and whole > 10 * cut
    assert cut == _ffi.pose_graph_plan([graphs[names.index("ring1024")]])[1] > 200000       # the largest graph, alone
    few, most = _ffi.pose_graph_plan(graphs[:12])
    assert max(single) <= most <= 200000 < sum(single)
    monkeypatch.setenv("ROAM_POSE_GRAPH_CHUNK_BYTES", str(1 << 40))                         # never raises the limit
    assert _ffi.pose_graph_plan(graphs)[1] == whole


def test_plan_refuses_a_graph_beyond_two_gigabytes():
    """32768 vertices that all see vertex 1: 5.4e8 blocks, 77 GB - refused by the host half, nothing is allocated for it"""
    from radarslampy_amd import _ffi
    V = 32768
    ij = np.stack([np.ones(V - 2, np.int32), np.arange(2, V, dtype=np.int32)], axis=1)
    graph = (np.zeros((V, 3)), np.arange(V) == 0, ij, np.zeros((len(ij), 3)), np.eye(3), None)
    blocks = (V - 1) + sum(range(1, V - 1))          # free rows 1 .. V - 2 all start at free column 0 (vertex 1)
    with pytest.raises(ValueError, match=f"graph 1: an envelope of {blocks} blocks"):
        _ffi.pose_graph_plan([PC.cases()["n2"]["graph"], graph])
    lib = _ffi.load_library()
    packed = _ffi.pose_graph_args([graph])
    rc = lib.roam_pose_graph_plan(1, _ffi._ptr(packed[0]), _ffi._ptr(packed[2]), _ffi._ptr(packed[3]), _ffi._ptr(packed[4]), None, None)
    assert rc == _ffi.ROAM_E_ARG
    # the same vertices as a chain are cheap
    chain = np.stack([np.arange(V - 1, dtype=np.int32), np.arange(1, V, dtype=np.int32)], axis=1)
    env, nbytes = _ffi.pose_graph_plan([(np.zeros((V, 3)), np.arange(V) == 0, chain, np.zeros((V - 1, 3)), np.eye(3), None)])
    assert env[0] == 2 * (V - 1) - 1 and nbytes < 32 << 20
    # what the ABI refuses structurally, straight at the library: no fixed vertex, an index out of range, i == j, no graph
    voff, eoff = np.array([0, 3], np.int32), np.array([0, 1], np.int32)
    for fixed, e in (([0, 0, 0], (0, 1)), ([1, 0, 0], (0, 3)), ([1, 0, 0], (2, 2))):
        rc = lib.roam_pose_graph_plan(1, _ffi._ptr(voff), _ffi._ptr(np.array(fixed, np.uint8)), _ffi._ptr(eoff),
                                      _ffi._ptr(np.array([e], np.int32)), None, None)
        assert rc == _ffi.ROAM_E_ARG, (fixed, e)
    assert lib.roam_pose_graph_plan(0, _ffi._ptr(voff), _ffi._ptr(np.ones(3, np.uint8)), _ffi._ptr(eoff), None, None, None) == _ffi.ROAM_E_ARG


def test_conditions_on_the_cases():
    """no accept / reject decision of a device-against-model comparison hangs on rounding"""
    for name, c in PC.cases().items():
        x, st, log = PC.reference(name)
        assert c["opts"][0] <= 8
        rho = np.array([t[2] for t in log])
        print(name, "iterations", int(st["iterations"]), "trials", int(st["trials"]), "rejected", int(st["rejected"]),
              "min |rho|", np.abs(rho).min() if len(rho) else None)
        assert (np.abs(rho) >= 1e-3).all(), name
        if c.get("exact"):          # every trial of the first iteration is a failed factorisation
            assert st["stop"] == 1 and st["iterations"] == 1 and st["trials"] == st["rejected"] == 10, name
            assert all(t[5] == np.inf for t in log) and np.array_equal(x, c["poses"]) and st["chi2_final"] == st["chi2_initial"] == 6.0
            assert st["lambda_final"] == 1e-30 * 2.0 ** 55
        else:
            assert st["stop"] == 0 and st["iterations"] == c["opts"][0], name
    assert PC.reference("reject")[1]["rejected"] >= 3
    c = PC.cases()["huber"]
    e, _, _ = M.edge_terms(c["poses"], c["ij"], c["meas"], M._Trig(), False)
    s2 = np.einsum("ea,eab,eb->e", e, c["info"], e)[c["huber"] > 0]
    assert (s2 <= 1.0).any() and (s2 > 1.0).any()
    # the wrap case: headings on both sides of +-pi, and the measured half turn
    c = PC.cases()["wrap"]
    assert (np.abs(np.diff(c["truth"][:, 2])) > 3.0).sum() >= 2 and abs(c["meas"][-1, 2] - np.pi) < 1e-9
    assert PC.reference("evaluate")[1]["trials"] == 0 and np.array_equal(PC.reference("evaluate")[0], c_poses("evaluate"))


def c_poses(name):
    return PC.cases()[name]["poses"]


def test_measured_spread_is_the_bar():
    per, bound = PC.measure_spread()
    for name, v in per.items():
        print(f"{name:20s} position {v[0]:.3g} m  angle {v[1]:.3g} rad  chi2 {v[2]:.3g} rel  lambda {v[3]:.3g} rel")
    print("bound (10 x the largest):", bound)
    # two float64 orders of one algorithm: far below anything a user sees, and not zero (the second order is another order)
    assert 0 < bound[0] < 1e-8 and 0 < bound[1] < 1e-9 and bound[2] < 1e-5 and bound[3] < 1e-5


def _whitened(c):
    """the whitened residual L^T e (Omega = L L^T) of a case over its free poses, and its analytic Jacobian (EdgeSE2's A and B)"""
    free = np.flatnonzero(~c["fixed"])
    cidx = np.full(len(c["fixed"]), -1)
    cidx[free] = np.arange(len(free))
    Ls = np.linalg.cholesky(c["info"])
    ij = c["ij"].astype(np.int64)

    def place(v):
        x = c["poses"].copy()
        x[free] = v.reshape(-1, 3)
        return x

    def res(v):
        e, _, _ = M.edge_terms(place(v), ij, c["meas"], M._Trig(), False)
        return np.einsum("eba,eb->ea", Ls, e).ravel()

    def jac(v):
        _, A, B = M.edge_terms(place(v), ij, c["meas"], M._Trig(), True)
        J = np.zeros((3 * len(ij), 3 * len(free)))
        for t in range(len(ij)):
            for k, D in ((cidx[ij[t, 0]], A[t]), (cidx[ij[t, 1]], B[t])):
                if k >= 0:
                    J[3 * t:3 * t + 3, 3 * k:3 * k + 3] += Ls[t].T @ D
        return J

    return free, place, res, jac


def test_analytic_jacobians_against_differences():
    """A and B of the model (and of the kernel, which states the same expressions) against central differences of the error"""
    for name in ("triangle", "wrap", "backward_duplicate"):
        c = PC.cases()[name]
        free, _, res, jac = _whitened(c)
        v = c["poses"][free].ravel()
        J, h = jac(v), 1e-6
        num = np.stack([(res(v + h * d) - res(v - h * d)) / (2 * h) for d in np.eye(len(v))], axis=1)
        assert np.abs(J - num).max() <= 1e-6 * max(1.0, np.abs(J).max()), name


def _scipy_optimum(c):
    """MINPACK's Levenberg-Marquardt from the case's start, with the analytic Jacobian: with its forward differences the stationary
    point of a loop that does not close is off by 1e-8 to 1e-6, more than the model's own rounding"""
    from scipy.optimize import least_squares
    free, place, res, jac = _whitened(c)
    r = least_squares(res, c["poses"][free].ravel(), jac=jac, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=200000)
    x = place(r.x)
    x[:, 2] = M.normalize(x[:, 2])
    return x, float(2 * r.cost)


SCIPY_CASES = [k for k, c in PC.cases().items() if c["huber"] is None and len(c["poses"]) <= 130 and k not in ("evaluate", "reject", "unanchored")]


@pytest.fixture(scope="module")
def converged():
    """name -> (model at 50 iterations, the same in the second order, SciPy's optimum, its chi2)"""
    out = {}
    for k in SCIPY_CASES:
        c = PC.cases()[k]
        args = (c["poses"], c["fixed"], c["ij"], c["meas"], c["info"], None, 50, 10, c["opts"][2])
        out[k] = (M.optimize(*args), M.optimize(*args, chol=True, trig_ulp=4, seed=11)) + _scipy_optimum(c)
    return out


@pytest.mark.parametrize("name", SCIPY_CASES)
def test_model_against_live_scipy(converged, name):
    """least_squares(method="lm") on the whitened residuals, tolerances 1e-15, against the model at 50 iterations: chi2 within 1e-9
    relative, poses within ten times what the model's own two orders differ by at that count - the largest over the cases, as
    measure_spread() takes it: the last steps are rounding-driven, and in a single case the two orders may by luck stop at the same
    point (ring40: 2e-15) while both sit 1e-11 from the optimum.
    ring1024 is left out: MINPACK's dense QR of 3072 columns takes minutes (its optimum is checked by the noise-free known answer
    below instead); the rejection case ends in another minimum by design; the unanchored case has no unique optimum."""
    (xa, sa, _), (xb, sb, _), xs, chi2 = converged[name]
    own = [PC.difference(a[0], a[1], b[0], b[1]) for a, b, _, _ in converged.values()]
    bound = (10 * max(o[0] for o in own), 10 * max(o[1] for o in own))
    d = PC.difference(xa, sa, xs, dict(chi2_final=chi2, lambda_final=sa["lambda_final"]))
    print(name, "chi2 model", float(sa["chi2_final"]), "scipy", chi2, "rel", d[2], "| poses", d[0], d[1], "| bound", bound)
    if chi2 > 1e-12:
        assert d[2] <= 1e-9
    else:
        assert sa["chi2_final"] <= 1e-12
    assert d[0] <= bound[0] and d[1] <= bound[1]


def noise_free_1024():
    """the 1024-vertex ring with exact measurements and a start 0.05 m / 0.005 rad off: the optimum is the truth"""
    r = PC.ring(1024, 3, PC.LOOPS[1024], noise=False)
    start = r["truth"] + np.random.default_rng(4).standard_normal((1024, 3)) * [0.05, 0.05, 0.005]
    start[0] = r["truth"][0]
    return r, start


def test_known_answers_of_the_model():
    # noise-free measurements, perturbed start: the truth comes back
    r = PC.ring(40, 1, PC.LOOPS[40], noise=False)
    start = r["truth"] + np.random.default_rng(2).standard_normal((40, 3)) * [0.3, 0.3, 0.05]
    start[0] = r["truth"][0]
    x, st, _ = M.optimize(start, r["fixed"], r["ij"], r["meas"], r["info"], None, 20)
    assert np.abs(x - r["truth"]).max() < 1e-9 and st["chi2_final"] < 1e-12
    # the same at the largest size: 1024 vertices, four loops
    r, start = noise_free_1024()
    # (lambda_0 = 1e-6, nearly Gauss-Newton: with the default damping the long chain's weak modes take more than 20 iterations)
    x, st, _ = M.optimize(start, r["fixed"], r["ij"], r["meas"], r["info"], None, 4, 10, 1e-6)
    d = np.abs(np.column_stack([x[:, :2] - r["truth"][:, :2], M.normalize(x[:, 2] - r["truth"][:, 2])])).max()
    print("noise-free N = 1024 after 4 iterations: distance to the truth", d, "chi2", float(st["chi2_final"]))
    assert d < 1e-9 and st["chi2_final"] < 1e-12
    # one edge: x_0 (+) z
    c = PC.cases()["n2"]
    x, st, _ = M.optimize(*c["graph"][:5], None, 20)
    assert np.abs(x - c["truth"]).max() < 1e-13 and st["chi2_final"] < 1e-22
    # the biased rings: the loops pull the drift back, the worst position error falls to a quarter at most
    for N in (65, 130):
        c = PC.cases()[f"ring{N}"]
        x, _, _ = M.optimize(*c["graph"][:5], None, 20)
        e0 = np.linalg.norm(c["poses"][:, :2] - c["truth"][:, :2], axis=1).max()
        e1 = np.linalg.norm(x[:, :2] - c["truth"][:, :2], axis=1).max()
        print(f"N = {N}: worst position error {e0:.2f} -> {e1:.2f} m")
        assert e1 <= e0 / 4
    # the gross outlier: with the kernel the worst error is below the one without
    err = {}
    for k in ("huber", "huber_off"):
        c = PC.cases()[k]
        x, _, _ = M.optimize(*c["graph"], 20)
        err[k] = np.linalg.norm(x[:, :2] - c["truth"][:, :2], axis=1).max()
    print("Huber case: worst position error", err)
    assert err["huber"] < err["huber_off"]


class _StubContext:
    """pose_graph_optimize that checks the arguments as the real one does and moves every free vertex by (1, 2, 0.5)"""

    def __init__(self):
        self.calls = []

    def pose_graph_optimize(self, graphs, max_iterations=20, max_trials=10, lambda_init=0.0):
        from radarslampy_amd import _ffi
        _ffi.pose_graph_args(graphs, max_iterations, max_trials, lambda_init)
        self.calls.append((len(graphs), max_iterations))
        stats = np.zeros(len(graphs), _ffi.POSE_GRAPH_STATS)
        stats["iterations"] = max_iterations
        return [np.where(np.asarray(g[1])[:, None], g[0], g[0] + [1.0, 2.0, 0.5]) for g in graphs], stats


def test_pose_graph_lib_over_a_stub():
    from radarslampy_amd import PoseGraphLib as PG, utils
    stub = _StubContext()
    g = PG.PoseGraphOptimization(stub)
    g.add_vertex("a", [1.0, 2.0, 0.3], fixed=True)
    g.add_vertex(("kf", 7), utils.convertPoseToTransform(np.array([2.0, 2.5, 0.4])))
    g.add_vertex(-5, np.array([3.0, 3.0, 0.5]))
    with pytest.raises(ValueError):
        g.add_vertex("a", [0, 0, 0])
    with pytest.raises(ValueError):
        g.add_vertex("b", [0, 0])
    mine = 2.0 * np.eye(3)
    g.add_edge(["a", ("kf", 7)], [1.0, 0.2, 0.1], mine)
    mine[0, 0] = 99.0                                   # the graph keeps its own copy
    assert np.array_equal(g.graph()[4][0], 2.0 * np.eye(3))
    g.add_edge((-5, "a"), utils.convertPoseToTransform(np.array([-2.0, -1.0, -0.2])), 4 * np.eye(3), robust_kernel=1.5)
    with pytest.raises(ValueError):
        g.add_edge(("a", "nobody"), [0, 0, 0])
    with pytest.raises(ValueError):
        g.add_edge(("a", -5), [0, 0, 0], np.eye(6))
    poses, fixed, ij, meas, info, hub = g.graph()
    assert np.array_equal(ij, [[0, 1], [2, 0]]) and ij.dtype == np.int32 and np.array_equal(fixed, [True, False, False])
    assert np.allclose(poses[1], [2.0, 2.5, 0.4], atol=1e-15) and np.allclose(meas[1], [-2.0, -1.0, -0.2], atol=1e-15)
    assert np.array_equal(hub, [0.0, 1.5]) and np.array_equal(info[1], 4 * np.eye(3))
    g.optimize(7)
    assert stub.calls == [(1, 7)] and g.stats["iterations"] == 7
    assert np.allclose(g.get_pose("a"), [1.0, 2.0, 0.3]) and np.allclose(g.get_pose(("kf", 7)), [3.0, 4.5, 0.9])
    assert g.get_pose(-5).shape == (3,)
    # several graphs, one call
    h = PG.PoseGraphOptimization()
    h.add_vertex(0, [0, 0, 0], fixed=True)
    PG.optimizeGraphs([h, g], 3)
    assert stub.calls[-1] == (2, 3) and h.stats["iterations"] == 3 and np.allclose(g.get_pose(-5), [5.0, 7.0, 1.5])
    # odometryEdges composed back gives the poses
    poses = PC.cases()["wrap"]["truth"]
    z = PG.odometryEdges(poses)
    assert z.shape == (39, 3)
    back = [poses[0]]
    for zk in z:
        back.append(PC.compose(back[-1], zk))
    assert np.abs(np.array(back) - poses).max() < 1e-12
    assert np.allclose(z[0], PC.relative(poses[0], poses[1]), atol=1e-15)

    # graphFromKeyframes on objects with .pose
    class KF:
        def __init__(self, p):
            self.pose = p

    kfs = [KF(p) for p in poses[:6]]
    g = PG.graphFromKeyframes(kfs, loopEdges=[(0, 5, PC.relative(poses[0], poses[5])), (1, 4, [0.1, 0.2, 0.3], 9 * np.eye(3), 2.0)],
                              odomInformation=PC.OMEGA, loopInformation=PC.LOOP_SCALE * PC.OMEGA, ctx=stub)
    p, fixed, ij, meas, info, hub = g.graph()
    assert np.array_equal(p, poses[:6]) and np.array_equal(fixed, [True] + [False] * 5)
    assert np.array_equal(ij, [[0, 1], [1, 2], [2, 3], [3, 4], [4, 5], [0, 5], [1, 4]]) and np.array_equal(meas[:5], z[:5])
    assert np.array_equal(info[0], PC.OMEGA) and np.array_equal(info[5], PC.LOOP_SCALE * PC.OMEGA) and np.array_equal(info[6], 9 * np.eye(3))
    assert np.array_equal(hub, [0, 0, 0, 0, 0, 0, 2.0])
    assert M.chi2_of(p, ij[:5].astype(np.int64), meas[:5], info[:5], np.zeros(5)) < 1e-24
