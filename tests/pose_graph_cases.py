"""Inputs of the pose-graph tests (tests/test_pose_graph_cpu.py, tests/test_gpu_pose_graph.py) and measure_spread(), which gives the
device its bar.  Every case is a dict: poses (V, 3) start, truth (V, 3), fixed (V,), ij (E, 2), meas (E, 3), info (E, 3, 3),
huber (E,) or None, opts (max_iterations, max_trials, lambda_init) of the step-by-step comparison, and the tuple
graph = (poses, fixed, ij, meas, info, huber) as Context.pose_graph_optimize takes it.

The iteration counts are at most 8: the accept / reject decisions of a comparison must not hang on rounding, so every trial of the
model at that count has |rho| >= 1e-3 (asserted by the CPU test).  rho = (cur - tmp) / (d^T (lambda d + b) + 1e-3) falls below that
as soon as an iteration gains less than about 1e-6 in chi2, which the small exact cases reach after one or two iterations - their
counts are the largest that keep the condition."""
import functools

import numpy as np

import pose_graph_model as model

NOISE = np.array([0.02, 0.02, 0.002])
BIAS = np.array([0.01, 0.0, 0.004])
# a full, non-diagonal information matrix: the inverse of a covariance with the noise's deviations and correlations 0.3, -0.2, 0.1
_C = np.array([[1.0, 0.3, -0.2], [0.3, 1.0, 0.1], [-0.2, 0.1, 1.0]]) * np.outer(NOISE, NOISE)
_Oi = np.linalg.inv(_C)
OMEGA = (_Oi + _Oi.T) / 2
LOOP_SCALE = 25.0


def relative(a, b):
    """a^-1 b of two poses (x, y, theta)"""
    c, s = np.cos(a[2]), np.sin(a[2])
    dx, dy = b[0] - a[0], b[1] - a[1]
    return np.array([c * dx + s * dy, c * dy - s * dx, model.normalize(b[2] - a[2])])


def compose(a, z):
    """a (+) z"""
    c, s = np.cos(a[2]), np.sin(a[2])
    return np.array([a[0] + c * z[0] - s * z[1], a[1] + s * z[0] + c * z[1], model.normalize(a[2] + z[2])])


def circle(N, radius, laps=1, phase=0.0):
    """N poses on a circle, headings tangent"""
    phi = phase + 2 * np.pi * laps * np.arange(N) / N
    return np.stack([radius * np.cos(phi), radius * np.sin(phi), model.normalize(phi + np.pi / 2)], axis=1)


def _case(poses, truth, fixed, ij, meas, info, huber=None, opts=(8, 10, 0.0)):
    ij = np.asarray(ij, np.int32).reshape(-1, 2)
    info = np.ascontiguousarray(np.broadcast_to(info, (len(ij), 3, 3)))
    d = dict(poses=np.asarray(poses, np.float64), truth=np.asarray(truth, np.float64), fixed=np.asarray(fixed, bool), ij=ij,
             meas=np.asarray(meas, np.float64).reshape(-1, 3), info=info, huber=None if huber is None else np.asarray(huber, np.float64),
             opts=opts)
    d["graph"] = (d["poses"], d["fixed"], d["ij"], d["meas"], d["info"], d["huber"])
    return d


def ring(N, seed, loops=(), bias=False, radius=None, fixed=(0,), laps=1, phase=0.0, noise=True, opts=(8, 10, 0.0)):
    """the ring: consecutive edges = true relative poses + seeded noise (+ a bias per step), loop edges = true relative poses at 25
    Omega; the start is the odometry composed from vertex 0"""
    rng = np.random.default_rng(seed)
    truth = circle(N, (10.0 if N == 40 else 20.0) if radius is None else radius, laps, phase)
    ij, meas, info = [], [], []
    for k in range(N - 1):
        z = relative(truth[k], truth[k + 1]) + (rng.standard_normal(3) * NOISE if noise else 0.0) + (BIAS if bias else 0.0)
        ij.append((k, k + 1)); meas.append(z); info.append(OMEGA)
    for a, b in loops:
        ij.append((a, b)); meas.append(relative(truth[a], truth[b])); info.append(LOOP_SCALE * OMEGA)
    poses = [truth[0]]
    for k in range(N - 1):
        poses.append(compose(poses[-1], meas[k]))
    poses = np.array(poses)
    fx = np.zeros(N, bool)
    fx[list(fixed)] = True
    poses[fx] = truth[fx]
    return _case(poses, truth, fx, ij, meas, np.array(info), opts=opts)


LOOPS = {40: [(0, 39)], 65: [(0, 64), (20, 50)], 130: [(0, 129), (10, 70), (40, 100)],
         1024: [(0, 1023), (100, 900), (300, 700), (50, 500)]}


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case, in a fixed order"""
    c = {}
    # one edge, vertex 0 fixed: the answer is x_0 (+) z with chi2 0
    x0, z = np.array([3.0, -2.0, 0.7]), np.array([1.5, 0.25, -0.4])
    c["n2"] = _case([x0, compose(x0, z) + [0.4, -0.3, 0.2]], [x0, compose(x0, z)], [1, 0], [(0, 1)], [z], OMEGA, opts=(2, 10, 0.0))
    # triangle whose loop does not close
    tri = np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 2.0], [2.0, 3.5, -2.1]])
    zs = [relative(tri[0], tri[1]) + [0.1, -0.05, 0.02], relative(tri[1], tri[2]) + [-0.08, 0.06, -0.03], relative(tri[2], tri[0]) + [0.05, 0.1, 0.04]]
    c["triangle"] = _case(tri + [[0, 0, 0], [0.3, -0.2, 0.1], [-0.2, 0.25, -0.15]], tri, [1, 0, 0], [(0, 1), (1, 2), (2, 0)], zs, OMEGA,
                          opts=(3, 10, 0.0))
    for N in (40, 65, 130):
        c[f"ring{N}"] = ring(N, 100 + N, LOOPS[N], bias=True, opts=(7 if N == 40 else 8, 10, 0.0))
    c["ring1024"] = ring(1024, 1124, LOOPS[1024], opts=(3, 10, 0.0))
    # vertex compaction
    c["fixed_middle"] = ring(40, 201, LOOPS[40], bias=True, fixed=(17,), opts=(7, 10, 0.0))
    c["fixed_last"] = ring(40, 202, LOOPS[40], bias=True, fixed=(39,), opts=(7, 10, 0.0))
    c["fixed_two"] = ring(40, 203, LOOPS[40], bias=True, fixed=(0, 23), opts=(5, 10, 0.0))
    # an edge given backwards (39 -> 0, and 21 -> 20 in the chain) and a duplicated edge
    r = ring(40, 204, [], bias=True)
    ij, meas, info = r["ij"].copy(), r["meas"].copy(), r["info"].copy()
    ij[20] = (21, 20)
    meas[20] = relative(compose(np.zeros(3), meas[20]), np.zeros(3))
    ij = np.vstack([ij, [(39, 0)], ij[7:8], [(12, 30)], [(12, 30)]])
    meas = np.vstack([meas, relative(r["truth"][39], r["truth"][0]), meas[7] + [0.01, -0.01, 0.001], relative(r["truth"][12], r["truth"][30]),
                      relative(r["truth"][12], r["truth"][30]) + [0.02, 0.0, -0.002]])
    info = np.concatenate([info, np.stack([LOOP_SCALE * OMEGA, OMEGA, LOOP_SCALE * OMEGA, OMEGA])])
    c["backward_duplicate"] = _case(r["poses"], r["truth"], r["fixed"], ij, meas, info)
    # two laps: the heading crosses +-pi twice; vertices 3 and 13 face opposite ways, their loop measures pi - 5e-10
    r = ring(40, 205, [(0, 39)], bias=True, laps=2, phase=0.05)
    z = relative(r["truth"][3], r["truth"][13])
    z[2] = np.pi - 5e-10
    c["wrap"] = _case(r["poses"], r["truth"], r["fixed"], np.vstack([r["ij"], [(3, 13)]]), np.vstack([r["meas"], z]),
                      np.concatenate([r["info"], [LOOP_SCALE * OMEGA]]))
    # Huber: delta = 1 on the loop edges, one of them a gross outlier; the loop (8, 10) agrees with the odometry, so at the start it is
    # the one kernel edge inside delta
    r = ring(65, 206, LOOPS[65], bias=True)
    ij = np.vstack([r["ij"], [(5, 40)], [(8, 10)]])
    meas = np.vstack([r["meas"], relative(r["truth"][5], r["truth"][40]) + [6.0, -4.0, 0.5], relative(r["poses"][8], r["poses"][10])])
    info = np.concatenate([r["info"], [LOOP_SCALE * OMEGA, LOOP_SCALE * OMEGA]])
    hub = np.zeros(len(ij))
    hub[64:] = 1.0
    c["huber"] = _case(r["poses"], r["truth"], r["fixed"], ij, meas, info, hub)
    c["huber_off"] = _case(r["poses"], r["truth"], r["fixed"], ij, meas, info, None)
    # rejected trials: far from the truth with almost no damping
    r = ring(40, 207, LOOPS[40])
    start = r["truth"] + np.random.default_rng(239).standard_normal((40, 3)) * [3.0, 3.0, 1.0]
    start[:, 2] = model.normalize(start[:, 2])
    start[0] = r["truth"][0]
    c["reject"] = _case(start, r["truth"], r["fixed"], r["ij"], r["meas"], r["info"], opts=(6, 10, 1e-9))
    # failed factorisations: the pair (2, 3) hangs on no fixed vertex, so H is singular there, and with lambda_0 = 1e-30 the damping
    # is absorbed (1 + lambda == 1 up to lambda = 1e-30 * 2^45 of the tenth trial).  Headings 0, integer coordinates and Omega = I
    # make every operation exact in any order: the second pivot of the pair is 1 - 1 = 0 on the device as in LAPACK, every trial of
    # the first iteration fails (tmp = inf) and is rejected, and the run ends with the trials exhausted and the poses untouched.
    # exact: the device must give the model's bits; the case takes no part in measure_spread(), whose +-4 ulp on cos(0) would make
    # the pivot a matter of rounding
    un = np.array([[0.0, 0.0, 0.0], [2.0, 1.0, 0.0], [5.0, -3.0, 0.0], [5.0, -3.0, 0.0]])
    c["unanchored"] = dict(_case(un, un, [1, 0, 0, 0], [(0, 1), (2, 3)], [[1.0, 1.0, 0.0], [1.0, 2.0, 0.0]], np.eye(3), opts=(3, 10, 1e-30)),
                           exact=True)
    # evaluate only
    c["evaluate"] = dict(c["ring40"], opts=(0, 10, 0.0))
    return c


def batch(n, seed=7):
    """n graphs of mixed sizes: the cases shuffled, the largest at most once -> (list of graphs, list of case names)"""
    names = [k for k in cases() if k not in ("ring1024", "evaluate")]
    rng = np.random.default_rng(seed)
    pick = [names[i] for i in rng.integers(0, len(names), n)]
    if n >= 300:
        pick[n // 3] = "ring1024"
    return [cases()[k]["graph"] for k in pick], pick


@functools.lru_cache(maxsize=None)
def reference(name):
    """the model's run of a case at its options: (poses, stats, log), computed once"""
    c = cases()[name]
    it, tr, lam = c["opts"]
    return model.optimize(c["poses"], c["fixed"], c["ij"], c["meas"], c["info"], c["huber"], it, tr, lam)


def difference(xa, sa, xb, sb):
    """(position, angle, chi2 relative, lambda relative) between two runs"""
    rel = lambda a, b: abs(a - b) / max(abs(a), abs(b)) if a != b else 0.0
    return (float(np.abs(xa[:, :2] - xb[:, :2]).max()), float(np.abs(model.normalize(xa[:, 2] - xb[:, 2])).max()),
            rel(float(sa["chi2_final"]), float(sb["chi2_final"])), rel(float(sa["lambda_final"]), float(sb["lambda_final"])))


@functools.lru_cache(maxsize=None)
def measure_spread():
    """The model a second time in another float64 order - Cholesky and two triangular solves instead of solve, every sin and cos moved
    by a seeded +-4 ulp (HIP documents 2 ulp for them on the device, glibc stays below 1) - against reference(), over all cases.
    (the case marked exact is left out: its bar is equality)
    -> (per case {name: (position, angle, chi2 rel, lambda rel)}, bound: ten times the largest of each over the cases).  The bound is
    the device's bar against reference()."""
    per = {}
    for name, c in cases().items():
        if c.get("exact"):
            continue
        it, tr, lam = c["opts"]
        xa, sa, _ = reference(name)
        xb, sb, _ = model.optimize(c["poses"], c["fixed"], c["ij"], c["meas"], c["info"], c["huber"], it, tr, lam, chol=True, trig_ulp=4,
                                   seed=11)
        assert tuple(sa[k] for k in ("iterations", "trials", "rejected", "stop")) == tuple(sb[k] for k in ("iterations", "trials", "rejected", "stop")), name
        per[name] = difference(xa, sa, xb, sb)
    bound = tuple(10.0 * max(v[q] for v in per.values()) for q in range(4))
    return per, bound
