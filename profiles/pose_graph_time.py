"""Time of the device pose-graph optimiser (roam_pose_graph_optimize) on two workloads, each in a process of its own under its own
`timeout`: a lone ring of 4096 vertices with 16 loop edges at 20 iterations (one workgroup: the latency of one solve), and 4096 graphs
of 12 vertices in one call (the batched shape the kernel is made for).  Wall clock around the blocking call, two warm runs, best of
three.  As context only, SciPy's least_squares (trf, sparse analytic Jacobian, 20 evaluations) on the lone graph on the host.  The
record in docs/MEASUREMENT.md comes from

    python profiles/pose_graph_time.py
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LIMITS = {"lone": 240, "batch": 120, "scipy": 240}      # seconds per workload


def ring(N, loops, seed, radius=20.0):
    """N poses on a circle, odometry with noise and a small bias, loop edges at the true relative poses -> a graph tuple"""
    rng = np.random.default_rng(seed)
    phi = 2 * np.pi * np.arange(N) / N
    truth = np.stack([radius * np.cos(phi), radius * np.sin(phi), (phi + 1.5 * np.pi) % (2 * np.pi) - np.pi], axis=1)

    def rel(a, b):
        c, s = np.cos(a[2]), np.sin(a[2])
        dx, dy = b[0] - a[0], b[1] - a[1]
        return np.array([c * dx + s * dy, c * dy - s * dx, (b[2] - a[2] + np.pi) % (2 * np.pi) - np.pi])

    ij = [(k, k + 1) for k in range(N - 1)] + list(loops)
    meas = [rel(truth[k], truth[k + 1]) + rng.standard_normal(3) * [0.02, 0.02, 0.002] + [0.002, 0.0, 0.0005] for k in range(N - 1)]
    meas += [rel(truth[a], truth[b]) for a, b in loops]
    info = np.array([np.diag([2500.0, 2500.0, 250000.0]) * (1.0 if t < N - 1 else 25.0) for t in range(len(ij))])
    poses = [truth[0]]
    for z in meas[:N - 1]:
        a = poses[-1]
        c, s = np.cos(a[2]), np.sin(a[2])
        poses.append(np.array([a[0] + c * z[0] - s * z[1], a[1] + s * z[0] + c * z[1], (a[2] + z[2] + np.pi) % (2 * np.pi) - np.pi]))
    return (np.array(poses), np.arange(N) == 0, np.array(ij, np.int32), np.array(meas), info, None)


def lone_graph():
    return ring(4096, [(100 + 120 * k, 4000 - 110 * k) for k in range(16)], 1)


def best_of(fn, warm=2, runs=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return min(ts), ts, out


def run_device(workload):
    from radarslampy_amd import _ffi
    graphs = [lone_graph()] if workload == "lone" else [ring(12, [(0, 11), (2, 9)], 100 + g, radius=3.0) for g in range(4096)]
    env, nbytes = _ffi.pose_graph_plan(graphs)
    ctx = _ffi.Context(0)
    t, ts, (poses, stats) = best_of(lambda: ctx.pose_graph_optimize(graphs, max_iterations=20))
    ctx.close()
    return dict(workload=workload, graphs=len(graphs), vertices=int(sum(len(g[0]) for g in graphs)), envelope_blocks=int(env.sum()),
                scratch_bytes=nbytes, iterations=20, seconds=t, runs_s=ts, us_per_graph=1e6 * t / len(graphs),
                trials=int(stats["trials"].sum()), rejected=int(stats["rejected"].sum()),
                chi2_initial=float(stats["chi2_initial"].sum()), chi2_final=float(stats["chi2_final"].sum()))


def run_scipy():
    from scipy.optimize import least_squares
    from scipy.sparse import lil_matrix
    poses, fixed, ij, meas, info, _ = lone_graph()
    free = np.flatnonzero(~fixed)
    cidx = np.full(len(poses), -1)
    cidx[free] = np.arange(len(free))
    w = np.sqrt(np.diagonal(info, axis1=1, axis2=2))
    ij = ij.astype(np.int64)

    def terms(v, jac):
        x = poses.copy()
        x[free] = v.reshape(-1, 3)
        xi, xj = x[ij[:, 0]], x[ij[:, 1]]
        c, s, cz, sz = np.cos(xi[:, 2]), np.sin(xi[:, 2]), np.cos(meas[:, 2]), np.sin(meas[:, 2])
        dx, dy = xj[:, 0] - xi[:, 0], xj[:, 1] - xi[:, 1]
        ux, uy = c * dx + s * dy - meas[:, 0], c * dy - s * dx - meas[:, 1]
        e = np.stack([cz * ux + sz * uy, cz * uy - sz * ux, (xj[:, 2] - xi[:, 2] - meas[:, 2] + np.pi) % (2 * np.pi) - np.pi], 1) * w
        if not jac:
            return e.ravel()
        E, o, z = len(ij), np.ones(len(ij)), np.zeros(len(ij))
        Z = np.stack([np.stack([cz, sz, z], 1), np.stack([-sz, cz, z], 1), np.stack([z, z, o], 1)], 1)
        A = Z @ np.stack([np.stack([-c, -s, c * dy - s * dx], 1), np.stack([s, -c, -c * dx - s * dy], 1), np.stack([z, z, -o], 1)], 1)
        B = Z @ np.stack([np.stack([c, s, z], 1), np.stack([-s, c, z], 1), np.stack([z, z, o], 1)], 1)
        J = lil_matrix((3 * E, 3 * len(free)))
        for t in range(E):
            for k, D in ((cidx[ij[t, 0]], A[t]), (cidx[ij[t, 1]], B[t])):
                if k >= 0:
                    J[3 * t:3 * t + 3, 3 * k:3 * k + 3] = w[t][:, None] * D
        return J.tocsr()

    t0 = time.perf_counter()
    r = least_squares(lambda v: terms(v, False), poses[free].ravel(), jac=lambda v: terms(v, True), method="trf", tr_solver="lsmr", max_nfev=20)
    return dict(workload="scipy", context_only=True, solver="least_squares trf / lsmr, sparse analytic Jacobian, max_nfev 20",
                seconds=time.perf_counter() - t0, nfev=int(r.nfev), chi2_final=float(2 * r.cost))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(LIMITS))
    args = ap.parse_args()
    if args.workload:
        print(json.dumps(run_scipy() if args.workload == "scipy" else run_device(args.workload)))
        return 0
    for w in ("lone", "batch", "scipy"):          # a fresh process each; the first one that fails ends the run
        r = subprocess.run(["timeout", "-k", "10", str(LIMITS[w]), sys.executable, os.path.abspath(__file__), "--workload", w])
        if r.returncode != 0:
            print(json.dumps(dict(workload=w, failed=r.returncode)))
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
