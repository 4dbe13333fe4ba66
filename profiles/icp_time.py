"""Time of the batched 2-D ICP kernel (roam_icp2d_batch, csrc/icp.hip) on the shape loop-closure verification gives it: clouds of about
4 500 points (a radar scan's polar peaks), a lone pair (one workgroup: the latency of one verification) and a batch of 256 such pairs
(one per compute unit).  HIP events around the kernel launches alone, the pairs uploaded once, two warm launches first
(roam_time_icp2d_batch); each workload in a process of its own under its own `timeout`.  There is no parent to compare with: the
numbers are a record, in docs/KERNELS.md, from

    python profiles/icp_time.py
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LIMITS = {"lone": 120, "batch": 180}      # seconds per workload
POINTS, RADIUS_M = 4500, 87.0


def pair(seed):
    """two views of one scatter of reflectors in a disc of the radar's range: 60 % of each cloud is common, the rest clutter; the views
    differ by 0.05 rad and 0.6 m, the seed is 0.02 rad off with no translation"""
    rng = np.random.default_rng(seed)

    def disc(n):
        r, a = RADIUS_M * np.sqrt(rng.random(n)), 2 * np.pi * rng.random(n)
        return np.stack([r * np.cos(a), r * np.sin(a)], 1)
    common = disc(int(0.6 * POINTS))
    th, t = 0.05, np.array([0.5, -0.33])
    c, s = np.cos(th), np.sin(th)
    src = np.concatenate([common + 0.05 * rng.standard_normal(common.shape), disc(POINTS - len(common))])
    dst = np.concatenate([common @ np.array([[c, s], [-s, c]]) + t + 0.05 * rng.standard_normal(common.shape), disc(POINTS - len(common))])
    return src[rng.permutation(POINTS)], dst[rng.permutation(POINTS)]


def run(workload):
    from radarslampy_amd import _ffi
    n = 1 if workload == "lone" else 256
    pairs = [pair(100 + k) for k in range(n)]
    init = (0.05 - 0.02, 0.0, 0.0)
    ctx = _ffi.Context(0)
    poses, stats = ctx.icp2d_batch(pairs, init)
    reps = 10 if n == 1 else 3
    ms = [ctx.time_icp2d_batch(pairs, init, reps=reps) for _ in range(3)]
    ctx.close()
    its = stats["iterations"].astype(float) + 1.0                    # searches: one per update and the scoring pass
    evals = float(np.sum(its * POINTS * POINTS))
    best = min(ms)
    return dict(workload=workload, pairs=n, points=POINTS, reps=reps, ms_per_launch=best, runs_ms=ms, ms_per_pair=best / n,
                iterations_mean=float(stats["iterations"].mean()), iterations_max=int(stats["iterations"].max()),
                status_counts=np.bincount(stats["status"], minlength=3).tolist(), inliers_mean=float(stats["n_inliers"].mean()),
                distance_evaluations=evals, evaluations_per_second=evals / (best * 1e-3),
                pose_error_max=[float(np.abs(poses[:, 0] - 0.05).max()), float(np.abs(poses[:, 1:] - [0.5, -0.33]).max())])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(LIMITS))
    args = ap.parse_args()
    if args.workload:
        print(json.dumps(run(args.workload)))
        return 0
    for w in ("lone", "batch"):               # a fresh process each; the first one that fails ends the run
        r = subprocess.run(["timeout", "-k", "10", str(LIMITS[w]), sys.executable, os.path.abspath(__file__), "--workload", w])
        if r.returncode != 0:
            print(json.dumps(dict(workload=w, failed=r.returncode)))
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
