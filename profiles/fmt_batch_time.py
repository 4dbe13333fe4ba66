"""Per-pair time of the Fourier-Mellin rotation prior at the live shape (400 x 2025, clip 1012, downsample 10), three ways in one
process: Engine.fmt_rotation on resident pool records (8 records, indices cycling), Context.fmt_rotation_batch from host memory, and
one Context.fmt_rotation call per pair (roam_fmt_rotation: n = 1 of the batched pass, from host memory).  Wall clock around the blocking calls, two warm
runs, best of three.  The figures of docs/KERNELS.md "Batched rotation prior" come from

    python profiles/fmt_batch_time.py --pairs 1024 --host-pairs 256
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def best_of(fn, warm=2, runs=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--host-pairs", type=int, default=256, help="pairs of the host-memory batch (3.2 MB per image)")
    args = ap.parse_args()
    from radarslampy_amd import _ffi, synth
    from radarslampy_amd.engine import Engine
    recs, poses, _ = synth.make_sequence(3, 8, n_movers=6)
    polar = np.stack([r[:, 11:11 + 2025].astype(np.float32) / np.float32(255.) for r in recs])
    ctx = _ffi.Context(0)
    eng = Engine(1, 8, ctx=ctx, retrack_on_device=False)
    for t in range(8):
        eng.upload_scan(t, recs[t])
    prev = np.arange(args.pairs) % 8
    curr = (prev + 1) % 8
    t_eng, all_eng = best_of(lambda: eng.fmt_rotation(prev, curr))
    hp, hc = prev[:args.host_pairs], curr[:args.host_pairs]
    A, B = polar[hp], polar[hc]
    t_host, all_host = best_of(lambda: ctx.fmt_rotation_batch(A, B))

    def singles():
        for i in range(args.pairs):
            ctx.fmt_rotation(polar[prev[i]], polar[curr[i]])
    t_one, all_one = best_of(singles)
    got = eng.fmt_rotation(prev[:8], curr[:8])
    one = np.array([ctx.fmt_rotation(polar[prev[i]], polar[curr[i]]) for i in range(8)])
    print(json.dumps(dict(pairs=args.pairs, host_pairs=args.host_pairs,
                          engine_us_per_pair=1e6 * t_eng / args.pairs, host_batch_us_per_pair=1e6 * t_host / args.host_pairs,
                          single_call_us_per_pair=1e6 * t_one / args.pairs,
                          engine_runs_s=all_eng, host_batch_runs_s=all_host, single_runs_s=all_one,
                          max_angle_difference_rad=float(np.abs(got[:, 0] - one[:, 0]).max()))))
    eng.close()
    ctx.close()


if __name__ == "__main__":
    main()
