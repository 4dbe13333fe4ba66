"""Per-pair time of the Fourier-Mellin registration at the live shape (400 x 2025, clip 1012, downsample 10) at cart_downsample 20 and
5, three ways in one process: Engine.fmt_register on resident pool records (8 records, indices cycling), Context.fmt_register_batch
from host memory, and the four-call Python composition that the pass replaces, one pair at a time (FMT.getRotationUsingFMT,
parseData.convertPolarImageToCartesian twice, FMT.rotateImg, FMT.getTranslationUsingPhaseCorrelation).  Beside them
Engine.fmt_rotation on the same pairs: what the translation half adds.  Wall clock around the blocking calls, two warm runs, best of
three.  The figures of docs/KERNELS.md "Batched registration" come from

    python profiles/fmt_register_time.py --pairs 1024 --host-pairs 128 --composed-pairs 32
"""
import argparse
import json
import math
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
    ap.add_argument("--host-pairs", type=int, default=128, help="pairs of the host-memory batch (3.2 MB per image)")
    ap.add_argument("--composed-pairs", type=int, default=32, help="pairs put through the four-call composition")
    args = ap.parse_args()
    from radarslampy_amd import FMT, _ffi, parseData, synth
    from radarslampy_amd.engine import Engine
    recs, poses, _ = synth.make_sequence(3, 8, n_movers=6)
    polar = np.stack([r[:, 11:11 + 2025].astype(np.float32) / np.float32(255.) for r in recs])
    ctx = _ffi.Context(0)
    eng = Engine(1, 8, ctx=ctx, retrack_on_device=False)
    for t in range(8):
        eng.upload_scan(t, recs[t])
    prev = np.arange(args.pairs) % 8
    curr = (prev + 1) % 8
    hp, hc = prev[:args.host_pairs], curr[:args.host_pairs]
    A, B = polar[hp], polar[hc]
    t_rot, all_rot = best_of(lambda: eng.fmt_rotation(prev, curr))
    out = dict(pairs=args.pairs, host_pairs=args.host_pairs, composed_pairs=args.composed_pairs,
               engine_rotation_only_us_per_pair=1e6 * t_rot / args.pairs, engine_rotation_only_runs_s=all_rot)
    for cds in (20, 5):
        t_eng, all_eng = best_of(lambda: eng.fmt_register(prev, curr, cart_downsample=cds))
        t_host, all_host = best_of(lambda: ctx.fmt_register_batch(A, B, cart_downsample=cds))

        def composed():
            res = []
            for i in range(args.composed_pairs):
                a, b = polar[prev[i]], polar[curr[i]]
                ang, sc, rr = FMT.getRotationUsingFMT(a, b)
                ca = parseData.convertPolarImageToCartesian(a, downsampleFactor=cds)
                cb = parseData.convertPolarImageToCartesian(b, downsampleFactor=cds)
                (dx, dy), tr = FMT.getTranslationUsingPhaseCorrelation(FMT.rotateImg(ca, math.degrees(ang)), cb)
                res.append((ang, sc, rr, dx, dy, tr))
            return np.array(res)
        t_one, all_one = best_of(composed)
        got = eng.fmt_register(prev[:8], curr[:8], cart_downsample=cds)
        one = composed()[:8]
        out[f"cart_downsample_{cds}"] = dict(
            engine_us_per_pair=1e6 * t_eng / args.pairs, host_batch_us_per_pair=1e6 * t_host / args.host_pairs,
            composed_us_per_pair=1e6 * t_one / args.composed_pairs, engine_runs_s=all_eng, host_batch_runs_s=all_host, composed_runs_s=all_one,
            max_translation_difference_px=float(np.abs(got[:len(one), 3:5] - one[:, 3:5]).max()))
    print(json.dumps(out))
    eng.close()
    ctx.close()


if __name__ == "__main__":
    main()
