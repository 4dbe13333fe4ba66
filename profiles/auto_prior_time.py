"""Cost of the motion prior as a mode of the engine (Engine.set_auto_prior).  The figures of docs/KERNELS.md "In-step motion prior":

    python profiles/auto_prior_time.py

(a) one sequence, --frames frames (8 distinct synthetic scans played ping-pong) through a one-lane engine fed as RawROAMSystem feeds it
    (pinned ring, uploads three frames ahead, results read two steps late), scan pairs per second, three ways in alternating runs of
    one process: no prior | the blocking chain per pair (Engine.fmt_register -> FMT.flowPriorFromFMT -> Engine.set_motion_prior ->
    step) | the mode.
(b) --lanes lanes (every lane plays the same 8 records, so the records come from the caches: the figure is the difference, not the
    step), milliseconds per step with the mode off and on, alternating.
Wall clock around the loops, the last result on the host before the clock stops."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RING, LOOKAHEAD, LAG = 8, 3, 2


def one_sequence(ctx, recs, frames, mode):
    from radarslampy_amd import FMT
    from radarslampy_amd.engine import Engine
    n = len(recs)
    frame = lambda k: recs[(k % (2 * n - 2)) if (k % (2 * n - 2)) < n else 2 * n - 2 - (k % (2 * n - 2))]
    eng = Engine(1, RING, ctx=ctx, retrack_on_device=True, stage_events=False)
    pinned = ctx.host_alloc((RING, 400, 3779))
    if mode == "auto":
        eng.set_auto_prior(True)

    def up(k):
        pinned[k % RING] = frame(k)
        eng.upload_scans_async(k % RING, pinned[k % RING], n=1)

    for k in range(1 + LOOKAHEAD):
        up(k)
    eng.synchronize()
    eng.init_lane_detect(0, 0, np.zeros(3))
    seeded = 0
    t0 = time.perf_counter()
    for k in range(1, frames):
        if mode == "chain":
            reg = eng.fmt_register([(k - 1) % RING], [k % RING])
            eng.set_motion_prior(FMT.flowPriorFromFMT(reg[:, 0], reg[:, 3:5]))
        eng.step([k % RING])
        eng.fence()
        if k + LOOKAHEAD < frames:
            up(k + LOOKAHEAD)
        if k - 1 - LAG >= 0:
            eng.results_array(k - 1 - LAG)
            if mode == "auto":
                seeded += int(eng.step_prior(k - 1 - LAG)["source"][0] == 1)
    for s in range(max(0, frames - 1 - LAG), frames - 1):
        eng.results_array(s)
    dt = time.perf_counter() - t0
    ctx.host_free(pinned)
    eng.close()
    return (frames - 1) / dt, seeded


def many_lanes(ctx, recs, lanes, steps, rounds):
    from radarslampy_amd.engine import Engine
    n = len(recs)
    eng = Engine(lanes, n, ctx=ctx, retrack_on_device=True)
    for t in range(n):
        eng.upload_scan(t, recs[t])
    eng.init_lanes_detect(0, np.zeros(lanes, np.int32), np.zeros((lanes, 3)))
    k, out = 0, {"off": [], "on": []}

    def run(count):
        nonlocal k
        t0 = time.perf_counter()
        for _ in range(count):
            k += 1
            j = k % (2 * n - 2)
            eng.step(np.full(lanes, j if j < n else 2 * n - 2 - j, np.int32))
        eng.results_array()
        return 1e3 * (time.perf_counter() - t0) / count

    run(3)
    for _ in range(rounds):
        for mode in ("off", "on"):
            eng.set_auto_prior(mode == "on")
            run(2)
            out[mode].append(run(steps))
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--lanes", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args()
    from radarslampy_amd import _ffi, synth
    recs, _, _ = synth.make_sequence(3, 8, n_movers=6)
    ctx = _ffi.Context(0)
    res = {"one_sequence_pairs_per_s": {"none": [], "chain": [], "auto": []}}
    one_sequence(ctx, recs, 24, "auto")                                      # warm: twiddle tables, scratch, code objects
    for _ in range(args.rounds):
        for mode in ("none", "chain", "auto"):
            rate, seeded = one_sequence(ctx, recs, args.frames, mode)
            res["one_sequence_pairs_per_s"][mode].append(round(rate, 1))
            if mode == "auto":
                res["auto_pairs_seeded_of_read"] = [seeded, max(0, args.frames - 1 - LAG)]
    if args.lanes > 0:
        res["lanes"] = args.lanes
        res["ms_per_step"] = {m: [round(v, 2) for v in vs] for m, vs in many_lanes(ctx, recs, args.lanes, args.steps, args.rounds).items()}
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
