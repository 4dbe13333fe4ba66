"""CPU: tests/bench_workload.py restates bench.py's workload (rank 0 of a plain run) - the GPU test test_gpu_bench_scale.py drives an
engine through it and follows a subset of its lane classes on the oracle, so the helper must be bench's workload and the subset
must reach every phase and every sequence."""
import numpy as np

import bench
import bench_workload as W


def test_constants_are_bench_defaults():
    args = bench.parse_args([])
    assert W.WORK == bench.WORK_RETRACK == dict(n_static=460, n_movers=120, scintillation=0.6)
    assert (W.FRAMES, W.DISTINCT, W.LANES) == (args.frames, args.distinct, args.lanes) == (7, 16, 4096)
    assert args.retrack_slots == 0 and not (args.h2d or args.no_retrack or args.endless or args.no_md)
    assert W.seeds()[:3] == [5, 22, 39] and len(W.seeds()) == 16
    cyc, period = W.cycle()
    assert cyc == [0, 1, 2, 3, 4, 5, 6, 5, 4, 3, 2, 1] and period == 12


def test_one_period_plays_the_ping_pong_once_per_lane():
    B, D, T = 4096, W.DISTINCT, W.FRAMES
    cyc, period = W.cycle()
    pool0, t0 = W.first_frames(B)
    assert np.array_equal(pool0 - np.arange(B) * T, t0)
    idx = np.stack([W.scan_indices(B, D, T, s) for s in range(period)])          # (steps, lanes)
    new = (idx & W.STEP_NEW_SEQUENCE) != 0
    frame = (idx & ~W.STEP_NEW_SEQUENCE) - np.arange(B)[None, :] * T              # every lane reads its own private slots
    assert (frame >= 0).all() and (frame < T).all()
    assert (new.sum(axis=0) == 1).all()                                           # exactly one restart per lane and period ...
    assert (frame[new] == 0).all()                                                # ... on frame 0
    for b in range(B):
        d, p = W.lane_class(b)
        assert d == b % D
        # from the first frame on, the lane walks the ping-pong cycle once, starting at its phase
        assert [t0[b]] + list(frame[:, b]) == [cyc[(p + s) % period] for s in range(period + 1)], b
    # the class of a lane never changes: over two periods its frames and restarts are what class_frames gives
    for b in range(0, B, 37):
        f0, frames, restarts = W.class_frames(W.lane_class(b), 2 * period)
        idx2 = np.array([W.scan_indices(B, D, T, s)[b] for s in range(2 * period)])
        assert f0 == t0[b]
        assert list((idx2 & ~W.STEP_NEW_SEQUENCE) - b * T) == frames
        assert list((idx2 & W.STEP_NEW_SEQUENCE) != 0) == restarts


def test_copies_give_every_lane_its_sequence():
    B, D, T = 100, W.DISTINCT, W.FRAMES
    src = {d * T + t: (d, t) for d in range(D) for t in range(T)}
    for dst, s in W.copies(B):
        src[dst] = src[s]
    for b in range(B):
        for t in range(T):
            assert src[b * T + t] == (W.lane_class(b)[0], t)


def test_classes_are_populated():
    cls = W.all_classes()
    assert len(cls) == 16 * 12 == 192 and len(set(cls)) == 192
    for B, least in ((4096, 21), (2085, 10)):
        count = {}
        for b in range(B):
            c = W.lane_class(b)
            count[c] = count.get(c, 0) + 1
        assert set(count) == set(cls), B
        assert min(count.values()) == least, (B, min(count.values()))


def test_oracle_subset_covers_every_phase_and_sequence():
    sub = W.oracle_subset()
    assert len(sub) == 16
    assert {d for d, _ in sub} == set(range(16)) and {p for _, p in sub} == set(range(12))
    assert set(sub) <= set(W.all_classes())
    for c in sub:                                       # the GPU test's 14 regular steps restart every class at least once
        assert sum(W.class_frames(c, 14)[2]) >= 1, c
