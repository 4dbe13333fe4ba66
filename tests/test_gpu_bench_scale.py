"""GPU (-m gpu): the benchmark's configuration - a 4 096-lane engine on its default settings, on bench.py's WORK_RETRACK workload - lane
by lane against the oracle.

Only at that size does the engine take the two-stream detection (launch_retrack: chunks of 1 024 detections, the determinants of chunk c
on a second stream beside the integral images of chunk c + 1, the two halves of a 2 048-slot scratch alternating), the default
retrack_slots of 2 048 and the step schedule of engines of >= 256 lanes (the pyramid and the peaks of later steps waiting for the
detection's events).  B = 2 085 takes the same forms with a ragged last workgroup in every per-lane launch, and its forced step ends in
a chunk of 37 detections: the two-pass integral kernels inside the two-stream form.

A lane's history is fixed by its class (sequence, phase) (tests/bench_workload.py), so:
  * all lanes of a class must give the same records and features, byte for byte;
  * every class must equal the same class on a 192-lane reference engine - one lane per class, 64 scratch slots: one stream, the
    two-pass integral kernels, the small-batch schedule;
  * one class per sequence, covering every phase, must equal the oracle's loop body.
The engines run in a child process (a 4 096-lane engine holds ~212 GB, which the child gives back); the oracle runs first, on the CPU."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import bench_workload as W                      # noqa: E402

pytestmark = pytest.mark.gpu

S = 14                      # regular steps, back to back: more than one period (12), so every class restarts
CHECKPOINTS = (7, 14)       # the engine is synchronised and every lane's features read after this many steps
FORCED = S                  # index of the last step: set_retrack(2), every lane detects
POS_TOL = 1e-4              # m
ANG_TOL = 1e-5              # rad
ORACLE_PROCS = 8
CHUNK = 1024                # detections per launch in the two-stream form (engine.hip, roam_engine_create)


# ------------------------------------------------------------------------------------------------ child: the engines
def _features(out, key, eng, lanes):
    f = [eng.lane_features(b) for b in lanes]
    out[key + "_n"] = np.array([len(x) for x in f], np.int64)
    out[key] = np.concatenate(f).astype(np.float32).reshape(-1, 2)


def _records(r):
    return np.ascontiguousarray(r).view(np.uint8).reshape(len(r), -1)


def _child(B, seq_path, out_path):
    from radarslampy_amd import _ffi
    from radarslampy_amd.engine import Engine
    z = np.load(seq_path)
    recs, poses = z["recs"], z["poses"]
    D, T = recs.shape[:2]
    out = {}
    t_start = time.perf_counter()
    ctx = _ffi.Context(0)
    # ---- the benchmark's engine (bench.py:379-397), no keyframe map (bench reserves none)
    eng = Engine(B, B * T, ctx=ctx, motion_distortion=True, retrack_on_device=True)
    out["detect_chunk"] = np.array(eng.detect_chunk())
    for d in range(D):
        for t in range(T):
            eng.upload_scan(d * T + t, recs[d, t])
    for dst, src in W.copies(B, D, T):
        eng.copy_scan(dst, src)
    eng.synchronize()
    pool0, t0 = W.first_frames(B, D, T)
    eng.init_lanes_detect(0, pool0, poses[np.arange(B) % D, t0])
    _features(out, "big_f0", eng, range(B))
    res = {}
    chunk_ms, traced = [], 0
    for s in range(S):
        eng.step(W.scan_indices(B, D, T, s))
        if s >= 2 and s - 2 not in res:
            res[s - 2] = eng.results_array(s - 2)              # bench.py:463-496: records read two steps behind the enqueue front
        if s + 1 in CHECKPOINTS:
            eng.synchronize()
            for k in range(s + 1):
                if k not in res:
                    res[k] = eng.results_array(k)
            _features(out, f"big_f{s + 1}", eng, range(B))
            chunk_ms.append(eng.kernel_chunk_ms("doh_integral", s + 1 - traced))      # (synchronises: read at the checkpoints only)
            traced = s + 1
    eng.set_retrack(2)                                        # every lane detects: 4 (B = 4096) / 3 (B = 2085) chunks
    eng.step(W.scan_indices(B, D, T, FORCED))
    res[FORCED] = eng.results_array(FORCED)
    _features(out, f"big_f{FORCED + 1}", eng, range(B))
    chunk_ms.append(eng.kernel_chunk_ms("doh_integral", 1))
    out["big_chunk_ms"] = np.concatenate(chunk_ms)
    out["big_res"] = np.stack([_records(res[k]) for k in range(FORCED + 1)])
    eng.close()
    out["big_s"] = np.array(time.perf_counter() - t_start)
    # ---- the reference engine: one lane per class, 64 scratch slots (one stream, two-pass integral kernels, B < 256 schedule)
    classes = W.all_classes(D, T)
    R = len(classes)
    plan = [W.class_frames(c, FORCED + 1, T) for c in classes]
    ref = Engine(R, D * T, ctx=ctx, motion_distortion=True, retrack_on_device=True, retrack_slots=64)
    ref.map_reserve(8)
    for d in range(D):
        for t in range(T):
            ref.upload_scan(d * T + t, recs[d, t])
    ref.synchronize()
    ref.init_lanes_detect(0, [d * T + plan[k][0] for k, (d, _) in enumerate(classes)],
                          np.array([poses[d, plan[k][0]] for k, (d, _) in enumerate(classes)]))
    _features(out, "ref_f0", ref, range(R))
    rres = []
    subset = [classes.index(c) for c in W.oracle_subset(D, T)]
    for s in range(FORCED + 1):
        if s == FORCED:
            ref.set_retrack(2)
        ref.step(np.array([(d * T + plan[k][1][s]) | (W.STEP_NEW_SEQUENCE if plan[k][2][s] else 0) for k, (d, _) in enumerate(classes)], np.int32))
        rres.append(_records(ref.results_array()))
        if s + 1 in CHECKPOINTS or s == FORCED:
            _features(out, f"ref_f{s + 1}", ref, range(R))
        if s + 1 == S:
            kfs = [ref.live_keyframe(k)["prunedUndistortedLocals"] for k in subset]
            out["ref_kf_n"] = np.array([len(x) for x in kfs], np.int64)
            out["ref_kf"] = np.concatenate(kfs).reshape(-1, 2)
    out["ref_res"] = np.stack(rres)
    ref.close()
    ctx.close()
    out["total_s"] = np.array(time.perf_counter() - t_start)
    np.savez(out_path, **out)


# ------------------------------------------------------------------------------------------------ parent: oracle, checks
@pytest.fixture(scope="module")
def workload(tmp_path_factory):
    """the 16 sequences (rendered in the workers) and the oracle's run of every subset class, before the GPU is touched"""
    import multiprocessing as mp
    sub = W.oracle_subset()
    assert [d for d, _ in sub] == list(range(W.DISTINCT))
    jobs = [(c, W.seeds()[c[0]], FORCED + 1, W.FRAMES) for c in sub]
    pool = mp.get_context("spawn").Pool(max(1, min(ORACLE_PROCS, os.cpu_count() or 1, len(jobs))))
    try:
        got = pool.map(W.oracle_class, jobs)
        pool.close()
        pool.join()
    except BaseException:
        pool.terminate()
        raise
    path = str(tmp_path_factory.mktemp("bench_scale") / "sequences.npz")
    np.savez(path, recs=np.stack([np.stack(g[0]) for g in got]), poses=np.stack([g[1] for g in got]))
    return path, {c: g[2] for c, g in zip(sub, got)}


def _split(flat, n):
    return np.split(flat, np.cumsum(n)[:-1])


@pytest.mark.parametrize("B", [4096, 2085])
def test_bench_configuration_lane_by_lane(B, workload, tmp_path):
    from radarslampy_amd import _ffi
    seq_path, want = workload
    out_path = str(tmp_path / "engines.npz")
    # the engine's defaults, as bench runs it: no ROAM_* knob reaches the child (ROAM_LIB, an A/B build of the library, and ROAM_DEVICE do)
    env = {k: v for k, v in os.environ.items() if not k.startswith("ROAM_") or k in ("ROAM_LIB", "ROAM_DEVICE")}
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(B), seq_path, out_path], capture_output=True, text=True,
                       timeout=900, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    print(f"B={B}: engines {time.perf_counter() - t0:.1f} s")
    z = np.load(out_path)
    dt = np.ctypeslib.as_array((_ffi.LaneResult * 1)()).dtype
    big = z["big_res"]                                                # (S + 1, B, 128) u8
    ref = z["ref_res"]                                                # (S + 1, 192, 128) u8
    big_r = [np.frombuffer(big[s].tobytes(), dt) for s in range(FORCED + 1)]
    ref_r = [np.frombuffer(ref[s].tobytes(), dt) for s in range(FORCED + 1)]
    classes = W.all_classes()
    lane_cls = [classes.index(W.lane_class(b)) for b in range(B)]
    members = [[b for b in range(B) if lane_cls[b] == k] for k in range(len(classes))]
    ckpt = (0,) + CHECKPOINTS + (FORCED + 1,)
    bf = {c: _split(z[f"big_f{c}"], z[f"big_f{c}_n"]) for c in ckpt}
    rf = {c: _split(z[f"ref_f{c}"], z[f"ref_f{c}_n"]) for c in ckpt}

    # ---- the configuration is bench's: two-stream detection in chunks of 1 024, ceil(B / 1024) chunks per step
    assert int(z["detect_chunk"]) == CHUNK
    ms = z["big_chunk_ms"]
    nc = -(-B // CHUNK)
    assert ms.shape == (FORCED + 1, nc), ms.shape
    held = []
    for s in range(FORCED + 1):
        n = int(np.count_nonzero(big_r[s]["flags"] & 8))             # lanes that detected in the step (bench.py:511-513)
        h = [min(max(n - CHUNK * c, 0), CHUNK) for c in range(nc)]
        held.append(h)
        for c in range(nc):
            if h[c]:
                assert ms[s, c] > 0, (B, s, c, h, ms[s])
    if B == 4096:
        assert max(sum(1 for x in h if x) for h in held[:S]) >= 2, held
        assert held[FORCED] == [1024] * 4, held[FORCED]
    else:
        assert held[FORCED] == [1024, 1024, 37], held[FORCED]

    # ---- the workload is not vacuous
    for s in range(FORCED + 1):
        f = big_r[s]["flags"]
        assert ((f & 1) == 1).all(), (B, s, "clique not proven", np.flatnonzero((f & 1) == 0)[:8])
        assert (((f >> 8) & 15) == 0).all(), (B, s, "overflow", np.flatnonzero((f >> 8) & 15)[:8])
        if 1 <= s < S:
            frac = np.count_nonzero(f & 8) / B
            assert 0.25 <= frac <= 0.65, (B, s, frac)
            rej = np.count_nonzero(big_r[s]["n_inliers"] < big_r[s]["n_good"]) / B
            assert rej >= 0.20, (B, s, rej)
            assert np.count_nonzero(f & 2) > 0, (B, s, "no keyframe added")
    assert (big_r[FORCED]["flags"] & 8).all()

    # ---- within a class, lanes are equal; every class equals its lane of the reference engine
    for k, lanes in enumerate(members):
        b0 = lanes[0]
        for s in range(FORCED + 1):
            same = (big[s, lanes] == big[s, b0]).all(axis=1)
            assert same.all(), (B, "class", classes[k], "step", s, "lanes differ", [lanes[i] for i in np.flatnonzero(~same)][:8])
            if big[s, b0].tobytes() != ref[s, k].tobytes():
                diff = [n for n in dt.names if not np.array_equal(big_r[s][n][b0], ref_r[s][n][k])]
                raise AssertionError((B, "class", classes[k], "step", s, "differs from the reference engine in", diff))
        for c in ckpt:
            for b in lanes:
                assert np.array_equal(bf[c][b], bf[c][b0]), (B, "class", classes[k], "features after", c, "lane", b, "vs", b0)
            assert np.array_equal(bf[c][b0], rf[c][k]), (B, "class", classes[k], "features after", c, "big vs reference engine")

    # ---- every subset class equals the oracle
    sub = W.oracle_subset()
    kf = _split(z["ref_kf"], z["ref_kf_n"])
    for i, cls in enumerate(sub):
        k = classes.index(cls)
        w = want[cls]
        assert np.array_equal(rf[0][k], w["features0"]), (cls, "first features")
        for s in range(FORCED + 1):
            got, ws = ref_r[s][k], w["steps"][s]
            tag = (cls, s)
            for name in ("n_tracked", "n_good", "n_inliers", "n_peaks", "n_after_retrack"):
                assert int(got[name]) == ws[name], (tag, name, int(got[name]), ws[name])
            fl = int(got["flags"])
            assert bool(fl & 2) == ws["new_keyframe"] and bool(fl & 4) == ws["retrack"] and bool(fl & 8) == ws["retracked_on_device"], (tag, fl, ws)
            p = np.array(got["pose"])
            assert np.abs(p[:2] - ws["pose"][:2]).max() <= POS_TOL and abs(p[2] - ws["pose"][2]) <= ANG_TOL, (tag, p, ws["pose"])
            if s + 1 in ckpt:
                assert np.array_equal(rf[s + 1][k], ws["features"]), (tag, "features", len(rf[s + 1][k]), len(ws["features"]))
        wk = w["steps"][S - 1]["kf_locals"]
        assert kf[i].shape == wk.shape and np.abs(kf[i] - wk).max() <= 1e-4, (cls, "live keyframe after step", S, kf[i].shape, wk.shape)


if __name__ == "__main__":
    _child(int(sys.argv[1]), sys.argv[2], sys.argv[3])
