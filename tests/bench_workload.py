"""The benchmark's workload as a test helper: what bench.py::_run_rank does on rank 0 of a plain run (no --h2d, --no-retrack or
--endless), restated so that a test can drive an engine through the same steps and follow any one lane on the CPU oracle.

The constants come from bench itself (WORK_RETRACK, the defaults of parse_args); only the inline parts of _run_rank are restated here,
each with the bench line it follows.  A lane's whole history is set by its CLASS (sequence, phase): lanes of one class see the same
records, start on the same frame and restart at the same steps."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench                                                 # noqa: E402  (no side effects: main() runs under __main__ only)

STEP_NEW_SEQUENCE = 0x40000000                               # roam_abi.h ROAM_STEP_NEW_SEQUENCE (= _ffi.STEP_NEW_SEQUENCE; no HIP import here)
WORK = bench.WORK_RETRACK
_DEFAULTS = bench.parse_args([])
FRAMES, DISTINCT, LANES = _DEFAULTS.frames, _DEFAULTS.distinct, _DEFAULTS.lanes


def seeds(D=DISTINCT, rank=0):
    # bench.py:327  render_sequences([1000 * rank + 17 * d + 5 for d in range(Dn_)], ...)
    return [1000 * rank + 17 * d + 5 for d in range(D)]


def cycle(T=FRAMES):
    # bench.py:375-376  period = 2 * T - 2; cyc_full = 0, 1, .., T-1, T-2, .., 1
    return list(range(T)) + list(range(T - 2, 0, -1)), 2 * T - 2


def phases(B, D=DISTINCT, T=FRAMES):
    # bench.py:390  en.phase = (b // Dn) % period
    _, period = cycle(T)
    return (np.arange(B) // D) % period


def lane_class(b, D=DISTINCT, T=FRAMES):
    """(sequence, phase) of lane b: the lane plays sequence b % D (bench.py:387, its records are copies of that original), from
    phase (b // D) % period of the ping-pong cycle (bench.py:390)"""
    _, period = cycle(T)
    return b % D, (b // D) % period


def first_frames(B, D=DISTINCT, T=FRAMES):
    """(pool index, frame) of every lane's init_lanes_detect: bench.py:391 t0s = cyc_full[phase[b]], bench.py:397 pool b * T + t0"""
    cyc, _ = cycle(T)
    t0 = np.array([cyc[p] for p in phases(B, D, T)])
    return np.arange(B) * T + t0, t0


def copies(B, D=DISTINCT, T=FRAMES):
    """(dst, src) of the private record copies: bench.py:381-387, lanes 0..D-1 hold the originals d * T + t, lane b >= D gets
    copy_scan(b * T + t, (b % D) * T + t)"""
    return [(b * T + t, (b % D) * T + t) for b in range(D, B) for t in range(T)]


def scan_indices(B, D=DISTINCT, T=FRAMES, step=0):
    """the int32 scan indices of bench's step `step` (0-based): bench.py:413-415, ph = (phase + step + 1) % period, index
    b * T + cyc_full[ph], OR'd with STEP_NEW_SEQUENCE where ph == 0 (bench.py:408, 414)"""
    cyc, period = cycle(T)
    ph = (phases(B, D, T) + step + 1) % period
    idx = np.arange(B) * T + np.array(cyc)[ph]
    return (idx | np.where(ph == 0, STEP_NEW_SEQUENCE, 0)).astype(np.int32)


def class_frames(cls, steps, T=FRAMES):
    """frames of class cls = (sequence, phase): (first frame, [frame of step 0 .. steps - 1], [restart flag of each step]) - what
    scan_indices gives every lane of the class, in the sequence's own frame numbers"""
    _, p = cls
    cyc, period = cycle(T)
    ph = [(p + s + 1) % period for s in range(steps)]
    return cyc[p], [cyc[q] for q in ph], [q == 0 for q in ph]


def all_classes(D=DISTINCT, T=FRAMES):
    _, period = cycle(T)
    return [(d, p) for p in range(period) for d in range(D)]


def oracle_subset(D=DISTINCT, T=FRAMES):
    """the classes the GPU test follows on the oracle: (d, d % period), one per sequence, every phase at least once"""
    _, period = cycle(T)
    return [(d, d % period) for d in range(D)]


# ------------------------------------------------------------------------------------------------ CPU work (spawn-pool workers)
def render(seed, T=FRAMES):
    """one of bench's sequences: bench.py:240-243 with md on (bench.py:327 `not args.no_md`) and the retrack workload"""
    from radarslampy_amd import synth
    return synth.make_sequence(seed, T, distortion=True, **WORK)


def oracle_class(job):
    """render the class's sequence and run it on the oracle's loop body for `steps` steps, the last one a forced detection
    (set_retrack(2): every lane appends getFeatures of the scan to what it tracked).  Returns the records, the ground-truth poses and,
    per step, the oracle's fields, the features after it and the live keyframe's pruned undistorted locals."""
    (d, p), seed, steps, T = job
    import oracle
    recs, poses, _ = render(seed, T)
    det = lambda cart: oracle.getFeatures(cart)[0]                     # noqa: E731
    t0, frames, restarts = class_frames((d, p), steps, T)
    cart0 = oracle.convertPolarImageToCartesian(recs[t0][:, 11:11 + 2025].astype(np.float32) / np.float32(255.))
    feat0 = oracle.append_dedupe(np.empty((0, 2)), det(cart0))
    pipe = oracle.OdometryPipeline(recs[t0], feat0, poses[t0], detect=det)
    out = dict(features0=np.ascontiguousarray(feat0, np.float32), steps=[])
    for s, (f, rs) in enumerate(zip(frames, restarts)):
        forced = s == steps - 1
        if rs:
            pipe.blobCoord = np.empty((0, 2), np.float32)               # a new sequence starts with no features (bench.py:232-233)
        w = pipe.step(recs[f])
        if forced and not w["retrack"]:
            cart = pipe.warp(recs[f][:, pipe.off:pipe.off + pipe.clip].astype(np.float32) / 255.)[0]
            pipe.blobCoord = np.ascontiguousarray(oracle.append_dedupe(pipe.blobCoord, det(cart)), np.float32)
        detected = bool(w["retrack"]) or forced
        out["steps"].append(dict(
            n_tracked=w["n_tracked"], n_good=w["n_good"], n_inliers=w["n_inliers"], n_peaks=w["n_peaks"], retrack=bool(w["retrack"]),
            retracked_on_device=detected, new_keyframe=bool(w["new_keyframe"]), n_after_retrack=len(pipe.blobCoord) if detected else 0,
            pose=np.asarray(w["pose"], np.float64), features=pipe.blobCoord.copy(),
            kf_locals=None if forced else pipe.old_kf.prunedUndistortedLocals.copy()))
    return recs, poses, out
