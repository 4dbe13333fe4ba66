#!/usr/bin/env python3
"""Generator of tests/golden/backend_edges.npz.  RUNS ONLY IN THE BUILD CONTAINER (like make_goldens.py, whose import stubs it
shares): the reference's ANMS.ssc and getTransformKLT.calculateTransformSVD on the reference-pinned subsets of
tests/backend_edge_cases.py.

Stored per case: its name, the reference's output (selected indices, all cases end to end with their offsets; R, h) and a SHA-256
of the input it was given - the tests recompute the hash from the seeded module, the inputs themselves are not stored.  Nothing of
the reference's source travels: only arrays.  The file is written without timestamps, so that a second run gives the same bytes."""
import os
import sys
import zipfile

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.dirname(OUT))
from make_goldens import REF, _install_stubs, quiet  # noqa: E402
import backend_edge_cases as bc  # noqa: E402


def save_deterministic(path, arrays):
    """an .npz (np.load reads it) whose bytes depend on the arrays alone: fixed entry dates, sorted names"""
    import io
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    _install_stubs()
    sys.path.insert(0, REF)
    os.chdir(REF)
    with quiet():
        import ANMS as r_anms
        import getTransformKLT as r_klt
    names, hashes, sels = [], [], []
    for case in bc.ssc_cases():
        if not bc.ssc_reference_pinned(case):
            continue
        name, kp, num_ret, tol, cols, rows = case
        sel = r_anms.ssc(kp, num_ret, tol, cols, rows)
        # the reference returns the selected ROWS; its result list is in input order, so the indices follow by walking kp once
        # (identical keypoints: the first unused one, which is the one a greedy pass in input order accepts)
        idx, j = [], 0
        for row in sel:
            while not np.array_equal(kp[j], row):
                j += 1
            idx.append(j)
            j += 1
        names.append(name); hashes.append(bytes.fromhex(bc.sha(kp))); sels.append(np.asarray(idx, np.int32))
    n_ssc = len(names)
    assert n_ssc >= 60, n_ssc
    out = dict(ssc_names=np.array(names), ssc_sha=np.frombuffer(b"".join(hashes), np.uint8).reshape(-1, 32),
               ssc_sel=np.concatenate(sels), ssc_off=np.cumsum([0] + [len(v) for v in sels]).astype(np.int32))
    names, hashes, Rs, hs = [], [], [], []
    for name, s, t in bc.kabsch_cases()[0]:
        if len(s) > 4097:
            continue
        with quiet():
            R, h = r_klt.calculateTransformSVD(s, t)
        names.append(name); hashes.append(bytes.fromhex(bc.sha(s, t)))
        Rs.append(np.asarray(R, np.float64)); hs.append(np.asarray(h, np.float64))
    n_kab = len(names)
    out.update(kabsch_names=np.array(names), kabsch_sha=np.frombuffer(b"".join(hashes), np.uint8).reshape(-1, 32),
               kabsch_R=np.stack(Rs), kabsch_h=np.stack(hs))
    path = os.path.join(OUT, "backend_edges.npz")
    save_deterministic(path, out)
    print("backend_edges.npz", os.path.getsize(path), "bytes,", n_ssc, "SSC cases,", n_kab, "Kabsch cases")


if __name__ == "__main__":
    main()
