"""Build libroam_hip.so in-tree (radarslampy_amd/csrc/libroam_hip.so) with hipcc for gfx950.

hipcc cross-compiles without a GPU, so this runs in the build container and the .so
travels with the snapshot to the GPU box."""
import concurrent.futures as cf
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(CSRC, "libroam_hip.so")
ARCH = "gfx950"
FLAGS = ["-O3", f"--offload-arch={ARCH}", "-fPIC", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
         "-Wall", "-Wno-unused-function", "-Wno-unused-variable", "-Wno-unused-but-set-variable"]
# per-file additions.  retrack_det.hip: its determinant kernel lives on 8-byte LDS reads, and the backend's load/store optimizer pairs them
# into ds_read2_b64, which moves 8 bytes per lane at HALF the rate of ds_read_b64 on gfx950 (128 against 256 B/clk per CU).
# The other three retrack units were one file with it and keep the flags because their machine code is not the same without them
# (device assembly compared kernel by kernel): retrack_integral.hip - rt_integral_kernel, rt_integ_cols_kernel, rt_integ_rows_kernel (328
# instead of 324 registers), rt_boxtab_kernel; retrack_blobs.hip - rt_emit_kernel, rt_blobs_kernel<true/false>, rt_book_kernel;
# retrack.hip - rt_collect_kernel, rt_append_kernel.  Whether the paired form is any slower there has not been measured.
NO_PAIRING = ["-Xclang", "-target-feature", "-Xclang", "-load-store-opt", "-mllvm", "-amdgpu-load-store-vectorizer=0"]
EXTRA = {f: NO_PAIRING for f in ("retrack.hip", "retrack_integral.hip", "retrack_det.hip", "retrack_blobs.hip")}


def fingerprint(sources):
    """hash of what decides a kernel's machine code: the named translation units, every header of csrc/, and this file's flags.
    The PMC records under profiles/ carry it (taken when the counters are MEASURED) and bench.py reports their traffic figures only
    while it still matches."""
    import hashlib
    h = hashlib.sha256()
    files = [os.path.join(CSRC, f) for f in sorted(sources)] + [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".inc"))]
    for f in files:
        h.update(os.path.basename(f).encode() + b"\0" + open(f, "rb").read())
    h.update(repr((FLAGS, sorted((k, v) for k, v in EXTRA.items() if k in sources))).encode())
    return h.hexdigest()[:16]


def _sources():
    return sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))


def _stale(out, deps):
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps)


def build(force: bool = False, verbose: bool = False) -> str:
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    hdrs = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".inc"))] + [os.path.join(HERE, "..", "include", "roam_abi.h")]
    objs, jobs = [], []
    for s in _sources():
        src = os.path.join(CSRC, s)
        obj = os.path.join(CSRC, s[:-4] + ".o")
        objs.append(obj)
        if force or _stale(obj, [src, os.path.abspath(__file__)] + hdrs):
            jobs.append([hipcc] + FLAGS + EXTRA.get(s, []) + ["-c", src, "-o", obj])

    def run(cmd):
        r = subprocess.run(cmd, capture_output=True, text=True)
        return cmd, r

    with cf.ThreadPoolExecutor(max_workers=min(6, max(1, len(jobs)))) as ex:
        for cmd, r in ex.map(run, jobs):
            if verbose or r.returncode != 0:
                sys.stderr.write(" ".join(cmd) + "\n" + r.stdout + r.stderr)
            if r.returncode != 0:
                raise RuntimeError("hipcc failed: " + " ".join(cmd))
    if force or jobs or _stale(LIB, objs):
        cmd = [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", LIB] + objs + ["-ldl", "-lz"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise RuntimeError("link failed")
    return LIB


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--fingerprint":
        print(fingerprint(sys.argv[2:]))
    else:
        print(build(force="--force" in sys.argv, verbose=True))
