"""Shared by the in-step motion prior's tests (tests/test_auto_prior_cpu.py without a GPU, tests/test_gpu_auto_prior.py with one): the
scan pairs the GPU test registers, the CPU chain on them with a perturbed rotation matrix, and a NumPy restatement of
fmtr_prior_kernel.  Everything is computed once per process and never modified.

The pairs: the three lanes of tests/test_gpu_engine_flow.py in the (1024, 400, 1027, 1) layout over five frames - lanes 0 and 1 step
forward (t - 1, t), lane 2 backwards (5 - t, 4 - t) - registered with clip_px = 0, downsample = 8, cart_downsample = 8 (R = 128, a
Cartesian side of 256), and the 8 degree pair of tests/klt_flow_cases.py in the Oxford layout with the defaults (1012 / 10 / 20).

Tolerances of the in-step pass against the blocking pass on the same pool pair.  Angle, scale and rotation response: the same kernels
on the same records, then exactly rounded IEEE operations in one order on both sides: equal bits.  dx, dy and the translation response
see the device's cos / sin in the rotation matrix where the blocking pass has the host's.  Accuracy relied on: HIP's published table
of device math functions gives 2 ulp for float64 sin and cos, glibc documents its own below 1 ulp, so the two differ by at most 3 ulp;
4 ulp is perturbed here.  perturbation_study() moves every entry of the forward matrix by +- 4 ulp (one entry at a time, and all six
together), and also cos and sin themselves by +- 4 ulp before the matrix is made (the translation entries multiply them by the centre,
which is more than 4 ulp of those entries), and counts the 1/32-px source coordinates of rotateImg that change.  Measured: none on any
pair, so the turned images are the blocking pass's bit for bit and the bound is the phase correlation's own (tests/fmt_register_cases.py:
6.6e-11 px, 4.0e-12 relative)."""
import math

import numpy as np

import fmt_register_cases as frc
import warp_affine_model as wam

SMALL = dict(clip_px=0, downsample=8, cart_downsample=8)
OXFORD = dict(clip_px=1012, downsample=10, cart_downsample=20)
ULPS = 4
TOL_PX = frc.PC_TOL_PX
TOL_RESPONSE_REL = frc.PC_TOL_RESPONSE_REL
KLT_MAX_GUESS = float(1 << 20)
PRIOR_MAX_LINEAR = 64.0
_cache = {}


def small_steps(frames):
    """-> per step t = 1 .. frames - 1 the (prev, curr) pool indices of the three lanes"""
    return [((t - 1, t - 1, frames - t), (t, t, frames - 1 - t)) for t in range(1, frames)]


def pairs():
    """-> [(name, src polar, tgt polar, parameters)]: every distinct pair the GPU test registers"""
    if "pairs" not in _cache:
        import klt_flow_cases as K
        import test_gpu_engine_flow as EF
        clip, rows, stride, off = EF.LAYOUT
        recs = EF._inputs()[0]
        pol = [r[:, off:off + clip].astype(np.float32) / np.float32(255.) for r in recs]
        out, seen = [], set()
        for prev, curr in small_steps(EF.FRAMES):
            for a, b in zip(prev, curr):
                if (a, b) not in seen:
                    seen.add((a, b))
                    out.append((f"small {a}->{b}", pol[a], pol[b], SMALL))
        r = K.rotation_pair()
        out.append(("oxford 8 deg", K.polar(r["recs"][0]), K.polar(r["recs"][1]), OXFORD))
        _cache["pairs"] = out
    return _cache["pairs"]


def _ulp_step(v, k):
    for _ in range(abs(k)):
        v = np.nextafter(v, np.inf if k > 0 else -np.inf)
    return float(v)


def perturbation_study():
    """-> [(name, variants tried, coordinates that changed, largest |change of dx or dy| px, largest relative change of the response)]"""
    if "study" not in _cache:
        import oracle
        out = []
        for name, src, tgt, p in pairs():
            r = frc.cpu_chain(src, tgt, p["clip_px"], p["downsample"], p["cart_downsample"])
            S = r["src_cart"].shape[0]
            angle, dx, dy, resp = r["out6"][0], r["out6"][3], r["out6"][4], r["out6"][5]
            c = float(np.float32(S / 2))
            rad = math.degrees(angle) * math.pi / 180.0
            base = wam.rotation_matrix_2d((S / 2, S / 2), math.degrees(angle), 1.0).ravel()
            X0, Y0 = wam.fixed_coords(wam.invert_affine(base), S, S)
            variants = []
            for k in (-ULPS, ULPS):
                for i in range(6):
                    m = base.copy()
                    m[i] = _ulp_step(m[i], k)
                    variants.append(m)
                variants.append(np.array([_ulp_step(v, k) for v in base]))
                for ka, kb in ((k, 0), (0, k), (k, k), (k, -k)):
                    a, b = _ulp_step(math.cos(rad), ka), _ulp_step(math.sin(rad), kb)
                    variants.append(np.array([a, b, (1 - a) * c - b * c, -b, a, b * c + (1 - a) * c]))
            flips, dpx, drel = 0, 0.0, 0.0
            for m in variants:
                X, Y = wam.fixed_coords(wam.invert_affine(m), S, S)
                n = int(np.count_nonzero(X != X0) + np.count_nonzero(Y != Y0))
                flips += n
                if n:
                    (x, y), s = oracle.phaseCorrelate(wam.remap_fixed(r["src_cart"], X, Y), r["tgt_cart"])
                    dpx = max(dpx, abs(float(x) - dx), abs(float(y) - dy))
                    drel = max(drel, abs(float(s) - resp) / abs(resp))
            out.append((name, len(variants), flips, dpx, drel))
        _cache["study"] = out
    return _cache["study"]


def prior_model(angle, dx, dy, rot_response, trans_response, cols, cart_downsample, min_rot=0.0, min_trans=0.0, shifts=(0.0, 0.0),
                cos=math.cos, sin=math.sin):
    """fmtr_prior_kernel for a lane that has a pair, operation by operation -> (affine (6,) float32, use): float64 throughout, the
    centre (Rc, Rc) as float32, one rounding to float32 per entry; the gate and roam_engine_set_motion_prior's limits"""
    r_reg, r_trk = cols // cart_downsample, cols // 2
    c, s = float(np.float32(r_reg)), r_trk / r_reg
    with np.errstate(all="ignore"):
        deg = np.float64(angle) * (180.0 / math.pi)
        rad = float(deg * math.pi / 180.0)
        a, b = (cos(rad), sin(rad)) if math.isfinite(rad) else (math.nan, math.nan)
        M = np.array([a, b, (1 - a) * c - b * c, -b, a, b * c + (1 - a) * c], np.float64)
        M[2] = s * (M[2] + np.float64(dx))
        M[5] = s * (M[5] + np.float64(dy))
        f = M.astype(np.float32)
    use = bool(rot_response >= min_rot and trans_response >= min_trans)
    use = use and all(math.isfinite(float(v)) for v in (shifts[0], shifts[1], rot_response, angle, dx, dy, trans_response))
    for k in range(6):
        use = use and bool(abs(f[k]) <= (KLT_MAX_GUESS if k % 3 == 2 else PRIOR_MAX_LINEAR))
    return f, use
