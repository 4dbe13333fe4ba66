"""GPU (-m gpu): getBlobsFromCart(method="log") - the Laplacian-of-Gaussian layers and their 3x3x3 maxima (log.hip) against the
model of tests/log_model.py (bit-identical to scipy.ndimage, test_log_cpu.py), on the two real scans of tests/golden/peaks.npz at
three parameter sets, f32 and f64 input; then the whole stage (host prune) and getFeatures (SSC-ANMS) against the oracle."""
import ctypes as C

import numpy as np
import pytest

import log_model as M
import oracle

pytestmark = pytest.mark.gpu

PARAMS = [(0.01, 10, 3, 5e-4), (1, 10, 3, 0.01), (1, 30, 10, 0.01)]


@pytest.fixture(scope="module")
def ctx():
    from radarslampy_amd import _ffi
    c = _ffi.Context(0)
    assert "gfx950" in c.device_info()["arch"]
    yield c
    c.close()


@pytest.fixture(scope="module")
def carts(golden):
    g = golden("peaks")
    return [oracle.convertPolarImageToCartesian(g[f"real{i}_u8"].astype(np.float32) / 255.) for i in (0, 1)]


_model_cache = {}


def _model(carts, scan, p):
    if (scan, p) not in _model_cache:
        sig = M.sigma_list(*p[:3])
        lay = M.fast_layers(carts[scan], sig)
        _model_cache[(scan, p)] = (sig, lay) + M.fast_maxima(lay, p[3])
    return _model_cache[(scan, p)]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("p", PARAMS)
def test_layers_and_maxima_real_scans(ctx, carts, p):
    for scan in (0, 1):
        sig, lay, rcs, val = _model(carts, scan, p)
        for img in (carts[scan], carts[scan].astype(np.float64)):
            grcs, gval, glay = ctx.log_maxima(img, sig, p[3], want_layers=True)
            assert np.array_equal(glay, lay), (scan, p, img.dtype)
            assert np.array_equal(grcs, rcs) and np.array_equal(gval, val), (scan, p, img.dtype, len(grcs), len(rcs))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("p", PARAMS)
def test_getblobs_and_getfeatures_log(carts, p):
    from radarslampy_amd import getFeatures as gf
    params = dict(min_sigma=p[0], max_sigma=p[1], num_sigma=p[2], threshold=p[3], method="log")
    for scan in (0, 1):
        sig, _, rcs, val = _model(carts, scan, p)
        want = M.blobs(rcs, val, sig)
        got = gf.getBlobsFromCart(carts[scan], **params)
        assert np.array_equal(got, want), (scan, p, len(got), len(want))
        coords, sigmas = gf.getFeatures(carts[scan], params)
        kp = oracle.adaptiveNMS(carts[scan].shape, want)
        assert np.array_equal(coords, np.fliplr(kp[:, :2])) and np.array_equal(sigmas, kp[:, 2]), (scan, p)


@pytest.mark.timeout(120)
def test_edge_cases(ctx):
    rng = np.random.default_rng(4)
    cases = [(rng.random((33, 47)), [10.0, 30.0], 0.0),            # radius 40 / 120: reflected more than once
             (rng.random((3, 3)), [0.01, 1.0, 5.0], 0.0),
             (rng.random((7, 9)).astype(np.float32), [2.0], 0.0),   # num_sigma = 1
             (rng.random((64, 80)), M.sigma_list(1, 30, 12), 0.01),  # num_sigma >= 10
             (rng.random((40, 300)), M.sigma_list(0.5, 4, 32), 0.0)]
    for img, sig, thr in cases:
        lay = M.layers(img, sig)
        rcs, val = M.maxima(lay, thr)
        grcs, gval, glay = ctx.log_maxima(img, sig, thr, want_layers=True)
        assert np.array_equal(glay, lay), (img.shape, sig)
        assert len(rcs) > 0 and np.array_equal(grcs, rcs) and np.array_equal(gval, val), (img.shape, sig)
    # constant image, one sigma: a trivial cube has no peaks (without the rule every pixel would be one)
    grcs, _ = ctx.log_maxima(np.full((20, 30), 0.25), [2.0], 0.0)
    assert len(grcs) == 0
    # capacity: the true count comes back with ROAM_E_CAPACITY, and the wrapper's retry returns everything
    from radarslampy_amd import _ffi
    from radarslampy_amd.gaussian import laplace_kernels
    img, sig = rng.random((64, 80)), [1.0, 2.0]
    rcs, val = M.maxima(M.layers(img, sig), 0.0)
    ks = [laplace_kernels(s) for s in sig]
    radius = np.array([k[0] for k in ks], np.int32)
    kernels = np.concatenate([np.concatenate([k0, k2]) for _, k0, k2 in ks])
    scale = np.array([s * s for s in sig])
    out_rcs, out_val, n = np.empty((5, 3), np.int32), np.empty(5), C.c_int32(0)
    rc = ctx.lib.roam_log_maxima(ctx.h, _ffi._ptr(img), 8, 80, 64, 2, _ffi._ptr(radius), _ffi._ptr(kernels), _ffi._ptr(scale), 0.0,
                                 _ffi._ptr(out_rcs), _ffi._ptr(out_val), 5, C.byref(n), None)
    assert rc == _ffi.ROAM_E_CAPACITY and n.value == len(rcs) > 5
    assert np.array_equal(out_rcs, rcs[:5]) and np.array_equal(out_val, val[:5])
    grcs, gval = ctx.log_maxima(img, sig, 0.0, cap=5)
    assert np.array_equal(grcs, rcs) and np.array_equal(gval, val)
