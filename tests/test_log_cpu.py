"""CPU (-m "not gpu"): the host-side numbers of getBlobsFromCart(method="log") against the live scipy / scikit-image construct -
the NumPy model of tests/log_model.py against scipy.ndimage.gaussian_laplace, the product's weights and sigma list - and
roam_prune_blobs beyond the 32767 points / pairs of its 16-bit form against the oracle and a literal replay of _prune_blobs."""
import math

import numpy as np
import pytest

import log_model as M

SHAPES = [(3, 3), (7, 9), (33, 47), (64, 80)]
SIGMAS = [0.01, 0.5, 1, 5.005, 10, 30]


def test_model_equals_live_scipy_gaussian_laplace():
    from scipy import ndimage
    rng = np.random.default_rng(11)
    for sh in SHAPES:
        img = np.round(rng.random(sh) * 255) / 255
        for s in SIGMAS:
            assert np.array_equal(M.gaussian_laplace(img, s), ndimage.gaussian_laplace(img, [s, s])), (sh, s)
    assert np.array_equal(M.layers(img, M.sigma_list(1, 30, 10)), M.fast_layers(img, M.sigma_list(1, 30, 10)))


def test_weight_helper_equals_scipy_kernels():
    from scipy.ndimage import _filters
    from radarslampy_amd.gaussian import laplace_kernels
    for s in SIGMAS + list(M.sigma_list(1, 30, 10)) + list(M.sigma_list(0.01, 10, 3)):
        r, k0, k2 = laplace_kernels(np.float64(s))
        assert r == int(4.0 * float(s) + 0.5)
        assert np.array_equal(k0, _filters._gaussian_kernel1d(s, 0, r)[::-1]), s
        assert np.array_equal(k2, _filters._gaussian_kernel1d(s, 2, r)[::-1]), s
        assert np.array_equal(k0, k0[::-1]) and np.array_equal(k2, k2[::-1]), s     # the symmetric correlate1d path


def test_sigma_list_is_blob_logs():
    from radarslampy_amd.gaussian import blob_log_sigmas
    for a in [(1, 30, 10), (0.01, 10, 3), (1, 10, 3), (0.5, 7.3, 13), (2, 2, 1), (1, 30, 32)]:
        assert np.array_equal(blob_log_sigmas(*a), M.sigma_list(*a)), a
    assert (blob_log_sigmas(1, 30, 10) != np.linspace(1, 30, 10)).sum() == 7        # not blob_doh's linspace


def test_model_maxima_fast_path_and_trivial_cube():
    rng = np.random.default_rng(5)
    for sh, sig in [((33, 47), [0.01, 1, 2]), ((7, 9), [3.0]), ((64, 80), M.sigma_list(1, 30, 10))]:
        lay = M.layers(rng.random(sh), sig)
        a, b = M.maxima(lay, 0.0), M.fast_maxima(lay, 0.0)
        assert len(a[0]) > 0 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    lay = M.layers(np.full((9, 11), 0.3), [2.0])           # constant image, one sigma: trivial cube, no peaks
    assert len(M.maxima(lay, 0.0)[0]) == 0 and len(M.fast_maxima(lay, 0.0)[0]) == 0


def test_getblobs_refuses_dog_and_sequence_sigmas():
    from radarslampy_amd import getFeatures as gf
    img = np.zeros((16, 16), np.float32)
    with pytest.raises(NotImplementedError):
        gf.getBlobsFromCart(img, method="dog")
    with pytest.raises(NotImplementedError):
        gf.getBlobsFromCart(img, min_sigma=(1, 2), max_sigma=(3, 4), method="log")


def _real_log_candidates(golden, scan, params):
    """the candidates of a real scan in blob_log's order (response, stable), from the NumPy / scipy model"""
    import oracle
    g = golden("peaks")
    cart = oracle.convertPolarImageToCartesian(g[f"real{scan}_u8"].astype(np.float32) / 255.)
    mn, mx, num, thr = params
    sig = M.sigma_list(mn, mx, num)
    rcs, val = M.fast_maxima(M.fast_layers(cart, sig), thr)
    idx = np.argsort(-val, kind="stable")
    lm = rcs[idx].astype(np.float64)
    lm[:, -1] = sig[rcs[idx][:, -1]]
    return lm


def test_prune_beyond_16bit_limits_equals_oracle(golden):
    """47 261 candidates / ~1.1 M pairs: the 16-bit form returns ROAM_E_CAPACITY here, the wide one must equal the oracle"""
    import oracle
    from radarslampy_amd import getFeatures as gf
    lm = _real_log_candidates(golden, 0, (0.01, 10, 3, 5e-4))
    assert len(lm) > 32767
    got = gf._prune_blobs(lm, 0.5)
    assert np.array_equal(got, oracle.prune_blobs(lm, 0.5))
    assert len(got) < len(lm)


def test_prune_wide_equals_live_ckdtree_and_set_order(golden):
    """a crop of ~50 k pairs (more than the 16-bit form holds) with duplicate (row, col) blobs of different sigmas, against
    _prune_blobs executed on the live cKDTree.query_pairs set"""
    import oracle
    from scipy import spatial
    from radarslampy_amd import getFeatures as gf
    from test_oracle_reference_dump import _overlap
    lm = _real_log_candidates(golden, 0, (1, 10, 3, 0.01))
    b = lm[(lm[:, 0] >= 700) & (lm[:, 0] < 1000) & (lm[:, 1] >= 700) & (lm[:, 1] < 1300)]
    rng = np.random.default_rng(2)
    dup = b[rng.choice(len(b), 300, replace=False)].copy()
    dup[:, 2] = np.where(dup[:, 2] == 10.0, 1.0, 10.0)
    b = np.concatenate([b, dup])[np.argsort(rng.random(len(b) + len(dup)), kind="stable")]
    pairs = spatial.cKDTree(b[:, :2]).query_pairs(2 * b[:, 2].max() * math.sqrt(2))
    assert 40000 < len(pairs) < 80000, len(pairs)
    want = b.copy()
    for i, j in pairs:                              # the set's own iteration order
        b1, b2 = want[i], want[j]
        if _overlap(b1, b2) > 0.5:
            if b1[2] > b2[2]:
                b2[2] = 0
            else:
                b1[2] = 0
    got = gf._prune_blobs(b, 0.5)
    assert np.array_equal(got, want[want[:, 2] > 0])
    assert np.array_equal(got, oracle.prune_blobs(b, 0.5))
