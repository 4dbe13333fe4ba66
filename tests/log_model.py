"""NumPy model of the image-scale part of skimage.feature.blob_log (scikit-image 0.19.2) as getFeatures.getBlobsFromCart calls
it with method="log": sigma list, layers -gaussian_laplace(img, s) * s**2 (scipy.ndimage arithmetic restated term for term), and
the 3x3x3 maxima of peak_local_max.  `fast_*` compute the same numbers with scipy.ndimage itself (the test_log_cpu tests hold the
two equal bit for bit); the GPU tests use them on whole scans, where the NumPy restatement would take minutes."""
import numpy as np


def sigma_list(min_sigma, max_sigma, num_sigma):
    """blob_log, log_scale=False, scalar sigmas: the first of the (identical) per-axis columns"""
    min_s = np.full(2, min_sigma, dtype=float)
    max_s = np.full(2, max_sigma, dtype=float)
    scale = np.linspace(0, 1, num_sigma)[:, np.newaxis]
    return (scale * (max_s - min_s) + min_s)[:, 0]


def reflect_index(k, n):
    """scipy.ndimage mode 'reflect' (d c b a | a b c d | d c b a), repeated for any distance"""
    m = np.mod(k, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def kernel1d(sigma, order, radius):
    """scipy.ndimage._filters._gaussian_kernel1d restated"""
    exponent_range = np.arange(order + 1)
    sigma2 = sigma * sigma
    x = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / sigma2 * x ** 2)
    phi_x = phi_x / phi_x.sum()
    if order == 0:
        return phi_x
    q = np.zeros(order + 1)
    q[0] = 1
    Q_deriv = np.diag(exponent_range[1:], 1) + np.diag(np.ones(order) / -sigma2, -1)
    for _ in range(order):
        q = Q_deriv.dot(q)
    return (x[:, None] ** exponent_range).dot(q) * phi_x


def correlate1d_sym(x, w, axis):
    """NI_Correlate1D's symmetric path: t = x[i] w[r]; for j = r..1: t += (x[i-j] + x[i+j]) w[r-j]"""
    r = len(w) // 2
    assert np.array_equal(w, w[::-1])
    xm = np.moveaxis(x, axis, -1)
    n = xm.shape[-1]
    i = np.arange(n)
    t = xm * w[r]
    for j in range(r, 0, -1):
        t = t + (xm[..., reflect_index(i - j, n)] + xm[..., reflect_index(i + j, n)]) * w[r - j]
    return np.moveaxis(t, -1, axis)


def gaussian_laplace(img, sigma):
    """scipy.ndimage.gaussian_laplace(img, sigma) for a float64 2-D image and a scalar sigma"""
    radius = int(4.0 * float(sigma) + 0.5)
    k0, k2 = kernel1d(sigma, 0, radius)[::-1], kernel1d(sigma, 2, radius)[::-1]
    a = correlate1d_sym(correlate1d_sym(img, k2, 0), k0, 1)
    b = correlate1d_sym(correlate1d_sym(img, k0, 0), k2, 1)
    return a + b


def layers(img, sigmas):
    """(num_sigma, h, w): -gaussian_laplace(img, s) * mean([s, s]) ** 2"""
    img = np.asarray(img, np.float64)
    return np.stack([-gaussian_laplace(img, s) * np.mean([s, s]) ** 2 for s in sigmas])


def fast_layers(img, sigmas):
    from scipy import ndimage
    img = np.asarray(img, np.float64)
    return np.stack([-ndimage.gaussian_laplace(img, [s, s]) * np.mean([s, s]) ** 2 for s in sigmas])


def _peak_mask(cube, image_max, threshold):
    out = cube == image_max
    if cube.size == 1:
        return cube > threshold
    if np.all(out):                                 # a trivial image has no peaks
        out[:] = False
    return out & (cube > threshold)


def maxima(lay, threshold):
    """peak_local_max(stack(layers, -1), threshold_abs=threshold, footprint=ones((3,3,3)), threshold_rel=0, exclude_border=False)
    before its sort: (rcs (n,3) int32 [row, col, sigma_index] in C order, values (n,) f64)"""
    cube = np.moveaxis(lay, 0, -1)
    p = np.pad(cube, 1, mode="constant", constant_values=0.0)
    h, w, s = cube.shape
    m = np.full(cube.shape, -np.inf)
    for dr in range(3):
        for dc in range(3):
            for ds in range(3):
                m = np.maximum(m, p[dr:dr + h, dc:dc + w, ds:ds + s])
    thr = max(threshold, 0.0 * cube.max())
    idx = np.nonzero(_peak_mask(cube, m, thr))
    return np.transpose(idx).astype(np.int32), cube[idx]


def fast_maxima(lay, threshold):
    from scipy import ndimage
    cube = np.moveaxis(lay, 0, -1)
    m = ndimage.maximum_filter(cube, footprint=np.ones((3, 3, 3)), mode="constant")
    thr = max(threshold, 0.0 * cube.max())
    idx = np.nonzero(_peak_mask(cube, m, thr))
    return np.transpose(idx).astype(np.int32), cube[idx]


def blobs(rcs, val, sigmas, overlap=0.5):
    """response order (stable, as the product's DoH path), sigma lookup, oracle prune"""
    import oracle
    if len(rcs) == 0:
        return np.empty((0, 3))
    idx = np.argsort(-val, kind="stable")
    lm = rcs[idx].astype(np.float64)
    lm[:, -1] = np.asarray(sigmas)[rcs[idx][:, -1]]
    return oracle.prune_blobs(lm, overlap)
