"""Host-side numbers of skimage.feature.blob_log (scikit-image 0.19.2) that the LoG kernels (csrc/log.hip) take from the caller:
the sigma list and scipy.ndimage's Gaussian weights, computed with NumPy exactly as the reference's stack computes them (libm's
exp and NumPy's need not agree to the last bit, so the device never evaluates them)."""
import numpy as np

TRUNCATE = 4.0          # scipy.ndimage.gaussian_filter1d's default


def blob_log_sigmas(min_sigma, max_sigma, num_sigma):
    """blob_log's sigma list for scalar sigmas: linspace(0, 1, num) * (max - min) + min.  (Not linspace(min, max, num), which
    blob_doh uses: the two differ in the last bit for e.g. (1, 30, 10).)"""
    scale = np.linspace(0, 1, num_sigma)
    return scale * (float(max_sigma) - float(min_sigma)) + float(min_sigma)


def gaussian_kernel1d(sigma, order, radius):
    """scipy.ndimage._filters._gaussian_kernel1d"""
    if order < 0:
        raise ValueError('order must be non-negative')
    exponent_range = np.arange(order + 1)
    sigma2 = sigma * sigma
    x = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / sigma2 * x ** 2)
    phi_x = phi_x / phi_x.sum()
    if order == 0:
        return phi_x
    q = np.zeros(order + 1)
    q[0] = 1
    D = np.diag(exponent_range[1:], 1)              # D @ q(x) = q'(x)
    P = np.diag(np.ones(order) / -sigma2, -1)       # P @ q(x) = q(x) * p'(x)
    Q_deriv = D + P
    for _ in range(order):
        q = Q_deriv.dot(q)
    q = (x[:, None] ** exponent_range).dot(q)
    return q * phi_x


def laplace_kernels(sigma):
    """-> (radius, k0, k2): the correlation weights gaussian_filter1d applies for orders 0 and 2 (kernel reversed, as scipy
    passes it to correlate1d), radius int(4 sigma + 0.5)"""
    radius = int(TRUNCATE * float(sigma) + 0.5)
    return (radius, np.ascontiguousarray(gaussian_kernel1d(sigma, 0, radius)[::-1]),
            np.ascontiguousarray(gaussian_kernel1d(sigma, 2, radius)[::-1]))
