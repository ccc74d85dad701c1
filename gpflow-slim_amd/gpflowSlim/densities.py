"""Log-densities.

Mirrors gpflowSlim/densities.py: gaussian :24-25, bernoulli / poisson / exponential / student_t :33-70 (what the
likelihoods' logp are made of; numpy on the host), lognormal / gamma / beta / laplace (what gpflowSlim.priors is made of),
multivariate_normal :73-95.  The triangular
solve of multivariate_normal runs on the GPU (csrc: recursive trsm); the scalar reductions of
an [N, R] host array stay on the host.
"""
import numpy as np
from scipy.special import gammaln

from . import _backend as be


def gaussian(x, mu, var):
    """densities.py:24-25"""
    return -0.5 * (np.log(2 * np.pi) + np.log(var) + np.square(mu - x) / var)


def bernoulli(p, y):
    """densities.py:33-34"""
    return np.log(np.where(np.equal(y, 1), p, 1 - p))


def poisson(lamb, y):
    """densities.py:37-38"""
    return y * np.log(lamb) - lamb - gammaln(y + 1.)


def exponential(lamb, y):
    """densities.py:41-42"""
    return - y / lamb - np.log(lamb)


def student_t(x, mean, scale, deg_free):
    """densities.py:50-60"""
    const = gammaln((deg_free + 1.) * 0.5) - gammaln(deg_free * 0.5) \
        - 0.5 * (np.log(np.square(scale)) + np.log(deg_free) + np.log(np.pi))
    return const - 0.5 * (deg_free + 1.) * \
        np.log(1. + (1. / deg_free) * (np.square((x - mean) / scale)))


def lognormal(x, mu, var):
    """densities.py:28-30"""
    lnx = np.log(x)
    return gaussian(lnx, mu, var) - lnx


def gamma(shape, scale, x):
    """densities.py:45-47"""
    return -shape * np.log(scale) - gammaln(shape) + (shape - 1.) * np.log(x) - x / scale


def beta(alpha, beta, y):
    """densities.py:60-66 (y clipped to [1e-6, 1 - 1e-6] as there)"""
    y = np.clip(y, 1e-6, 1 - 1e-6)
    return (alpha - 1.) * np.log(y) + (beta - 1.) * np.log(1. - y) + gammaln(alpha + beta) - gammaln(alpha) - gammaln(beta)


def laplace(mu, sigma, y):
    """densities.py:69-70"""
    return -np.abs(mu - y) / sigma - np.log(2. * sigma)


def multivariate_normal(x, mu, L):
    """densities.py:73-95.  L is the Cholesky factor of the covariance; x, mu vectors or [N, R]
    matrices (columns independent)."""
    x = np.asarray(x, dtype=np.float64)
    d = x - mu
    alpha = be.get_handle().trsm_lower(L, d, trans=False)
    num_col = 1 if x.ndim == 1 else x.shape[1]
    num_dims = x.shape[0]
    ret = -0.5 * num_dims * num_col * np.log(2 * np.pi)
    ret += -num_col * np.sum(np.log(np.diag(L)))
    ret += -0.5 * np.sum(np.square(alpha))
    return ret


def multivariate_normal_feature(x, mu, C, var):
    """densities.py:98-124: log N(x; mu, C C^T + var I) for a host matrix of features C [N, F] in O(N F^2), columns of x
    independent.  The Gram matrix, its factor and the solves run on the device (csrc/gps_rff.hip, the feature map being the
    identity on C).  Two deliberate differences from the reference: it adds settings.jitter to diag(L) inside the logarithm
    (a shift of about 2 sum 1e-6 / L_ii away from the density it names), which is left out here; and it leaves out the
    number of columns R on the log-determinant and on N log 2 pi, which is kept here, so that the value equals
    ``multivariate_normal`` on the factor of C C^T + var I for every R (at R = 1: the reference's value without its 1e-6)."""
    x = np.asarray(x, dtype=np.float64)
    d = x - mu
    if d.ndim == 1:
        d = d[:, None]
    C = np.ascontiguousarray(C, dtype=np.float64)
    desc, keep = be.make_rff(be.RFF_EXPLICIT, C.shape[1], C.shape[1])
    return be.get_handle().rff_lml(desc, C, float(np.squeeze(var)), np.ascontiguousarray(d))
