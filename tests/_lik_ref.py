"""CPU restatement (numpy / scipy) of the reference's non-Gaussian likelihoods, for the tests of gpflowSlim.likelihoods and of
the device kernels (csrc/lik.hip).  Line numbers: gpflowSlim/likelihoods.py and gpflowSlim/densities.py of the reference.

Everything takes the number of Gauss-Hermite nodes as an argument (the reference's default is 20, :34), so that the
restatement itself can be pinned at many nodes against closed forms, mpmath integrals and Monte-Carlo (tests/test_lik_cpu.py).
Kinds: "bernoulli" (probit link), "poisson" (exp link, params: binsize), "exponential" (exp link), "student_t" (params:
scale, deg_free), "multiclass" (RobustMax, params: epsilon), "gaussian" (params: variance; :186-188).

Also: analytic derivatives of the variational expectations in (mu, var, first parameter) -- what autodiff through :121-152
and :404-425 yields, pinned against central differences in test_lik_cpu.py -- and the SVGP bound
scale * sum var_exp - KL (models/svgp.py:108-125) composed with oracle/gp_oracle.py's conditional and gauss_kl.
"""
import os
import sys

import numpy as np
from scipy.special import erf, gammaln

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import oracle.gp_oracle as orc  # noqa: E402

KINDS = ("bernoulli", "poisson", "exponential", "student_t", "multiclass")
KIND_ID = {"gaussian": 0, "bernoulli": 1, "poisson": 2, "exponential": 3, "student_t": 4, "multiclass": 5}
_INV_S2PI = 1.0 / np.sqrt(2.0 * np.pi)


def gh(n_gh=20):
    """quadrature.hermgauss; weights normalised as :142"""
    x, w = np.polynomial.hermite.hermgauss(n_gh)
    return x, w / np.sqrt(np.pi)


def probit(x):
    """:269-270"""
    return 0.5 * (1.0 + erf(x / np.sqrt(2.0))) * (1 - 2e-3) + 1e-3


def student_const(scale, nu):
    """densities.py:51-55"""
    return gammaln((nu + 1.) * 0.5) - gammaln(nu * 0.5) - 0.5 * (np.log(np.square(scale)) + np.log(nu) + np.log(np.pi))


def logp(kind, params, F, Y):
    """log p(y | f) of the elementwise kinds"""
    if kind == "bernoulli":                                   # densities.py:33-34 through :278
        p = probit(F)
        return np.log(np.where(np.equal(Y, 1), p, 1 - p))
    if kind == "poisson":                                     # densities.py:37-38 through :213
        lamb = np.exp(F) * params[0]
        return Y * np.log(lamb) - lamb - gammaln(Y + 1.)
    if kind == "exponential":                                 # densities.py:41-42 through :231
        lamb = np.exp(F)
        return -Y / lamb - np.log(lamb)
    if kind == "student_t":                                   # densities.py:50-60 through :259
        s, nu = params
        return student_const(s, nu) - 0.5 * (nu + 1.) * np.log(1. + (1. / nu) * (np.square((Y - F) / s)))
    if kind == "gaussian":
        return -0.5 * (np.log(2 * np.pi) + np.log(params[0]) + np.square(F - Y) / params[0])
    raise ValueError(kind)


def _dlogp(kind, params, F, Y):
    """(d logp / d f, d logp / d first parameter)"""
    if kind == "bernoulli":
        p = probit(F)
        dp = (1 - 2e-3) * _INV_S2PI * np.exp(-0.5 * F * F)
        return np.where(np.equal(Y, 1), dp / p, -dp / (1 - p)), np.zeros_like(F)
    if kind == "student_t":
        s, nu = params
        r = (Y - F) / s
        t = (nu + 1.) * r / (nu * s * (1. + r * r / nu))
        return t, -1. / s + t * r
    raise ValueError(kind)


def cond_mean_var(kind, params, F):
    """conditional_mean, conditional_variance"""
    if kind == "bernoulli":
        p = probit(F)
        return p, p - np.square(p)                            # :293-298
    if kind == "poisson":
        lam = np.exp(F) * params[0]
        return lam, lam                                       # :215-219
    if kind == "exponential":
        return np.exp(F), np.square(np.exp(F))                # :233-237
    if kind == "student_t":
        return F.copy(), F * 0.0 + params[1] / (params[1] - 2.0)   # :261-266
    raise ValueError(kind)


def quad_varexp(kind, params, mu, var, Y, n_gh=20):
    """the generic rule :121-152"""
    x, w = gh(n_gh)
    shape = np.shape(mu)
    mu, var, Y = [np.reshape(e, (-1, 1)) for e in (mu, var, Y)]
    X = x.reshape(1, -1) * np.sqrt(2.0 * var) + mu
    return np.reshape(np.matmul(logp(kind, params, X, np.tile(Y, [1, n_gh])), w.reshape(-1, 1)), shape)


def prob_is_largest(Y, mu, var, n_gh=20):
    """RobustMax.prob_is_largest, :404-425.  Y [N] or [N, 1] integer labels; mu, var [N, K]."""
    x, w = gh(n_gh)
    Y = np.asarray(Y).astype(np.int64).reshape(-1)
    n, K = mu.shape
    on = np.zeros((n, K)); on[np.arange(n), Y] = 1.0
    mu_s = np.sum(on * mu, 1); var_s = np.sum(on * var, 1)
    X = mu_s.reshape(-1, 1) + x * np.sqrt(np.clip(2. * var_s, 1e-10, np.inf)).reshape(-1, 1)
    dist = (X[:, None, :] - mu[:, :, None]) / np.sqrt(np.clip(var, 1e-10, np.inf))[:, :, None]
    cdfs = 0.5 * (1.0 + erf(dist / np.sqrt(2.0)))
    cdfs = cdfs * (1 - 2e-4) + 1e-4
    cdfs = cdfs * (1.0 - on)[:, :, None] + on[:, :, None]
    return np.matmul(np.prod(cdfs, axis=1), w.reshape(-1, 1))


def varexp(kind, params, mu, var, Y, n_gh=20):
    """variational_expectations of each class: [N, K] ([N, 1] for multiclass)"""
    if kind == "poisson":                                     # :220-224
        return Y * mu - np.exp(mu + var / 2) * params[0] - gammaln(Y + 1) + Y * np.log(params[0])
    if kind == "exponential":                                 # :240-243
        return -np.exp(-mu + var / 2) * Y - mu
    if kind == "gaussian":                                    # :186-188
        return -0.5 * np.log(2 * np.pi) - 0.5 * np.log(params[0]) - 0.5 * (np.square(Y - mu) + var) / params[0]
    if kind == "multiclass":                                  # :449-454
        eps = params[0]
        p = prob_is_largest(Y, mu, var, n_gh)
        return p * np.log(1 - eps) + (1. - p) * np.log(eps / (mu.shape[1] - 1.))
    return quad_varexp(kind, params, mu, var, Y, n_gh)


def varexp_grad(kind, params, mu, var, Y, n_gh=20):
    """(var_exp, d/d mu [N, K], d/d var [N, K], d sum(var_exp) / d params[0]) -- analytic"""
    ve = varexp(kind, params, mu, var, Y, n_gh)
    if kind == "poisson":
        ex = np.exp(mu + var / 2) * params[0]
        return ve, Y - ex, -0.5 * ex, 0.0
    if kind == "exponential":
        ex = np.exp(-mu + var / 2) * Y
        return ve, ex - 1.0, -0.5 * ex, 0.0
    if kind == "gaussian":
        s2 = params[0]
        return ve, (Y - mu) / s2, np.full(mu.shape, -0.5 / s2), float(np.sum(-0.5 / s2 + 0.5 * (np.square(Y - mu) + var) / s2 ** 2))
    if kind == "multiclass":
        x, w = gh(n_gh)
        eps = params[0]
        n, K = mu.shape
        Yi = np.asarray(Y).astype(np.int64).reshape(-1)
        on = np.zeros((n, K)); on[np.arange(n), Yi] = 1.0
        mu_s = np.sum(on * mu, 1); var_s = np.sum(on * var, 1)
        sdy = np.sqrt(np.clip(2. * var_s, 1e-10, np.inf))
        sd = np.sqrt(np.clip(var, 1e-10, np.inf))
        X = mu_s[:, None] + x[None, :] * sdy[:, None]                       # N x H
        d = (X[:, None, :] - mu[:, :, None]) / sd[:, :, None]               # N x K x H
        c = 0.5 * (1.0 + erf(d / np.sqrt(2.0))) * (1 - 2e-4) + 1e-4
        cm = c * (1.0 - on)[:, :, None] + on[:, :, None]
        P = np.prod(cm, axis=1)                                             # N x H
        t = w[None, None, :] * (P[:, None, :] / c) * ((1 - 2e-4) * _INV_S2PI * np.exp(-0.5 * d * d)) * (1.0 - on)[:, :, None]
        dmu = -np.sum(t, 2) / sd
        dvar = np.where(var >= 1e-10, -np.sum(t * d, 2) / (2.0 * np.where(var >= 1e-10, var, 1.0)), 0.0)
        dmu_y = -np.sum(dmu, 1)
        dvar_y = np.where(2. * var_s >= 1e-10, np.sum(np.sum(t * x[None, None, :], 2) / sd, 1) / sdy, 0.0)
        dmu = dmu + on * dmu_y[:, None]
        dvar = dvar + on * dvar_y[:, None]
        g = np.log(1 - eps) - np.log(eps / (K - 1.))
        return ve, g * dmu, g * dvar, 0.0
    x, w = gh(n_gh)
    sd = np.sqrt(2.0 * var)
    F = mu[..., None] + sd[..., None] * x
    dl, dpar = _dlogp(kind, params, F, np.asarray(Y)[..., None] * np.ones_like(F))
    return ve, np.sum(dl * w, -1), np.sum(dl * w * x, -1) / sd, float(np.sum(dpar * w))


def predict_mean_and_var(kind, params, mu, var, n_gh=20):
    if kind == "bernoulli":                                   # :280-283
        p = probit(mu / np.sqrt(1 + var))
        return p, p - np.square(p)
    if kind == "multiclass":                                  # :456-466
        ps = np.stack([predict_nonlog_density(params, mu, var, np.full((mu.shape[0], 1), i), n_gh).reshape(-1)
                       for i in range(mu.shape[1])]).T
        return ps, ps - np.square(ps)
    return quad_predict_mean_and_var(kind, params, mu, var, n_gh)


def quad_predict_mean_and_var(kind, params, mu, var, n_gh=20):
    """:45-86"""
    x, w = gh(n_gh)
    shape = np.shape(mu)
    mu, var = [np.reshape(e, (-1, 1)) for e in (mu, var)]
    X = x[None, :] * np.sqrt(2.0 * var) + mu
    cm, cv = cond_mean_var(kind, params, X)
    E_y = np.reshape(np.matmul(cm, w.reshape(-1, 1)), shape)
    V_y = np.reshape(np.matmul(cv + np.square(cm), w.reshape(-1, 1)), shape) - np.square(E_y)
    return E_y, V_y


def predict_nonlog_density(params, mu, var, Y, n_gh=20):
    """:471-477"""
    eps = params[0]
    p = prob_is_largest(Y, mu, var, n_gh)
    return p * (1 - eps) + (1. - p) * (eps / (mu.shape[1] - 1.))


def predict_density(kind, params, mu, var, Y, n_gh=20):
    if kind == "bernoulli":                                   # :288-290
        p = predict_mean_and_var(kind, params, mu, var)[0]
        return np.log(np.where(np.equal(Y, 1), p, 1 - p))
    if kind == "multiclass":                                  # :468-469
        return np.log(predict_nonlog_density(params, mu, var, Y, n_gh))
    x, w = gh(n_gh)                                           # :88-119
    shape = np.shape(mu)
    mu, var, Y = [np.reshape(e, (-1, 1)) for e in (mu, var, Y)]
    X = x[None, :] * np.sqrt(2.0 * var) + mu
    return np.reshape(np.log(np.matmul(np.exp(logp(kind, params, X, np.tile(Y, [1, n_gh]))), w.reshape(-1, 1))), shape)


def svgp_bound(kind, params, spec, X, Y, Z, q_mu, q_sqrt, whiten=True, num_data=None, mean_X=None, n_gh=20, jitter=orc.JITTER):
    """models/svgp.py:101-130: scale * sum variational_expectations(conditional) - gauss_kl"""
    Kp = None if whiten else orc.K(spec, Z) + jitter * np.eye(Z.shape[0])
    KL = orc.gauss_kl(q_mu, q_sqrt, Kp)
    fmean, fvar = orc.conditional(X, Z, spec, q_mu, full_cov=False, q_sqrt=q_sqrt, white=whiten, jitter=jitter)
    if mean_X is not None:
        fmean = fmean + mean_X
    scale = float(num_data or X.shape[0]) / float(X.shape[0])
    return float(np.sum(varexp(kind, params, fmean, fvar, Y, n_gh)) * scale - KL)


def sample_inputs(kind, n, k, rng, var_lo=1e-6, var_hi=10.0):
    """seeded (mu, var, Y, params) for a kind: var log-uniform in [var_lo, var_hi]"""
    mu = rng.standard_normal((n, k)) * 1.5
    var = np.exp(rng.uniform(np.log(var_lo), np.log(var_hi), (n, k)))
    if kind == "bernoulli":
        return mu, var, (rng.random((n, k)) < 0.5).astype(float), []
    if kind == "poisson":
        return mu * 0.5, var, rng.poisson(2.0, (n, k)).astype(float), [0.7]
    if kind == "exponential":
        return mu * 0.5, var, rng.exponential(1.0, (n, k)), []
    if kind == "student_t":
        return mu, var, mu + rng.standard_t(3.0, (n, k)), [0.8, 3.0]
    if kind == "multiclass":
        return mu, var, rng.integers(0, k, (n, 1)).astype(float), [1e-3]
    if kind == "gaussian":
        return mu, var, mu + rng.standard_normal((n, k)), [0.3]
    raise ValueError(kind)
