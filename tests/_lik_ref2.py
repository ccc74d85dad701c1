"""CPU restatement (numpy / scipy) of the reference's Gamma, Beta and Ordinal likelihoods, in the style of tests/_lik_ref.py
(whose ``gh`` and ``probit`` it uses): for the tests of gpflowSlim.likelihoods and of the device kernels (csrc/lik.hip).  Line
numbers: gpflowSlim/likelihoods.py and gpflowSlim/densities.py of the reference.

Kinds and their ``params``:
  "gamma"    [shape]                  exp link; the latent gives the scale                         :301-333, densities.py:45-47
  "beta"     [scale]                  probit link; alpha = m s, beta = s - alpha                   :336-376, densities.py:60-66
  "ordinal"  [sigma, bin_edges]       labels 0 .. len(bin_edges)                                   :554-631

Also the analytic derivatives of the variational expectations in (mu, var, first parameter) -- what autodiff through :121-152
yields, pinned against central differences in tests/test_lik2_cpu.py -- and the SVGP bound composed with the oracle.
"""
import os
import sys

import numpy as np
from scipy.special import digamma, erfc, gammaln

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lik_ref as ref1  # noqa: E402

orc = ref1.orc
gh, probit = ref1.gh, ref1.probit

KINDS = ("gamma", "beta", "ordinal")
KIND_ID = {"gamma": 6, "beta": 7, "ordinal": 8}
_INV_S2PI = 1.0 / np.sqrt(2.0 * np.pi)
_SQUASH = 1 - 2e-3


def _ordinal_bins(params, Y):
    """:599-603: the scaled edges left and right of each label's bin, +-inf at the ends"""
    sigma, edges = params[0], np.asarray(params[1], dtype=float)
    Yi = np.asarray(Y).astype(np.int64)
    left = np.concatenate([edges / sigma, [np.inf]])
    right = np.concatenate([[-np.inf], edges / sigma])
    return left[Yi], right[Yi]


def probit_difference(zl, zr):
    """probit(zl) - probit(zr), zl >= zr: (1 - 2e-3) (Phi(zl) - Phi(zr)) as a difference of two erfc on the side where both Phi are
    small.  :605-606 subtract the two probits as they are, which in a far tail leaves their rounding next to the 1e-6 floor: that
    formula in numpy sits 1.35e-11 of max(1, |log p|) from the 40-digit value, and its dvar at var = 1e-6, where the quotient by
    sqrt(2 var) multiplies by another 707, 8.1e-9 (measured on the inputs of tests/test_gpu_lik2.py at 32 edges) -- more than the
    device may differ from this restatement at all.  This form is the same number to a few eps of itself; the package's
    host class and the device kernels take it the same way, so the sides still differ in libm and summation order only."""
    zl, zr = np.broadcast_arrays(np.asarray(zl, dtype=float), np.asarray(zr, dtype=float))
    up = (zl + zr) > 0.0
    ea = erfc(np.where(up, zr, -zl) / np.sqrt(2.0))
    eb = erfc(np.where(up, zl, -zr) / np.sqrt(2.0))                          # (an infinite edge is always here: exactly 0)
    return _SQUASH * (0.5 * (ea - eb))


def logp(kind, params, F, Y):
    """log p(y | f)"""
    if kind == "gamma":                                       # densities.py:45-47 through :319
        shape, scale = params[0], np.exp(F)
        return -shape * np.log(scale) - gammaln(shape) + (shape - 1.) * np.log(Y) - Y / scale
    if kind == "beta":                                        # densities.py:60-66 through :365-369
        mean = probit(F)
        alpha = mean * params[0]
        beta = params[0] - alpha
        y = np.clip(Y, 1e-6, 1 - 1e-6)
        return (alpha - 1.) * np.log(y) + (beta - 1.) * np.log(1. - y) + gammaln(alpha + beta) - gammaln(alpha) - gammaln(beta)
    if kind == "ordinal":                                     # :598-606
        left, right = _ordinal_bins(params, Y)
        return np.log(probit_difference(left - F / params[0], right - F / params[0]) + 1e-6)
    raise ValueError(kind)


def _dlogp(kind, params, F, Y):
    """(d logp / d f, d logp / d first parameter)"""
    if kind == "gamma":
        return -params[0] + Y * np.exp(-F), -F - digamma(params[0]) + np.log(Y)
    if kind == "beta":
        s = params[0]
        m = probit(F)
        dm = _SQUASH * _INV_S2PI * np.exp(-0.5 * F * F)
        alpha = m * s
        beta = s - alpha
        y = np.clip(Y, 1e-6, 1 - 1e-6)
        ly, l1y = np.log(y), np.log(1. - y)
        pa, pb = digamma(alpha), digamma(beta)
        return s * dm * (ly - l1y - pa + pb), m * ly + (1 - m) * l1y + digamma(s) - m * pa - (1 - m) * pb
    if kind == "ordinal":
        sigma = params[0]
        left, right = _ordinal_bins(params, Y)
        left, right = np.broadcast_to(left, np.shape(F)), np.broadcast_to(right, np.shape(F))
        zl, zr = left - F / sigma, right - F / sigma
        P = probit_difference(zl, zr) + 1e-6
        fl, fr = np.isfinite(left), np.isfinite(right)
        zl0, zr0 = np.where(fl, zl, 0.0), np.where(fr, zr, 0.0)              # (an infinite edge contributes exactly zero)
        nl = np.where(fl, _INV_S2PI * np.exp(-0.5 * zl0 * zl0), 0.0)
        nr = np.where(fr, _INV_S2PI * np.exp(-0.5 * zr0 * zr0), 0.0)
        al_f, ar_f = zl0 * sigma, zr0 * sigma                                # a_l - f, a_r - f
        return -(1.0 / sigma) * _SQUASH * (nl - nr) / P, _SQUASH * (-nl * al_f + nr * ar_f) / (sigma * sigma * P)
    raise ValueError(kind)


def cond_mean_var(kind, params, F):
    """conditional_mean, conditional_variance"""
    if kind == "gamma":                                       # :321-326
        return params[0] * np.exp(F), params[0] * np.square(np.exp(F))
    if kind == "beta":                                        # :371-376
        m = probit(F)
        return m, (m - np.square(m)) / (params[0] + 1.)
    if kind == "ordinal":                                     # :608-631
        sigma, edges = params[0], np.asarray(params[1], dtype=float)
        left = np.concatenate([edges / sigma, [np.inf]])
        right = np.concatenate([[-np.inf], edges / sigma])
        phi = probit(left - np.reshape(F, (-1, 1)) / sigma) - probit(right - np.reshape(F, (-1, 1)) / sigma)
        Ys = np.arange(edges.size + 1, dtype=float).reshape(-1, 1)
        E_y, E_y2 = phi @ Ys, phi @ np.square(Ys)
        return np.reshape(E_y, np.shape(F)), np.reshape(E_y2 - np.square(E_y), np.shape(F))
    raise ValueError(kind)


def quad_varexp(kind, params, mu, var, Y, n_gh=20):
    """the generic rule :121-152"""
    x, w = gh(n_gh)
    shape = np.shape(mu)
    mu, var, Y = [np.reshape(e, (-1, 1)) for e in (mu, var, Y)]
    X = x.reshape(1, -1) * np.sqrt(2.0 * var) + mu
    return np.reshape(np.matmul(logp(kind, params, X, np.tile(Y, [1, n_gh])), w.reshape(-1, 1)), shape)


def varexp(kind, params, mu, var, Y, n_gh=20):
    """variational_expectations of each class: [N, K]"""
    if kind == "gamma":                                       # :328-331
        shape = params[0]
        return -shape * mu - gammaln(shape) + (shape - 1.) * np.log(Y) - Y * np.exp(-mu + var / 2.)
    return quad_varexp(kind, params, mu, var, Y, n_gh)


def varexp_grad(kind, params, mu, var, Y, n_gh=20):
    """(var_exp, d/d mu [N, K], d/d var [N, K], d sum(var_exp) / d params[0]) -- analytic"""
    ve = varexp(kind, params, mu, var, Y, n_gh)
    if kind == "gamma":
        ex = Y * np.exp(-mu + var / 2.)
        return ve, -params[0] + ex, -0.5 * ex, float(np.sum(-mu - digamma(params[0]) + np.log(Y)))
    x, w = gh(n_gh)
    sd = np.sqrt(2.0 * var)
    F = mu[..., None] + sd[..., None] * x
    dl, dpar = _dlogp(kind, params, F, np.asarray(Y)[..., None] * np.ones_like(F))
    return ve, np.sum(dl * w, -1), np.sum(dl * w * x, -1) / sd, float(np.sum(dpar * w))


def predict_density(kind, params, mu, var, Y, n_gh=20):
    """:88-119"""
    x, w = gh(n_gh)
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


def ordinal_edges(n_edges):
    """a table for the tests: n_edges evenly spaced edges over [-2, 2] (one edge: 0.3)"""
    return np.array([0.3]) if n_edges == 1 else np.linspace(-2.0, 2.0, n_edges)


def sample_inputs(kind, n, k, rng, var_lo=1e-6, var_hi=10.0, param=None, n_edges=3):
    """seeded (mu, var, Y, params) for a kind: var log-uniform in [var_lo, var_hi]; param: the first parameter.
    beta: Y holds exact 0 and 1 (the clip of densities.beta).  ordinal: mu is spread over three bin ranges and the labels are
    drawn independently of it, so that label 0 and the top label occur and many points lie wholly in the far tail of their
    bin, where the 1e-6 floor under the logarithm is all that is left."""
    mu = rng.standard_normal((n, k)) * 1.5
    var = np.exp(rng.uniform(np.log(var_lo), np.log(var_hi), (n, k)))
    if kind == "gamma":
        return mu * 0.5, var, rng.gamma(2.0, 1.0, (n, k)) + 1e-3, [1.7 if param is None else param]
    if kind == "beta":
        Y = rng.beta(2.0, 3.0, (n, k))
        Y.flat[0], Y.flat[-1] = 0.0, 1.0
        return mu, var, Y, [3.0 if param is None else param]
    if kind == "ordinal":
        Y = rng.integers(0, n_edges + 1, (n, k)).astype(float)
        Y.flat[0], Y.flat[-1] = 0.0, float(n_edges)
        return mu * 4.0, var, Y, [0.7 if param is None else param, ordinal_edges(n_edges)]
    raise ValueError(kind)
