"""Numpy restatement of the reference's sparse MCMC model (gpflowSlim/models/sgpmc.py:83-104 with conditionals.py:80-103 at
white=True, q_sqrt=None) with its analytic gradient -- the yardstick of tests/test_gpu_sgpmc.py, itself checked on the CPU
(tests/test_sgpmc_ref_cpu.py).

    Lm = chol(Kuu + jitter I) ; A = Lm^-1 Kuf [M, N] ; fmean = A^T V + mean [N, R] ; fvar = Kdiag - colsum(A^2) [N]
    loglik = sum_i var_exp(fmean_i, fvar_i, Y_i)                       (fvar shared by all latents)

With E = d loglik / d fmean, H = d loglik / d fvar per latent (tests/_lik_ref.py: varexp_grad) and h = sum_q H[:, q]:

    grad_V = A E ; grad_mean = E ; Kdiag_bar = h ; Abar = V E^T - 2 A diag(h) ; Kuf_bar = Lm^-T Abar

and two ways to the cotangent of Kuu:

    "generic"  Lm_bar = -tril(Kuf_bar A^T) ; Psym = Phi(Lm^T Lm_bar) + Phi(.)^T          -- the adjoint as inducing_backward forms it
    "seed"     W = A diag(h) A^T ; Psym[i][j] = 2 W[i][j] - V[max(i, j)] . grad_V[min(i, j)]    -- what the device uses:
               Lm_bar = -tril(Lm^-T C) with C = V grad_V^T - 2 W, and tril(Lm^T Lm_bar) = -tril(C) because an upper times a
               strictly upper triangle is strictly upper

then 2 Kuu_bar = Lm^-T Psym Lm^-1 and  d / d slot = <Kuf_bar, dKuf> + 1/2 <2 Kuu_bar, dKuu> + sum_i h_i dKdiag_i  (tests/_kern_ref.py);
d / d Z through Kuf (cotangent Kuf_bar) and Kuu (both arguments move: the first-argument gradient against 2 Kuu_bar).
Everything data-sized is local to a block of data points: `chunk` streams the data in column blocks and adds up.

Likelihood kinds and their parameters: tests/_lik_ref.py ("multiclass": Y [N, 1] labels, R >= 2 latent functions).
"""
import os
import sys

import numpy as np
import scipy.linalg as sl

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gpmc_ref as gr  # noqa: E402
import _kern_ref as kr  # noqa: E402
import _lik_ref as lr  # noqa: E402

JITTER = 1e-6
KINDS = ("gaussian", "bernoulli", "poisson", "exponential", "student_t", "multiclass")


def make_case(kind, m, n, r, seed=0, d=2):
    """seeded (Z [m, d], X [n, d], V [m, r], Y, likelihood parameters, mean [n, r]); Z and X standard normal"""
    rng = np.random.default_rng(1000 * seed + 7 * n + 13 * m + r + len(kind))
    Z = rng.standard_normal((m, d))
    X = rng.standard_normal((n, d))
    V = 0.6 * rng.standard_normal((m, r))
    mean = np.full((n, r), 0.2)
    F = np.sin(X @ rng.standard_normal((d, r)))
    params = {"gaussian": [0.3], "bernoulli": [], "poisson": [0.7], "exponential": [], "student_t": [0.6, 3.0],
              "multiclass": [1e-3]}[kind]
    if kind == "bernoulli":
        Y = (F + 0.3 * rng.standard_normal((n, r)) > 0).astype(float)
    elif kind == "poisson":
        Y = rng.poisson(np.exp(F) * 0.7).astype(float)
    elif kind == "exponential":
        Y = rng.exponential(np.exp(F))
    elif kind == "student_t":
        Y = F + 0.3 * rng.standard_t(3.0, (n, r))
    elif kind == "multiclass":
        Y = np.argmax(F + 0.3 * rng.standard_normal((n, r)), axis=1).astype(float).reshape(-1, 1)
    else:
        Y = F + 0.5 * rng.standard_normal((n, r))
    return Z, X, V, Y, params, mean


def factor(spec, Z, jitter=JITTER):
    Kuu = kr.K(spec, Z) + jitter * np.eye(Z.shape[0])
    return Kuu, sl.cholesky(Kuu, lower=True)


def moments(spec, Z, X, V, mean=None, jitter=JITTER, Lm=None):
    """(A [M, N], fmean [N, R], fvar [N]) of the whitened conditional without q_sqrt"""
    if Lm is None:
        Lm = factor(spec, Z, jitter)[1]
    A = sl.solve_triangular(Lm, kr.K(spec, Z, X), lower=True)
    fmean = A.T @ V + (0.0 if mean is None else mean)
    return A, fmean, kr.Kdiag(spec, X) - np.sum(np.square(A), 0)


def _var(fvar, r):
    return np.repeat(fvar[:, None], r, axis=1)


def loglik(spec, Z, X, V, Y, kind, params, mean=None, jitter=JITTER):
    """sgpmc.py:83-89"""
    _, fmean, fvar = moments(spec, Z, X, V, mean, jitter)
    return float(np.sum(lr.varexp(kind, params, fmean, _var(fvar, V.shape[1]), Y)))


def kdiag_vjp(spec, X, h, block=256, absolute=False):
    """sum_i h_i d Kdiag_i / d slot, from the diagonals of d K / d slot block by block; absolute: sum_i |h_i d Kdiag_i / d slot|"""
    out = 0.0
    for i0 in range(0, X.shape[0], block):
        Xb, hb = X[i0:i0 + block], h[i0:i0 + block]
        out = out + np.array([np.sum(np.abs(np.diag(g) * hb) if absolute else np.diag(g) * hb) for g in kr.dK(spec, Xb)])
    return out


def _solve2(Lm, Psym):
    """Lm^-T Psym Lm^-1"""
    Y = sl.solve_triangular(Lm, Psym.T, lower=True, trans="T").T           # Psym Lm^-1
    return sl.solve_triangular(Lm, Y, lower=True, trans="T")


def grad(spec, Z, X, V, Y, kind, params, mean=None, jitter=JITTER, path="seed", chunk=None):
    """dict(loglik, slots, glik, gV, gmean, gZ, Kuu, Lm, Kbar2, slots_abs, gZ_abs); the last two: the sums of the absolute values of
    the terms that slots and gZ add up (the Kuf, Kuu and Kdiag contractions cancel by orders of magnitude at cond_2(Kuu) of 1e7:
    the size of what is being summed is what a rounding error of these two is relative to)"""
    n, r = X.shape[0], V.shape[1]
    Kuu, Lm = factor(spec, Z, jitter)
    ll, glik = 0.0, 0.0
    gV = np.zeros_like(V)
    gmean = np.zeros((n, r))
    gZ = np.zeros_like(Z)
    W = np.zeros_like(Kuu)                                          # seed: A diag(h) A^T ; generic: Kuf_bar A^T
    slots, slots_abs, gZ_abs = 0.0, 0.0, np.zeros_like(Z)
    step = n if chunk is None else chunk
    for c0 in range(0, n, step):
        sl_ = slice(c0, min(n, c0 + step))
        Xc, Yc = X[sl_], Y[sl_]
        A, fmean, fvar = moments(spec, Z, Xc, V, None if mean is None else mean[sl_], jitter, Lm)
        ve, E, H, dpar = lr.varexp_grad(kind, params, fmean, _var(fvar, r), Yc)
        h = np.sum(H, 1)
        ll += float(np.sum(ve)); glik += float(dpar)
        gmean[sl_] = E
        gV += A @ E
        Abar = V @ E.T - 2.0 * A * h
        KufBar = sl.solve_triangular(Lm, Abar, lower=True, trans="T")
        W += (A * h) @ A.T if path == "seed" else KufBar @ A.T
        slots = slots + kr.vjp_slots(spec, KufBar, Z, Xc) + kdiag_vjp(spec, Xc, h)
        gZ += kr.input_vjp(spec, KufBar, Z, Xc)
        slots_abs = slots_abs + kr.vjp_slots(spec, KufBar, Z, Xc, absolute=True) + kdiag_vjp(spec, Xc, h, absolute=True)
        gZ_abs += kr.input_vjp(spec, KufBar, Z, Xc, absolute=True)
    if path == "seed":
        Psym = 2.0 * W - gr.seed(V, gV)
    elif path == "generic":
        P = Lm.T @ (-np.tril(W))
        Psym = gr.phi(P) + gr.phi(P).T
    else:
        raise ValueError(path)
    Kbar2 = _solve2(Lm, Psym)
    slots = slots + 0.5 * kr.vjp_slots(spec, Kbar2, Z)
    gZ += kr.input_vjp(spec, Kbar2, Z)
    slots_abs = slots_abs + 0.5 * kr.vjp_slots(spec, Kbar2, Z, absolute=True)
    gZ_abs += kr.input_vjp(spec, Kbar2, Z, absolute=True)
    return dict(loglik=ll, slots=np.asarray(slots), glik=glik, gV=gV, gmean=gmean, gZ=gZ, Kuu=Kuu, Lm=Lm, Kbar2=Kbar2,
                slots_abs=np.asarray(slots_abs), gZ_abs=gZ_abs)
