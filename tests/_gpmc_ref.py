"""Numpy restatement of the reference's whitened MCMC model (gpflowSlim/models/gpmc.py:72-77) with its analytic gradient -- the
yardstick of tests/test_gpu_gpmc.py, itself checked on the CPU (tests/test_gpmc_ref_cpu.py).

    K = kern.K(X) + jitter I ; L = chol(K) ; F = L V + mean ; loglik = sum log p(Y | F)

With G = d loglik / d F:  d / d V = U = L^T G ;  d / d mean = G ;  the cotangent of L is Lbar = tril(G V^T), and the Cholesky
adjoint (Murray 2016) gives  Kbar = 1/2 (S + S^T),  S = L^-T Phi(L^T Lbar) L^-1,  Phi = lower triangle with halved diagonal;
d / d slot = sum_ij Kbar_ij dK_ij / d slot (tests/_kern_ref.py).  Two ways to Phi's argument:

    "outer"  tril(U V^T)                  -- (L^T Lbar)_ij = U_i . V_j for i >= j: what the device's seed kernel uses
    "dense"  tril(L^T tril(G V^T))        -- the product, as the generic adjoint forms it

Likelihood kinds and their parameters: tests/_lik_ref.py (everything elementwise; no MultiClass).
"""
import os
import sys

import numpy as np
import scipy.linalg as sl

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _kern_ref as kr  # noqa: E402
import _lik_ref as lr  # noqa: E402

JITTER = 1e-6
KINDS = ("gaussian", "bernoulli", "poisson", "exponential", "student_t")


def rbf_spec(variance=1.3, ls=(0.5, 0.7)):
    return {"type": "rbf", "dims": list(range(len(ls))), "variance": float(variance), "lengthscales": np.array(ls, dtype=float)}


def matern_linear_spec():
    return ("sum", [{"type": "matern52", "dims": [0, 1], "variance": 0.9, "lengthscales": np.array([0.8, 1.1])},
                    {"type": "linear", "dims": [0, 1], "variance": np.array([0.3, 0.2])}])


def make_case(kind, n, r, seed=0, d=2):
    """seeded (X [n, d], V [n, r], Y [n, r], likelihood parameters, mean [n, r])"""
    rng = np.random.default_rng(1000 * seed + 7 * n + r + len(kind))
    X = rng.standard_normal((n, d))
    V = 0.6 * rng.standard_normal((n, r))
    mean = np.full((n, r), 0.2)
    F = np.sin(X @ rng.standard_normal((d, r)))
    params = {"gaussian": [0.3], "bernoulli": [], "poisson": [0.7], "exponential": [], "student_t": [0.6, 3.0]}[kind]
    if kind == "bernoulli":
        Y = (F + 0.3 * rng.standard_normal((n, r)) > 0).astype(float)
    elif kind == "poisson":
        Y = rng.poisson(np.exp(F) * 0.7).astype(float)
    elif kind == "exponential":
        Y = rng.exponential(np.exp(F))
    elif kind == "student_t":
        Y = F + 0.3 * rng.standard_t(3.0, (n, r))
    else:
        Y = F + 0.5 * rng.standard_normal((n, r))
    return X, V, Y, params, mean


def dlogp(kind, params, F, Y):
    """(d log p / d F [n, r], d sum log p / d params[0])"""
    if kind in ("bernoulli", "student_t"):
        g, gp = lr._dlogp(kind, params, F, Y)
        return g, float(np.sum(gp))
    _, g, _, gp = lr.varexp_grad(kind, params, F, np.zeros_like(F), Y)      # (the closed forms at fvar = 0 are log p itself)
    return g, float(gp)


def factor(spec, X, jitter=JITTER):
    K = kr.K(spec, X) + jitter * np.eye(X.shape[0])
    return K, sl.cholesky(K, lower=True)


def loglik(spec, X, V, Y, kind, params, mean=None, jitter=JITTER):
    """gpmc.py:72-77"""
    _, L = factor(spec, X, jitter)
    F = L @ V + (0.0 if mean is None else mean)
    return float(np.sum(lr.logp(kind, params, F, Y)))


def phi(P):
    out = np.tril(P)
    out[np.diag_indices_from(out)] *= 0.5
    return out


def seed(U, V):
    """Phi(P) + Phi(P)^T for P = tril(U V^T): entry (i, j) is U[max(i, j)] . V[min(i, j)]"""
    P = np.tril(U @ V.T)
    return P + P.T - np.diag(np.diag(P))


def grad(spec, X, V, Y, kind, params, mean=None, jitter=JITTER, path="outer"):
    """dict(loglik, slots, glik, gV, gmean, Kbar, U, G, L, K)"""
    K, L = factor(spec, X, jitter)
    F = L @ V + (0.0 if mean is None else mean)
    G, glik = dlogp(kind, params, F, Y)
    U = L.T @ G
    if path == "outer":
        P = np.tril(U @ V.T)
    elif path == "dense":
        P = np.tril(L.T @ np.tril(G @ V.T))
    else:
        raise ValueError(path)
    S = sl.solve_triangular(L, sl.solve_triangular(L, phi(P), lower=True, trans="T").T, lower=True, trans="T").T   # L^-T Phi L^-1
    Kbar = 0.5 * (S + S.T)
    slots = np.array([np.sum(Kbar * g) for g in kr.dK(spec, X)])
    return dict(loglik=float(np.sum(lr.logp(kind, params, F, Y))), slots=slots, glik=glik, gV=U, gmean=G, Kbar=Kbar, U=U, G=G, L=L, K=K)


# ---- the parameters behind the slots, for differences -------------------------------------------------------------------------------
def param_refs(spec):
    """[(leaf, name, index or None)] in the order of kr.fold: stationary leaves (variance, lengthscales) and linear ones"""
    out = []
    for leaf in kr.leaves(spec):
        t = leaf["type"]
        if t in kr.STATIONARY and t != "ratquad":
            out.append((leaf, "variance", None))
            name = "lengthscales"
        elif t == "linear":
            name = "variance"
        else:
            raise NotImplementedError(t)
        if np.size(leaf[name]) > 1:
            out += [(leaf, name, i) for i in range(np.size(leaf[name]))]
        else:
            out.append((leaf, name, None))
    return out


def get_param(ref):
    leaf, name, i = ref
    return float(leaf[name]) if i is None else float(leaf[name][i])


def set_param(ref, value):
    leaf, name, i = ref
    if i is None:
        leaf[name] = float(value)
    else:
        leaf[name][i] = value


def five_point(f, x, h):
    return (-f(x + 2 * h) + 8.0 * f(x + h) - 8.0 * f(x - h) + f(x - 2 * h)) / (12.0 * h)
