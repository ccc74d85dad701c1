"""Analytic fp64 reference (numpy / scipy / LAPACK) for the gradient of the exact-GP log-marginal likelihood with respect to the
INPUT points -- what gps_gpr_lml_grad_x returns and the GPLVM trains on -- and the input sets that tests/test_gpu_gplvm_point.py
runs, so that tests/test_gplvm_point_ref_cpu.py can prove the reference on exactly those.

    d LML / d x_i = sum_j W_ij d k(x_i, x_j) / d x_i ,   W = a a^T - R K_y^-1 ,   a = K_y^-1 Y ,   K_y = K + s2 I

a and K_y^-1 come from LAPACK as in tests/_grad_ref.py (Cholesky, cho_solve, dpotri on the same factor) and once more from
eigh (K_y^-1 = Q diag(1 / lambda) Q^T): the difference of the two gradients, in units of max(1, |g|_inf), is the reference's own
spread, and lambda gives cond(K_y).  The kernel part is input_vjp of tests/_kern_ref.py / _kern_ref2.py / _coregion_ref.py, the
analytic forms the kernel-matrix VJP tests use (first argument only):  ref = input_vjp(W / 2) + input_vjp((W / 2)^T).
The diagonal term is part of it (White sits on i == j, ArcCosine keeps its diagonal special case).

A Neural Kernel Network has no analytic input form here: its d k / d x_i comes from central differences of the oracle's K(X + h e_d,
X) with one Richardson step (nkn_input_vjp), whose own error is estimated from the two step lengths and added to the spread.
"""
import collections
import os
import sys

import numpy as np
import scipy.linalg as sl

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import _coregion_ref as cr  # noqa: E402   (every leaf type: it falls through to _kern_ref2 and _kern_ref)
import oracle.gp_oracle as orc  # noqa: E402

EPS = np.finfo(np.float64).eps
XRef = collections.namedtuple("XRef", "g lml a Kinv cond spread")
_cache = {}


def gate(cond):
    """the rule of tests/test_gpu_grad_large.py: |got - ref| <= gate * max(1, |ref|_inf)"""
    return max(1e-8, 2 * EPS * cond)


def _weights(Ky, Y, route):
    n, r = Y.shape
    if route == "chol":
        c = sl.cho_factor(Ky, lower=True)
        a = sl.cho_solve(c, Y)
        inv, info = sl.lapack.dpotri(c[0], lower=1)
        assert info == 0
        Kinv = np.tril(inv) + np.tril(inv, -1).T
        lml = -0.5 * n * r * np.log(2.0 * np.pi) - r * np.sum(np.log(np.diag(c[0]))) - 0.5 * np.sum(Y * a)
        return a, Kinv, lml, None
    lam, Q = sl.eigh(Ky)
    Kinv = (Q / lam) @ Q.T
    Kinv = 0.5 * (Kinv + Kinv.T)
    return Kinv @ Y, Kinv, None, lam


def grad_x_from(W, spec, X, input_vjp=None):
    input_vjp = input_vjp or cr.input_vjp
    return input_vjp(spec, 0.5 * W, X) + input_vjp(spec, 0.5 * W.T, X)


def grad_x_ref(spec, X, Y, noise, K=None, input_vjp=None, extra_spread=None):
    """XRef of the GPR (spec, X, Y, noise).  K: the kernel matrix if it is not cr._K64(spec, X) (a network: the oracle's)."""
    X = np.asarray(X, dtype=np.float64)
    n, r = Y.shape
    Ky = (cr._K64(spec, X) if K is None else K) + noise * np.eye(n)
    a, Kinv, lml, _ = _weights(Ky, Y, "chol")
    g = grad_x_from(a @ a.T - r * Kinv, spec, X, input_vjp)
    a2, Kinv2, _, lam = _weights(Ky, Y, "eigh")
    g2 = grad_x_from(a2 @ a2.T - r * Kinv2, spec, X, input_vjp)
    spread = float(np.abs(g - g2).max() / max(1.0, np.abs(g).max()))
    if extra_spread is not None:
        spread += extra_spread(a @ a.T - r * Kinv)
    return XRef(g, lml, a, Kinv, float(lam[-1] / lam[0]), spread)


def lml_longdouble(spec, X, Y, noise):
    """the LML in np.longdouble throughout (kernel values, a textbook Cholesky, the solves): for central differences"""
    ld = np.longdouble
    n, r = Y.shape
    A = np.asarray(cr.K(spec, np.asarray(X, dtype=ld), dtype=ld), dtype=ld) + ld(noise) * np.eye(n, dtype=ld)
    L = np.zeros((n, n), dtype=ld)
    for j in range(n):
        L[j, j] = np.sqrt(A[j, j] - np.dot(L[j, :j], L[j, :j]))
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    al = np.zeros((n, r), dtype=ld)
    Yl = np.asarray(Y, dtype=ld)
    for i in range(n):
        al[i] = (Yl[i] - L[i, :i] @ al[:i]) / L[i, i]
    return -ld(0.5) * n * r * np.log(2 * ld(np.pi)) - r * np.sum(np.log(np.diag(L))) - ld(0.5) * np.sum(al * al)


def central_differences(spec, X, Y, noise, h=1e-6):
    """d LML / d X by central differences of lml_longdouble with one Richardson step (error O(h^4) + 1e-19 / h)"""
    ld = np.longdouble
    X = np.asarray(X, dtype=ld)
    G = np.zeros(X.shape, dtype=ld)

    def f(i, d, step):
        Xp = X.copy()
        Xp[i, d] += ld(step)
        return lml_longdouble(spec, Xp, Y, noise)
    for i in range(X.shape[0]):
        for d in range(X.shape[1]):
            d1 = (f(i, d, h) - f(i, d, -h)) / (2 * ld(h))
            d2 = (f(i, d, 2 * h) - f(i, d, -2 * h)) / (4 * ld(h))
            G[i, d] = (4 * d1 - d2) / 3
    return np.asarray(G, dtype=np.float64)


# ---- Neural Kernel Network: d k / d x_i by differences of the oracle's kernel --------------------------------------------------
def _nkn_terms(ospec, W, X, h):
    G = np.zeros_like(X)
    for d in range(X.shape[1]):
        E = np.zeros_like(X)
        E[:, d] = h
        G[:, d] = np.sum(W * (orc.K(ospec, X + E, X) - orc.K(ospec, X - E, X)), 1) / (2 * h)
    return G


def nkn_input_vjp(ospec, W, X, h=3e-5):
    """sum_j W_ij d k(x_i, x_j) / d x_i of an oracle spec (no White among its primitives: K(X + h, X) has no diagonal term).  The
    Matern primitives are only a few times differentiable at r = 0, where the diagonal terms sit: the step is short, and the
    result is compared with twice the step (nkn_ref) rather than trusted for its order."""
    return (4 * _nkn_terms(ospec, W, X, h) - _nkn_terms(ospec, W, X, 2 * h)) / 3


def nkn_ref(ospec, X, Y, noise):
    def extra(W):        # the difference scheme's own error: the same W at twice the step length
        a = grad_x_from(W, ospec, X, lambda s, V, X_: nkn_input_vjp(s, V, X_, 3e-5))
        b = grad_x_from(W, ospec, X, lambda s, V, X_: nkn_input_vjp(s, V, X_, 6e-5))
        return float(np.abs(a - b).max() / max(1.0, np.abs(a).max()))
    return grad_x_ref(ospec, X, Y, noise, K=orc.K(ospec, X), input_vjp=lambda s, W, X_: nkn_input_vjp(s, W, X_), extra_spread=extra)


# ---- the input sets of the GPU tests ------------------------------------------------------------------------------------------
def data(n, d, r, seed, origin=False, scale=1.0):
    rng = np.random.default_rng(seed)
    X = scale * rng.standard_normal((n, d))
    if origin:
        X[n // 2] = 0.0                      # a real point at the origin: only the padding mask tells it from a padded column
    Y = np.sin(X @ rng.standard_normal((d, r))) + 0.1 * rng.standard_normal((n, r))
    return X, Y


def alone(gpf, d=3):
    """every kernel alone (and the two smallest combinations) over d = 3 columns; obs_var per kernel keeps cond(K_y) small where
    Kdiag grows with |x|^2"""
    k = gpf.kernels
    ls = np.linspace(0.8, 1.7, d)
    w = np.array([0.7, -0.4, 0.5])[:d]
    return {
        "rbf_ard": (k.RBF(d, variance=1.3, lengthscales=ls, ARD=True), 0.1),
        "matern12": (k.Matern12(d, variance=0.7, lengthscales=ls * 1.2, ARD=True), 0.1),
        "matern32": (k.Matern32(d, variance=1.1, lengthscales=ls * 1.3, ARD=True), 0.1),
        "matern52": (k.Matern52(d, variance=0.9, lengthscales=ls * 1.5, ARD=True), 0.1),
        "exponential": (k.Exponential(d, variance=1.2, lengthscales=ls * 0.9, ARD=True), 0.1),
        "ratquad": (k.RatQuad(d, alpha=1.7, variance=0.9, lengthscales=ls * 1.1, ARD=True), 0.1),
        "periodic": (k.Periodic(d, period=2.5, variance=0.8, lengthscales=1.2), 0.1),
        "linear": (k.Linear(d, variance=np.array([0.5, 0.3, 0.4])[:d], ARD=True), 0.3),
        "polynomial": (k.Polynomial(d, degree=2.0, variance=np.array([0.2, 0.15, 0.1])[:d], offset=0.8, ARD=True), 0.5),
        "cosine": (k.Cosine(d, variance=0.9, lengthscales=ls * 1.4, ARD=True, weights=w), 0.2),
        "arccosine0": (k.ArcCosine(d, order=0, variance=0.8, weight_variances=np.array([0.6, 0.9, 0.4])[:d], bias_variance=0.7, ARD=True), 0.2),
        "arccosine1": (k.ArcCosine(d, order=1, variance=0.6, weight_variances=np.array([0.6, 0.9, 0.4])[:d], bias_variance=0.7, ARD=True), 0.3),
        "arccosine2": (k.ArcCosine(d, order=2, variance=0.3, weight_variances=np.array([0.3, 0.4, 0.2])[:d], bias_variance=0.5, ARD=True), 0.5),
        "white_plus_rbf": (k.Sum([k.White(d, variance=0.2), k.RBF(d, variance=1.1, lengthscales=ls, ARD=True)]), 0.1),
        "constant_times_rbf": (k.Product([k.Constant(d, variance=0.4), k.RBF(d, variance=1.1, lengthscales=ls, ARD=True)]), 0.1),
    }


def four_prims(gpf, d=3):
    """a 4-primitive Sum / Product: the largest program the simple kernel takes"""
    k = gpf.kernels
    ls = np.linspace(0.8, 1.7, d)
    return k.Sum([k.Product([k.RBF(d, variance=1.2, lengthscales=ls, ARD=True), k.Periodic(d, period=3.0, variance=0.9, lengthscales=1.5)]),
                  k.Matern32(2, variance=0.7, lengthscales=[2.0, 1.1], ARD=True, active_dims=[2, 0]), k.White(d, variance=0.2)])


def spec_of(kern, d_all):
    return cr.spec_of(kern, d_all)


def noise_of(gpf, obs_var):
    return float(np.squeeze(gpf.likelihoods.Gaussian(var=obs_var).variance))


EDGE_N = (1, 2, 33, 65, 127, 128, 129, 257)
ALONE_N = (33, 129)
ROUTE_N = (300, 1500)


def reference(gpf, key, kern, X, Y, obs_var):
    """cached XRef of a GPR case; key names the case"""
    if key not in _cache:
        _cache[key] = grad_x_ref(spec_of(kern, X.shape[1]), X, Y, noise_of(gpf, obs_var))
    return _cache[key]


def plain_cases(gpf):
    """{key: (kern, X, Y, obs_var)} of every case of the GPU tests whose reference is grad_x_ref on cr's analytic forms"""
    out = {}
    al = alone(gpf)
    for n in EDGE_N:
        for r in (1, 3):
            for name in ("rbf_ard", "matern12"):
                X, Y = data(n, 3, r, 100 + n + r, origin=(n == 129 and r == 1))
                out["edge-%s-%d-%d" % (name, n, r)] = (al[name][0], X, Y, al[name][1])
    for n in ALONE_N:
        for name, (kern, ov) in al.items():
            if name in ("rbf_ard", "matern12"):
                continue
            X, Y = data(n, 3, 2, 200 + n, scale=0.8)
            out["alone-%s-%d" % (name, n)] = (kern, X, Y, ov)
    k = gpf.kernels
    X, Y = data(129, 1, 2, 31)
    out["dim-1"] = (k.Matern52(1, variance=1.1, lengthscales=0.9), X, Y, 0.1)
    X, Y = data(129, 32, 2, 32, scale=0.5)
    out["dim-32"] = (k.RBF(32, variance=1.2, lengthscales=np.linspace(1.5, 3.0, 32), ARD=True), X, Y, 0.1)
    X, Y = data(129, 4, 2, 33)
    out["dim-subset"] = (k.RBF(2, variance=1.1, lengthscales=[0.9, 1.4], ARD=True, active_dims=[2, 0]), X, Y, 0.1)
    X, Y = data(129, 3, 2, 34)
    out["four"] = (four_prims(gpf), X, Y, 0.1)
    for n in ROUTE_N:
        for r in (2, 17):
            X, Y = data(n, 3, r, 300 + n)                 # (the same X for both R: X is drawn first)
            out["route-%d-%d" % (n, r)] = (al["rbf_ard"][0], X, Y, 0.1)
    X, Y = data(2176, 3, 2, 35)
    out["route-2176-2"] = (al["rbf_ard"][0], X, Y, 0.1)
    X, Y = data(1409, 3, 1, 36)
    out["slices-1409"] = (al["matern32"][0], X, Y, 0.1)
    return out


def general_cases(gpf):
    """{key: (kern, X, Y, obs_var)} of the programs the general kernel takes: the 6- and 8-primitive programs of the existing
    gradient / VJP tests and RBF * Coregion (label column 3 of 4; one output index carried by no row)"""
    import _grad_ref as gr
    from test_gpu_kmat_vjp import _programs
    out = {}
    X, Y = data(129, 3, 2, 41)
    out["six"] = (gr.six_case(gpf, 3)[0], X, Y, 0.1)
    X, Y = data(129, 3, 2, 42)
    out["eight"] = (_programs(gpf)["eight"], X, Y, 0.1)
    rng = np.random.default_rng(43)
    P, R = 3, 2
    co = gpf.kernels.Coregion(1, P, R, active_dims=[3])
    co._W.assign(rng.standard_normal((P, R)))
    co._kappa.assign(0.5 + rng.random(P))
    rbf = gpf.kernels.RBF(3, variance=1.2, lengthscales=np.array([0.8, 1.1, 1.6]), ARD=True, active_dims=[0, 1, 2])
    Xc = rng.standard_normal((129, 4))
    Xc[:, 3] = cr.draw_labels(rng, 129, P, skip=1)
    Yc = np.sin(Xc[:, :3] @ rng.standard_normal((3, 2))) * (1.0 + 0.3 * np.floor(Xc[:, 3:4])) + 0.1 * rng.standard_normal((129, 2))
    out["rbf_times_coregion"] = (rbf * co, Xc, Yc, 0.1)
    return out


def nkn_case(gpf, n=65, d=3):
    """(kern, oracle spec, X, Y, obs_var) of the Neural Kernel Network of the existing gradient tests"""
    from test_gpu_parity import _nkn_case
    kern, ospec = _nkn_case(gpf, d, False)
    X, Y = data(n, d, 1, 44)
    return kern, ospec, X, Y, 0.1


def nkn_reference(gpf, n=65):
    key = ("nkn", n)
    if key not in _cache:
        kern, ospec, X, Y, ov = nkn_case(gpf, n)
        _cache[key] = nkn_ref(ospec, X, Y, noise_of(gpf, ov))
    return _cache[key]


def gplvm_clusters(n=200, seed=3):
    """(Y, labels) of the synthetic clusters of examples/gplvm.py"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_example_gplvm", os.path.join(ROOT, "examples", "gplvm.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.synthetic(n, seed=seed)


def nn_agreement(X, labels):
    """fraction of points whose nearest neighbour (other than itself) in X carries the same label"""
    D = np.sum((X[:, None, :] - X[None, :, :]) ** 2, -1)
    np.fill_diagonal(D, np.inf)
    return float(np.mean(labels[np.argmin(D, 1)] == labels))
