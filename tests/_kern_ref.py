"""Numpy restatement of RatQuad, Linear and Polynomial (reference gpflowSlim/kernels.py:447-554) and of what the tests
combine them with, op for op, with their analytic parameter derivatives -- the yardstick of tests/test_gpu_newkernels.py,
itself checked against central differences on the CPU (tests/test_kern_ref_cpu.py).

A kernel is a *spec*: a leaf ``{"type", "dims", ...constrained parameter values...}`` or ``("sum" | "product", [specs])``.

    ratquad     variance, lengthscales, alpha   variance * (1 + 0.5 * r2 * (1 / alpha)) ** (-alpha)            :470-471
    linear      variance                        (X * variance) @ X2.T                                           :499-505
    polynomial  variance, offset, degree        (linear + offset) ** degree                                     :550-551
    rbf         variance, lengthscales          variance * exp(-r2 / 2)                                         :436-439
    periodic    variance, lengthscales, period  variance * exp(-0.5 * sum_d (sin(pi (x_d - x'_d) / p) / l)^2)  :806-819
    constant    variance                        variance everywhere                                             :345-350

r2 = max(|a|^2 + |b|^2 - 2 a.b, 0) with a = x / lengthscales (Stationary.square_dist, :408-421: the clamp included).
``variance`` / ``lengthscales`` of linear, polynomial, rbf and ratquad are a scalar (isotropic) or one value per active dim.

Slots are the device's gradient slots (include/gpflowslim_hip.h): per leaf in program order, one per *active dim* for
lengthscales and Linear / Polynomial variances whether the parameter is a scalar or not; ``fold`` sums them onto the
parameter elements in ``kern.parameters`` order.  Periodic has values only (the tests differentiate no Periodic here).
"""
import numpy as np
import scipy.linalg as sl


def _cols(leaf, X):
    return np.asarray(X, dtype=np.float64)[:, leaf["dims"]]


def _per_dim(value, nd):
    v = np.atleast_1d(np.asarray(value, dtype=np.float64)).ravel()
    return v if v.size == nd else np.full(nd, v[0])


def square_dist(leaf, X, X2):
    """kernels.py:408-421"""
    ls = _per_dim(leaf["lengthscales"], len(leaf["dims"]))
    A = _cols(leaf, X) / ls
    B = A if X2 is None else _cols(leaf, X2) / ls
    As = np.sum(np.square(A), 1)
    Bs = np.sum(np.square(B), 1)
    dist = -2.0 * (A @ B.T) + (As[:, None] + Bs[None, :])
    return np.maximum(dist, 0.0)


def _linear(leaf, X, X2):
    v = _per_dim(leaf["variance"], len(leaf["dims"]))
    A = _cols(leaf, X)
    B = A if X2 is None else _cols(leaf, X2)
    return (A * v) @ B.T


def leaf_K(leaf, X, X2=None):
    t = leaf["type"]
    if t == "ratquad":
        r2 = square_dist(leaf, X, X2)
        return leaf["variance"] * np.power(1.0 + 0.5 * r2 * (1.0 / leaf["alpha"]), -1.0 * leaf["alpha"])
    if t == "linear":
        return _linear(leaf, X, X2)
    if t == "polynomial":
        return (_linear(leaf, X, X2) + leaf["offset"]) ** leaf["degree"]
    if t == "rbf":
        return leaf["variance"] * np.exp(-square_dist(leaf, X, X2) / 2.0)
    if t == "periodic":
        A = _cols(leaf, X)
        B = A if X2 is None else _cols(leaf, X2)
        r = np.pi * (A[:, None, :] - B[None, :, :]) / leaf["period"]
        return leaf["variance"] * np.exp(-0.5 * np.sum(np.square(np.sin(r) / leaf["lengthscales"]), -1))
    if t == "constant":
        n = np.shape(X)[0]
        return np.full((n, n if X2 is None else np.shape(X2)[0]), float(leaf["variance"]))
    raise ValueError(t)


def leaf_Kdiag(leaf, X):
    """kernels.py:428-429, 507-510, 553-554, 803-804"""
    t = leaf["type"]
    if t in ("linear", "polynomial"):
        v = _per_dim(leaf["variance"], len(leaf["dims"]))
        s = np.sum(np.square(_cols(leaf, X)) * v, 1)
        return s if t == "linear" else (s + leaf["offset"]) ** leaf["degree"]
    return np.full(np.shape(X)[0], float(leaf["variance"]))


def K(spec, X, X2=None):
    if isinstance(spec, dict):
        return leaf_K(spec, X, X2)
    op, children = spec
    out = K(children[0], X, X2)
    for c in children[1:]:
        out = out + K(c, X, X2) if op == "sum" else out * K(c, X, X2)
    return out


def Kdiag(spec, X):
    if isinstance(spec, dict):
        return leaf_Kdiag(spec, X)
    op, children = spec
    out = Kdiag(children[0], X)
    for c in children[1:]:
        out = out + Kdiag(c, X) if op == "sum" else out * Kdiag(c, X)
    return out


def _diff2(leaf, X, X2, d):
    """(x_d - x'_d)^2 of active dim number d, unscaled"""
    A = _cols(leaf, X)[:, d]
    B = A if X2 is None else _cols(leaf, X2)[:, d]
    return np.square(A[:, None] - B[None, :])


def _outer(leaf, X, X2, d):
    A = _cols(leaf, X)[:, d]
    B = A if X2 is None else _cols(leaf, X2)[:, d]
    return A[:, None] * B[None, :]


def leaf_dK(leaf, X, X2=None):
    """d K / d slot, one matrix per slot of this leaf"""
    t = leaf["type"]
    nd = len(leaf["dims"])
    if t in ("ratquad", "rbf"):
        Kv = leaf_K(leaf, X, X2)
        ls = _per_dim(leaf["lengthscales"], nd)
        r2 = square_dist(leaf, X, X2)
        if t == "rbf":
            dK_dr2 = -0.5 * Kv
        else:
            u = 0.5 * r2 / leaf["alpha"]
            dK_dr2 = -0.5 * Kv / (1.0 + u)
        out = [Kv / leaf["variance"]]
        out += [dK_dr2 * (-2.0 * _diff2(leaf, X, X2, d) / ls[d] ** 3) for d in range(nd)]      # d r2 / d l_d
        if t == "ratquad":
            out.append(Kv * (u / (1.0 + u) - np.log1p(u)))
        return out
    if t == "linear":
        return [_outer(leaf, X, X2, d) for d in range(nd)]
    if t == "polynomial":
        deg = leaf["degree"]
        core = deg * (_linear(leaf, X, X2) + leaf["offset"]) ** (deg - 1)
        return [core * _outer(leaf, X, X2, d) for d in range(nd)] + [core]
    if t == "constant":
        return [np.ones_like(leaf_K(leaf, X, X2))]
    raise NotImplementedError("no derivatives for %s here" % t)


def dK(spec, X, X2=None):
    """d K / d slot for every slot of the program, in slot order"""
    if isinstance(spec, dict):
        return leaf_dK(spec, X, X2)
    op, children = spec
    if op == "sum":
        return [g for c in children for g in dK(c, X, X2)]
    vals = [K(c, X, X2) for c in children]
    out = []
    for i, c in enumerate(children):
        others = np.ones_like(vals[0])
        for j, v in enumerate(vals):
            if j != i:
                others = others * v
        out += [g * others for g in dK(c, X, X2)]
    return out


def leaves(spec):
    if isinstance(spec, dict):
        return [spec]
    return [l for c in spec[1] for l in leaves(c)]


def fold(spec, slots):
    """slot values -> one value per parameter element, in kern.parameters order (a scalar lengthscale / variance receives
    the sum of its per-dim slots)"""
    out, s = [], 0
    for leaf in leaves(spec):
        t, nd = leaf["type"], len(leaf["dims"])

        def per_dim(name):
            nonlocal s
            vals = list(slots[s:s + nd]); s += nd
            return vals if np.size(leaf[name]) > 1 else [np.sum(vals, axis=0)]
        if t in ("rbf", "ratquad"):
            out.append(slots[s]); s += 1
            out += per_dim("lengthscales")
            if t == "ratquad":
                out.append(slots[s]); s += 1
        elif t in ("linear", "polynomial"):
            out += per_dim("variance")
            if t == "polynomial":
                out.append(slots[s]); s += 1
        elif t == "constant":
            out.append(slots[s]); s += 1
        else:
            raise NotImplementedError(t)
    assert s == len(slots)
    return np.array(out)


def vjp_slots(spec, W, X, X2=None):
    """sum_ij W_ij d K_ij / d slot"""
    return np.array([np.sum(W * g) for g in dK(spec, X, X2)])


def input_vjp(spec, W, X, X2=None):
    """G[i, :] = sum_j W_ij d k(x_i, x'_j) / d x_i (first argument only), for a single leaf, analytically"""
    assert isinstance(spec, dict)
    leaf, t = spec, spec["type"]
    X = np.asarray(X, dtype=np.float64)
    B = X if X2 is None else np.asarray(X2, dtype=np.float64)
    G = np.zeros_like(X)
    nd = len(leaf["dims"])
    if t == "ratquad":
        ls = _per_dim(leaf["lengthscales"], nd)
        Kv = leaf_K(leaf, X, X2)
        Q = W * (-0.5 * Kv / (1.0 + 0.5 * square_dist(leaf, X, X2) / leaf["alpha"]))
        for d, col in enumerate(leaf["dims"]):
            G[:, col] += np.sum(Q * 2.0 * (X[:, col][:, None] - B[:, col][None, :]), 1) / ls[d] ** 2
        return G
    v = _per_dim(leaf["variance"], nd)
    core = np.ones_like(W) if t == "linear" else leaf["degree"] * (_linear(leaf, X, X2) + leaf["offset"]) ** (leaf["degree"] - 1)
    for d, col in enumerate(leaf["dims"]):
        G[:, col] += (W * core) @ B[:, col] * v[d]
    return G


def lml_and_grad(spec, X, Y, noise):
    """GPR log marginal likelihood (LAPACK Cholesky of K + noise I) and its analytic gradient: per slot
    1/2 sum_ij (a a^T - r K_y^-1)_ij d K_ij / d slot, and the same with d K_y / d noise = I"""
    n, r = Y.shape
    Ky = K(spec, X) + noise * np.eye(n)
    L = sl.cholesky(Ky, lower=True)
    a = sl.cho_solve((L, True), Y)
    lml = -0.5 * n * r * np.log(2.0 * np.pi) - r * np.sum(np.log(np.diag(L))) - 0.5 * np.sum(Y * a)
    W = a @ a.T - r * sl.cho_solve((L, True), np.eye(n))
    slots = np.array([0.5 * np.sum(W * g) for g in dK(spec, X)])
    return lml, slots, 0.5 * np.trace(W)


def gpr_predict(spec, X, Y, noise, Xs, full_cov=False):
    """models/gpr.py:119-131"""
    n = X.shape[0]
    L = sl.cholesky(K(spec, X) + noise * np.eye(n), lower=True)
    A = sl.solve_triangular(L, K(spec, X, Xs), lower=True)
    V = sl.solve_triangular(L, Y, lower=True)
    mean = A.T @ V
    var = K(spec, Xs) - A.T @ A if full_cov else Kdiag(spec, Xs) - np.sum(np.square(A), 0)
    return mean, var


def conditional(spec, Xn, Z, f, white, jitter=1e-6):
    """conditionals.py:60-121 without q_sqrt, marginal variances: (fmean [N, K], fvar [N, K])"""
    m = Z.shape[0]
    Lm = sl.cholesky(K(spec, Z) + jitter * np.eye(m), lower=True)
    A = sl.solve_triangular(Lm, K(spec, Z, Xn), lower=True)
    fvar = Kdiag(spec, Xn) - np.sum(np.square(A), 0)
    if not white:
        A = sl.solve_triangular(Lm.T, A, lower=False)
    return A.T @ f, np.tile(fvar[:, None], [1, f.shape[1]])
