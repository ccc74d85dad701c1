"""Numpy restatement of the kernels (reference gpflowSlim/kernels.py:327-610, 769-819), op for op, with their analytic
parameter and input derivatives -- the yardstick of tests/test_gpu_newkernels.py and tests/test_gpu_kmat_vjp.py, itself checked
on the CPU against central differences and against the same formulas at 50 digits (tests/test_kern_ref_cpu.py).

A kernel is a *spec*: a leaf ``{"type", "dims", ...constrained parameter values...}`` or ``("sum" | "product", [specs])``.

    ratquad     variance, lengthscales, alpha   variance * (1 + 0.5 * r2 * (1 / alpha)) ** (-alpha)            :470-471
    linear      variance                        (X * variance) @ X2.T                                           :499-505
    polynomial  variance, offset, degree        (linear + offset) ** degree                                     :550-551
    rbf         variance, lengthscales          variance * exp(-r2 / 2)                                         :436-439
    periodic    variance, lengthscales, period  variance * exp(-0.5 * sum_d (sin(pi (x_d - x'_d) / p) / l)^2)  :806-819
    constant    variance                        variance everywhere                                             :345-350
    white       variance                        variance on i == j of K(X, X), 0 in K(X, X2)                    :332-338
    matern12    variance, lengthscales          variance * exp(-rad)                                            :573-577
    exponential variance, lengthscales          variance * exp(-rad / 2)                                        :561-565
    matern32    variance, lengthscales          variance * (1 + sqrt3 rad) exp(-sqrt3 rad)                      :589-594
    matern52    variance, lengthscales          variance * (1 + sqrt5 rad + 5/3 rad^2) exp(-sqrt5 rad)          :605-610

r2 = max(|a|^2 + |b|^2 - 2 a.b, 0) with a = x / lengthscales (Stationary.square_dist, :408-421: the clamp included) and
rad = sqrt(r2 + 1e-12) (Stationary.euclid_dist, :424-426) for the VALUES K / leaf_K return by default.  Every DERIVATIVE here
(and K(..., diff=True), the sibling values they are multiplied with) takes r2 = sum_d ((x_d - x'_d) / l_d)^2 from the coordinate
differences: the expanded form has no correct digit left at a separation of 1e-5, and rad's 1e-12 turns an error of 1e-15 in
r2 near 0 into 5e-10 in a Matern-1/2 value.
``variance`` / ``lengthscales`` of linear, polynomial and the stationary kernels are a scalar (isotropic) or one value per
active dim.

Slots are the device's gradient slots (include/gpflowslim_hip.h): per leaf in program order, one per *active dim* for
lengthscales and Linear / Polynomial variances whether the parameter is a scalar or not; ``fold`` sums them onto the
parameter elements in ``kern.parameters`` order.  Stationary kernels: [variance, one per active dim]; Periodic: [variance,
lengthscale, period]; White, Constant: [variance].
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


STATIONARY = ("rbf", "ratquad", "matern12", "matern32", "matern52", "exponential")
_SQRT3, _SQRT5 = np.sqrt(3.0), np.sqrt(5.0)


def scaled_diff(leaf, X, X2):
    """(x_d - x'_d) / l_d per active dim, [n, m, nd]: the difference first (exact for nearby points), then the scale"""
    ls = _per_dim(leaf["lengthscales"], len(leaf["dims"]))
    A = _cols(leaf, X)
    B = A if X2 is None else _cols(leaf, X2)
    return (A[:, None, :] - B[None, :, :]) / ls


def _stationary(leaf, r2):
    """(k, d k / d r2) of a stationary leaf at the squared scaled distance r2"""
    t, v = leaf["type"], leaf["variance"]
    if t == "rbf":
        k = v * np.exp(-r2 / 2.0)
        return k, -0.5 * k
    if t == "ratquad":
        u = 0.5 * r2 * (1.0 / leaf["alpha"])
        k = v * np.power(1.0 + u, -1.0 * leaf["alpha"])
        return k, -0.5 * k / (1.0 + u)
    rad = np.sqrt(r2 + 1e-12)
    if t == "matern12":
        k = v * np.exp(-rad)
        return k, -k / (2.0 * rad)
    if t == "exponential":
        k = v * np.exp(-0.5 * rad)
        return k, -k / (4.0 * rad)
    if t == "matern32":
        e = v * np.exp(-_SQRT3 * rad)
        return (1.0 + _SQRT3 * rad) * e, -1.5 * e
    if t == "matern52":
        e = v * np.exp(-_SQRT5 * rad)
        return (1.0 + _SQRT5 * rad + 5.0 / 3.0 * np.square(rad)) * e, -(5.0 / 6.0) * (1.0 + _SQRT5 * rad) * e
    raise ValueError(t)


def _periodic_arg(leaf, X, X2):
    """u_d = pi (x_d - x'_d) / period, [n, m, nd]"""
    A = _cols(leaf, X)
    B = A if X2 is None else _cols(leaf, X2)
    return np.pi * (A[:, None, :] - B[None, :, :]) / leaf["period"]


def leaf_K(leaf, X, X2=None, diff=False):
    """diff: r2 of the stationary kernels from the coordinate differences instead of Stationary.square_dist"""
    t = leaf["type"]
    if t in STATIONARY:
        r2 = np.sum(np.square(scaled_diff(leaf, X, X2)), -1) if diff else square_dist(leaf, X, X2)
        return _stationary(leaf, r2)[0]
    if t == "white":
        n = np.shape(X)[0]
        return float(leaf["variance"]) * np.eye(n) if X2 is None else np.zeros((n, np.shape(X2)[0]))
    if t == "linear":
        return _linear(leaf, X, X2)
    if t == "polynomial":
        return (_linear(leaf, X, X2) + leaf["offset"]) ** leaf["degree"]
    if t == "periodic":
        r = _periodic_arg(leaf, X, X2)
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


def K(spec, X, X2=None, diff=False):
    if isinstance(spec, dict):
        return leaf_K(spec, X, X2, diff)
    op, children = spec
    out = K(children[0], X, X2, diff)
    for c in children[1:]:
        out = out + K(c, X, X2, diff) if op == "sum" else out * K(c, X, X2, diff)
    return out


def Kdiag(spec, X):
    if isinstance(spec, dict):
        return leaf_Kdiag(spec, X)
    op, children = spec
    out = Kdiag(children[0], X)
    for c in children[1:]:
        out = out + Kdiag(c, X) if op == "sum" else out * Kdiag(c, X)
    return out


def _outer(leaf, X, X2, d):
    A = _cols(leaf, X)[:, d]
    B = A if X2 is None else _cols(leaf, X2)[:, d]
    return A[:, None] * B[None, :]


def leaf_dK(leaf, X, X2=None):
    """d K / d slot, one matrix per slot of this leaf"""
    t = leaf["type"]
    nd = len(leaf["dims"])
    if t in STATIONARY:
        ls = _per_dim(leaf["lengthscales"], nd)
        D = scaled_diff(leaf, X, X2)
        r2 = np.sum(np.square(D), -1)
        Kv, dK_dr2 = _stationary(leaf, r2)
        out = [Kv / leaf["variance"]]
        out += [dK_dr2 * (-2.0 * np.square(D[:, :, d]) / ls[d]) for d in range(nd)]             # d r2 / d l_d
        if t == "ratquad":
            u = 0.5 * r2 / leaf["alpha"]
            out.append(Kv * (u / (1.0 + u) - np.log1p(u)))
        return out
    if t == "periodic":
        l, p = float(leaf["lengthscales"]), float(leaf["period"])
        U = _periodic_arg(leaf, X, X2)
        S = np.sum(np.square(np.sin(U)), -1)
        Kv = leaf["variance"] * np.exp(-0.5 * S / l ** 2)
        # d S / d p = -sum_d sin(2 u_d) u_d / p
        return [Kv / leaf["variance"], Kv * S / l ** 3, Kv / (2.0 * l ** 2) * np.sum(np.sin(2.0 * U) * U, -1) / p]
    if t == "white":
        return [leaf_K(leaf, X, X2) / leaf["variance"]]
    if t == "linear":
        return [_outer(leaf, X, X2, d) for d in range(nd)]
    if t == "polynomial":
        deg = leaf["degree"]
        core = deg * (_linear(leaf, X, X2) + leaf["offset"]) ** (deg - 1)
        return [core * _outer(leaf, X, X2, d) for d in range(nd)] + [core]
    if t == "constant":
        return [np.ones_like(leaf_K(leaf, X, X2))]
    raise NotImplementedError("no derivatives for %s here" % t)


def leaves_with_cofactors(spec, X, X2=None, cof=None):
    """(leaf, d K / d K_leaf entry by entry) in program order: the product of the siblings' values (from coordinate
    differences) under every Product on the way down; None: 1"""
    if isinstance(spec, dict):
        yield spec, cof
        return
    op, children = spec
    for i, c in enumerate(children):
        cc = cof
        if op == "product":
            for j, other in enumerate(children):
                if j != i:
                    v = K(other, X, X2, diff=True)
                    cc = v if cc is None else cc * v
        for item in leaves_with_cofactors(c, X, X2, cc):
            yield item


def dK(spec, X, X2=None):
    """d K / d slot for every slot of the program, in slot order"""
    return [g if cof is None else g * cof for leaf, cof in leaves_with_cofactors(spec, X, X2) for g in leaf_dK(leaf, X, X2)]


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
        if t in STATIONARY:
            out.append(slots[s]); s += 1
            out += per_dim("lengthscales")
            if t == "ratquad":
                out.append(slots[s]); s += 1
        elif t in ("linear", "polynomial"):
            out += per_dim("variance")
            if t == "polynomial":
                out.append(slots[s]); s += 1
        elif t in ("constant", "white"):
            out.append(slots[s]); s += 1
        elif t == "periodic":
            out += list(slots[s:s + 3]); s += 3
        else:
            raise NotImplementedError(t)
    assert s == len(slots)
    return np.array(out)


def vjp_slots(spec, W, X, X2=None, absolute=False):
    """sum_ij W_ij d K_ij / d slot; absolute: sum_ij |W_ij| |d K_ij / d slot|, the size of what is being summed"""
    if absolute:
        return np.array([np.sum(np.abs(W * g)) for g in dK(spec, X, X2)])
    return np.array([np.sum(W * g) for g in dK(spec, X, X2)])


def _leaf_input_terms(leaf, W, X, X2):
    """(column of X, T [n, m]) with T_ij = W_ij d k(x_i, x'_j) / d x_i[column], one pair per active dim"""
    t = leaf["type"]
    nd = len(leaf["dims"])
    if t in ("white", "constant"):
        return
    if t in STATIONARY:
        ls = _per_dim(leaf["lengthscales"], nd)
        D = scaled_diff(leaf, X, X2)
        Q = W * _stationary(leaf, np.sum(np.square(D), -1))[1]
        for d, col in enumerate(leaf["dims"]):
            yield col, Q * (2.0 * D[:, :, d] / ls[d])                                          # d r2 / d x_id
        return
    if t == "periodic":
        l, p = float(leaf["lengthscales"]), float(leaf["period"])
        U = _periodic_arg(leaf, X, X2)
        Q = W * leaf["variance"] * np.exp(-0.5 * np.sum(np.square(np.sin(U)), -1) / l ** 2) * (-0.5 / l ** 2)
        for d, col in enumerate(leaf["dims"]):
            yield col, Q * (np.sin(2.0 * U[:, :, d]) * (np.pi / p))                            # d S / d x_id
        return
    B = _cols(leaf, X if X2 is None else X2)
    v = _per_dim(leaf["variance"], nd)
    core = np.ones_like(W) if t == "linear" else leaf["degree"] * (_linear(leaf, X, X2) + leaf["offset"]) ** (leaf["degree"] - 1)
    for d, col in enumerate(leaf["dims"]):
        yield col, (W * core) * (B[:, d] * v[d])[None, :]


def input_vjp(spec, W, X, X2=None, absolute=False):
    """G[i, :] = sum_j W_ij d k(x_i, x'_j) / d x_i (first argument only), analytically, for a leaf or a tree (the chain factor of
    a leaf: leaves_with_cofactors); absolute: sum_j |W_ij| |d k(x_i, x'_j) / d x_i| instead"""
    X = np.asarray(X, dtype=np.float64)
    terms = {}                                               # column -> W_ij d K_ij / d x_i[column] of the whole tree
    for leaf, cof in leaves_with_cofactors(spec, X, X2):
        for col, T in _leaf_input_terms(leaf, W if cof is None else W * cof, X, X2):
            terms[col] = T if col not in terms else terms[col] + T
    G = np.zeros_like(X)
    for col, T in terms.items():
        G[:, col] = np.sum(np.abs(T) if absolute else T, 1)
    return G


def spec_of(kern, d_all):
    """the reference spec of a kernel tree, from the constrained values the product itself holds"""
    import gpflowSlim as gpf
    k = gpf.kernels
    if isinstance(kern, (k.Sum, k.Product)):
        assert not kern.const_list
        return ("sum" if isinstance(kern, k.Sum) else "product", [spec_of(c, d_all) for c in kern.kern_list])

    def val(x):
        x = np.asarray(x, dtype=np.float64)
        return x.copy() if x.size > 1 else float(np.squeeze(x))
    if isinstance(kern, (k.White, k.Constant)):
        return {"type": "white" if isinstance(kern, k.White) else "constant", "dims": [], "variance": val(kern.variance)}
    dims = kern._dims(False, d_all)
    if isinstance(kern, k.RatQuad):
        return {"type": "ratquad", "dims": dims, "variance": val(kern.variance), "lengthscales": val(kern.lengthscales), "alpha": val(kern.alpha)}
    if isinstance(kern, k.Polynomial):
        return {"type": "polynomial", "dims": dims, "variance": val(kern.variance), "offset": val(kern.offset), "degree": kern.degree}
    if isinstance(kern, k.Linear):
        return {"type": "linear", "dims": dims, "variance": val(kern.variance)}
    if isinstance(kern, k.Periodic):
        return {"type": "periodic", "dims": dims, "variance": val(kern.variance), "lengthscales": val(kern.lengthscales), "period": val(kern.period)}
    for name in ("RBF", "Matern12", "Matern32", "Matern52", "Exponential"):
        if type(kern) is getattr(k, name):
            return {"type": name.lower(), "dims": dims, "variance": val(kern.variance), "lengthscales": val(kern.lengthscales)}
    raise TypeError(type(kern))


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
