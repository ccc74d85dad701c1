"""Numpy restatement of Cosine and ArcCosine (reference gpflowSlim/kernels.py:617-646, 649-766), op for op, with their analytic
parameter and input derivatives, in float64 or long double -- the yardstick of tests/test_gpu_cosine_arccosine.py, itself
checked on the CPU against the same formulas at 50 digits and against long-double central differences
(tests/test_kern_ref2_cpu.py).  Every other leaf type, and everything that does not depend on the leaf, is tests/_kern_ref.py.

    cosine     variance, lengthscales, weights                  variance * cos(a_i - a'_j),  a = sum_d x_d w_d / l_d  (the active
                                                                columns sliced FIRST: the deliberate difference from :634-636)
    arccosine  variance, bias_variance, weight_variances, order variance / pi * J_order(theta) * (n_i n'_j)^(order / 2)
               P_ij = sum_d w_d x_id x'_jd + b,  n_i = P_ii,  theta = acos(1e-15 + (1 - 2e-15) P_ij / sqrt(n_i) / sqrt(n'_j))

Slots (include/gpflowslim_hip.h): cosine [variance, l per active dim, w per active dim]; arccosine [variance, bias_variance,
w per active dim].  ArcCosine order 0 on the diagonal of K(X, X): cos(theta) does not depend on anything there, and every
derivative through it is exactly 0 (DESIGN: the reference's autodiff returns rounding noise times 2e7).
"""
import numpy as np
import scipy.linalg as sl

import _kern_ref as kr

JITTER = 1e-15
NEW = ("cosine", "arccosine")


def _cols(leaf, X, dtype):
    return np.asarray(X, dtype=dtype)[:, leaf["dims"]]


def _per_dim(value, nd, dtype):
    v = np.atleast_1d(np.asarray(value, dtype=dtype)).ravel()
    return v if v.size == nd else np.full(nd, v[0], dtype=dtype)


# ---- Cosine ------------------------------------------------------------------------------------------------------------------
def _cos_parts(leaf, X, X2, dtype):
    nd = len(leaf["dims"])
    ls = _per_dim(leaf["lengthscales"], nd, dtype)
    w = np.asarray(leaf["weights"], dtype=dtype).ravel()
    A = _cols(leaf, X, dtype)
    B = A if X2 is None else _cols(leaf, X2, dtype)
    prod = (A / ls) @ w
    prod2 = (B / ls) @ w
    r = prod[:, None] - prod2[None, :]
    return ls, w, A, B, r


def _pi(dtype):
    return np.pi if dtype == np.float64 else np.arccos(np.asarray(-1.0, dtype=dtype))


# ---- ArcCosine ---------------------------------------------------------------------------------------------------------------
def _J(order, theta):
    """kernels.py:727-738"""
    pi = _pi(theta.dtype)
    if order == 0:
        return pi - theta
    if order == 1:
        return np.sin(theta) + (pi - theta) * np.cos(theta)
    return 3. * np.sin(theta) * np.cos(theta) + (pi - theta) * (1. + 2. * np.cos(theta) ** 2)


def _arc_parts(leaf, X, X2, dtype):
    nd = len(leaf["dims"])
    w = _per_dim(leaf["weight_variances"], nd, dtype)
    b = np.asarray(leaf["bias_variance"], dtype=dtype)
    A = _cols(leaf, X, dtype)
    B = A if X2 is None else _cols(leaf, X2, dtype)
    ni = np.sum(w * np.square(A), 1) + b
    nj = np.sum(w * np.square(B), 1) + b
    P = (w * A) @ B.T + b
    cos_theta = P / np.sqrt(ni)[:, None] / np.sqrt(nj)[None, :]
    jit = np.asarray(JITTER, dtype=dtype)
    theta = np.arccos(jit + (1 - 2 * jit) * cos_theta)
    return w, b, A, B, ni, nj, P, cos_theta, theta


def arc_theta(leaf, X, X2=None, dtype=np.float64):
    return _arc_parts(leaf, X, X2, dtype)[-1]


def _arc_K(leaf, X, X2, dtype):
    w, b, A, B, ni, nj, P, cos_theta, theta = _arc_parts(leaf, X, X2, dtype)
    o = leaf["order"]
    v = np.asarray(leaf["variance"], dtype=dtype)
    return v * (1. / _pi(dtype)) * _J(o, theta) * np.sqrt(ni)[:, None] ** o * np.sqrt(nj)[None, :] ** o


def _arc_partials(leaf, X, X2, dtype):
    """(K, d K / d P, d K / d n_i, d K / d n_j), [n, m] each"""
    w, b, A, B, ni, nj, P, u, theta = _arc_parts(leaf, X, X2, dtype)
    o = leaf["order"]
    v = np.asarray(leaf["variance"], dtype=dtype)
    pi = _pi(dtype)
    kappa = 1 - 2 * np.asarray(JITTER, dtype=dtype)
    sij = np.sqrt(ni)[:, None] * np.sqrt(nj)[None, :]
    Kv = v * (1. / pi) * _J(o, theta) * sij ** o
    if o == 0:
        dJ = 1.0 / np.sin(theta)
        if X2 is None:
            dJ[np.diag_indices_from(dJ)] = 0.0
    elif o == 1:
        dJ = pi - theta
    else:
        dJ = 4.0 * _J(1, theta)
    Am = v / pi * kappa * dJ * sij ** o
    h = 0.5 * (o * Kv - Am * u)
    return Kv, Am / sij, h / ni[:, None], h / nj[None, :], w, A, B


# ---- leaves ------------------------------------------------------------------------------------------------------------------
def leaf_K(leaf, X, X2=None, dtype=np.float64, diff=False):
    t = leaf["type"]
    if t == "cosine":
        r = _cos_parts(leaf, X, X2, dtype)[-1]
        return np.asarray(leaf["variance"], dtype=dtype) * np.cos(r)
    if t == "arccosine":
        return _arc_K(leaf, X, X2, dtype)
    return kr.leaf_K(leaf, X, X2, diff)


def leaf_Kdiag(leaf, X, dtype=np.float64):
    t = leaf["type"]
    if t == "cosine":
        return np.full(np.shape(X)[0], leaf["variance"], dtype=dtype)
    if t == "arccosine":
        nd = len(leaf["dims"])
        w = _per_dim(leaf["weight_variances"], nd, dtype)
        n = np.sum(w * np.square(_cols(leaf, X, dtype)), 1) + np.asarray(leaf["bias_variance"], dtype=dtype)
        theta = np.zeros((), dtype=dtype)
        return np.asarray(leaf["variance"], dtype=dtype) * (1. / _pi(dtype)) * _J(leaf["order"], theta) * n ** leaf["order"]
    return kr.leaf_Kdiag(leaf, X)


def leaf_dK(leaf, X, X2=None, dtype=np.float64):
    """d K / d slot, one matrix per slot of this leaf"""
    t = leaf["type"]
    nd = len(leaf["dims"])
    if t == "cosine":
        ls, w, A, B, r = _cos_parts(leaf, X, X2, dtype)
        v = np.asarray(leaf["variance"], dtype=dtype)
        s = v * np.sin(r)
        D = A[:, None, :] - B[None, :, :]
        return [np.cos(r)] + [s * D[:, :, d] * w[d] / ls[d] ** 2 for d in range(nd)] + [-s * D[:, :, d] / ls[d] for d in range(nd)]
    if t == "arccosine":
        Kv, dP, dni, dnj, w, A, B = _arc_partials(leaf, X, X2, dtype)
        out = [Kv / np.asarray(leaf["variance"], dtype=dtype), dP + dni + dnj]
        for d in range(nd):
            out.append(dP * (A[:, d][:, None] * B[:, d][None, :]) + dni * np.square(A[:, d])[:, None] + dnj * np.square(B[:, d])[None, :])
        return out
    return kr.leaf_dK(leaf, X, X2)


def _leaf_input_terms(leaf, W, X, X2, dtype=np.float64):
    """(column of X, T [n, m]) with T_ij = W_ij d k(x_i, x'_j) / d x_i[column] (first argument only)"""
    t = leaf["type"]
    if t == "cosine":
        ls, w, A, B, r = _cos_parts(leaf, X, X2, dtype)
        Q = -W * np.asarray(leaf["variance"], dtype=dtype) * np.sin(r)
        for d, col in enumerate(leaf["dims"]):
            yield col, Q * (w[d] / ls[d])
        return
    if t == "arccosine":
        Kv, dP, dni, dnj, w, A, B = _arc_partials(leaf, X, X2, dtype)
        for d, col in enumerate(leaf["dims"]):
            yield col, W * (dP * (w[d] * B[:, d])[None, :] + dni * (2.0 * w[d] * A[:, d])[:, None])
        return
    for item in kr._leaf_input_terms(leaf, W, X, X2):
        yield item


# ---- trees: tests/_kern_ref.py's recursions over these leaves -------------------------------------------------------------------
def K(spec, X, X2=None, dtype=np.float64, diff=False):
    if isinstance(spec, dict):
        return leaf_K(spec, X, X2, dtype, diff)
    op, children = spec
    out = K(children[0], X, X2, dtype, diff)
    for c in children[1:]:
        out = out + K(c, X, X2, dtype, diff) if op == "sum" else out * K(c, X, X2, dtype, diff)
    return out


def Kdiag(spec, X, dtype=np.float64):
    if isinstance(spec, dict):
        return leaf_Kdiag(spec, X, dtype)
    op, children = spec
    out = Kdiag(children[0], X, dtype)
    for c in children[1:]:
        out = out + Kdiag(c, X, dtype) if op == "sum" else out * Kdiag(c, X, dtype)
    return out


def leaves_with_cofactors(spec, X, X2=None, cof=None):
    if isinstance(spec, dict):
        yield spec, cof
        return
    op, children = spec
    for i, c in enumerate(children):
        cc = cof
        if op == "product":
            for j, other in enumerate(children):
                if j != i:
                    v = np.asarray(K(other, X, X2, dtype=np.longdouble, diff=True), dtype=np.float64)
                    cc = v if cc is None else cc * v
        for item in leaves_with_cofactors(c, X, X2, cc):
            yield item


def dK(spec, X, X2=None):
    """d K / d slot for every slot of the program, in slot order.  The new leaves in long double, rounded once: the order-0
    ArcCosine VALUE (its variance slot, and the cofactor of its siblings) carries 1.7e-9 of fp64 rounding noise on the diagonal."""
    return [g if cof is None else g * cof for leaf, cof in leaves_with_cofactors(spec, X, X2)
            for g in (np.asarray(q, dtype=np.float64) for q in leaf_dK(leaf, X, X2, dtype=np.longdouble))]


def _nslots(leaf):
    t, nd = leaf["type"], len(leaf["dims"])
    if t in kr.STATIONARY:
        return 1 + nd + (1 if t == "ratquad" else 0)
    return {"linear": nd, "polynomial": nd + 1, "constant": 1, "white": 1, "periodic": 3}[t]


def fold(spec, slots):
    """slot values -> one value per parameter element, in kern.parameters order"""
    out, s = [], 0
    for leaf in kr.leaves(spec):
        t, nd = leaf["type"], len(leaf["dims"])
        if t == "cosine":
            out.append(slots[s]); s += 1
            vals = list(slots[s:s + nd]); s += nd
            out += vals if np.size(leaf["lengthscales"]) > 1 else [np.sum(vals, axis=0)]
            out += list(slots[s:s + nd]); s += nd
        elif t == "arccosine":
            out += [slots[s], slots[s + 1]]; s += 2
            vals = list(slots[s:s + nd]); s += nd
            out += vals if np.size(leaf["weight_variances"]) > 1 else [np.sum(vals, axis=0)]
        else:
            k = _nslots(leaf)
            out += list(kr.fold(leaf, slots[s:s + k])); s += k
    assert s == len(slots)
    return np.array(out)


def vjp_slots(spec, W, X, X2=None):
    return np.array([np.sum(W * g) for g in dK(spec, X, X2)])


def input_vjp(spec, W, X, X2=None):
    X = np.asarray(X, dtype=np.float64)
    G = np.zeros_like(X)
    for leaf, cof in leaves_with_cofactors(spec, X, X2):
        for col, T in _leaf_input_terms(leaf, W if cof is None else W * cof, X, X2, dtype=np.longdouble):
            G[:, col] += np.asarray(np.sum(T, 1), dtype=np.float64)
    return G


def spec_of(kern, d_all):
    import gpflowSlim as gpf
    k = gpf.kernels
    if isinstance(kern, (k.Sum, k.Product)):
        assert not kern.const_list
        return ("sum" if isinstance(kern, k.Sum) else "product", [spec_of(c, d_all) for c in kern.kern_list])

    def val(x):
        x = np.asarray(x, dtype=np.float64)
        return x.copy() if x.size > 1 else float(np.squeeze(x))
    if isinstance(kern, k.Cosine):
        return {"type": "cosine", "dims": kern._dims(False, d_all), "variance": val(kern.variance), "lengthscales": val(kern.lengthscales),
                "weights": np.asarray(kern.weights, dtype=np.float64).ravel().copy()}
    if isinstance(kern, k.ArcCosine):
        return {"type": "arccosine", "dims": kern._dims(False, d_all), "order": int(kern.order), "variance": val(kern.variance),
                "bias_variance": val(kern.bias_variance), "weight_variances": val(kern.weight_variances)}
    return kr.spec_of(kern, d_all)


def _K64(spec, X, X2=None):
    """the VALUES that go into a factorisation: the new leaves in long double, rounded once (an order-0 ArcCosine entry on the
    diagonal carries 1.7e-9 of fp64 rounding noise otherwise, which a solve with K + noise I amplifies)"""
    return np.asarray(K(spec, X, X2, dtype=np.longdouble), dtype=np.float64)


def lml_and_grad(spec, X, Y, noise):
    """as tests/_kern_ref.py's, over these leaves"""
    n, r = Y.shape
    Ky = _K64(spec, X) + noise * np.eye(n)
    L = sl.cholesky(Ky, lower=True)
    a = sl.cho_solve((L, True), Y)
    lml = -0.5 * n * r * np.log(2.0 * np.pi) - r * np.sum(np.log(np.diag(L))) - 0.5 * np.sum(Y * a)
    W = a @ a.T - r * sl.cho_solve((L, True), np.eye(n))
    slots = np.array([0.5 * np.sum(W * g) for g in dK(spec, X)])
    return lml, slots, 0.5 * np.trace(W)


def gpr_predict(spec, X, Y, noise, Xs, full_cov=False):
    n = X.shape[0]
    L = sl.cholesky(_K64(spec, X) + noise * np.eye(n), lower=True)
    A = sl.solve_triangular(L, _K64(spec, X, Xs), lower=True)
    V = sl.solve_triangular(L, Y, lower=True)
    var = _K64(spec, Xs) - A.T @ A if full_cov else Kdiag(spec, Xs) - np.sum(np.square(A), 0)
    return A.T @ V, var


def conditional(spec, Xn, Z, f, white, jitter=1e-6):
    m = Z.shape[0]
    Lm = sl.cholesky(_K64(spec, Z) + jitter * np.eye(m), lower=True)
    A = sl.solve_triangular(Lm, _K64(spec, Z, Xn), lower=True)
    fvar = Kdiag(spec, Xn) - np.sum(np.square(A), 0)
    if not white:
        A = sl.solve_triangular(Lm.T, A, lower=False)
    return A.T @ f, np.tile(fvar[:, None], [1, f.shape[1]])


# ---- the 50-digit fixture (tests/golden/mp/make_newkern_golden.py) -------------------------------------------------------------
def load_fixture():
    """(X, X2, Y, noise, {case: (spec, {"K", "K2", "lml", "grad", "grad_noise"})})"""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mp", "newkern.npz"))
    cases = {}
    for name in [str(s) for s in z["names"]]:
        t = str(z[name + "/type"])
        spec = {"type": t, "dims": [int(d) for d in z[name + "/dims"]]}
        for key in (("variance", "lengthscales", "weights") if t == "cosine" else ("variance", "bias_variance", "weight_variances", "order")):
            v = z[name + "/" + key]
            spec[key] = int(v) if key == "order" else (v.copy() if v.ndim else float(v))
        cases[name] = (spec, {k: z[name + "/" + k] for k in ("K", "K2", "lml", "grad", "grad_noise")})
    return z["X"], z["X2"], z["Y"], float(z["noise"]), cases


def kernel_of(spec, d_all):
    """the gpflowSlim kernel of a leaf spec of one of the two new types"""
    import gpflowSlim as gpf
    nd = len(spec["dims"])
    dims = None if spec["dims"] == list(range(d_all)) else spec["dims"]
    if spec["type"] == "cosine":
        ard = np.size(spec["lengthscales"]) > 1
        return gpf.kernels.Cosine(nd, variance=spec["variance"], lengthscales=spec["lengthscales"], ARD=ard, active_dims=dims,
                                  weights=spec["weights"])
    ard = np.size(spec["weight_variances"]) > 1
    return gpf.kernels.ArcCosine(nd, order=spec["order"], variance=spec["variance"], weight_variances=spec["weight_variances"],
                                 bias_variance=spec["bias_variance"], ARD=ard, active_dims=dims)


def arc0_tolerance(spec, ref_K, X, X2=None):
    """The per-entry tolerance of an order-0 ArcCosine value: |d K / d c| = variance / (pi sin(theta)), a rounding of a few eps in
    c moves entry (i, j) by that much:  variance / pi * 16 eps / sin(theta_ref_ij) + 1e-12 max|K|  (theta_ref in long double)."""
    theta = np.asarray(arc_theta(spec, X, X2, dtype=np.longdouble), dtype=np.float64)
    return float(spec["variance"]) / np.pi * 16.0 * np.finfo(np.float64).eps / np.sin(theta) + 1e-12 * np.abs(ref_K).max()
