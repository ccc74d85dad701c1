"""Numpy restatement of Coregion (reference gpflowSlim/kernels.py:822-881) as the reference writes it -- B = W W^T + diag(kappa),
then a gather of B by the integer labels -- with its analytic parameter derivatives, in float64 or long double: the yardstick of
tests/test_gpu_coregion.py, itself checked on the CPU against long-double central differences (tests/test_coregion_ref_cpu.py).
Every other leaf type is tests/_kern_ref2.py's (and through it tests/_kern_ref.py's); the tree recursions are restated over
these leaves the way _kern_ref2.py restates _kern_ref.py's.

    coregion   W [P, R], kappa [P]      K(x, y) = B[a, b],  a = (int) x[dims[0]] truncated toward zero like tf.cast (:869)

Slots (include/gpflowslim_hip.h): [W row-major, kappa_0 ..]:  d K_ij / d kappa_p = [a_i = p] [b_j = p],
d K_ij / d W[p, r] = [a_i = p] W[b_j, r] + W[a_i, r] [b_j = p].  The label column has no input derivative.
"""
import numpy as np
import scipy.linalg as sl

import _kern_ref as kr
import _kern_ref2 as k2


def labels(leaf, X):
    """tf.cast(X[:, 0], tf.int32) of the sliced column (kernels.py:868-869)"""
    return np.trunc(np.asarray(X, dtype=np.float64)[:, leaf["dims"][0]]).astype(np.int64)


def coregion_B(leaf, dtype=np.float64):
    """kernels.py:874"""
    W = np.asarray(leaf["W"], dtype=dtype)
    return W @ W.T + np.diag(np.asarray(leaf["kappa"], dtype=dtype))


# ---- leaves ------------------------------------------------------------------------------------------------------------------
def leaf_K(leaf, X, X2=None, dtype=np.float64, diff=False):
    if leaf["type"] != "coregion":
        return k2.leaf_K(leaf, X, X2, dtype, diff)
    a = labels(leaf, X)
    b = a if X2 is None else labels(leaf, X2)
    return coregion_B(leaf, dtype)[b].T[a]                                   # kernels.py:875: gather, transpose, gather


def leaf_Kdiag(leaf, X, dtype=np.float64):
    if leaf["type"] != "coregion":
        return k2.leaf_Kdiag(leaf, X, dtype)
    W = np.asarray(leaf["W"], dtype=dtype)
    return (np.sum(np.square(W), 1) + np.asarray(leaf["kappa"], dtype=dtype))[labels(leaf, X)]      # kernels.py:880-881


def leaf_dK(leaf, X, X2=None, dtype=np.float64):
    """d K / d slot, one matrix per slot of this leaf"""
    if leaf["type"] != "coregion":
        return k2.leaf_dK(leaf, X, X2, dtype)
    W = np.asarray(leaf["W"], dtype=dtype)
    P, R = W.shape
    a = labels(leaf, X)
    b = a if X2 is None else labels(leaf, X2)
    out = []
    for p in range(P):
        for r in range(R):
            out.append((a == p)[:, None] * W[b, r][None, :] + W[a, r][:, None] * (b == p)[None, :])
    for p in range(P):
        out.append(np.asarray((a == p)[:, None] * (b == p)[None, :], dtype=dtype))
    return out


def _leaf_input_terms(leaf, W, X, X2, dtype=np.float64):
    if leaf["type"] == "coregion":
        return                                   # the label is an index
    for item in k2._leaf_input_terms(leaf, W, X, X2, dtype):
        yield item


# ---- trees ---------------------------------------------------------------------------------------------------------------------
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
    """(leaf, d K / d K_leaf entry by entry) in program order: the product of the siblings' values under every Product on the way
    down; None: 1"""
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
    """d K / d slot for every slot of the program, in slot order (long double, rounded once)"""
    return [g if cof is None else g * cof for leaf, cof in leaves_with_cofactors(spec, X, X2)
            for g in (np.asarray(q, dtype=np.float64) for q in leaf_dK(leaf, X, X2, dtype=np.longdouble))]


def nslots(leaf):
    if leaf["type"] == "coregion":
        P, R = np.shape(leaf["W"])
        return P * (R + 1)
    if leaf["type"] == "cosine":
        return 1 + 2 * len(leaf["dims"])
    if leaf["type"] == "arccosine":
        return 2 + len(leaf["dims"])
    return k2._nslots(leaf)


def fold(spec, slots):
    """slot values -> one value per parameter element, in kern.parameters order (Coregion: W row-major, then kappa)"""
    out, s = [], 0
    for leaf in kr.leaves(spec):
        n = nslots(leaf)
        out += list(slots[s:s + n]) if leaf["type"] == "coregion" else list(k2.fold(leaf, slots[s:s + n]))
        s += n
    assert s == len(slots)
    return np.array(out)


def slot_owner(spec):
    """per slot: (index of the leaf in program order, output index p of a Coregion slot or None)"""
    out = []
    for li, leaf in enumerate(kr.leaves(spec)):
        if leaf["type"] == "coregion":
            P, R = np.shape(leaf["W"])
            out += [(li, p) for p in range(P) for _ in range(R)] + [(li, p) for p in range(P)]
        else:
            out += [(li, None)] * nslots(leaf)
    return out


def vjp_slots(spec, W, X, X2=None):
    return np.array([np.sum(W * g) for g in dK(spec, X, X2)])


def input_vjp(spec, W, X, X2=None):
    """G[i, d] = sum_j W_ij d k(x_i, x'_j) / d x_i[d], first argument only; the label columns stay 0"""
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
    if isinstance(kern, k.Coregion):
        return {"type": "coregion", "dims": kern._dims(False, d_all),
                "W": np.array(kern.W, dtype=np.float64).reshape(kern.output_dim, kern.rank), "kappa": np.array(kern.kappa, dtype=np.float64)}
    return k2.spec_of(kern, d_all)


def _K64(spec, X, X2=None):
    return np.asarray(K(spec, X, X2, dtype=np.longdouble), dtype=np.float64)


def lml_and_grad(spec, X, Y, noise):
    """GPR log marginal likelihood (LAPACK Cholesky of K + noise I) and its analytic gradient: per slot
    1/2 sum_ij (a a^T - r K_y^-1)_ij d K_ij / d slot, and the same with d K_y / d noise = I"""
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


# ---- cases --------------------------------------------------------------------------------------------------------------------
def draw_coregion(rng, P, R, col):
    """a Coregion leaf with random W and kappa in [0.5, 1.5)"""
    return {"type": "coregion", "dims": [col], "W": rng.standard_normal((P, R)), "kappa": 0.5 + rng.random(P)}


def draw_labels(rng, n, P, skip=None):
    """n labels in [0, P) as floats with a fractional part (the cast truncates it), none of them `skip`"""
    allowed = np.array([p for p in range(P) if p != skip])
    return allowed[rng.integers(0, allowed.size, n)] + 0.75 * rng.random(n)


def kernel_of(spec, d_all):
    """the gpflowSlim kernel of a spec tree"""
    import gpflowSlim as gpf
    k = gpf.kernels
    if not isinstance(spec, dict):
        kerns = [kernel_of(c, d_all) for c in spec[1]]
        return (k.Sum if spec[0] == "sum" else k.Product)(kerns)
    t, dims = spec["type"], spec["dims"]
    if t == "coregion":
        P, R = np.shape(spec["W"])
        kern = k.Coregion(1, P, R, active_dims=dims)
        kern._W.assign(np.asarray(spec["W"], dtype=np.float64))
        kern._kappa.assign(spec["kappa"])
        return kern
    if t == "white":
        return k.White(1, variance=spec["variance"])
    cls = {"rbf": k.RBF, "matern32": k.Matern32, "matern52": k.Matern52, "matern12": k.Matern12}[t]
    return cls(len(dims), variance=spec["variance"], lengthscales=spec["lengthscales"], ARD=np.size(spec["lengthscales"]) > 1, active_dims=dims)
