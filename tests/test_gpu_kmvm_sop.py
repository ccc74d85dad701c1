"""GPU tests of the matrix-free path on sums of products of primitives (csrc/kmvm_sop.hip), by the rules of tests/test_gpu_kmvm.py.
Product: |out - ref| <= tol sum_p |K_ip| |V_pt|, tol = max(8 spread, 64 eps), spread the same scaled error of a plain fp64 numpy
evaluation against the long-double one, under the cap tol <= 1e-11 on the reference itself.  Stationary leaves are _kmvm_ref.K_ld /
_kern_ref.K; for Periodic and Cosine the long-double side is the direct form (sin^2, the cosine of the difference) and the fp64
comparator the cos / sin feature form the device uses.  Matern12 and Exponential stay in rectangular cases (test_gpu_kmvm.py says
why).  White is the index diagonal of K(X, X) and 0 against an X2.  A spec is a list of terms, a term a list of leaves.
"""
import os
import sys
import warnings
from unittest import mock

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _kern_ref as kr  # noqa: E402
import _kmvm_ref as mr  # noqa: E402
from test_gpu_kmvm import KERNELS, gpf  # noqa: E402, F401

pytestmark = pytest.mark.gpu
EPS, LD = np.finfo(np.float64).eps, mr.LD
PI = 4 * np.arctan(LD(1))
per = lambda dims, ls=1.1: {"type": "periodic", "dims": list(dims), "variance": 0.8, "lengthscales": ls, "period": 1.7}  # noqa: E731
const = lambda v, scalar=False: {"type": "constant", "variance": v, "scalar": scalar}  # noqa: E731
WHITE, R3, W16, _REF = {"type": "white", "variance": 0.6}, range(3), np.sqrt(16 / 3.0), {}


def st(kind, dims, seed=0, wide=1.0):
    lf = mr.leaf(kind, dims, seed)
    return dict(lf, lengthscales=lf["lengthscales"] * wide)


def cosk(dims, seed):
    rng = np.random.default_rng(seed)
    return {"type": "cosine", "dims": list(dims), "variance": 0.9, "lengthscales": rng.uniform(0.7, 1.3, len(dims)),
            "weights": rng.normal(size=len(dims))}


CHECKED = [[st("rbf", R3, 1), per(R3)], [st("matern52", R3, 2)], [const(0.25, True)]]          # RBF.Periodic + Matern52 + 0.25
SOLVED = CHECKED[:2]
MAUNA = [[st("rbf", [0], 1)], [st("rbf", [0], 2), per([0])], [st("ratquad", [0], 3)], [st("rbf", [0], 4)], [WHITE]]
# name -> (spec, n, n2 (None: K(X, X)), T, d_all, diag_add, forced chunks)
PRODUCTS = {
    "one_point": ([[st("rbf", [0], 1), per([0])]], 1, None, 1, 1, 0.37, 0),
    "tile_minus_one": ([[st("rbf", R3, 1), per(R3)]], 63, None, 3, 3, 0.37, 0),
    "sum_disjoint_dims": ([[st("rbf", [0, 1], 1)], [st("matern32", [2], 2)]], 65, None, 17, 3, 0.37, 0),
    "mauna_white_diagonal": (MAUNA, 65, None, 17, 1, 0.0, 0),
    "mauna_rect_wide": (MAUNA, 65, 130, 3, 1, 0.0, 0),
    "mixture_rect_tall": ([[st("rbf", [0, 1], 1), cosk([0, 1], 5)], [st("rbf", [0, 1], 2), cosk([0, 1], 6)]], 130, 5, 16, 2, 0.0, 0),
    "constant_factor_and_term": ([[st("rbf", R3, 1), const(0.7)], [const(0.25, True)]], 65, None, 1, 3, 0.37, 0),
    "ratquad_factor": ([[st("ratquad", R3, 1), per(R3)], [st("matern52", R3, 2)]], 65, 130, 17, 3, 0.0, 0),
    "sixteen_primitives": ([[st("rbf", [0, 1], s), per([s % 2]), const(0.5 + 0.1 * s)] for s in range(5)] + [[WHITE]],
                           65, None, 17, 2, 0.37, 0),
    "sixty_four_rows": ([[st("rbf", range(16), 1, W16)], [st("rbf", range(16, 32), 2, W16)], [per(range(16), 3.0)]],
                        65, None, 17, 32, 0.37, 0),
    "clamp_duplicates": ([[st("matern32", R3, 1), st("rbf", R3, 2)]], 65, None, 3, 3, 0.37, 0),
    "three_chunks": (CHECKED, 200, None, 17, 3, 0.37, 3),
    "two_passes_two_chunks": (CHECKED, 130, None, 65, 3, 0.37, 2),
    "matern12_exponential_rect": ([[st("matern12", R3, 1), per(R3)], [st("exponential", R3, 2)]], 65, 130, 3, 3, 0.0, 0),
}


def leaf_K(lf, X, X2, dt):
    """one leaf in dtype dt: long double by the direct formulas, fp64 by the forms the device uses"""
    t, n, m = lf["type"], len(X), len(X if X2 is None else X2)
    if t in ("constant", "white"):
        return lf["variance"] * (np.ones((n, m), dtype=dt) if t == "constant" else np.eye(n, m, dtype=dt) * (X2 is None))
    if t not in ("periodic", "cosine"):
        return mr.K_ld(lf, X, X2) if dt is LD else kr.K(lf, X, X2)
    A = np.asarray(X, dtype=dt)[:, lf["dims"]]
    B = A if X2 is None else np.asarray(X2, dtype=dt)[:, lf["dims"]]
    v, ls = dt(lf["variance"]), np.asarray(lf["lengthscales"], dtype=dt)
    if t == "cosine":
        a, b = (M @ (np.asarray(lf["weights"], dtype=dt) / ls) for M in (A, B))
        return v * (np.cos(a[:, None] - b[None, :]) if dt is LD else np.outer(np.cos(a), np.cos(b)) + np.outer(np.sin(a), np.sin(b)))
    if dt is LD:
        s = np.sin(PI * (A[:, None, :] - B[None, :, :]) / dt(lf["period"]))
        return v * np.exp(-0.5 * np.sum(np.square(s), -1) / (ls * ls))
    a, b = 2 * np.pi * A / lf["period"], 2 * np.pi * B / lf["period"]
    dot = np.cos(a) @ np.cos(b).T + np.sin(a) @ np.sin(b).T
    return v * np.exp(-0.5 * ((0.5 * A.shape[1] - 0.5 * dot) / (ls * ls)))


def spec_K(spec, X, X2=None, dt=LD):
    return sum(np.prod([leaf_K(lf, X, X2, dt) for lf in term], axis=0) for term in spec)


def dense(spec, X, noise):
    """_kmvm_ref.dense for a spec: (K + noise I in long double, its 2-norm condition number)"""
    A = spec_K(spec, X) + LD(noise) * np.eye(len(X), dtype=LD)
    w = np.linalg.eigvalsh(np.asarray(A, dtype=np.float64))
    return A, float(w[-1] / w[0])


def kern_of(gpf, spec):
    k = gpf.kernels

    def one(lf):
        t = lf["type"]
        if t in ("constant", "white"):
            return lf["variance"] if lf.get("scalar") else getattr(k, t.capitalize())(1, variance=lf["variance"])
        nd = len(lf["dims"])
        if t == "periodic":
            return k.Periodic(nd, period=lf["period"], variance=lf["variance"], lengthscales=lf["lengthscales"], active_dims=lf["dims"])
        kw = dict(variance=lf["variance"], lengthscales=lf["lengthscales"], active_dims=lf["dims"], ARD=True)
        if t == "cosine":
            return k.Cosine(nd, weights=lf["weights"], **kw)
        return getattr(k, KERNELS[t])(nd, **(dict(kw, alpha=lf["alpha"]) if t == "ratquad" else kw))
    terms = [k.Product([one(lf) for lf in term]) if len(term) > 1 else one(term[0]) for term in spec]
    return k.Sum(terms) if len(terms) > 1 else terms[0]


def _product_case(name):
    if name not in _REF:
        spec, n, n2, T, d_all, diag_add, split = PRODUCTS[name]
        rng = np.random.default_rng(sum(map(ord, name)))
        X = rng.normal(size=(n, d_all))
        if name == "clamp_duplicates":
            X[7] = X[40]                       # two identical points: r2 = rounding, clamped at 0
        X2 = None if n2 is None else rng.normal(size=(n2, d_all))
        V = rng.normal(size=(n if n2 is None else n2, T))
        Kl, Vl = spec_K(spec, X, X2), np.asarray(V, dtype=LD)
        ref, r64 = Kl @ Vl, spec_K(spec, X, X2, np.float64) @ V
        if X2 is None:
            ref, r64 = ref + LD(diag_add) * Vl, r64 + diag_add * V
        scale = np.abs(Kl) @ np.abs(Vl)
        _REF[name] = (spec, X, X2, V, ref, scale, float(np.max(np.abs(r64 - ref) / scale)))
    return _REF[name]


def _run_product(gpf, name):
    spec, X, X2, V = _product_case(name)[:4]
    gpf._backend.kmvm_set_split(gpf.get_handle(), PRODUCTS[name][6])
    try:
        return gpf.conjugate_gradient.kernel_matmul(kern_of(gpf, spec), X, V, X2=X2, diag_add=PRODUCTS[name][5])
    finally:
        gpf._backend.kmvm_set_split(gpf.get_handle(), 0)


@pytest.mark.parametrize("name", list(PRODUCTS))
def test_product_entry_by_entry(gpf, name):
    ref, scale, spread = _product_case(name)[4:]
    tol = max(8 * spread, 64 * EPS)
    assert tol <= 1e-11, "the reference's own spread (%.3g) leaves no room under the hard cap" % spread
    out = _run_product(gpf, name)
    err = float(np.max(np.abs(out - ref) / scale))
    print("%s: spread %.3g tol %.3g error %.3g" % (name, spread, tol, err))
    assert out.shape == ref.shape and np.all(np.isfinite(out)) and err <= tol


def test_equal_bytes_and_the_lone_primitive_route(gpf):
    assert np.array_equal(_run_product(gpf, "three_chunks"), _run_product(gpf, "three_chunks"))
    be, k, (X, V) = gpf._backend, gpf.kernels, _product_case("tile_minus_one")[1:4:2]
    assert np.array_equal(gpf.conjugate_gradient.kernel_matmul(k.RBF(3), X, V), be.kmvm(gpf.get_handle(), k.RBF(3)._program(3), X, V))
    with pytest.raises(RuntimeError, match=r"gps_kmvm_sop failed \(-4\)"):        # a Sum under a Product, refused by the library too
        be.kmvm_sop(gpf.get_handle(), ((k.RBF(3) + k.RBF(3)) * k.RBF(3))._program(3), X, V)


@pytest.mark.parametrize("n", [65, 200])
@pytest.mark.parametrize("T", [1, 17])
def test_batched_cg(gpf, n, T):
    """test_gpu_kmvm.py::test_batched_cg's three bounds against the long-double dense solve; lanczos=True returns the same x"""
    rng = np.random.default_rng(1000 + n + T)
    X, B = rng.normal(size=(n, 3)), rng.normal(size=(n, T))
    if T > 1:
        B[:, 0], B[:, -1] = 0.3, 0.0
    A, cond = dense(SOLVED, X, 0.5)
    xs, tol = mr.solve(A, B), 1e-9
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        x, info = gpf.conjugate_gradient.kernel_cgsolver(kern_of(gpf, SOLVED), X, B, 0.5, max_iter=4 * n, tol=tol)
        x2, info2 = gpf.conjugate_gradient.kernel_cgsolver(kern_of(gpf, SOLVED), X, B, 0.5, max_iter=4 * n, tol=tol, lanczos=True)
    assert np.all(info["converged"]) and np.all(info["iterations"] < 4 * n)
    nrm = lambda a: np.linalg.norm(np.asarray(a, dtype=np.float64), axis=0)        # noqa: E731
    assert np.all(nrm(A @ x.astype(LD) - B) <= 10 * tol * nrm(B)) and np.all(nrm(x - xs) <= cond * 10 * tol * nrm(xs))
    if T > 1:
        assert np.all(x[:, -1] == 0.0) and info["iterations"][-1] == 0 and info["relative_residual"][-1] == 0.0
    assert np.array_equal(x, x2) and info2["alpha"].shape == (int(np.max(info["iterations"])), T)


@pytest.mark.parametrize("n_new", [5, 19])
def test_predict_f_iterative(gpf, n_new):
    """test_gpu_kmvm.py::test_predict_f_iterative's bounds; the prior variance is sum_terms prod variances, White's included"""
    n, R, noise, tol, spec = 200, 2, 0.5, 1e-9, SOLVED + [[WHITE]]
    rng = np.random.default_rng(77 + n_new)
    X, Xs, Y, c = rng.normal(size=(n, 3)), rng.normal(size=(n_new, 3)), rng.normal(size=(n, R)), np.array([0.4, -1.1])
    m = gpf.models.GPR(X, Y, kern_of(gpf, spec), mean_function=gpf.mean_functions.Constant(c), obs_var=noise)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        mean, var = m.predict_f_iterative(Xs, max_iter=4 * n, tol=tol)
    (A, cond), Ks = dense(spec, X, noise), spec_K(spec, X, Xs)
    alpha, Z = mr.solve(A, Y - c), mr.solve(A, Ks)
    ref_mean = np.asarray(Ks.T @ alpha + c, dtype=np.float64)
    ref_var = np.asarray(sum(np.prod([lf["variance"] for lf in term]) for term in spec) - np.sum(Ks * Z, 0), dtype=np.float64)
    nrm = lambda a: np.linalg.norm(np.asarray(a, dtype=np.float64), axis=0)        # noqa: E731
    assert mean.shape == (n_new, R) and var.shape == (n_new, R) and np.array_equal(var[:, 0], var[:, 1])
    assert np.all(nrm(mean - ref_mean) <= cond * 10 * tol * np.linalg.norm(np.asarray(Ks, dtype=np.float64), 2) * nrm(alpha))
    assert np.all(np.abs(var[:, 0] - ref_var) <= cond * 10 * tol * nrm(Ks) * nrm(Z))


def test_refusals_before_the_backend(gpf, monkeypatch):
    be, cg, k = gpf._backend, gpf.conjugate_gradient, gpf.kernels
    launched = mock.Mock(side_effect=AssertionError("the backend was entered"))
    for name in ("kmvm", "kmvm_sop", "kmvm_grad", "kernel_cg", "kernel_cg_lanczos", "kernel_cg_sop", "kernel_predict",
                 "kernel_predict_sop", "kernel_predict_pcg", "kernel_pchol", "kernel_precond_solve", "kernel_pcg"):
        monkeypatch.setattr(be, name, launched)
    X, V, comp = np.ones((4, 2)), np.ones((4, 1)), k.RBF(2) * k.Periodic(2) + k.Matern52(2)
    m = gpf.models.GPR(X, V, comp, obs_var=0.5)
    for call, match in [
            (lambda: cg.kernel_cgsolver(comp, X, V, 0.5, precond_rank=2), "preconditioner"),
            (lambda: cg.kernel_logdet(comp, X, 0.5, precond_rank=2), "preconditioner"),
            (lambda: m.predict_f_iterative(X, precond_rank=2), "preconditioner"),
            (lambda: cg.kernel_pivoted_cholesky(comp, X, 2), "preconditioner"),
            (lambda: cg.kernel_precond_solve(comp, X, V, 0.5, 2), "preconditioner"),
            (lambda: cg.kernel_grad_form(comp, X, V, V), "gradient form"),
            (lambda: m.compute_log_likelihood_and_gradients_iterative(), "training"),
            (lambda: (setattr(m, "iterative", {}), m.compute_log_likelihood_and_gradients()), "training"),
            (lambda: cg.kernel_matmul((k.RBF(2) + k.Matern32(2)) * k.Periodic(2), X, V), "expand"),
            (lambda: cg.kernel_matmul(k.Periodic(2), X, V), "one stationary kernel")] + [
            (lambda f=f: cg.kernel_matmul(k.RBF(2) + f, X, V), "one stationary kernel")
            for f in (k.Linear(2), k.Polynomial(2), k.ArcCosine(2), k.Coregion(1, 2, 1, active_dims=[1]))]:
        with pytest.raises(NotImplementedError, match=match):
            call()
    with pytest.raises(ValueError, match="64 feature rows"):      # 16 + 16 + 2 x 17 -> 36 rows
        cg.kernel_matmul(k.RBF(16, ARD=True) + k.RBF(16, ARD=True) + k.Periodic(17), np.ones((4, 17)), V)
