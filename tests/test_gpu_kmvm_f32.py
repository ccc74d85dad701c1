"""GPU tests of the mixed-precision matrix-free path (csrc/kmvm_f32.hip, kcg_solve_mixed of csrc/gps_kmvm.hip), by the rules of
tests/test_gpu_kmvm.py: the fp32 fused product entry by entry against the long-double dense product, the refined solve and the
prediction under the fp64 solver's own bounds, the fallback to the fp64 loop, and the refusals.

Product tolerance, per entry: |out - ref| <= tol sum_p |K_ip| |V_pt| with tol = 8 spread32, spread32 the same scaled error of a
numpy float32 restatement of what the kernel computes (features centred in fp64 then rounded, the expanded and clamped r2, r2 = 0
on the diagonal of K(X, X), the formula and the product in float32), under a hard cap of 1e-5.
"""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _kmvm_ref as mr  # noqa: E402

pytestmark = pytest.mark.gpu
KERNELS = {"rbf": "RBF", "matern12": "Matern12", "matern52": "Matern52", "ratquad": "RatQuad"}


@pytest.fixture(scope="module")
def gpf():
    import gpflowSlim
    return gpflowSlim


def _kern(gpf, lf):
    kw = dict(variance=lf["variance"], lengthscales=lf["lengthscales"], active_dims=lf["dims"], ARD=True)
    if lf["type"] == "ratquad":
        kw["alpha"] = lf["alpha"]
    return getattr(gpf.kernels, KERNELS[lf["type"]])(len(lf["dims"]), **kw)


# name -> (kernel, n, n2 (None: K(X, X)), T, D, diag_add, forced chunks, shift of every coordinate)
PRODUCTS = {
    "tile_plus_one": ("rbf", 65, None, 1, 3, 0.37, 0, 0.0),
    "kb8_tb4": ("matern12", 200, None, 17, 9, 0.37, 0, 0.0),               # the KB = 8, TB = 4 instance
    "32_dims_three_chunks": ("ratquad", 130, None, 5, 32, 0.37, 3, 0.0),
    "rect": ("matern52", 65, 130, 3, 3, 0.0, 0, 0.0),
    "shifted_by_50": ("rbf", 130, None, 3, 3, 0.0, 0, 50.0),               # |a|^2 / r2 ~ 1e4: fails without the centring
}
_REF = {}


def _product_case(name):
    """(leaf, X, X2, V, long-double product, its scale, spread32)"""
    if name not in _REF:
        kind, n, n2, T, d, diag_add, _, shift = PRODUCTS[name]
        rng = np.random.default_rng(sum(map(ord, name)))
        X = rng.normal(size=(n, d)) + shift
        X2 = None if n2 is None else rng.normal(size=(n2, d)) + shift
        V = rng.normal(size=(n if n2 is None else n2, T))
        lf = mr.leaf(kind, range(d), n + T)
        lf["lengthscales"] = lf["lengthscales"] * np.sqrt(d / 3.0)         # (r2 stays near 6 at any D, as in test_gpu_kmvm.py)
        ref, scale, _ = mr.product(lf, X, V, X2, diag_add)
        A, B = mr._scaled(lf, X, np.float64), None if X2 is None else mr._scaled(lf, X2, np.float64)
        mean = np.mean(A if B is None else np.concatenate([A, B]), 0)
        A32 = (A - mean).astype(np.float32)
        B32 = A32 if B is None else (B - mean).astype(np.float32)
        # (the Matern formulas of _kern_ref multiply by float64 constants: rounded back, never a wider tolerance than all-float32)
        K32 = mr._block(lf, A32, B32, np.float32, np.arange(n) if B is None else None).astype(np.float32)
        V32 = V.astype(np.float32)
        out32 = K32 @ V32 + (np.float32(diag_add) * V32 if B is None else 0)
        assert out32.dtype == np.float32
        _REF[name] = (lf, X, X2, V, ref, scale, float(np.max(np.abs(out32 - ref) / scale)))
    return _REF[name]


def _run_product(gpf, name, precision):
    lf, X, X2, V = _product_case(name)[:4]
    h = gpf.get_handle()
    gpf._backend.kmvm_set_split(h, PRODUCTS[name][6])
    try:
        return gpf.conjugate_gradient.kernel_matmul(_kern(gpf, lf), X, V, X2=X2, diag_add=PRODUCTS[name][5], precision=precision)
    finally:
        gpf._backend.kmvm_set_split(h, 0)


@pytest.mark.parametrize("name", list(PRODUCTS))
def test_product_entry_by_entry(gpf, name):
    ref, scale, spread32 = _product_case(name)[4:]
    tol = 8 * spread32
    assert tol <= 1e-5, "the float32 restatement's own spread (%.3g) leaves no room under the hard cap" % spread32
    out = _run_product(gpf, name, "fp32")
    err = float(np.max(np.abs(out - ref) / scale))
    print("%s: spread32 %.3g tol %.3g error %.3g" % (name, spread32, tol, err))
    assert out.shape == ref.shape and np.all(np.isfinite(out))
    assert err <= tol
    assert not np.array_equal(out, _run_product(gpf, name, "fp64"))        # the fp32 path ran
    assert np.array_equal(out, _run_product(gpf, name, "fp32"))            # equal bytes from call to call


_CG = {}


def _cg_case(n, T, noise, clustered=False):
    """RBF in 3 dims; with more than one column the last is exactly zero.  clustered: 20 clusters of 10 points 1e-3 apart -- 180
    eigenvalues of K below 4e-5, so K + noise I is as ill-conditioned as the noise is small, yet CG sees few distinct eigenvalues"""
    if (n, T, noise) not in _CG:
        rng = np.random.default_rng(1000 + n + T)
        X = rng.normal(size=(n, 3))
        if clustered:
            X = np.repeat(X[:n // 10], 10, 0) + 1e-3 * rng.normal(size=(n, 3))
        B = rng.normal(size=(n, T))
        if T > 1:
            B[:, -1] = 0.0
        lf = mr.leaf("rbf", range(3), n)
        A, cond = mr.dense(lf, X, noise)
        _CG[(n, T, noise)] = (lf, X, B, A, cond, mr.solve(A, B))
    return _CG[(n, T, noise)]


def _check_solve(case, x, info, tol, max_iter):
    """the three bounds of test_gpu_kmvm.py::test_batched_cg against the long-double dense solve"""
    lf, X, B, A, cond, xs = case
    assert np.all(info["converged"]) and np.all(info["iterations"] < max_iter)
    res = np.linalg.norm(np.asarray(A @ x.astype(mr.LD) - B, dtype=np.float64), axis=0)
    fwd = np.linalg.norm(np.asarray(x - xs, dtype=np.float64), axis=0)
    print("cond %.3g info %s residual %s forward %s" % (cond, info, res, fwd))
    assert np.all(res <= 10 * tol * np.linalg.norm(B, axis=0))
    assert np.all(fwd <= cond * 10 * tol * np.linalg.norm(np.asarray(xs, dtype=np.float64), axis=0))


@pytest.mark.parametrize("n", [65, 200])
@pytest.mark.parametrize("T", [1, 17])
def test_mixed_solve(gpf, n, T):
    case = _cg_case(n, T, 0.5)
    tol = 1e-9
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        x, info = gpf.conjugate_gradient.kernel_cgsolver(_kern(gpf, case[0]), case[1], case[2], 0.5, max_iter=4 * n, tol=tol,
                                                         precision="mixed")
    _check_solve(case, x, info, tol, 4 * n)
    live = slice(0, T - 1 if T > 1 else 1)
    assert np.all(info["outer_iterations"][live] >= 2)
    assert info["fp32_products"] > info["fp64_products"] and not np.any(info["fell_back"])
    if T > 1:
        assert np.all(x[:, -1] == 0.0) and info["iterations"][-1] == 0 and info["relative_residual"][-1] == 0.0


def test_fallback(gpf):
    """noise 5e-6 on the clustered points (cond 1.2e7).  On the CPU, with K in float32 (smallest eigenvalue of K32 + noise I:
    2.4e-6, not 5e-6 -- condition number x fp32 error ~ 1) the refinement's fp64 residual goes 0.14, 0.068, 0.055 |b| and stalls
    at the third outer step (second column: 0.22, 0.17, at the second), while the fp64 loop alone reaches 1e-9 in 272 of the
    4 n = 800 iterations.  max_iter = 8 n here: the stalled corrections have spent theirs before the fp64 loop starts."""
    n, T, noise, tol = 200, 3, 5e-6, 1e-9
    case = _cg_case(n, T, noise, clustered=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        x, info = gpf.conjugate_gradient.kernel_cgsolver(_kern(gpf, case[0]), case[1], case[2], noise, max_iter=8 * n, tol=tol,
                                                         precision="mixed")
    assert np.all(info["fell_back"][:-1]) and not info["fell_back"][-1]
    _check_solve(case, x, info, tol, 8 * n)


def test_predict_f_iterative_mixed(gpf):
    """the bounds of test_gpu_kmvm.py::test_predict_f_iterative"""
    n, n_new, R, noise, tol = 200, 5, 2, 0.5, 1e-9
    rng = np.random.default_rng(77 + n_new)
    X, Xs, Y = rng.normal(size=(n, 3)), rng.normal(size=(n_new, 3)), rng.normal(size=(n, R))
    lf = mr.leaf("matern52", range(3), n_new)
    m = gpf.models.GPR(X, Y, _kern(gpf, lf), obs_var=noise)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        mean, var = m.predict_f_iterative(Xs, max_iter=4 * n, tol=tol, precision="mixed")
    A, cond = mr.dense(lf, X, noise)
    Ks = mr.K_ld(lf, X, Xs)
    alpha, Z = mr.solve(A, Y), mr.solve(A, Ks)
    ref_mean = np.asarray(Ks.T @ alpha, dtype=np.float64)
    ref_var = np.asarray(lf["variance"] - np.sum(Ks * Z, 0), dtype=np.float64)
    nrm = lambda a: np.linalg.norm(np.asarray(a, dtype=np.float64), axis=0)        # noqa: E731
    assert mean.shape == (n_new, R) and var.shape == (n_new, R) and np.array_equal(var[:, 0], var[:, 1])
    assert np.all(nrm(mean - ref_mean) <= cond * 10 * tol * np.linalg.norm(np.asarray(Ks, dtype=np.float64), 2) * nrm(alpha))
    assert np.all(np.abs(var[:, 0] - ref_var) <= cond * 10 * tol * nrm(Ks) * nrm(Z))


def test_refusals(gpf, monkeypatch):
    """every combination the mixed-precision path does not serve: refused by name, before the backend is entered"""
    be, cg, k = gpf._backend, gpf.conjugate_gradient, gpf.kernels

    def launched(*a, **kw):
        raise AssertionError("the backend was entered")
    for name in ("kmvm", "kmvm_f32", "kmvm_sop", "kernel_cg", "kernel_cg_mixed", "kernel_cg_lanczos", "kernel_pcg", "kernel_predict",
                 "kernel_predict_mixed", "kernel_predict_lanczos", "kernel_predict_pcg"):
        monkeypatch.setattr(be, name, launched)
    X, V = np.ones((4, 2)), np.ones((4, 1))
    m = gpf.models.GPR(X, V, k.RBF(2), obs_var=0.1)
    for call, match in [
            (lambda: cg.kernel_matmul(k.RBF(2), X, V, precision="mixed"), "precision must be 'fp64' or 'fp32'"),
            (lambda: cg.kernel_cgsolver(k.RBF(2), X, V, 0.1, precision="fp32"), "precision must be 'fp64' or 'mixed'"),
            (lambda: cg.kernel_cgsolver(k.RBF(2), X, V, 0.1, precision="mixed", lanczos=True), "together with lanczos"),
            (lambda: cg.kernel_cgsolver(k.RBF(2), X, V, 0.1, precision="mixed", precond_rank=2), "together with precond_rank"),
            (lambda: m.predict_f_iterative(X, precision="mixed", variance="lanczos"), "together with variance"),
            (lambda: m.predict_f_iterative(X, precision="mixed", precond_rank=2), "together with precond_rank"),
            (lambda: m.predict_f_iterative(X, precision="single"), "precision must be"),
            (lambda: m.compute_log_likelihood_and_gradients_iterative(precision="mixed"), "together with training")]:
        with pytest.raises(ValueError, match=match):
            call()
    comp = k.RBF(2) + k.Matern32(2)
    for call in (lambda: cg.kernel_matmul(comp, X, V, precision="fp32"),
                 lambda: cg.kernel_cgsolver(comp, X, V, 0.1, precision="mixed"),
                 lambda: gpf.models.GPR(X, V, comp, obs_var=0.1).predict_f_iterative(X, precision="mixed")):
        with pytest.raises(NotImplementedError, match="knows one primitive"):
            call()
