"""GPU tests of the matrix-free exact-GP path (csrc/kmvm.hip, csrc/gps_kmvm.hip): the fused product entry by entry against the
long-double reference of tests/_kmvm_ref.py, equal bytes from call to call, the batched conjugate gradients, predict_f_iterative
and the refusals.

Product tolerance, per entry: |out - ref| <= tol sum_p |K_ip| |V_pt|, tol = max(8 spread, 64 eps) with spread the same scaled
error of the fp64 numpy evaluation against the long-double one, under a hard cap of 1e-11 on the reference itself.  The symmetric
cases use kernels whose value is flat at r = 0 (RBF, RatQuad, Matern32 / 52): the expanded distance leaves r2 ~ 1e-16 |a|^2 on the
diagonal where the device has an exact 0, which sqrt(r2 + 1e-12) turns into 5e-10 in a Matern12 / Exponential value (tests/_kern_ref.py
says the same); those two are checked on rectangular products, and the near-duplicate case runs RBF.  The Matern epsilon itself is
exercised by a rectangular Matern12 pair at the origin and 1e-9 from it: no cancellation there (norms 0 and 3e-18, dot product 0),
so r2 ~ 1e-18 is exact to rounding on both sides and sqrt(r2 + 1e-12) decides the value.
"""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _kern_ref as kr  # noqa: E402
import _kmvm_ref as mr  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
KERNELS = {"rbf": "RBF", "matern12": "Matern12", "matern32": "Matern32", "matern52": "Matern52", "exponential": "Exponential",
           "ratquad": "RatQuad"}


@pytest.fixture(scope="module")
def gpf():
    import gpflowSlim
    return gpflowSlim


def _kern(gpf, lf, d_all):
    kw = dict(variance=lf["variance"], lengthscales=lf["lengthscales"], active_dims=lf["dims"], ARD=True)
    if lf["type"] == "ratquad":
        kw["alpha"] = lf["alpha"]
    return getattr(gpf.kernels, KERNELS[lf["type"]])(len(lf["dims"]), **kw)


# name -> (kernel, n, n2 (None: K(X, X)), T, d_all, active dims (None: all), diag_add, forced chunks, special points: False, "dup" or
# "origin")
PRODUCTS = {
    "one_point": ("rbf", 1, None, 1, 1, None, 0.37, 0, False),
    "tile_minus_one": ("matern52", 63, None, 3, 3, None, 0.0, 0, False),
    "one_tile_nine_dims": ("ratquad", 64, None, 16, 9, None, 0.37, 0, False),
    "tile_plus_one": ("rbf", 65, None, 17, 3, None, 0.0, 0, False),
    "matern32_one_column": ("matern32", 65, None, 1, 3, None, 0.37, 0, False),
    "four_tiles_33_columns": ("matern52", 200, None, 33, 3, None, 0.37, 0, False),
    "three_chunks": ("rbf", 200, None, 17, 9, None, 0.37, 3, False),
    "rect_wide": ("matern12", 65, 130, 3, 3, None, 0.0, 0, False),
    "rect_tall": ("matern12", 130, 5, 16, 1, None, 0.0, 0, False),
    "rect_exponential": ("exponential", 130, 5, 17, 3, None, 0.0, 0, False),
    "active_dims_subset": ("ratquad", 65, 130, 1, 6, [4, 0, 2], 0.0, 0, False),
    "near_duplicates": ("rbf", 65, None, 3, 3, None, 0.37, 0, "dup"),
    "matern_epsilon": ("matern12", 65, 130, 3, 3, None, 0.0, 0, "origin"),
    "two_passes_two_chunks": ("rbf", 130, None, 65, 3, None, 0.37, 2, False),     # T = 65: passes of 64 + 1 columns; 3 tiles in chunks of 1, 2
    # the dimension edges of the two instances (KB = 2: up to 8 feature rows, kbn 1 -> 2 from D = 5; KB = 8: D = 16 and 32 fill four
    # and all eight feature groups)
    "four_dims": ("rbf", 65, None, 17, 4, None, 0.37, 0, False),
    "five_dims": ("matern52", 65, None, 17, 5, None, 0.37, 0, False),
    "eight_dims": ("ratquad", 65, None, 17, 8, None, 0.37, 0, False),
    "sixteen_dims": ("matern32", 65, None, 17, 16, None, 0.37, 0, False),
    "thirty_two_dims": ("rbf", 65, None, 17, 32, None, 0.37, 0, False),
    "rect_exponential_twelve_dims": ("exponential", 65, 130, 17, 12, None, 0.0, 0, False),
}
# These cases multiply the leaf's lengthscales by sqrt(D / 3): r2 stays near 6 and the off-diagonal entries O(1e-2 .. 1).  With
# lengthscales near 1 at D = 32 the matrix is numerically diagonal and the comparison checks nothing.
WIDE = ("four_dims", "five_dims", "eight_dims", "sixteen_dims", "thirty_two_dims", "rect_exponential_twelve_dims")
_REF = {}


def _product_case(name):
    if name not in _REF:
        kind, n, n2, T, d_all, dims, diag_add, split, dup = PRODUCTS[name]
        rng = np.random.default_rng(sum(map(ord, name)))
        X = rng.normal(size=(n, d_all))
        if dup == "dup":
            X[7] = X[40]                       # two identical points: r2 = rounding, clamped at 0
            X[12] = X[50] + 1e-9               # ... and one pair 1e-9 apart
        X2 = None if n2 is None else rng.normal(size=(n2, d_all))
        if dup == "origin":
            X[0], X2[0] = 0.0, 1e-9
        V = rng.normal(size=(n if n2 is None else n2, T))
        lf = mr.leaf(kind, range(d_all) if dims is None else dims, n + T)
        if name in WIDE:
            lf["lengthscales"] = lf["lengthscales"] * np.sqrt(d_all / 3.0)
        _REF[name] = (lf, X, X2, V) + mr.product(lf, X, V, X2, diag_add)
    return _REF[name]


def _run_product(gpf, name):
    lf, X, X2, V = _product_case(name)[:4]
    d_all, diag_add, split = PRODUCTS[name][4], PRODUCTS[name][6], PRODUCTS[name][7]
    h = gpf.get_handle()
    gpf._backend.kmvm_set_split(h, split)
    try:
        return gpf.conjugate_gradient.kernel_matmul(_kern(gpf, lf, d_all), X, V, X2=X2, diag_add=diag_add)
    finally:
        gpf._backend.kmvm_set_split(h, 0)


@pytest.mark.parametrize("name", list(PRODUCTS))
def test_product_entry_by_entry(gpf, name):
    ref, scale, spread = _product_case(name)[4:]
    if name == "three_chunks":            # a forced count is taken as it is: 4 column tiles in chunks of 1, 1, 2
        assert gpf._backend.kmvm_chunking(200, 200, 3) == [(0, 1), (1, 2), (2, 4)]
    tol = max(8 * spread, 64 * EPS)
    assert tol <= 1e-11, "the reference's own spread (%.3g) leaves no room under the hard cap" % spread
    out = _run_product(gpf, name)
    err = float(np.max(np.abs(out - ref) / scale))
    print("%s: spread %.3g tol %.3g error %.3g" % (name, spread, tol, err))
    assert out.shape == ref.shape and np.all(np.isfinite(out))
    assert err <= tol


def test_equal_bytes(gpf):
    a, b = _run_product(gpf, "three_chunks"), _run_product(gpf, "three_chunks")
    assert np.array_equal(a, b)


_CG = {}


def _cg_case(n, T):
    """RBF in 3 dims, noise 0.5; columns: [0] the all-ones vector scaled (an easy direction), [-1] exactly zero, the others random
    (T = 1 has room for one column only: a random one)"""
    if (n, T) not in _CG:
        rng = np.random.default_rng(1000 + n + T)
        X = rng.normal(size=(n, 3))
        B = rng.normal(size=(n, T))
        if T > 1:
            B[:, 0], B[:, -1] = 0.3, 0.0
        lf = mr.leaf("rbf", range(3), n)
        A, cond = mr.dense(lf, X, 0.5)
        _CG[(n, T)] = (lf, X, B, A, cond, mr.solve(A, B))
    return _CG[(n, T)]


@pytest.mark.parametrize("n", [65, 200])
@pytest.mark.parametrize("T", [1, 5, 17])
def test_batched_cg(gpf, n, T):
    """Per column against the long-double dense A: converged; true residual |A x - b| <= 10 tol |b| (the recurrence residual stops
    at tol |b| and differs from the true one by O(eps cond iterations) ~ 1e-11 |b|, far below 9 tol |b|); forward error
    |x - x*| <= cond(A) 10 tol |x*|; the zero column exact zeros after 0 iterations."""
    lf, X, B, A, cond, xs = _cg_case(n, T)
    tol = 1e-9
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        x, info = gpf.conjugate_gradient.kernel_cgsolver(_kern(gpf, lf, 3), X, B, 0.5, max_iter=4 * n, tol=tol)
    assert np.all(info["converged"]) and np.all(info["iterations"] < 4 * n)
    res = np.linalg.norm(np.asarray(A @ x.astype(mr.LD) - B, dtype=np.float64), axis=0)
    fwd = np.linalg.norm(np.asarray(x - xs, dtype=np.float64), axis=0)
    print("n %d T %d cond %.3g iterations %s residual %s forward %s" % (n, T, cond, info["iterations"], res, fwd))
    assert np.all(res <= 10 * tol * np.linalg.norm(B, axis=0))
    assert np.all(fwd <= cond * 10 * tol * np.linalg.norm(np.asarray(xs, dtype=np.float64), axis=0))
    if T > 1:
        assert np.all(x[:, -1] == 0.0) and info["iterations"][-1] == 0 and info["relative_residual"][-1] == 0.0
        assert info["iterations"][0] < np.max(info["iterations"][1:-1])          # the columns stop at different iterations


def test_cg_out_of_iterations_warns(gpf):
    lf, X, B = _cg_case(200, 5)[:3]
    with pytest.warns(UserWarning, match="did not reach tol"):
        x, info = gpf.conjugate_gradient.kernel_cgsolver(_kern(gpf, lf, 3), X, B, 0.5, max_iter=3, tol=1e-9)
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(info["relative_residual"]))
    assert not np.any(info["converged"][:-1]) and np.all(info["iterations"][:-1] == 3)
    assert info["converged"][-1] and info["iterations"][-1] == 0                  # (the zero column)


@pytest.mark.parametrize("kind", ["matern52", "rbf"])
@pytest.mark.parametrize("n_new", [5, 19])
def test_predict_f_iterative(gpf, kind, n_new):
    """mean and variance against the long-double dense solve under the bound of test_batched_cg carried through the products:
    |mean - ref| <= cond 10 tol |K(Xnew, X)| |alpha*| per output, |var_j - ref_j| <= cond 10 tol |k_j| |x_j*| per test point."""
    n, R, noise, tol = 200, 2, 0.5, 1e-9
    rng = np.random.default_rng(77 + n_new)
    X, Xs, Y = rng.normal(size=(n, 3)), rng.normal(size=(n_new, 3)), rng.normal(size=(n, R))
    lf = mr.leaf(kind, range(3), n_new)
    c = np.array([0.4, -1.1])
    m = gpf.models.GPR(X, Y, _kern(gpf, lf, 3), mean_function=gpf.mean_functions.Constant(c), obs_var=noise)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        mean, var = m.predict_f_iterative(Xs, max_iter=4 * n, tol=tol)
    A, cond = mr.dense(lf, X, noise)
    Ks = mr.K_ld(lf, X, Xs)
    alpha, Z = mr.solve(A, Y - c), mr.solve(A, Ks)
    ref_mean = np.asarray(Ks.T @ alpha + c, dtype=np.float64)
    ref_var = np.asarray(lf["variance"] - np.sum(Ks * Z, 0), dtype=np.float64)
    m64, v64 = kr.gpr_predict(lf, X, Y - c, noise, Xs)                             # (the fp64 yardstick agrees with the long-double one)
    assert np.max(np.abs(m64 + c - ref_mean)) <= 1e-10 and np.max(np.abs(v64 - ref_var)) <= 1e-10
    nrm = lambda a: np.linalg.norm(np.asarray(a, dtype=np.float64), axis=0)        # noqa: E731
    assert mean.shape == (n_new, R) and var.shape == (n_new, R) and np.array_equal(var[:, 0], var[:, 1])
    bound_mean = cond * 10 * tol * np.linalg.norm(np.asarray(Ks, dtype=np.float64), 2) * nrm(alpha)
    bound_var = cond * 10 * tol * nrm(Ks) * nrm(Z)
    print("cond %.3g mean error %s of %s, var error %.3g of %.3g" % (cond, nrm(mean - ref_mean), bound_mean,
                                                                     np.max(np.abs(var[:, 0] - ref_var)), np.min(bound_var)))
    assert np.all(nrm(mean - ref_mean) <= bound_mean)
    assert np.all(np.abs(var[:, 0] - ref_var) <= bound_var)


def test_refuses_33_dims(gpf, monkeypatch):
    """33 active dims (the instances hold 32 feature rows): refused on the host, before the product or the gradient form reaches
    the backend's entry"""
    be, cg = gpf._backend, gpf.conjugate_gradient

    def launched(*a, **k):
        raise AssertionError("the backend was entered")
    monkeypatch.setattr(be, "kmvm", launched)
    monkeypatch.setattr(be, "kmvm_grad", launched)
    X, V = np.ones((4, 33)), np.ones((4, 1))
    with pytest.raises(ValueError, match="at most 32 active dims"):
        cg.kernel_matmul(gpf.kernels.RBF(33, lengthscales=np.ones(33), ARD=True), X, V)
    with pytest.raises(ValueError, match="at most 32 active dims"):
        cg.kernel_grad_form(gpf.kernels.Matern52(33), X, V, V)


def test_refusals(gpf):
    be, cg, k = gpf._backend, gpf.conjugate_gradient, gpf.kernels
    h = gpf.get_handle()
    X, V = np.ones((4, 2)), np.ones((4, 1))
    with pytest.raises(RuntimeError, match=r"gps_kmvm failed \(-4\)"):             # GPS_ERR_UNSUPPORTED
        be.kmvm(h, (k.RBF(2) + k.RBF(2))._program(2), X, V)
    with pytest.raises(NotImplementedError, match="one stationary kernel"):
        cg.kernel_matmul(k.Periodic(2), X, V)

    class Featured(k.RBF):
        def features(self, X):
            return X
    with pytest.raises(NotImplementedError, match="one stationary kernel"):
        gpf.models.GPR(X, V, Featured(2)).predict_f_iterative(X)
    h._arm_scales(np.ones((4, 2)), X)                                             # Multiscale scales armed: the existing refusal
    with pytest.raises(RuntimeError, match="Multiscale feature scales are armed"):
        be.kmvm(h, k.RBF(2)._program(2), X, V)
    assert be.kmvm(h, k.RBF(2)._program(2), X, V).shape == (4, 1)                  # (disarmed by the refusal)
