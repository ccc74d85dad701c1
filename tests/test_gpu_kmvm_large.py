"""The matrix-free exact-GP path above its launch-geometry thresholds (csrc/kmvm.hip, csrc/pchol.hip, csrc/gps_kmvm.hip): the
sizes at which the chunk rule cuts unequal multi-tile chunks, the gradient form folds over more than one workgroup, the CG
vector kernels stride their rows past KCG_MAX_BLOCKS workgroups, the pivot search folds across workgroups (and takes a second
pass), and the preconditioner's Gram / L^T V / L S launches reach their caps gb, tg, lsg.  tests/test_kmvm_ref_cpu.py proves on
the CPU that every size below is above the threshold it names, from the project's own sources.

No dense matrix above n = 2112: the references are tests/_kmvm_ref.py's product_rows, factor_columns and sample_rows, O(rows n)
and O(n k^2).  All cases: noise 0.5, seeds fixed by name, points ~ N(0, 1) in D = 3 under an ARD RBF leaf unless the case says
otherwise.  Tolerances: test_gpu_kmvm.py's rule, tol = max(8 spread, 64 eps) times the natural scale, under a cap on the
reference's own spread (1e-11 product and form, 1e-9 factor and preconditioner); the CG conditions are test_batched_cg's with the
residual on the sampled rows.  Printed spreads, tolerances, errors and iteration counts: docs/LAB_NOTES.md.
"""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _kmvm_ref as mr  # noqa: E402
from test_gpu_kmvm import _kern  # noqa: E402
from test_gpu_kmvm_train import _kern as _form_kern, dense_form  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
LD = mr.LD
NOISE = 0.5
CAP_PRODUCT, CAP_FACTOR = 1e-11, 1e-9

# The sizes, in one place (tests/test_kmvm_ref_cpu.py checks each against the geometry it is here for)
PRODUCT_SYM = [(2112, 17), (8300, 65)]                       # (n, T): 33 tiles in 32 chunks of 1 or 2 ; 130 tiles in 8 chunks of 16 or 17, two passes
PRODUCT_RECT = [("matern12", 130, 2112, 3), ("matern12", 130, 4200, 3)]      # (kernel, n, n2, T): 33 one-tile chunks ; 66 tiles under the 64-chunk cap
FORM_SIZES = [(300, 5), (520, 5), (2112, 17)]                # (n, C), P != Q: nblk 2, 3, 9 ; the last on 32 auto chunks
N_CG, T_CG, CG_TOL, CG_MAX_ITER, PCG_RANK = 8300, 3, 1e-9, 1000, 33
# (kernel, n, D, rank cap, X[7] = X[290])
FACTORS = [("rbf", 300, 3, 33, True), ("matern32", 520, 3, 64, False), ("rbf", 4200, 3, 128, False), ("rbf", 65600, 2, 8, False)]
PRECOND = [(4200, 17, 33), (8300, 17, 33), (32800, 1, 16)]   # (n, T, rank)


@pytest.fixture(scope="module")
def gpf():
    import gpflowSlim
    return gpflowSlim


def _seed(name):
    return sum(map(ord, name))


def points(name, kind, n, D):
    """(leaf, X) of the named case"""
    rng = np.random.default_rng(_seed(name))
    return mr.leaf(kind, range(D), _seed(name) + n), rng.normal(size=(n, D))


# ---- product ---------------------------------------------------------------------------------------------------------------------
_PRODUCT = {}


def product_case(n, T):
    if (n, T) not in _PRODUCT:
        lf, X = points("product_%d" % n, "rbf", n, 3)
        V = np.random.default_rng(n + T).normal(size=(n, T))
        rows = mr.sample_rows(n)
        _PRODUCT[(n, T)] = (lf, X, V, rows) + mr.product_rows(lf, X, V, rows, 0.37)
    return _PRODUCT[(n, T)]


@pytest.mark.parametrize("n,T", PRODUCT_SYM)
def test_product_rows_sampled(gpf, n, T):
    lf, X, V, rows, ref, scale, spread = product_case(n, T)
    chunks = gpf._backend.kmvm_chunking(n, n, 0)
    lengths = sorted({b - a for a, b in chunks})
    assert len(chunks) > 1 and len(lengths) == 2 and lengths[1] >= 2          # unequal chunks, some of more than one tile
    tol = max(8 * spread, 64 * EPS)
    assert tol <= CAP_PRODUCT, "the reference's own spread (%.3g) leaves no room under the hard cap" % spread
    kern = _kern(gpf, lf, 3)
    out, out2 = (gpf.conjugate_gradient.kernel_matmul(kern, X, V, diag_add=0.37) for _ in range(2))
    err = float(np.max(np.abs(out[rows] - ref) / scale))
    print("product n %d T %d (%d chunks of %s tiles, %d rows): spread %.3g tol %.3g error %.3g"
          % (n, T, len(chunks), lengths, len(rows), spread, tol, err))
    assert out.shape == (n, T) and np.all(np.isfinite(out))
    assert err <= tol
    assert np.array_equal(out, out2)                                          # equal bytes from call to call


@pytest.mark.parametrize("kind,n,n2,T", PRODUCT_RECT)
def test_product_rectangular(gpf, kind, n, n2, T):
    name = "rect_%s_%d_%d" % (kind, n, n2)
    lf, X = points(name, kind, n, 3)
    rng = np.random.default_rng(_seed(name) + 1)
    X2, V = rng.normal(size=(n2, 3)), rng.normal(size=(n2, T))
    ref, scale, spread = mr.product(lf, X, V, X2)
    tol = max(8 * spread, 64 * EPS)
    assert tol <= CAP_PRODUCT, "the reference's own spread (%.3g) leaves no room under the hard cap" % spread
    out = gpf.conjugate_gradient.kernel_matmul(_kern(gpf, lf, 3), X, V, X2=X2)
    err = float(np.max(np.abs(out - ref) / scale))
    print("%s: %d chunks, spread %.3g tol %.3g error %.3g" % (name, len(gpf._backend.kmvm_chunking(n, n2, 0)), spread, tol, err))
    assert out.shape == ref.shape and np.all(np.isfinite(out)) and err <= tol


# ---- gradient form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,C", FORM_SIZES)
def test_form_slot_by_slot(gpf, n, C):
    """test_gpu_kmvm_train.py::test_form_slot_by_slot's rule where kmvm_grad_fold_kernel adds more than one workgroup's partial"""
    name = "form_%d" % n
    lf, X = points(name, "rbf", n, 3)
    rng = np.random.default_rng(_seed(name) + C)
    P, Q = rng.standard_normal((n, C)), rng.standard_normal((n, C))
    ref, scale = dense_form(lf, X, P, Q, LD), dense_form(lf, X, P, Q, LD, absolute=True)
    spread = float(np.max(np.abs(dense_form(lf, X, P, Q, np.float64) - ref) / scale))
    tol = max(8 * spread, 64 * EPS)
    assert tol <= CAP_PRODUCT, "the reference's own spread (%.3g) leaves no room under the hard cap" % spread
    out = [gpf.conjugate_gradient.kernel_grad_form(_form_kern(gpf, lf), X, P, Q) for _ in range(2)]
    got = np.append(out[0][0], out[0][1])
    err = np.asarray(np.abs(got - ref) / scale, dtype=np.float64)
    print("form n %d C %d: spread %.3g tol %.3g errors %s" % (n, C, spread, tol, err))
    assert got.shape == ref.shape and np.all(np.isfinite(got)) and np.all(err <= tol)
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]    # equal bytes from call to call


# ---- batched CG, PCG and the log-determinant past KCG_MAX_BLOCKS workgroups ---------------------------------------------------------
_CG = {}


def cg_case():
    if "case" not in _CG:
        lf, X = points("cg_large", "rbf", N_CG, 3)
        B = np.random.default_rng(_seed("cg_large") + 1).normal(size=(N_CG, T_CG))
        B[:, 0] = 0.3
        rows = mr.sample_rows(N_CG)
        _CG["case"] = (lf, X, B, rows)
        _CG["A"] = mr.K_rows(lf, X, rows)                          # long-double rows of K, once for every residual below
    return _CG["case"]


def plain_solve(gpf):
    """the plain loop's two calls, run once and shared by the CG and the PCG test"""
    if "plain" not in _CG:
        lf, X, B, _ = cg_case()
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            _CG["plain"] = [gpf.conjugate_gradient.kernel_cgsolver(_kern(gpf, lf, 3), X, B, NOISE, max_iter=CG_MAX_ITER, tol=CG_TOL)
                            for _ in range(2)]
    return _CG["plain"]


def sampled_residual(x):
    """max_i |(A x - b)_i| over the sampled rows, per column, with A x from long-double rows of K"""
    lf, X, B, rows = cg_case()
    xl = np.asarray(x, dtype=LD)
    Ax = _CG["A"] @ xl + LD(NOISE) * xl[rows]
    return np.asarray(np.max(np.abs(Ax - B[rows].astype(LD)), axis=0), dtype=np.float64)


def test_batched_cg_past_max_blocks(gpf):
    """every column converged below max_iter; on the sampled rows |(A x - b)_i| <= 10 tol |b|_2 (test_batched_cg's bound on the
    norm, which bounds every entry); two calls give equal bytes"""
    B = cg_case()[2]
    (x, info), (x2, info2) = plain_solve(gpf)
    assert np.all(info["converged"]) and np.all(info["iterations"] < CG_MAX_ITER)
    res, bound = sampled_residual(x), 10 * CG_TOL * np.linalg.norm(B, axis=0)
    print("cg n %d: iterations %s sampled residual %s bound %s" % (N_CG, info["iterations"], res, bound))
    assert np.all(np.isfinite(x)) and np.all(res <= bound)
    assert np.array_equal(x, x2) and np.array_equal(info["iterations"], info2["iterations"])
    assert np.array_equal(info["relative_residual"], info2["relative_residual"])


def test_pcg_past_max_blocks(gpf):
    """precond_rank = 33: the same residual condition, fewer iterations than the plain loop, and x within the two solves' forward
    bounds of each other: |x_pcg - x_cg|_inf <= 2 cond_bound 10 tol |x|_inf with cond_bound = (n variance + noise) / noise
    (lambda_max(K) <= tr K = n variance, lambda_min >= noise): a bound, not a measurement"""
    lf, X, B, _ = cg_case()
    (xp, infop), _ = plain_solve(gpf)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        x, info = gpf.conjugate_gradient.kernel_cgsolver(_kern(gpf, lf, 3), X, B, NOISE, max_iter=CG_MAX_ITER, tol=CG_TOL,
                                                         precond_rank=PCG_RANK)
    assert np.all(info["converged"]) and np.all(info["iterations"] < CG_MAX_ITER) and info["rank"] == PCG_RANK
    res, bound = sampled_residual(x), 10 * CG_TOL * np.linalg.norm(B, axis=0)
    cond_bound = (N_CG * lf["variance"] + NOISE) / NOISE
    diff = float(np.max(np.abs(x - xp)))
    print("pcg n %d rank %d: iterations %s (plain %s) sampled residual %s bound %s; |x_pcg - x_cg| %.3g of %.3g"
          % (N_CG, info["rank"], info["iterations"], infop["iterations"], res, bound, diff,
             2 * cond_bound * 10 * CG_TOL * np.max(np.abs(xp))))
    assert np.all(np.isfinite(x)) and np.all(res <= bound)
    assert np.max(info["iterations"]) < np.max(infop["iterations"])
    assert diff <= 2 * cond_bound * 10 * CG_TOL * float(np.max(np.abs(xp)))


def test_logdet_past_max_blocks(gpf):
    """three +-1 probes through the plain Lanczos loop: it converges (kernel_logdet raises otherwise), alpha has one row per
    iteration, two calls give equal bytes.  (What ties the tridiagonal to log is checked at small n.)"""
    lf, X, _, _ = cg_case()
    Z = np.random.default_rng(_seed("logdet_large")).integers(0, 2, size=(N_CG, 3)) * 2.0 - 1.0
    (est, per, info), (est2, per2, info2) = (gpf.conjugate_gradient.kernel_logdet(_kern(gpf, lf, 3), X, NOISE, probes=Z, tol=CG_TOL,
                                                                                   max_iter=CG_MAX_ITER) for _ in range(2))
    print("logdet n %d: iterations %s estimate %.10g" % (N_CG, info["iterations"], est))
    assert np.all(info["converged"]) and np.all(info["iterations"] < CG_MAX_ITER)
    assert info["alpha"].shape == (np.max(info["iterations"]), 3) and np.all(np.isfinite(per)) and est == np.mean(per)
    assert est == est2 and np.array_equal(per, per2) and np.array_equal(info["alpha"], info2["alpha"])
    assert np.array_equal(info["beta"], info2["beta"])


# ---- pivoted Cholesky past one workgroup -------------------------------------------------------------------------------------------
def factor_points(kind, n, D, cap, dup):
    lf, X = points("factor_%d" % n, kind, n, D)
    if dup:
        X[7] = X[290]                                            # two identical points in different workgroups
    return lf, X


@pytest.mark.parametrize("kind,n,D,cap,dup", FACTORS)
def test_factor(gpf, kind, n, D, cap, dup):
    """test_gpu_pchol.py::test_factor's assertions against factor_columns with the device's pivots.  piv[0] == 0 is a tie of all n
    diagonal entries: the cross-workgroup fold's lowest-index rule."""
    rel_tol = 1e-10
    lf, X = factor_points(kind, n, D, cap, dup)
    kern = _kern(gpf, lf, D)
    L, piv, trace = gpf.conjugate_gradient.kernel_pivoted_cholesky(kern, X, cap, rel_tol)
    L2, piv2, trace2 = gpf.conjugate_gradient.kernel_pivoted_cholesky(kern, X, cap, rel_tol)
    assert np.array_equal(L, L2) and np.array_equal(piv, piv2) and trace == trace2            # equal bytes from call to call
    k, var = len(piv), lf["variance"]
    assert L.shape == (n, k) and 1 <= k <= min(cap, n) and len(set(piv.tolist())) == k and piv[0] == 0
    assert np.all((piv >= 0) & (piv < n))
    if dup:
        assert not {7, 290} <= set(piv.tolist())
    Lr, dr, dp, dmax = mr.factor_columns(lf, X, piv, LD)
    L64, d64, _, _ = mr.factor_columns(lf, X, piv, np.float64)
    col = np.asarray(np.sqrt(dp) / var, dtype=np.float64)                                    # 1 / (the scale of column m)
    spread = max(float(np.max(np.abs(L64 - Lr) * col)), float(np.max(np.abs(d64 - dr))) / var)
    tol = max(8 * spread, 64 * EPS)
    assert tol <= CAP_FACTOR, "the reference's own spread (%.3g) leaves no room under the hard cap" % spread
    err = float(np.max(np.abs(L - Lr) * col))
    gap = float(np.max(dmax - dp)) / var
    print("%s n %d cap %d: rank %d spread %.3g tol %.3g L error %.3g pivot gap %.3g trace %.6g (ref %.6g)"
          % (kind, n, cap, k, spread, tol, err, gap, trace, float(np.sum(dr))))
    assert np.all(np.isfinite(L)) and err <= tol and gap <= tol
    assert abs(trace - float(np.sum(dr))) <= tol * n * var
    if k < min(cap, n):
        assert float(dr.max()) <= (rel_tol + tol) * var


# ---- the preconditioner's apply past gb, tg, lsg ----------------------------------------------------------------------------------
def woodbury(L, V, s, dtype):
    """((V - L C^-1 L^T V) / s, C^-1 L^T V, C = s I + L^T L) in `dtype`, O(n k)"""
    Ld, Vd = L.astype(dtype), V.astype(dtype)
    C = dtype(s) * np.eye(L.shape[1], dtype=dtype) + Ld.T @ Ld
    t = Ld.T @ Vd
    y = mr.solve(C, t) if dtype is LD else np.linalg.solve(C, t)
    return (Vd - Ld @ y) / dtype(s), y, C


@pytest.mark.parametrize("n,T,rank", PRECOND)
def test_precond_solve_logdet_sample(gpf, n, T, rank):
    """M^-1 V against Woodbury in long double with the device's own L (test_factor checks that L), under
    test_gpu_pchol.py::test_precond_solve_logdet_sample's scale and spread rule; the independent residual
    |L (L^T out) + s out - V| <= tol (|L| |L^T| |out| + s |out| + |V|) entry by entry; log det M against slogdet(C) + (n - k) log s;
    at n = 8300 the sample L G1 + sqrt(s) V under that test's 64 eps rule."""
    lf, X = points("precond_%d" % n, "rbf", n, 3)
    kern = _kern(gpf, lf, 3)
    L, _, _ = gpf.conjugate_gradient.kernel_pivoted_cholesky(kern, X, rank)
    k = L.shape[1]
    rng = np.random.default_rng(n)
    V, G1 = rng.normal(size=(n, T)), rng.normal(size=(rank, T))
    out, logdet = gpf.conjugate_gradient.kernel_precond_solve(kern, X, V, NOISE, rank)
    ref, y, C = woodbury(L, V, NOISE, LD)
    r64, _, C64 = woodbury(L, V, NOISE, np.float64)
    aL = np.abs(L)
    scale = (np.abs(V) + aL @ np.abs(np.asarray(y, dtype=np.float64))) / NOISE
    spread = float(np.max(np.abs(r64 - ref) / scale))
    tol = max(8 * spread, 64 * EPS)
    assert tol <= CAP_FACTOR
    err = float(np.max(np.abs(out - ref) / scale))
    Ll, ol = L.astype(LD), out.astype(LD)
    resid = np.abs(Ll @ (Ll.T @ ol) + LD(NOISE) * ol - V.astype(LD))
    rscale = aL @ (aL.T @ np.abs(out)) + NOISE * np.abs(out) + np.abs(V)
    rerr = float(np.max(resid / rscale))
    w = np.linalg.eigvalsh(C64)
    ld_ref = np.linalg.slogdet(C64)[1] + (n - k) * np.log(NOISE)
    ld_scale = float(np.sum(np.abs(np.log(w)))) + (n - k) * abs(np.log(NOISE))
    ld_tol = max(8 * abs(float(np.sum(np.log(w))) + (n - k) * np.log(NOISE) - ld_ref) / ld_scale, 64 * EPS)
    print("precond n %d T %d rank %d: spread %.3g tol %.3g error %.3g residual %.3g; logdet %.12g (ref %.12g, tol %.3g)"
          % (n, T, k, spread, tol, err, rerr, logdet, ld_ref, ld_tol * ld_scale))
    assert out.shape == (n, T) and np.all(np.isfinite(out))
    assert err <= tol and rerr <= tol
    assert abs(logdet - ld_ref) <= ld_tol * ld_scale
    if n == 8300:
        smp, _ = gpf.conjugate_gradient.kernel_precond_solve(kern, X, V, NOISE, rank, G1=G1)
        s_ref = Ll @ G1[:k].astype(LD) + np.sqrt(LD(NOISE)) * V.astype(LD)
        s_scale = aL @ np.abs(G1[:k]) + np.sqrt(NOISE) * np.abs(V)
        s_err = float(np.max(np.abs(smp - s_ref) / s_scale))
        print("  sample error %.3g of %.3g" % (s_err, 64 * EPS))
        assert s_err <= 64 * EPS
