"""GPU tests of the Lanczos variance estimates of the matrix-free path (csrc/lanczos.hip) against tests/_lanczos_ref.py: dense K_y
and Lanczos with double Gram-Schmidt in long double.  Late Lanczos vectors are ill-conditioned functions of the start vector, so
only the first 5 coefficients are compared with the reference; beyond that the tests check invariants (Q^T Q = I, Q^T K_y Q =
tridiag(alpha, beta)), the epilogue against the estimate formed in long double from the device's own Q, and known answers (the
exact variance at full rank, the Galerkin bound var_exact <= var_lanczos <= Kdiag at every rank).

Bounds: the largest error measured on an MI355X over the cases below, times a margin of about 10 for other reduction orders.
  max |Q^T Q - I|                                 measured 0.21 k eps   (matern32, N 70, rank 5)     bound ORTH = 2 k eps
  max |Q^T K_y Q - T| / |K_y|_2                   measured 0.14 k eps   (matern32, N 70, rank 5)     bound TRID = 1.5 k eps
  first 5 alpha, beta against the reference       measured 2.75 eps |K_y|_2 (composite, N 70)        bound COEF = 30 eps |K_y|_2
  var against the estimate on the device's own Q  measured 12.2 eps Kdiag (rbf_ard, N 257, rank 65)  bound EPI = 120 eps Kdiag
  var_exact - var (all ranks), |var - var_exact| at full rank
                                                  measured 5.0 eps Kdiag (rbf_ard, repeated points; 3.8 at rank = N = 70)
                                                                                                      bound FULL = 50 eps Kdiag
The breakdown cases stop at rank 35 (RBF, Matern32) and 36 (composite) of 70.
"""
import os
import sys
from unittest import mock

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lanczos_ref as lr  # noqa: E402
from test_gpu_kmvm_sop import dense, gpf, kern_of, per, spec_K, st  # noqa: E402, F401

pytestmark = pytest.mark.gpu
EPS, LD, NOISE, R3 = np.finfo(np.float64).eps, lr.LD, 1e-2, range(3)
SPECS = {"rbf_ard": [[st("rbf", R3, 1)]], "matern32": [[st("matern32", R3, 2)]],
         "rbf_periodic_plus_matern52": [[st("rbf", R3, 1), per(R3)], [st("matern52", R3, 2)]]}
SHAPES = [(70, 5, 7), (70, 70, 7), (130, 17, 130), (257, 64, 7), (257, 65, 130)]          # (N, rank, N*)
ORTH, TRID, COEF, EPI, FULL = 2.0, 1.5, 30.0, 120.0, 50.0          # multiples of k eps (ORTH, TRID), of eps (COEF), of eps Kdiag (EPI, FULL)
_REF = {}


def _case(name, n, n_new, repeat=False):
    """(spec, X, Xnew, Y, dense K_y, |K_y|_2, K(X, Xnew), Kdiag), long double where it matters; computed once"""
    key = (name, n, n_new, repeat)
    if key not in _REF:
        rng = np.random.default_rng(sum(map(ord, name)) + n + n_new)
        X = rng.normal(size=(n, 3))
        if repeat:
            X[n // 2:] = X[:n // 2]                # every point twice: the Krylov space of a symmetric start has n / 2 dimensions
        Xs, Y, spec = rng.normal(size=(n_new, 3)), rng.normal(size=(n, 2)), SPECS[name]
        A = dense(spec, X, NOISE)[0]
        kdiag = sum(np.prod([lf["variance"] for lf in term]) for term in spec)
        _REF[key] = (spec, X, Xs, Y, A, np.linalg.norm(np.asarray(A, dtype=np.float64), 2), spec_K(spec, X, Xs), kdiag)
    return _REF[key]


def _invariants(Q, al, be, A, nrm):
    """(max |Q^T Q - I|, max |Q^T K_y Q - tridiag(alpha, beta)| / |K_y|_2) in units of k eps"""
    Ql, k = Q.astype(LD), Q.shape[1]
    T = np.diag(al.astype(LD)) + np.diag(be.astype(LD), 1) + np.diag(be.astype(LD), -1)
    return (float(np.max(np.abs(Ql.T @ Ql - np.eye(k)))) / (k * EPS), float(np.max(np.abs(Ql.T @ A @ Ql - T))) / nrm / (k * EPS))


@pytest.mark.parametrize("name", list(SPECS))
@pytest.mark.parametrize("n,rank", [s[:2] for s in SHAPES])
def test_kernel_lanczos(gpf, name, n, rank):
    spec, X, _, _, A, nrm, _, _ = _case(name, n, 7)
    start = np.random.default_rng(n + rank).normal(size=n)
    Q, al, be = gpf.conjugate_gradient.kernel_lanczos(kern_of(gpf, spec), X, NOISE, start, rank)
    assert Q.shape == (n, rank) and al.shape == (rank,) and be.shape == (rank - 1,) and np.all(np.isfinite(Q))
    orth, trid = _invariants(Q, al, be, A, nrm)
    _, ral, rbe = lr.lanczos(A, start, min(rank, 6))
    coef = max(float(np.max(np.abs(al[:5] - ral[:5]))), float(np.max(np.abs(be[:5] - rbe[:5])))) / nrm / EPS
    print("%s n %d rank %d: orth %.3g k eps, trid %.3g k eps, first coefficients %.3g eps |K_y|" % (name, n, rank, orth, trid, coef))
    assert orth <= ORTH and trid <= TRID and coef <= COEF
    Q2, al2, be2 = gpf.conjugate_gradient.kernel_lanczos(kern_of(gpf, spec), X, NOISE, start, rank)
    assert Q.tobytes() == Q2.tobytes() and al.tobytes() == al2.tobytes() and be.tobytes() == be2.tobytes()


def _predict(gpf, name, n, rank, n_new, repeat=False):
    """(var of variance="lanczos", the device's own Q for the same start, the case): the start K(X, Xnew) 1 / N* is the fused
    product's, so kernel_lanczos on it retraces the run inside the prediction"""
    case = _case(name, n, n_new, repeat)
    spec, X, Xs, Y = case[:4]
    kern, cg = kern_of(gpf, spec), gpf.conjugate_gradient
    m = gpf.models.GPR(X, Y, kern, obs_var=NOISE)
    mean, var = m.predict_f_iterative(Xs, max_iter=8 * n, tol=1e-9, variance="lanczos", variance_rank=rank)
    start = cg.kernel_matmul(kern, X, np.full((n_new, 1), 1.0 / n_new), X2=Xs)[:, 0]
    Q, al, be = cg.kernel_lanczos(kern, X, NOISE, start, rank)
    assert mean.shape == (n_new, 2) and var.shape == (n_new, 2) and np.array_equal(var[:, 0], var[:, 1]) and np.all(np.isfinite(var))
    return m, mean, var[:, 0], Q, case


def _check_variance(name, var, Q, case, full):
    """items 2 and 3 of the issue: the epilogue against the long-double estimate on the device's Q; the Galerkin bound against the
    exact variance (equality at full rank); var <= Kdiag"""
    A, Ks, kdiag = case[4], case[6], case[7]
    est, exact = lr.estimate(A, Q, Ks, kdiag), lr.exact(A, Ks, kdiag)
    epi = float(np.max(np.abs(var - est))) / kdiag / EPS
    low = float(np.max(exact - var)) / kdiag / EPS
    print("%s: epilogue %.3g eps Kdiag, exact - var at most %.3g eps Kdiag, |var - exact| %.3g eps Kdiag"
          % (name, epi, low, float(np.max(np.abs(var - exact))) / kdiag / EPS))
    assert epi <= EPI and low <= FULL and np.all(var <= kdiag)
    if full:
        assert float(np.max(np.abs(var - exact))) / kdiag / EPS <= FULL


@pytest.mark.parametrize("name", list(SPECS))
@pytest.mark.parametrize("n,rank,n_new", SHAPES)
def test_predict_variance(gpf, name, n, rank, n_new):
    m, mean, var, Q, case = _predict(gpf, name, n, rank, n_new)
    assert Q.shape[1] == rank
    _check_variance("%s n %d rank %d" % (name, n, rank), var, Q, case, full=rank == n)
    mean_solve, _ = m.predict_f_iterative(case[2], max_iter=8 * n, tol=1e-9)
    assert mean.tobytes() == mean_solve.tobytes()


@pytest.mark.parametrize("name", list(SPECS))
def test_breakdown(gpf, name):
    """35 distinct points of 70 and a start vector that is equal on the copies: the run stops by itself, with what it has"""
    _, _, var, Q, case = _predict(gpf, name, 70, 70, 7, repeat=True)
    print("%s: rank found %d" % (name, Q.shape[1]))
    assert 1 <= Q.shape[1] <= 70 and np.all(np.isfinite(Q))
    _check_variance(name + " repeated", var, Q, case, full=False)


def test_refusals_before_the_backend(gpf, monkeypatch):
    be, cg, k = gpf._backend, gpf.conjugate_gradient, gpf.kernels
    launched = mock.Mock(side_effect=AssertionError("the backend was entered"))
    for name in ("kernel_lanczos", "kernel_predict_lanczos", "kernel_predict", "kernel_predict_sop", "kernel_predict_pcg"):
        monkeypatch.setattr(be, name, launched)
    X, Y = np.ones((4, 2)), np.ones((4, 1))
    m = gpf.models.GPR(X, Y, k.RBF(2), obs_var=0.5)
    for call, match in [(lambda: m.predict_f_iterative(X, variance="cholesky"), "variance must be"),
                        (lambda: m.predict_f_iterative(X, variance="lanczos", precond_rank=2), "lanczos.*precond_rank")] + [
                        (lambda r=r: m.predict_f_iterative(X, variance="lanczos", variance_rank=r), "Lanczos rank") for r in (0, 129, 5)] + [
                        (lambda r=r: cg.kernel_lanczos(k.RBF(2), X, 0.5, Y, r), "Lanczos rank") for r in (0, 129, 5)]:
        with pytest.raises(ValueError, match=match):
            call()
