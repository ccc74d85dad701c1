"""CPU tests of tests/_psi_ref.py, the reference the GPU tests of the Bayesian GPLVM compare against: the closed forms against
Gauss-Hermite quadrature and a 50-digit mpmath fixture, the analytic gradient against central differences, the limit S = 0."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _psi_ref as pr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("Q", [1, 2])
def test_closed_forms_against_gauss_hermite(Q):
    """<k(x, z)> and <k(z, x) k(x, z')> under N(mu, diag S) by a 60-point tensor Gauss-Hermite rule.  The integrands are entire and
    of Gaussian type, the rule is exact to far below fp64 for these widths; 1e-13 leaves room for the summation of 60^Q terms."""
    d = pr.inputs(4, 3, Q, seed=5 + Q)
    x, w = np.polynomial.hermite.hermgauss(60)
    grids = np.meshgrid(*([x] * Q), indexing="ij")
    W = np.prod(np.meshgrid(*([w] * Q), indexing="ij"), axis=0).ravel() / np.pi ** (Q / 2)
    nodes = np.stack([g.ravel() for g in grids], axis=1)              # [P, Q]
    p1, p2 = pr.psi1(d["var"], d["ls"], d["Z"], d["mu"], d["S"]), pr.psi2n(d["var"], d["ls"], d["Z"], d["mu"], d["S"])
    for n in range(4):
        X = d["mu"][n] + np.sqrt(2 * d["S"][n]) * nodes
        K = pr.rbf_K(d["var"], d["ls"], X, d["Z"])                    # [P, M]
        assert np.abs(W @ K / p1[n] - 1).max() <= 1e-13
        assert np.abs(np.einsum("p,pa,pb->ab", W, K, K) / p2[n] - 1).max() <= 1e-13


def _fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "mp", "bgplvm.npz"))
    return g, dict(var=float(g["variance"]), ls=g["lengthscales"], noise=float(g["noise"]), Z=g["Z"], mu=g["X_mean"], S=g["X_var"], Y=g["Y"])


def test_against_the_mpmath_fixture():
    g, a = _fixture()
    r = pr.psi_with_spread(a["var"], a["ls"], a["Z"], a["mu"], a["S"])
    assert np.abs(r["psi1"] / g["psi1"] - 1).max() <= 16 * np.finfo(float).eps
    assert np.abs(r["psi2"] / g["psi2"] - 1).max() <= 16 * np.finfo(float).eps
    assert r["psi1_spread"] <= 1e-14 and r["psi2_spread"] <= 1e-14
    F, mean, var = pr.bound(**a, Xnew=g["Xnew"])
    _, _, cov = pr.bound(**a, Xnew=g["Xnew"], full_cov=True)
    assert abs(F - g["F"]) <= 1e-12 * abs(g["F"]) and abs(pr.kl(a["mu"], a["S"]) - g["KL"]) <= 1e-13 * abs(g["KL"])
    assert np.abs(mean - g["mean"]).max() <= 1e-11 and np.abs(cov - g["cov"]).max() <= 1e-11
    assert np.abs(var - np.diag(g["cov"])).max() <= 1e-11
    Fl, ml, vl, cl = pr.bound_ld(**a, Xnew=g["Xnew"])
    assert abs(Fl - g["F"]) <= 1e-14 * abs(g["F"]) and np.abs(ml - g["mean"]).max() <= 1e-14 and np.abs(cl - g["cov"]).max() <= 1e-14
    assert np.array_equal(vl, np.diag(cl))
    F2, gr = pr.bound_grad(**a)
    assert abs(F2 - g["F"]) <= 1e-11 * abs(g["F"])
    for k in ("variance", "lengthscales", "noise", "Z", "X_mean", "X_var"):
        assert np.abs(np.asarray(gr[k]) - g["grad_" + k]).max() <= 1e-10 * max(1.0, np.abs(g["grad_" + k]).max()), k
    _, grl = pr.bound_grad(**a, dtype=np.longdouble)
    for k in ("variance", "lengthscales", "noise", "Z", "X_mean", "X_var"):
        assert np.abs(np.asarray(grl[k]) - g["grad_" + k]).max() <= 1e-13 * max(1.0, np.abs(g["grad_" + k]).max()), k


def test_analytic_gradient_against_central_differences():
    d = pr.inputs(7, 4, 2, R=2, seed=1)
    a = dict(var=d["var"], ls=d["ls"], noise=0.3, Z=d["Z"], mu=d["mu"], S=d["S"], Y=d["Y"], jitter=1e-3)   # (jitter: a well-conditioned Kuu, so that the differences resolve)
    _, g = pr.bound_grad(**a)
    names = {"variance": "var", "lengthscales": "ls", "noise": "noise", "Z": "Z", "X_mean": "mu", "X_var": "S"}
    for gname, aname in names.items():
        base = np.array(a[aname], dtype=np.float64)
        num = np.zeros(base.shape)
        for idx in np.ndindex(*base.shape) if base.shape else [()]:
            h = 1e-5
            up, dn = base.copy(), base.copy()
            up[idx] += h; dn[idx] -= h
            fu = pr.bound(**{**a, aname: up if base.shape else float(up)})[0]
            fd = pr.bound(**{**a, aname: dn if base.shape else float(dn)})[0]
            num[idx] = (fu - fd) / (2 * h)
        assert np.abs(num - np.asarray(g[gname])).max() <= 1e-6 * max(1.0, np.abs(num).max()), gname
    km, ks = pr.kl_grad(d["mu"], d["S"])
    h = 1e-6
    e = np.zeros_like(d["mu"]); e[2, 1] = h
    assert abs((pr.kl(d["mu"] + e, d["S"]) - pr.kl(d["mu"] - e, d["S"])) / (2 * h) - km[2, 1]) <= 1e-8
    assert abs((pr.kl(d["mu"], d["S"] + e) - pr.kl(d["mu"], d["S"] - e)) / (2 * h) - ks[2, 1]) <= 1e-7


def test_zero_variance_limit():
    d = pr.inputs(9, 5, 3, seed=8)
    S0 = np.zeros_like(d["S"])
    Kxz = pr.rbf_K(d["var"], d["ls"], d["mu"], d["Z"])
    assert np.abs(pr.psi1(d["var"], d["ls"], d["Z"], d["mu"], S0) / Kxz - 1).max() <= 1e-14
    assert np.abs(pr.psi2n(d["var"], d["ls"], d["Z"], d["mu"], S0).sum(0) / (Kxz.T @ Kxz) - 1).max() <= 1e-14
