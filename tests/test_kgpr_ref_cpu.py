"""CPU tests of tests/_kgpr_ref.py, the restatement the GPU tests of Kronecker GP regression compare against, and of the
selection helper of gpflowSlim/models/kgpr.py (pure numpy, no GPU).

Measured here on kr.CASES (RBF(.7, 1.3) x RBF(.5, .8), noise .1): at tol = 1e-20 the restated CG converges in 1 to 140
iterations with relative residual at most 2.0e-11; the two association orders K1 (S K2) and (K1 S) K2 agree to 1.7e-12 on the
converged x and to 2.4e-15 after five iterations, but at the reference's defaults (tol 1e-6, 100 iterations) they are 4.3e-5
apart on the full 24 x 20 grid and stop one or two iterations apart: the iterate, unlike the solution, is ill conditioned.
The converged restatement is within 1.7e-10 of the dense solve, its analytic gradient within 3.8e-11 of five-point differences
of the dense likelihood."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _kgpr_ref as kr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpflow-slim_amd"))
SMALL = [c for c in kr.CASES if c[0] * c[1] <= 600]


def _rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def _select():
    from gpflowSlim.models.kgpr import _select
    return _select


@pytest.mark.parametrize("case", kr.CASES, ids=lambda c: "%dx%d" % c[:2])
def test_cases_converge(case):
    """Every case of the GPU tests is usable: at tol = 1e-20 the restatement stops before 400 iterations with the
    preconditioned relative residual below 1e-10, in either association order."""
    X1, X2, Y, mask = kr.make_case(*case)
    K1, K2 = kr.kernels(X1, X2)
    C = kr.noise_of(mask, kr.THETA["s2"]) ** -0.5
    xs = []
    for order in ("k1_sk2", "k1s_k2"):
        x, k, _, _ = kr.cgsolver(K1, K2, C * Y, C, 400, 1e-20, order)
        assert k < 400
        assert kr.rel_residual(K1, K2, C, C * Y, x, order)[0] <= 1e-10
        xs.append(x)
    assert _rel(xs[0], xs[1]) <= 1e-10


@pytest.mark.parametrize("case", SMALL, ids=lambda c: "%dx%d-%g" % c[:3])
def test_converged_cg_against_the_dense_solve(case):
    X1, X2, Y, mask = kr.make_case(*case)
    K1, K2 = kr.kernels(X1, X2)
    res = kr.lml(K1, K2, Y, mask, kr.THETA["s2"], 400, 1e-20)
    dn = kr.dense_lml(X1, X2, Y, mask, kr.THETA)
    assert _rel(res["alpha"], dn["alpha"]) <= 1e-9
    assert _rel(res["x"], dn["x"]) <= 1e-9
    assert abs(res["lml"] - dn["lml"]) <= 1e-9 * max(1.0, abs(dn["lml"]))


@pytest.mark.parametrize("case", SMALL, ids=lambda c: "%dx%d-%g" % c[:3])
def test_gradient_against_central_differences(case):
    """Five-point differences of the DENSE likelihood with step 1e-3 theta: truncation O(step^4), rounding about
    eps |lml| / step = 1e-16 * 1e3 / 1e-3 = 1e-10; measured 3.8e-11 or less."""
    X1, X2, Y, mask = kr.make_case(*case)
    K1, K2 = kr.kernels(X1, X2)
    res = kr.lml(K1, K2, Y, mask, kr.THETA["s2"], 400, 1e-20)
    g = kr.gradient(X1, X2, Y, mask, kr.THETA, res)
    fd = kr.dense_gradient_fd(X1, X2, Y, mask, kr.THETA)
    for key in g:
        assert abs(g[key] - fd[key]) <= 1e-8 * max(1.0, abs(fd[key])), key


def _check_select(e1, e2, M):
    s1, s2, rng = _select()(e1, e2, M)
    m, n = len(e1), len(e2)
    assert rng.dtype == np.int32 and rng.shape == (m, 2)
    assert np.array_equal(s1, np.sort(e1)[::-1]) and np.array_equal(s2, np.sort(e2)[::-1])
    assert np.all(rng[:, 0] >= 0) and np.all(rng[:, 0] <= rng[:, 1]) and np.all(rng[:, 1] <= n)
    assert int((rng[:, 1] - rng[:, 0]).sum()) == M
    mine = np.concatenate([s1[i] * s2[rng[i, 0]:rng[i, 1]] for i in range(m)] + [np.zeros(0)])
    ref, _ = kr.select_full_sort(e1, e2, M)
    assert np.array_equal(np.sort(mine)[::-1], np.sort(ref)[::-1])
    # a row with e1 >= 0 takes a prefix of the descending e2, a row with e1 < 0 a suffix
    full = rng[:, 1] > rng[:, 0]
    assert np.all(rng[full & (s1 >= 0), 0] == 0) and np.all(rng[full & (s1 < 0), 1] == n)


@pytest.mark.parametrize("seed", range(12))
def test_select_against_the_full_sort(seed):
    rs = np.random.RandomState(seed)
    m, n = rs.randint(1, 40), rs.randint(1, 40)
    e1, e2 = rs.standard_normal(m) * 3, rs.standard_normal(n)
    kind = seed % 4
    if kind == 1:           # a decaying positive spectrum with rounding-level negatives, as an RBF matrix has
        e1 = np.sort(np.exp(-rs.uniform(0, 45, m))) * np.where(rs.uniform(size=m) < 0.2, -1e-3, 1.0)
        e2 = np.exp(-rs.uniform(0, 45, n))
    elif kind == 2:         # repeated eigenvalues: ties at the threshold
        e1 = rs.choice([-1.0, 0.0, 0.5, 2.0], m)
        e2 = rs.choice([-2.0, 0.0, 1.0, 4.0], n)
    elif kind == 3:         # every product equal
        e1, e2 = np.full(m, 1.5), np.full(n, -2.0)
    N = m * n
    for M in sorted({0, 1, N - 1, N, N // 2, rs.randint(0, N + 1)}):
        if 0 <= M <= N:
            _check_select(e1, e2, M)


def test_select_ties_go_to_the_lower_row_first():
    s1, s2, rng = _select()(np.array([2.0, 2.0, 2.0]), np.array([1.0, 1.0]), 3)
    assert rng.tolist() == [[0, 2], [0, 1], [0, 0]]


def test_select_counts_instead_of_sorting():
    """m = n = 3000 (N = 9e6): the threshold comes from at most 64 counting passes of O(m log n); the products selected match a
    direct count at the threshold."""
    rs = np.random.RandomState(3)
    e1, e2 = np.exp(-rs.uniform(0, 40, 3000)), np.exp(-rs.uniform(0, 40, 3000))
    M = 5_000_000
    s1, s2, rng = _select()(e1, e2, M)
    cnt = rng[:, 1] - rng[:, 0]
    assert int(cnt.sum()) == M
    smallest_in = min(s1[i] * s2[rng[i, 1] - 1] for i in range(3000) if cnt[i] > 0)
    largest_out = max(s1[i] * s2[rng[i, 1]] for i in range(3000) if rng[i, 1] < 3000)
    assert smallest_in >= largest_out


def test_against_the_mpmath_fixture():
    """m, n = 3, 2 with one masked cell, 50 digits (tests/golden/mp/make_kgpr_golden.py: mpmath.eigsy, an exact solve,
    mpmath.diff of the whole evaluation for the gradient): the converged restatement to 1e-12."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "mp", "kgpr.npz"))
    th = dict(zip(["var1", "ls1", "var2", "ls2", "s2"], g["theta"]))
    X1, X2, Y, mask = g["X1"], g["X2"], g["Y"], g["mask"]
    K1, K2 = kr.kernels(X1, X2, th)
    assert _rel(K1, g["K1"]) <= 1e-14 and _rel(K2, g["K2"]) <= 1e-14
    res = kr.lml(K1, K2, Y, mask, th["s2"], 400, 1e-30)
    assert res["M"] == int(g["M"])
    for key in ("lml", "logdet", "quadratic", "alpha", "x"):
        assert _rel(res[key], g[key]) <= 1e-12, key
    mean = kr.predict(res["alpha"], kr.rbf(X1, g["Xnew1"], th["var1"], th["ls1"]), kr.rbf(X2, g["Xnew2"], th["var2"], th["ls2"]))
    assert _rel(mean, g["mean"]) <= 1e-12
    grad = kr.gradient(X1, X2, Y, mask, th, res)
    assert _rel([grad[k] for k in ("var1", "ls1", "var2", "ls2", "s2")], g["grad"]) <= 1e-12
    dn = kr.dense_lml(X1, X2, Y, mask, th)
    assert _rel(dn["lml"], g["lml"]) <= 1e-12 and _rel(dn["alpha"], g["alpha"]) <= 1e-12
