"""GPU tests of GPMC (csrc/gps_gpmc.hip, the pointwise kernel of csrc/lik.hip, gpflowSlim/models/gpmc.py) against
tests/_gpmc_ref.py (tests/test_gpmc_ref_cpu.py checks that restatement) and tests/_lik_ref.py.

Gates.  The triangular products and the seed are dot products of at most N (R) terms whichever way they are associated, so
each side is within N eps of the exact value times sum |terms|: 3 N eps (|L| |V|)_i and 3 R eps |U| |V| bound the difference
(derived, not measured).  The pointwise likelihood differs from numpy in libm and summation order only: ELEM_TOL of
tests/test_gpu_lik.py.  Everything that goes through the factor of K + 1e-6 I is gated by the project's
solve_tol(K) = max(1e-8, 2 eps cond_2(K)), relative to max(1, max |reference|) of that output; the two restated CPU paths
differ by 2.2e-11 on these kernels (test_gpmc_ref_cpu.py), far inside it.

Sizes: the products at N = 1, 127, 128, 129 (the 128 tile edge), 700 (across the 512-row chunk and the 256-column stage) and
2100 (past the 2048 small-N limit of the factorisation; several row chunks), R = 1, 3, 16, 17 (each template and the 16-column
chunking); the entry points at N = 129 and 300 and once at 2100."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gpmc_ref as gr  # noqa: E402
import _kern_ref as kr  # noqa: E402
import _lik_ref as lr  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
ELEM_TOL = 1e-12          # tests/test_gpu_lik.py
JITTER = 1e-6


def _gpf():
    import gpflowSlim as gpf
    return gpf


def _rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))


def solve_tol(K):
    """tests/test_gpu_parity.py: two backward-stable fp64 solves differ by at most 2 eps cond_2(K), never gated below 1e-8
    (K symmetric positive definite: cond_2 from its extreme eigenvalues)"""
    w = np.linalg.eigvalsh(K)
    return max(1e-8, 2.0 * EPS * float(w[-1] / w[0]))


def _lik(kind, params):
    return _gpf()._backend.make_lik(lr.KIND_ID[kind], params, 20)


# ---- the skinny triangular products ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 127, 128, 129, 700, 2100])
def test_tri_skinny_products(handle, n):
    rng = np.random.default_rng(n)
    Lt = np.tril(rng.standard_normal((n, n)))
    L = Lt.copy()
    L[np.triu_indices(n, 1)] = np.nan                               # whatever sits above the diagonal must never be read
    aL = np.abs(Lt)
    for r in (1, 3, 16, 17):
        B = rng.standard_normal((n, r))
        for trans, M, aM in ((False, Lt, aL), (True, Lt.T, aL.T)):
            got = handle.tri_skinny(L, B, trans=trans)
            assert got.shape == (n, r) and not np.any(np.isnan(got)), (n, r, trans)
            bound = 3.0 * n * EPS * (aM @ np.abs(B))
            err = np.abs(got - M @ B)
            worst = float(np.max(err / np.maximum(bound, np.finfo(float).tiny)))
            print("tri_skinny n=%d r=%d trans=%d: worst error / bound %.3g" % (n, r, trans, worst))
            assert np.all(err <= bound), (n, r, trans, worst)
            assert np.array_equal(got, handle.tri_skinny(L, B, trans=trans)), (n, r, trans)      # bit for bit, run to run


# ---- the pointwise likelihood ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", gr.KINDS)
def test_lik_logp_values_and_derivatives(handle, kind):
    rng = np.random.default_rng(2000 + len(kind))
    n, k = 700, 3
    F, _, Y, params = lr.sample_inputs(kind, n, k, rng)
    lik = _lik(kind, params)
    rlp = lr.logp(kind, params, F, Y)
    rG, rdpar = gr.dlogp(kind, params, F, Y)
    lp = handle.lik_logp(lik, F, Y)
    lp2, G, dpar = handle.lik_logp(lik, F, Y, want_grad=True)
    assert lp == lp2 == handle.lik_logp(lik, F, Y)
    figures = {"sum": abs(lp - float(np.sum(rlp))) / max(1.0, abs(float(np.sum(rlp)))), "G": _rel(G, rG),
               "dpar": abs(dpar - rdpar) / max(1.0, abs(rdpar))}
    entry = np.abs(G - rG) / np.maximum(1.0, np.abs(rG))
    figures["G_entry"] = float(entry.max())
    pts = [abs(handle.lik_logp(lik, F[i:i + 1], Y[i:i + 1]) - float(np.sum(rlp[i]))) / max(1.0, abs(float(np.sum(rlp[i]))))
           for i in range(0, n, 97)]
    figures["point"] = max(pts)
    print("lik_logp %s: %s" % (kind, {a: "%.3g" % b for a, b in figures.items()}))
    for name, v in figures.items():
        assert v <= ELEM_TOL, (kind, name, v)


def test_lik_logp_refuses_multiclass(handle):
    with pytest.raises(NotImplementedError, match="piecewise constant"):
        handle.lik_logp(_lik("multiclass", [1e-3]), np.zeros((4, 3)), np.zeros((4, 3)))


# ---- the rank-R seed ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 3, 17])
@pytest.mark.parametrize("n", [129, 700])
def test_chol_seed(handle, n, r):
    rng = np.random.default_rng(10 * n + r)
    U, V = rng.standard_normal((n, r)), rng.standard_normal((n, r))
    P = handle.chol_seed(U, V)
    npad = -(-n // 128) * 128
    assert P.shape == (npad, npad)
    assert not np.any(P[n:, :]) and not np.any(P[:, n:])            # the padding is zero
    S = P[:n, :n]
    assert np.array_equal(S, S.T)
    lo = np.tril(np.ones((n, n), dtype=bool))
    ref = gr.seed(U, V)
    bound = 3.0 * r * EPS * np.where(lo, np.abs(U) @ np.abs(V).T, (np.abs(U) @ np.abs(V).T).T)
    err = np.abs(S - ref)
    print("chol_seed n=%d r=%d: worst error / bound %.3g" % (n, r, float(np.max(err / bound))))
    assert np.all(err <= bound)
    assert np.array_equal(P, handle.chol_seed(U, V))


# ---- gps_gpmc_lik / gps_gpmc_lik_grad ---------------------------------------------------------------------------------------------
def _kern(name):
    k = _gpf().kernels
    if name == "rbf":
        return k.RBF(2, variance=1.3, lengthscales=np.array([0.5, 0.7]), ARD=True)
    return k.Matern52(2, variance=0.9, lengthscales=np.array([0.8, 1.1]), ARD=True) + k.Linear(2, variance=np.array([0.3, 0.2]), ARD=True)


@functools.lru_cache(maxsize=None)
def _ref(kname, kind, n, r):
    """the restated likelihood and gradient of one case, computed once and left unchanged"""
    kern = _kern(kname)
    spec = kr.spec_of(kern, 2)
    X, V, Y, params, mean = gr.make_case(kind, n, r)
    res = gr.grad(spec, X, V, Y, kind, params, mean, jitter=JITTER)
    res.update(X=X, V=V, Y=Y, params=params, mean=mean, tol=solve_tol(res["K"]), prog=kern._program(2))
    return res


CASES = [(kn, kind, n, r) for kn in ("rbf", "matern52+linear") for kind in gr.KINDS for n in (129, 300) for r in (1, 3)]
CASES.append(("rbf", "bernoulli", 2100, 3))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s-%d-%d" % c)
def test_gpmc_lik_and_grad(handle, case):
    c = _ref(*case)
    assert c["tol"] <= 2.0 * EPS * 1e9                              # (every case stays below cond 1e9)
    lik = _lik(case[1], c["params"])
    ll = handle.gpmc_lik(c["prog"], c["X"], c["V"], c["Y"], JITTER, lik, mean=c["mean"])
    ll2, slots, glik, gV, gmean = handle.gpmc_lik_grad(c["prog"], c["X"], c["V"], c["Y"], JITTER, lik, mean=c["mean"])
    assert ll == ll2
    assert slots.shape == c["slots"].shape and gV.shape == c["gV"].shape
    figures = {"loglik": abs(ll - c["loglik"]) / max(1.0, abs(c["loglik"])), "slots": _rel(slots, c["slots"]),
               "glik": abs(glik - c["glik"]) / max(1.0, abs(c["glik"])), "gV": _rel(gV, c["gV"]), "gmean": _rel(gmean, c["gmean"])}
    print("gpmc %s: tol %.3g %s" % (case, c["tol"], {a: "%.3g" % b for a, b in figures.items()}))
    for name, v in figures.items():
        assert v <= c["tol"], (case, name, v, c["tol"])
    # without a mean the entry takes NULL: same thing as a zero mean
    if case[2] == 129:
        ll0 = handle.gpmc_lik(c["prog"], c["X"], c["V"], c["Y"], JITTER, lik)
        ref0 = gr.loglik(kr.spec_of(_kern(case[0]), 2), c["X"], c["V"], c["Y"], case[1], c["params"], None, JITTER)
        assert abs(ll0 - ref0) <= c["tol"] * max(1.0, abs(ref0))
    # bit for bit, run to run
    again = handle.gpmc_lik_grad(c["prog"], c["X"], c["V"], c["Y"], JITTER, lik, mean=c["mean"])
    assert again[0] == ll2 and np.array_equal(again[1], slots) and again[2] == glik and np.array_equal(again[3], gV)


def test_gpmc_not_positive_definite(handle):
    """every point the same and no jitter: K is all ones (exactly, with variance 1), the second pivot exactly zero"""
    gpf = _gpf()
    be = gpf._backend
    prog = be.make_program([be.primitive_node(be.K_RBF, 1.0, dims=(0, 1), lengthscales=(1.0, 1.0))])
    X, V, Y = np.zeros((129, 2)), np.ones((129, 1)), np.ones((129, 1))
    with pytest.raises(gpf.NotPositiveDefiniteError):
        handle.gpmc_lik(prog, X, V, Y, 0.0, _lik("bernoulli", []))
    with pytest.raises(gpf.NotPositiveDefiniteError):
        handle.gpmc_lik_grad(prog, X, V, Y, 0.0, _lik("bernoulli", []))
    c = _ref("rbf", "bernoulli", 129, 1)                            # the handle is usable afterwards
    ll = handle.gpmc_lik(c["prog"], c["X"], c["V"], c["Y"], JITTER, _lik("bernoulli", []), mean=c["mean"])
    assert abs(ll - c["loglik"]) <= c["tol"] * max(1.0, abs(c["loglik"]))


# ---- the model ------------------------------------------------------------------------------------------------------------------
def _model(kind="student_t", n=200, r=2, seed=3):
    gpf = _gpf()
    X, V, Y, params, _ = gr.make_case(kind, n, r, seed=seed)
    if kind == "student_t":
        like = gpf.likelihoods.StudentT(3.0)
        like._scale.assign(0.6)
    else:
        like = gpf.likelihoods.Bernoulli()
    m = gpf.models.GPMC(X, Y, _kern("rbf"), like, mean_function=gpf.mean_functions.Constant(np.full(r, 0.2)))
    m._V.assign(V)
    return m, X, V, Y


def test_model_objective_and_chain_rule(handle):
    m, X, V, Y = _model()
    spec = kr.spec_of(m.kern, 2)
    params = [float(np.squeeze(m.likelihood.scale)), 3.0]
    mean = np.asarray(m.mean_function(X)) * np.ones_like(V)
    ref = gr.grad(spec, X, V, Y, "student_t", params, mean, jitter=JITTER)
    tol = solve_tol(ref["K"])
    prior = float(np.sum(-0.5 * np.log(2 * np.pi) - 0.5 * V * V))
    obj = m.objective
    assert abs(obj + (ref["loglik"] + prior)) <= tol * max(1.0, abs(ref["loglik"] + prior))
    x0 = m._pack()
    f0, g = m._objective_and_grad(x0)
    assert f0 == obj
    # the chain to the unconstrained parameters against the restatement: kernel slots, likelihood scale, mean, V and its prior
    folded = kr.fold(spec, ref["slots"])                            # [variance, lengthscale 0, lengthscale 1]
    assert [p.name for p in m.parameters] == ["c", "variance", "ls", "scale", "V"]
    constrained = {"c": np.sum(ref["gmean"], axis=0), "variance": folded[:1], "ls": folded[1:], "scale": np.array([ref["glik"]]),
                   "V": ref["gV"].ravel()}
    want = [constrained[p.name] * np.atleast_1d(p.transform.forward_grad(p.vf_val)).ravel() for p in m.parameters]
    want[-1] = want[-1] - V.ravel()                                 # the N(0, 1) prior on V
    want = -np.concatenate(want)
    assert g.shape == want.shape
    assert np.abs(g - want).max() <= tol * max(1.0, np.abs(want).max())
    # ... and against five-point differences of `objective` on three entries: a lengthscale, the likelihood's scale, one of V.
    # Each evaluation is within tol max(1, |objective|) of the exact value (the gate above), which the step divides:
    # 1.5 tol max(1, |objective|) / h; the truncation error of the formula is below 10 x 6.6e-8 (test_gpmc_ref_cpu.py).
    offs = dict(zip([p.name for p in m.parameters], np.cumsum([0] + [int(np.size(p.vf_val)) for p in m.parameters])))
    picks = [offs["ls"] + 1, offs["scale"], offs["V"] + 17]
    h = 1e-3

    def f(x):
        m._unpack(x)
        return m.objective
    for i in picks:
        def fi(t, i=i):
            x = x0.copy()
            x[i] = t
            return f(x)
        fd = gr.five_point(fi, x0[i], h)
        gate = 1.5 * tol * max(1.0, abs(obj)) / h + 6.6e-7 * max(1.0, abs(g[i]))
        print("chain entry %d: analytic %.10g differences %.10g gate %.3g" % (i, g[i], fd, gate))
        assert abs(fd - g[i]) <= gate
    m._unpack(x0)


def test_model_optimize_predict_and_reproducibility(handle):
    gpf = _gpf()
    m, X, V, Y = _model("bernoulli", n=200, r=1, seed=4)
    m._V.assign(np.zeros_like(V))
    f0 = m.objective
    f1 = m.optimize(max_iter=20)
    assert np.isfinite(f1) and f1 < f0 and m.objective == pytest.approx(f1, rel=1e-12)
    Xs = np.random.default_rng(1).standard_normal((9, 2))
    mu, var = m.predict_f(Xs)
    cm, cv = handle.conditional(m.kern._program(2), X, Xs, m.V, JITTER, q_sqrt=None, white=True)
    assert np.array_equal(mu, cm + m.mean_function(Xs)) and np.array_equal(var, cv)
    mu_f, var_f = m.predict_f_full_cov(Xs)
    assert var_f.shape == (9, 9, 1) and np.abs(np.diagonal(var_f[:, :, 0]) - var[:, 0]).max() <= 1e-8
    p, _ = m.predict_y(Xs)
    assert p.shape == (9, 1) and np.all((p > 0) & (p < 1))
    assert np.all(np.isfinite(m.predict_density(Xs, np.ones((9, 1)))))
    # a likelihood the device does not know (here: Bernoulli hiding its descriptor) gets F from the device and is summed on the
    # host: same value, no gradient
    class Opaque(gpf.likelihoods.Bernoulli):
        def _device_spec(self):
            return None
    m3 = gpf.models.GPMC(X, Y, m.kern, Opaque(), mean_function=m.mean_function)
    m3._V.assign(m.V)
    ll = m.compute_log_likelihood()
    tol = solve_tol(kr.K(kr.spec_of(m.kern, 2), X) + JITTER * np.eye(X.shape[0]))
    assert abs(m3.compute_log_likelihood() - ll) <= tol * max(1.0, abs(ll))
    with pytest.raises(NotImplementedError, match="built-in likelihoods"):
        m3.compute_log_likelihood_and_gradients()
    # same seed, same result, bit for bit
    m2, _, _, _ = _model("bernoulli", n=200, r=1, seed=4)
    m2._V.assign(np.zeros_like(V))
    assert m2.objective == f0
    assert m2.optimize(max_iter=20) == f1
    assert all(np.array_equal(a.vf_val, b.vf_val) for a, b in zip(m.parameters, m2.parameters))
