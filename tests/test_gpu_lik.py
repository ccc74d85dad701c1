"""Non-Gaussian likelihoods on the device (csrc/lik.hip, gps_svgp_elbo_lik / gps_svgp_elbo_lik_grad) against the CPU
restatement of the reference in tests/_lik_ref.py (pinned on its own in tests/test_lik_cpu.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lik_ref as ref  # noqa: E402
import oracle.gp_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu
c = orc.constrained
EPS = np.finfo(float).eps
ELEM_TOL = 1e-12          # the elementwise gate of tests/test_gpu_parity.py: the sides differ in libm and summation order only
# ... except where a kind needs more: 10 x the measured maximum (docs/LAB_NOTES.md, "likelihood kernels").  Bernoulli's dvar =
# (sum_h w_h l'(f_h) x_h) / sqrt(2 var): the sum cancels down to O(sqrt var) and is then divided by sqrt(2 var), so at
# var = 1e-6 the rounding of its O(1) terms is amplified 707 x on BOTH sides; measured 1.4e-12.
ELEM_TOL_OF = {("bernoulli", "dvar"): 1.4e-11}


def solve_tol(K):
    """tests/test_gpu_parity.py: two backward-stable fp64 solves differ by at most 2 eps cond_2(K), never gated below 1e-8"""
    return max(1e-8, 2.0 * EPS * float(np.linalg.cond(K)))


def _lik(kind, params, n_gh=20):
    from gpflowSlim import _backend as be
    return be.make_lik(ref.KIND_ID[kind], params, n_gh)


def _rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


# ---- the kernels on their own ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,k", [("bernoulli", 3), ("poisson", 2), ("exponential", 2), ("student_t", 3), ("multiclass", 3),
                                    ("multiclass", 10), ("gaussian", 2)])
def test_lik_varexp_values_and_derivatives(handle, kind, k):
    """gps_lik_varexp on seeded moments with fvar in [1e-6, 10] (above the 1e-10 clips: every point counts): the sum, every
    point's own value (one-point calls), dmu, dvar and the parameter derivative against the restatement."""
    rng = np.random.default_rng(1000 + k + len(kind))
    n = 700
    mu, var, Y, params = ref.sample_inputs(kind, n, k, rng, var_lo=1e-6, var_hi=10.0)
    assert var.min() >= 1e-6 and var.max() <= 10.0
    lik = _lik(kind, params)
    rve, rdmu, rdvar, rdpar = ref.varexp_grad(kind, params, mu, var, Y)
    ve = handle.lik_varexp(lik, mu, var, Y)
    ve2, dmu, dvar, dpar = handle.lik_varexp(lik, mu, var, Y, want_grad=True)
    assert ve == ve2 == handle.lik_varexp(lik, mu, var, Y)                          # bit-reproducible, with or without derivatives
    scale = max(1.0, float(np.sum(np.abs(rve))))                                   # (a sum of n k terms of either sign)
    figures = {"sum": abs(ve - float(np.sum(rve))) / scale, "dmu": _rel(dmu, rdmu), "dvar": _rel(dvar, rdvar),
               "dpar": abs(dpar - rdpar) / max(1.0, abs(rdpar))}
    pts = []
    for i in range(0, n, 97):
        one = handle.lik_varexp(lik, mu[i:i + 1], var[i:i + 1], Y[i:i + 1])
        pts.append(abs(one - float(np.sum(rve[i]))) / max(1.0, abs(float(np.sum(rve[i])))))
    figures["point"] = max(pts)
    print("lik_varexp %s k=%d: %s" % (kind, k, {a: "%.3g" % b for a, b in figures.items()}))
    for name, v in figures.items():
        assert v <= ELEM_TOL_OF.get((kind, name), ELEM_TOL), (kind, name, v)


# ---- the fused bound and its gradient --------------------------------------------------------------------------------------------
def _problem(kind, k, whiten, q_diag, n=240, m_=30, d=2, seed=0, mean=None, train_inducing=False):
    import gpflowSlim as gpf
    rng = np.random.default_rng(seed + 17 * k + (3 if whiten else 0) + (5 if q_diag else 0))
    X = rng.standard_normal((n, d))
    F = np.sin(X @ rng.standard_normal((d, k)))
    params = {"bernoulli": [], "poisson": [0.7], "exponential": [], "student_t": [0.6, 3.0], "multiclass": [1e-3], "gaussian": [0.3]}[kind]
    if kind == "bernoulli":
        Y = (F + 0.3 * rng.standard_normal((n, k)) > 0).astype(float)
        like = gpf.likelihoods.Bernoulli()
    elif kind == "poisson":
        Y = rng.poisson(np.exp(F) * 0.7).astype(float)
        like = gpf.likelihoods.Poisson(binsize=0.7)
    elif kind == "exponential":
        Y = rng.exponential(np.exp(F))
        like = gpf.likelihoods.Exponential()
    elif kind == "student_t":
        Y = F + 0.3 * rng.standard_t(3.0, (n, k))
        like = gpf.likelihoods.StudentT(3.0)
        like._scale.assign(0.6)
    else:
        Y = np.argmax(F + 0.3 * rng.standard_normal((n, k)), 1).astype(float)[:, None]
        like = gpf.likelihoods.MultiClass(k)
    ls = np.linspace(0.5, 0.7, d)
    kern = gpf.kernels.RBF(d, variance=1.3, lengthscales=ls, ARD=True)
    theta = np.concatenate([[c(1.3)], c(ls)])

    def spec(th):
        return {"type": "rbf", "variance": th[0], "lengthscales": th[1:], "input_dim": d}

    Z = X[:m_].copy() + 0.05 * rng.standard_normal((m_, d))
    mf = gpf.mean_functions.Constant(np.full(k, 0.2)) if mean else None
    m = gpf.models.SVGP(X, Y, kern, like, Z=Z, q_diag=q_diag, whiten=whiten, num_data=3 * n, num_latent=k, mean_function=mf,
                        train_inducing=train_inducing)
    q_mu = rng.standard_normal((m_, k)) * 0.3
    if q_diag:
        q_sqrt = np.abs(rng.standard_normal((m_, k))) * 0.4 + 0.2
    else:
        q_sqrt = np.tril(rng.standard_normal((k, m_, m_)) * (0.5 / m_) + np.eye(m_) * 0.5).transpose(1, 2, 0).copy()
    if not whiten:
        # a q(u) on the scale of the prior p(u) = N(0, Kuu), as a fitted model has it: the whitened draw mapped through
        # chol(Kuu); diagonal q_sqrt: in units of the conditional standard deviations 1 / sqrt(diag(Kuu^-1)).  (Taken on the
        # whitened scale instead, q_sqrt^T Kuu^-1 kuf gives latent variances of 1e2 - 1e3 and exp(var / 2) overflows.)
        Kuu = orc.K(spec(theta), Z) + orc.JITTER * np.eye(m_)
        Lz = np.linalg.cholesky(Kuu)
        q_mu = Lz @ q_mu
        if q_diag:
            q_sqrt = q_sqrt / np.sqrt(np.diag(np.linalg.inv(Kuu)))[:, None]
        else:
            q_sqrt = np.stack([Lz @ np.tril(q_sqrt[:, :, q]) for q in range(k)], 2)
    m._q_mu.assign(q_mu)
    m._q_sqrt.assign(q_sqrt)
    q_sqrt = np.asarray(m.q_sqrt).copy()
    params = [float(np.squeeze(like.scale)), 3.0] if kind == "student_t" else params
    mean_X = np.asarray(m.mean_function(X)) if mean else None
    return m, dict(kind=kind, params=params, spec=spec, theta=theta, X=X, Y=Y, Z=Z, q_mu=q_mu, q_sqrt=q_sqrt, whiten=whiten,
                   num_data=3 * n, mean_X=mean_X)


def _ref_bound(P, **over):
    a = dict(P); a.update(over)
    return ref.svgp_bound(a["kind"], a["params"], a["spec"](a["theta"]), a["X"], a["Y"], a["Z"], a["q_mu"], a["q_sqrt"],
                          whiten=a["whiten"], num_data=a["num_data"], mean_X=a["mean_X"])


CASES = [("bernoulli", 2), ("poisson", 1), ("exponential", 2), ("student_t", 2), ("multiclass", 3), ("multiclass", 10)]


@pytest.mark.parametrize("q_diag", [False, True])
@pytest.mark.parametrize("whiten", [True, False])
@pytest.mark.parametrize("kind,k", CASES)
def test_svgp_lik_bound(handle, kind, k, whiten, q_diag):
    """the fused bound against the restatement composed with the oracle's conditional and gauss_kl, and against the package's
    own host fallback (same model, likelihood wrapped so that it is not recognised as built-in)"""
    m, P = _problem(kind, k, whiten, q_diag, mean=(kind == "student_t"))
    bound = m.compute_log_likelihood()
    rb = _ref_bound(P)
    tol = solve_tol(orc.K(P["spec"](P["theta"]), P["Z"]) + orc.JITTER * np.eye(P["Z"].shape[0]))
    print("bound %s k=%d whiten=%s q_diag=%s: %.12g ref %.12g rel %.3g (gate %.3g)" % (kind, k, whiten, q_diag, bound, rb, abs(bound - rb) / abs(rb), tol))
    assert abs(bound - rb) <= tol * abs(rb)
    assert m._device_lik() is not None
    inner = m.likelihood
    m.likelihood._device_spec = lambda: None                     # not recognised as built-in any more: host fallback
    assert m._device_lik() is None
    host = m.compute_log_likelihood()
    del inner._device_spec
    assert abs(bound - host) <= tol * abs(host), (bound, host)


@pytest.mark.parametrize("q_diag", [False, True])
@pytest.mark.parametrize("whiten", [True, False])
@pytest.mark.parametrize("kind,k", CASES)
def test_svgp_lik_gradient(handle, kind, k, whiten, q_diag):
    """the gradient (kernel parameters, q_mu, q_sqrt, StudentT.scale, mean-function parameters, Z) against central differences
    of the restatement: step and gate of tests/test_gpu_grad.py::test_svgp_bound_gradient_unwhitened"""
    m, P = _problem(kind, k, whiten, q_diag, mean=(kind in ("student_t", "bernoulli")), train_inducing=True)
    bound, grads = m.compute_log_likelihood_and_gradients()
    rb = _ref_bound(P)
    assert abs(bound - rb) <= 1e-8 * abs(rb)
    assert abs(bound - m.compute_log_likelihood()) <= 1e-9 * abs(bound)
    by = {id(p): g for p, g in grads}
    worst = [0.0]

    def cd(make, x0, hrel=1e-6):
        h = hrel * max(1.0, abs(x0))
        return (make(x0 + h) - make(x0 - h)) / (2 * h)

    def check(got, fd, what):
        worst[0] = max(worst[0], abs(got - fd) / max(1.0, abs(fd)))
        assert abs(got - fd) <= 2e-5 * max(1.0, abs(fd)), (what, got, fd)

    def con(p):
        return np.atleast_1d(by[id(p)] / p.transform.forward_grad(p.vf_val))

    got = np.concatenate([con(p).ravel() for p in m.kern.parameters])
    theta = P["theta"]
    assert got.shape == theta.shape
    for i in range(theta.size):
        def mk(v, i=i):
            th = theta.copy(); th[i] = v
            return _ref_bound(P, theta=th)
        check(got[i], cd(mk, theta[i]), ("theta", i))
    if kind == "student_t":
        s0 = P["params"][0]
        check(float(con(m.likelihood._scale)), cd(lambda v: _ref_bound(P, params=[v, 3.0]), s0), "scale")
    if P["mean_X"] is not None:
        gc = con(m.mean_function.c).ravel()
        for q in range(k):
            def mk(v, q=q):
                mx = P["mean_X"].copy(); mx[:, q] = v
                return _ref_bound(P, mean_X=mx)
            check(gc[q], cd(mk, 0.2), ("mean", q))
    rng2 = np.random.default_rng(2)
    m_ = P["Z"].shape[0]
    gq = by[id(m._q_mu)]
    for _ in range(4):
        a, q = int(rng2.integers(m_)), int(rng2.integers(k))
        def mk(v, a=a, q=q):
            qm = P["q_mu"].copy(); qm[a, q] = v
            return _ref_bound(P, q_mu=qm)
        check(gq[a, q], cd(mk, P["q_mu"][a, q]), ("q_mu", a, q))
    if q_diag:
        gs = by[id(m._q_sqrt)] / m._q_sqrt.transform.forward_grad(m._q_sqrt.vf_val)
        for _ in range(4):
            a, q = int(rng2.integers(m_)), int(rng2.integers(k))
            def mk(v, a=a, q=q):
                qs = P["q_sqrt"].copy(); qs[a, q] = v
                return _ref_bound(P, q_sqrt=qs)
            check(gs[a, q], cd(mk, P["q_sqrt"][a, q]), ("q_sqrt", a, q))
    else:
        rows, cols = np.tril_indices(m_, 0)
        gfree = by[id(m._q_sqrt)].reshape(k, -1)
        for _ in range(6):
            t, q = int(rng2.integers(rows.size)), int(rng2.integers(k))
            a, b = int(rows[t]), int(cols[t])
            def mk(v, a=a, b=b, q=q):
                qs = P["q_sqrt"].copy(); qs[a, b, q] = v
                return _ref_bound(P, q_sqrt=qs)
            check(gfree[q, t], cd(mk, P["q_sqrt"][a, b, q]), ("q_sqrt", a, b, q))
    gZ = by[id(m.feature._Z)]
    for _ in range(4):
        a, j = int(rng2.integers(m_)), int(rng2.integers(P["Z"].shape[1]))
        def mk(v, a=a, j=j):
            Z = P["Z"].copy(); Z[a, j] = v
            return _ref_bound(P, Z=Z)
        check(gZ[a, j], cd(mk, P["Z"][a, j]), ("Z", a, j))
    print("gradient %s k=%d whiten=%s q_diag=%s: worst |g - fd| / max(1, |fd|) = %.3g" % (kind, k, whiten, q_diag, worst[0]))


@pytest.mark.parametrize("q_diag", [False, True])
@pytest.mark.parametrize("whiten", [True, False])
def test_general_backward_reduces_to_the_gaussian(handle, whiten, q_diag):
    """With dmu = (Y - mu) / s2 and dvar = -1 / (2 s2) (GPS_LIK_GAUSSIAN, kept in the kind table for this) the general backward
    pass reproduces gps_svgp_elbo_grad to rounding: 1e-11 relative to the largest gradient entry."""
    import gpflowSlim as gpf
    from gpflowSlim._settings import settings
    rng = np.random.default_rng(8)
    n, m_, d, k = 300, 40, 3, 2
    X = rng.standard_normal((n, d)); Y = np.sin(X @ rng.standard_normal((d, k))) + 0.1 * rng.standard_normal((n, k))
    Z = X[:m_].copy()
    kern = gpf.kernels.RBF(d, variance=1.2, lengthscales=np.linspace(0.8, 1.5, d), ARD=True)
    prog = kern._program(d)
    q_mu = rng.standard_normal((m_, k)) * 0.3
    if q_diag:
        q_sqrt = np.abs(rng.standard_normal((m_, k))) * 0.4 + 0.2
    else:
        q_sqrt = np.tril(rng.standard_normal((k, m_, m_)) * (0.5 / m_) + np.eye(m_) * 0.5).transpose(1, 2, 0).copy()
    s2, jit = 0.3, settings.numerics.jitter_level
    a = handle.svgp_elbo_grad(prog, Z, X, Y, q_mu, q_sqrt, jit, s2, white=whiten, scale=3.0, want_grad_Z=True)
    b = handle.svgp_elbo_lik_grad(prog, Z, X, Y, q_mu, q_sqrt, jit, _lik("gaussian", [s2]), white=whiten, scale=3.0, want_grad_Z=True)
    assert abs(a[0] - b[0]) <= 1e-12 * abs(a[0])
    for name, ga, gb in zip(("slots", "noise", "q_mu", "q_sqrt", "mean", "Z"), a[1:], b[1:]):
        ga, gb = np.atleast_1d(ga), np.atleast_1d(gb)
        err = np.max(np.abs(ga - gb)) / np.max(np.abs(ga))
        print("reduction whiten=%s q_diag=%s %s: %.3g" % (whiten, q_diag, name, err))
        assert err <= 1e-11, (name, err)


# ---- training ------------------------------------------------------------------------------------------------------------------
def _bernoulli_data(seed=3, n=200):
    rng = np.random.default_rng(seed)
    y = (rng.random(n) < 0.5).astype(float)
    X = rng.standard_normal((n, 2)) * 0.6 + np.where(y[:, None] == 1, 1.6, -1.6) * np.array([1.0, 0.5])
    return X, y[:, None]


def _blobs(seed=4, n=240):
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 3, n)
    centres = np.array([[0.0, 2.5], [-2.5, -1.5], [2.5, -1.5]])
    return centres[y] + 0.55 * rng.standard_normal((n, 2)), y.astype(float)[:, None]


def test_training_bernoulli(handle):
    import gpflowSlim as gpf
    X, Y = _bernoulli_data()
    m = gpf.models.SVGP(X, Y, gpf.kernels.RBF(2, lengthscales=1.5), gpf.likelihoods.Bernoulli(), Z=X[:15].copy())
    b0 = m.compute_log_likelihood()
    vals = []
    for _ in range(6):                                           # the bound after each block of accepted steps
        m.optimize(max_iter=5)
        vals.append(m.compute_log_likelihood())
    print("bernoulli training: %.6g -> %s" % (b0, ["%.6g" % v for v in vals]))
    assert all(b >= a for a, b in zip([b0] + vals[:-1], vals))
    p, _ = m.predict_y(X)
    acc = float(np.mean((p > 0.5) == (Y == 1)))
    print("bernoulli training accuracy %.3f" % acc)
    assert acc > 0.95
    assert np.all(np.isfinite(m.predict_density(X, Y)))


def test_training_multiclass(handle):
    import gpflowSlim as gpf
    X, Y = _blobs()
    m = gpf.models.SVGP(X, Y, gpf.kernels.RBF(2, lengthscales=1.5), gpf.likelihoods.MultiClass(3), Z=X[:15].copy(), num_latent=3,
                        whiten=False)
    b0 = m.compute_log_likelihood()
    vals = []
    for _ in range(6):
        m.optimize(max_iter=5)
        vals.append(m.compute_log_likelihood())
    print("multiclass training: %.6g -> %s" % (b0, ["%.6g" % v for v in vals]))
    assert all(b >= a for a, b in zip([b0] + vals[:-1], vals))
    p, _ = m.predict_y(X)
    acc = float(np.mean(np.argmax(p, 1) == Y[:, 0].astype(int)))
    print("multiclass training accuracy %.3f" % acc)
    assert acc > 0.95


# ---- size -------------------------------------------------------------------------------------------------------------------------
def test_bernoulli_at_a_million_points(handle):
    """M = 1024, N = 10^6, K = 1: bound and gradient complete, and the bound is the sum over ten shards of 10^5 points evaluated
    separately (linear in the data term; the KL is counted once), to 1e-10 relative."""
    import gpflowSlim as gpf
    from gpflowSlim._settings import settings
    rng = np.random.default_rng(12)
    n, m_, d = 1000000, 1024, 4
    X = rng.standard_normal((n, d))
    Y = (np.sin(X[:, :1] * 1.3) + 0.4 * rng.standard_normal((n, 1)) > 0).astype(float)
    Z = rng.standard_normal((m_, d))
    kern = gpf.kernels.RBF(d, variance=1.1, lengthscales=1.4)
    prog = kern._program(d)
    q_mu = rng.standard_normal((m_, 1)) * 0.2
    q_sqrt = np.abs(rng.standard_normal((m_, 1))) * 0.3 + 0.3
    jit = settings.numerics.jitter_level
    lik = _lik("bernoulli", [])
    elbo, kl, ve = handle.svgp_elbo_lik(prog, Z, X, Y, q_mu, q_sqrt, jit, lik)
    res = handle.svgp_elbo_lik_grad(prog, Z, X, Y, q_mu, q_sqrt, jit, lik)
    assert res[0] == elbo and all(np.all(np.isfinite(np.atleast_1d(g))) for g in res[1:])
    parts = [handle.svgp_elbo_lik(prog, Z, X[s:s + 100000], Y[s:s + 100000], q_mu, q_sqrt, jit, lik) for s in range(0, n, 100000)]
    total = sum(p[2] for p in parts) - parts[0][1]
    print("N = 1e6 bound %.15g, ten shards %.15g, rel %.3g" % (elbo, total, abs(elbo - total) / abs(elbo)))
    assert abs(elbo - total) <= 1e-10 * abs(elbo)


def test_sharded_handle_refuses_the_gradient(handle):
    """like the sparse gradients: GPS_ERR_UNSUPPORTED while a collective is installed"""
    import ctypes
    import gpflowSlim as gpf
    from gpflowSlim import _backend as be
    h2 = gpf.Handle()
    fn = be.ALLREDUCE_FN(lambda ctx, ptr, cnt: 0)
    buf = ctypes.c_double(0)
    h2.set_allreduce(fn, ctypes.addressof(buf), 1)             # (never called, never dereferenced: the gradient refuses first)
    X = np.linspace(0, 1, 20)[:, None]; Y = (X > 0.5).astype(float)
    kern = gpf.kernels.RBF(1)
    with pytest.raises(Exception) as ei:
        h2.svgp_elbo_lik_grad(kern._program(1), X[:5].copy(), X, Y, np.zeros((5, 1)), np.ones((5, 1)), 1e-6, _lik("bernoulli", []))
    assert "sharded" in str(ei.value)
    h2.set_allreduce(None, 0, 0)
