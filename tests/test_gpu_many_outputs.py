"""The models at 5 to 129 output columns (latent functions), where the device code handles the columns in groups: pairs of
right-hand sides (csrc/trsv_wave.hip), 4 at a time (the gemv kernels of csrc/blas1.hip and the Psi1 VJPs of csrc/psi.hip), the first
8 in registers (svgp_abar_kernel), 8 per workgroup row (lik_rowsq_kernel), 1 / 4 / 16 planes and then 16 at a time
(skinny_xt_kernel, tri_skinny and chol_seed of csrc/skinny.hip), up to 16 columns in the one-launch
small-N path and up to 128 augmented rows (csrc/gps_gpr.hip).  R = 5, 9, 17 are a full group plus a remainder for the group sizes
2, 4, 8 and 16; R = 128 is the last count every entry point takes and 129 the first that the capped ones refuse.

The cases, their seeds and the gates live in tests/_many_outputs.py; tests/test_many_outputs_ref_cpu.py checks on the CPU that
every case is admissible and that the comparisons below can fail.  Shapes: N = 129 or 130 and M = 40 (one 128 tile edge crossed by
the data), M = 130 once.  Every device result is compared with a reference computed on the CPU in the same test."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gpmc_ref as gr  # noqa: E402
import _lik_ref as lr  # noqa: E402
import _many_outputs as mo  # noqa: E402
import _psi_ref as pr  # noqa: E402
import oracle.gp_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL = 1e-8                  # tests/test_gpu_parity.py: values
FD_TOL = 2e-5                # tests/test_gpu_grad.py: central differences of the oracle, relative step 1e-6
ELEM_TOL = 1e-12             # tests/test_gpu_lik.py
ELEM_TOL_OF = {("bernoulli", "dvar"): 1.4e-11}
JITTER = mo.JITTER
KCLASSES = ("gemm_f64", "potrf_base", "kmat", "trsv", "reduce", "other", "rff_features", "rff_contract")


def _gpf():
    import gpflowSlim as gpf
    return gpf


def _be():
    return _gpf()._backend


def _rbf_prog(variance, ls, dims=None):
    be = _be()
    ls = np.atleast_1d(np.asarray(ls, dtype=np.float64))
    dims = tuple(range(ls.size)) if dims is None else tuple(dims)
    return be.make_program([be.primitive_node(be.K_RBF, float(variance), dims=dims, lengthscales=tuple(float(v) for v in ls))])


def _orc_rbf(variance, ls):
    ls = np.asarray(ls, dtype=np.float64)
    return {"type": "rbf", "variance": float(variance), "lengthscales": ls, "input_dim": ls.size}


def _lik(kind, params):
    return _be().make_lik(lr.KIND_ID[kind], params, 20)


def _launches(handle):
    return sum(handle.profile_get(k)["launches"] for k in KCLASSES)


def _cd(make, x0, hrel=1e-6):
    h = hrel * max(1.0, abs(x0))
    return (make(x0 + h) - make(x0 - h)) / (2 * h)


def _fd_ok(got, fd, what):
    assert abs(got - fd) <= FD_TOL * max(1.0, abs(fd)), (what, got, fd)
    return abs(got - fd) / max(1.0, abs(fd))


def _con(by, p):
    """d / d(constrained value) from the model's gradient in the unconstrained one"""
    return np.atleast_1d(by[id(p)] / p.transform.forward_grad(p.vf_val))


# ---- 1. exact GPR: value and prediction -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [16, 17, 128, 129])
@pytest.mark.parametrize("kind", ["rbf_ard", "m52_plus_periodic"])
def test_gpr_value_and_prediction(handle, kind, r):
    """R = 16 is the last column count of the one-launch small-N path and 17 the first of the blocked one; 128 and 129 are the last
    with and the first without the augmented rows (gpr_plan of csrc/gps_gpr.hip)."""
    from test_gpu_parity import make_kernel, rel
    gpf = _gpf()
    n, d, ns = 200, 8, 9
    rng = np.random.default_rng(n + 17 * d + r)
    X = rng.standard_normal((n, d))
    Y = np.sin(X @ rng.standard_normal((d, r))) + 0.1 * rng.standard_normal((n, r))
    Xs = rng.standard_normal((ns, d))
    kern, spec = make_kernel(gpf, kind, d)
    m = gpf.models.GPR(X, Y, kern, obs_var=0.1)
    noise = orc.constrained(0.1)
    fallbacks = handle.profile_get("small_n_fallbacks")["launches"]
    handle.profile_reset()
    lml = m.compute_log_likelihood()
    launches = sum(handle.profile_get(k)["launches"] for k in KCLASSES[:6])
    ref = orc.gpr_lml(spec, X, Y, noise)
    print("gpr %s R=%d: lml rel %.3g, %d launches" % (kind, r, abs(lml - ref) / abs(ref), launches))
    assert abs(lml - ref) <= RTOL * abs(ref)
    if r == 16:         # the factorisation launch (+ kmat prep + kmat for programs it does not generate itself), and it did not give up
        assert launches <= 3, launches
        assert handle.profile_get("small_n_fallbacks")["launches"] == fallbacks
    else:
        assert launches > 3, launches
    mu, var = m.predict_f(Xs)
    rmu, rvar = orc.gpr_predict(spec, X, Y, noise, Xs)
    assert mu.shape == (ns, r) and var.shape == (ns, r)
    # column by column: a wrong column must not hide behind the largest one
    worst = max(max(rel(mu[:, q], rmu[:, q]), rel(var[:, q], rvar[:, q])) for q in range(r))
    print("gpr %s R=%d: worst column of predict_f %.3g" % (kind, r, worst))
    assert worst <= RTOL
    mu2, cov = m.predict_f_full_cov(Xs)
    _, rcov = orc.gpr_predict(spec, X, Y, noise, Xs, full_cov=True)
    assert cov.shape == (ns, ns, r)
    assert max(rel(mu2[:, q], rmu[:, q]) for q in range(r)) <= RTOL
    assert max(rel(cov[:, :, q], rcov[:, :, q] if rcov.ndim == 3 else rcov) for q in range(r)) <= RTOL


# ---- 2. SGPR: bound and every gradient entry against the long-double reference ---------------------------------------------------------
def _sgpr_got(handle, c, fitc=False):
    d = c["d"]
    prog = _rbf_prog(d["var"], d["ls"])
    bound, slots, gnoise, gmean, gZ = handle.sgpr_grad(prog, d["Z"], d["mu"], d["Y"], JITTER, d["noise"], fitc=fitc)
    return prog, bound, {"variance": slots[:1], "lengthscales": slots[1:], "noise": gnoise, "Z": gZ}, gmean


@pytest.mark.parametrize("shape", mo.SGPR_LD, ids=lambda s: "N%d_M%d_D%d_R%d" % s)
def test_sgpr_bound_and_gradient(handle, shape):
    c = mo.ld_case(*shape, True, None)
    d = c["d"]
    prog, bound, got, _ = _sgpr_got(handle, c)
    ref = orc.sgpr_bound(_orc_rbf(d["var"], d["ls"]), d["mu"], d["Y"], d["Z"], d["noise"])
    assert abs(ref - c["F"]) <= 1e-12 * abs(ref)                    # the two references are one function (S = 0)
    assert abs(bound - ref) <= RTOL * abs(ref), (bound, ref)
    value = handle.sgpr(prog, d["Z"], d["mu"], d["Y"], JITTER, d["noise"])[0]          # the value-only entry
    assert abs(value - bound) <= 1e-12 * abs(bound)
    fig = mo.check_ld(got, c)
    print("sgpr %s step %d: cond %.3g own %.3g ulp %.3g error / gate %s" % (shape, c["step"], c["kuu_cond"], max(c["own"][k] for k in c["names"]),
                                                                            max(c["ulp"][k] for k in c["names"]), {k: "%.3g" % v for k, v in fig.items()}))


def _linear_mean_model(cls, r, seed):
    """the model `cls` (SGPR or GPRFITC) on the inputs of the R-column SGPR case with a Linear mean function"""
    gpf = _gpf()
    d = mo.ld_inputs(129, 40, 8, r, True, 0)
    rng = np.random.default_rng(seed)
    X, Z, Y = d["mu"], d["Z"], d["Y"] + 0.3
    ls = np.asarray(d["ls"])
    kern = gpf.kernels.RBF(8, variance=d["var"], lengthscales=ls, ARD=True)
    theta = np.concatenate([[orc.constrained(d["var"])], orc.constrained(ls)])
    Am, bm = rng.standard_normal((8, r)) * 0.2, rng.standard_normal(r) * 0.1
    mf = gpf.mean_functions.Linear(Am.copy(), bm.copy())
    m = cls(X, Y, kern, Z=Z, obs_var=0.25, mean_function=mf)
    return m, mf, dict(X=X, Z=Z, Y=Y, theta=theta, A=Am, b=bm, noise=orc.constrained(0.25))


def test_sgpr_linear_mean_every_entry(handle):
    """R = 9 with mean_functions.Linear: every entry of b and of A by central differences of the oracle's bound (step and gate of
    tests/test_gpu_grad.py::test_sgpr_bound_gradient, which samples b[0] and three entries of A)."""
    gpf = _gpf()
    m, mf, P = _linear_mean_model(gpf.models.SGPR, 9, 5)

    def f(AA=P["A"], bb=P["b"]):
        return orc.sgpr_bound(_orc_rbf(P["theta"][0], P["theta"][1:]), P["X"], P["Y"], P["Z"], P["noise"], mean_X=P["X"] @ AA + bb)

    bound, grads = m.compute_log_likelihood_and_gradients()
    assert abs(bound - f()) <= RTOL * abs(f())
    by = {id(p): g for p, g in grads}
    gA, gb = np.reshape(by[id(mf.A)], P["A"].shape), np.ravel(by[id(mf.b)])
    worst = 0.0
    for q in range(9):
        def mkb(v, q=q):
            bb = P["b"].copy(); bb[q] = v
            return f(bb=bb)
        worst = max(worst, _fd_ok(gb[q], _cd(mkb, P["b"][q]), ("b", q)))
        for a in range(8):
            def mkA(v, a=a, q=q):
                AA = P["A"].copy(); AA[a, q] = v
                return f(AA=AA)
            worst = max(worst, _fd_ok(gA[a, q], _cd(mkA, P["A"][a, q]), ("A", a, q)))
    print("sgpr linear mean R=9: worst |g - fd| / max(1, |fd|) = %.3g" % worst)


# ---- 3. FITC ---------------------------------------------------------------------------------------------------------------------------
Z_ENTRIES = [(0, 0), (7, 1), (13, 2), (21, 3), (26, 4), (31, 5), (38, 6), (39, 7)]


@pytest.mark.parametrize("r", [5, 9, 17])
def test_fitc_value_and_gradient(handle, r):
    """value against orc.fitc_lml; gradient by central differences of the oracle in every kernel slot, the noise, 8 entries of Z
    and every entry of b of a Linear mean (step and gate of tests/test_gpu_grad.py::test_fitc_likelihood_gradient)"""
    gpf = _gpf()
    m, mf, P = _linear_mean_model(gpf.models.GPRFITC, r, 6 + r)

    def f(th=P["theta"], nz=P["noise"], ZZ=P["Z"], bb=P["b"]):
        return orc.fitc_lml(_orc_rbf(th[0], th[1:]), P["X"], P["Y"], ZZ, nz, mean_X=P["X"] @ P["A"] + bb)

    bound, grads = m.compute_log_likelihood_and_gradients()
    assert abs(bound - f()) <= RTOL * abs(f())
    by = {id(p): g for p, g in grads}
    got = np.concatenate([_con(by, p).ravel() for p in m.kern.parameters])
    assert got.shape == P["theta"].shape
    worst = 0.0
    for i in range(P["theta"].size):
        def mk(v, i=i):
            th = P["theta"].copy(); th[i] = v
            return f(th=th)
        worst = max(worst, _fd_ok(got[i], _cd(mk, P["theta"][i]), ("theta", i)))
    worst = max(worst, _fd_ok(float(_con(by, m.likelihood._variance)[0]), _cd(lambda v: f(nz=v), P["noise"]), "noise"))
    gz = by[id(m.feature._Z)]
    for a, b in Z_ENTRIES:
        def mk(v, a=a, b=b):
            ZZ = P["Z"].copy(); ZZ[a, b] = v
            return f(ZZ=ZZ)
        worst = max(worst, _fd_ok(gz[a, b], _cd(mk, P["Z"][a, b]), ("Z", a, b)))
    gb = np.ravel(by[id(mf.b)])
    for q in range(r):
        def mk(v, q=q):
            bb = P["b"].copy(); bb[q] = v
            return f(bb=bb)
        worst = max(worst, _fd_ok(gb[q], _cd(mk, P["b"][q]), ("b", q)))
    print("fitc R=%d: worst |g - fd| / max(1, |fd|) = %.3g" % (r, worst))


# ---- 4. SVGP, Gaussian likelihood --------------------------------------------------------------------------------------------------------
def _svgp_inputs(k, q_diag, n=129, m_=40, d=3):
    rng = np.random.default_rng(n + m_ + k)
    X = rng.standard_normal((n, d))
    Y = np.sin(X @ rng.standard_normal((d, k))) + 0.1 * rng.standard_normal((n, k))
    Z = X[:m_].copy()
    theta = np.concatenate([[1.3], np.linspace(0.8, 1.7, d)])
    q_mu = rng.standard_normal((m_, k)) * 0.3
    if q_diag:
        q_sqrt = np.abs(rng.standard_normal((m_, k))) * 0.4 + 0.2
    else:
        q_sqrt = np.tril(rng.standard_normal((k, m_, m_)) * (0.5 / m_) + np.eye(m_) * 0.5).transpose(1, 2, 0).copy()
    return X, Y, Z, theta, q_mu, q_sqrt


@pytest.mark.parametrize("q_diag", [False, True], ids=["full", "diag"])
@pytest.mark.parametrize("k", [5, 9, 17])
def test_svgp_gaussian_gradient(handle, k, q_diag):
    """whitened, against orc.svgp_elbo_grad with the gates of tests/test_gpu_grad.py::test_svgp_bound_gradient: 5e-6 on the kernel
    slots (the oracle's dK is a central difference), 1e-7 on the noise and on every entry of q_mu and q_sqrt"""
    X, Y, Z, theta, q_mu, q_sqrt = _svgp_inputs(k, q_diag)
    n, noise = X.shape[0], 0.3
    fn = lambda t: _orc_rbf(t[0], t[1:])
    res = handle.svgp_elbo_grad(_rbf_prog(theta[0], theta[1:]), Z, X, Y, q_mu, q_sqrt, JITTER, noise, white=True, scale=3.0)
    elbo, slots, gnoise, g_qmu, g_qs = res[:5]
    ref = orc.svgp_elbo(fn(theta), X, Y, Z, q_mu, q_sqrt, noise, whiten=True, num_data=3 * n)
    assert abs(elbo - ref) <= RTOL * abs(ref)
    g_ref, gn_ref, gq_ref, gs_ref, _ = orc.svgp_elbo_grad(fn, theta, X, Y, Z, q_mu, q_sqrt, noise, num_data=3 * n)
    assert slots.shape == g_ref.shape
    fig = {"slots": np.abs(slots - g_ref).max() / max(1.0, np.abs(g_ref).max()), "noise": abs(gnoise - gn_ref) / max(1.0, abs(gn_ref)),
           "q_mu": np.abs(g_qmu - gq_ref).max() / max(1.0, np.abs(gq_ref).max())}
    if q_diag:
        fig["q_sqrt"] = np.abs(g_qs - gs_ref).max() / max(1.0, np.abs(gs_ref).max())
    else:
        rows, cols = np.tril_indices(Z.shape[0], 0)
        fig["q_sqrt"] = np.abs(g_qs[rows, cols, :] - gs_ref[rows, cols, :]).max() / max(1.0, np.abs(gs_ref).max())
    print("svgp gaussian k=%d q_diag=%s: %s" % (k, q_diag, {a: "%.3g" % b for a, b in fig.items()}))
    assert g_qmu.shape == (Z.shape[0], k) and fig["slots"] <= 5e-6 and fig["noise"] <= 1e-7 and fig["q_mu"] <= 1e-7 and fig["q_sqrt"] <= 1e-7, fig
    # the last column on its own: a wrong column 8 or k - 1 must not hide behind a larger one
    assert np.abs(g_qmu[:, k - 1] - gq_ref[:, k - 1]).max() <= 1e-7 * max(1.0, np.abs(gq_ref[:, k - 1]).max())


def test_svgp_gaussian_unwhitened_gradient(handle):
    """k = 9, whiten=False, diagonal q_sqrt: central differences of the oracle's unwhitened bound (step and gate of
    tests/test_gpu_grad.py::test_svgp_bound_gradient_unwhitened) in every kernel slot, the noise and the entries of q_mu and
    q_sqrt of the latents 0, 7, 8 (the last one) at fixed rows"""
    k = 9
    X, Y, Z, theta, q_mu, q_sqrt = _svgp_inputs(k, True)
    n, noise = X.shape[0], 0.3
    Kuu = orc.K(_orc_rbf(theta[0], theta[1:]), Z) + JITTER * np.eye(Z.shape[0])
    q_mu = np.linalg.cholesky(Kuu) @ q_mu                           # a q(u) on the scale of the prior (tests/test_gpu_lik.py: _problem)
    q_sqrt = q_sqrt / np.sqrt(np.diag(np.linalg.inv(Kuu)))[:, None]

    def f(th=theta, nz=noise, qm=q_mu, qs=q_sqrt):
        return orc.svgp_elbo(_orc_rbf(th[0], th[1:]), X, Y, Z, qm, qs, nz, whiten=False, num_data=3 * n)

    elbo, slots, gnoise, g_qmu, g_qs = handle.svgp_elbo_grad(_rbf_prog(theta[0], theta[1:]), Z, X, Y, q_mu, q_sqrt, JITTER, noise,
                                                             white=False, scale=3.0)[:5]
    assert abs(elbo - f()) <= RTOL * abs(f())
    worst = 0.0
    for i in range(theta.size):
        def mk(v, i=i):
            th = theta.copy(); th[i] = v
            return f(th=th)
        worst = max(worst, _fd_ok(slots[i], _cd(mk, theta[i]), ("theta", i)))
    worst = max(worst, _fd_ok(gnoise, _cd(lambda v: f(nz=v), noise), "noise"))
    for a, q in [(3, 0), (11, 7), (17, 8), (39, 8)]:
        def mkm(v, a=a, q=q):
            qm = q_mu.copy(); qm[a, q] = v
            return f(qm=qm)
        worst = max(worst, _fd_ok(g_qmu[a, q], _cd(mkm, q_mu[a, q]), ("q_mu", a, q)))

        def mks(v, a=a, q=q):
            qs = q_sqrt.copy(); qs[a, q] = v
            return f(qs=qs)
        worst = max(worst, _fd_ok(g_qs[a, q], _cd(mks, q_sqrt[a, q]), ("q_sqrt", a, q)))
    print("svgp gaussian unwhitened k=9: worst |g - fd| / max(1, |fd|) = %.3g" % worst)


@pytest.mark.parametrize("k", [128, 129])
def test_svgp_gaussian_bound_at_128_and_129(handle, k):
    """the bound alone, diagonal q_sqrt.  gps_svgp_elbo has no cap: every buffer and launch of svgp_forward is sized by k (dAlpha
    [k][mp], dMean [n, k] + [n], dVar n (k + 1), dS1 [n, k] + 64, one varexp launch per latent), so 129 is a case like any other."""
    X, Y, Z, theta, q_mu, q_sqrt = _svgp_inputs(k, True)
    elbo, kl, ve = handle.svgp_elbo(_rbf_prog(theta[0], theta[1:]), Z, X, Y, q_mu, q_sqrt, JITTER, 0.3, white=True, scale=3.0)
    ref = orc.svgp_elbo(_orc_rbf(theta[0], theta[1:]), X, Y, Z, q_mu, q_sqrt, 0.3, whiten=True, num_data=3 * X.shape[0])
    rkl = orc.gauss_kl(q_mu, q_sqrt, None)
    print("svgp gaussian k=%d: elbo rel %.3g kl rel %.3g" % (k, abs(elbo - ref) / abs(ref), abs(kl - rkl) / abs(rkl)))
    assert abs(elbo - ref) <= RTOL * abs(ref) and abs(kl - rkl) <= RTOL * abs(rkl)


# ---- 5. SVGP with a likelihood, and the likelihood kernels alone ---------------------------------------------------------------------------
LIK_CASES = [("bernoulli", 9), ("student_t", 9), ("poisson", 17), ("multiclass", 17)]
Q_ROWS = (3, 11, 17, 29)


@pytest.mark.parametrize("q_diag", [False, True], ids=["full", "diag"])
@pytest.mark.parametrize("kind,k", LIK_CASES)
def test_svgp_lik_bound_and_gradient(handle, kind, k, q_diag):
    """_problem of tests/test_gpu_lik.py at n = 129, m = 30, whitened: the bound against ref.svgp_bound at solve_tol, the gradient as
    test_svgp_lik_gradient checks it, with the entries of q_mu and q_sqrt taken at the latents 0, 7, 8 and k - 1 (fixed)"""
    import test_gpu_lik as tl
    m, P = tl._problem(kind, k, True, q_diag, n=129, m_=30, mean=(kind == "student_t"), train_inducing=True)
    Kuu = orc.K(P["spec"](P["theta"]), P["Z"]) + orc.JITTER * np.eye(30)
    cond = float(np.linalg.cond(Kuu))
    assert cond <= mo.COND_CAP, cond
    tol = mo.solve_tol(Kuu)
    bound, grads = m.compute_log_likelihood_and_gradients()
    rb = tl._ref_bound(P)
    print("svgp %s k=%d q_diag=%s: bound rel %.3g (gate %.3g, cond %.3g)" % (kind, k, q_diag, abs(bound - rb) / abs(rb), tol, cond))
    assert abs(bound - rb) <= tol * abs(rb)
    assert abs(m.compute_log_likelihood() - rb) <= tol * abs(rb)
    by = {id(p): g for p, g in grads}
    worst = 0.0
    got = np.concatenate([_con(by, p).ravel() for p in m.kern.parameters])
    theta = P["theta"]
    for i in range(theta.size):
        def mk(v, i=i):
            th = theta.copy(); th[i] = v
            return tl._ref_bound(P, theta=th)
        worst = max(worst, _fd_ok(got[i], _cd(mk, theta[i]), ("theta", i)))
    if kind == "student_t":
        worst = max(worst, _fd_ok(float(_con(by, m.likelihood._scale)[0]), _cd(lambda v: tl._ref_bound(P, params=[v, 3.0]), P["params"][0]), "scale"))
        gc = _con(by, m.mean_function.c).ravel()
        for q in range(k):
            def mk(v, q=q):
                mx = P["mean_X"].copy(); mx[:, q] = v
                return tl._ref_bound(P, mean_X=mx)
            worst = max(worst, _fd_ok(gc[q], _cd(mk, 0.2), ("mean", q)))
    gq = by[id(m._q_mu)]
    rows, cols = np.tril_indices(30, 0)
    for a, q in zip(Q_ROWS, (0, 7, 8, k - 1)):
        def mk(v, a=a, q=q):
            qm = P["q_mu"].copy(); qm[a, q] = v
            return tl._ref_bound(P, q_mu=qm)
        worst = max(worst, _fd_ok(gq[a, q], _cd(mk, P["q_mu"][a, q]), ("q_mu", a, q)))
        if q_diag:
            gs = by[id(m._q_sqrt)] / m._q_sqrt.transform.forward_grad(m._q_sqrt.vf_val)

            def mk(v, a=a, q=q):
                qs = P["q_sqrt"].copy(); qs[a, q] = v
                return tl._ref_bound(P, q_sqrt=qs)
            worst = max(worst, _fd_ok(gs[a, q], _cd(mk, P["q_sqrt"][a, q]), ("q_sqrt", a, q)))
        else:
            b = a // 2                                               # one entry below the diagonal of L_q, row a
            t = int(np.flatnonzero((rows == a) & (cols == b))[0])

            def mk(v, a=a, b=b, q=q):
                qs = P["q_sqrt"].copy(); qs[a, b, q] = v
                return tl._ref_bound(P, q_sqrt=qs)
            worst = max(worst, _fd_ok(by[id(m._q_sqrt)].reshape(k, -1)[q, t], _cd(mk, P["q_sqrt"][a, b, q]), ("q_sqrt", a, b, q)))
    gZ = by[id(m.feature._Z)]
    for a, j in [(0, 0), (9, 1), (22, 0), (29, 1)]:
        def mk(v, a=a, j=j):
            Z = P["Z"].copy(); Z[a, j] = v
            return tl._ref_bound(P, Z=Z)
        worst = max(worst, _fd_ok(gZ[a, j], _cd(mk, P["Z"][a, j]), ("Z", a, j)))
    print("svgp %s k=%d q_diag=%s: worst |g - fd| / max(1, |fd|) = %.3g" % (kind, k, q_diag, worst))


def test_svgp_lik_bound_at_128(handle):
    import test_gpu_lik as tl
    m, P = tl._problem("poisson", 128, True, True, n=129, m_=30)
    Kuu = orc.K(P["spec"](P["theta"]), P["Z"]) + orc.JITTER * np.eye(30)
    assert float(np.linalg.cond(Kuu)) <= mo.COND_CAP
    bound, rb = m.compute_log_likelihood(), tl._ref_bound(P)
    assert abs(bound - rb) <= mo.solve_tol(Kuu) * abs(rb), (bound, rb)


VAREXP_CASES = [(kind, k) for kind in ("bernoulli", "poisson", "exponential", "student_t", "multiclass", "gaussian") for k in (9, 17, 128)
                if not (kind == "multiclass" and k == 9)]              # MultiClass takes 17 and 128 classes


@pytest.mark.parametrize("kind,k", VAREXP_CASES)
def test_lik_varexp_entry_by_entry(handle, kind, k):
    """gps_lik_varexp alone at n = 70 (lik_rowsq_kernel: 8 latents per workgroup row, the second grid axis): the sum, dmu, dvar and
    the parameter derivative against tests/_lik_ref.py, gates of tests/test_gpu_lik.py"""
    rng = np.random.default_rng(3000 + k + len(kind))
    mu, var, Y, params = lr.sample_inputs(kind, 70, k, rng, var_lo=1e-6, var_hi=10.0)
    lik = _lik(kind, params)
    rve, rdmu, rdvar, rdpar = lr.varexp_grad(kind, params, mu, var, Y)
    ve, dmu, dvar, dpar = handle.lik_varexp(lik, mu, var, Y, want_grad=True)
    assert ve == handle.lik_varexp(lik, mu, var, Y)
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))
    fig = {"sum": abs(ve - float(np.sum(rve))) / max(1.0, float(np.sum(np.abs(rve)))), "dmu": rel(dmu, rdmu), "dvar": rel(dvar, rdvar),
           "dpar": abs(dpar - rdpar) / max(1.0, abs(rdpar))}
    print("lik_varexp %s k=%d: %s" % (kind, k, {a: "%.3g" % b for a, b in fig.items()}))
    for name, v in fig.items():
        assert v <= ELEM_TOL_OF.get((kind, name), ELEM_TOL), (kind, k, name, v)


@pytest.mark.parametrize("k", [9, 17, 128])
@pytest.mark.parametrize("kind", gr.KINDS)
def test_lik_logp_entry_by_entry(handle, kind, k):
    rng = np.random.default_rng(4000 + k + len(kind))
    F, _, Y, params = lr.sample_inputs(kind, 70, k, rng)
    lik = _lik(kind, params)
    rlp = lr.logp(kind, params, F, Y)
    rG, rdpar = gr.dlogp(kind, params, F, Y)
    lp, G, dpar = handle.lik_logp(lik, F, Y, want_grad=True)
    assert lp == handle.lik_logp(lik, F, Y)
    fig = {"sum": abs(lp - float(np.sum(rlp))) / max(1.0, abs(float(np.sum(rlp)))),
           "G": float(np.max(np.abs(G - rG) / np.maximum(1.0, np.abs(rG)))), "dpar": abs(dpar - rdpar) / max(1.0, abs(rdpar))}
    print("lik_logp %s k=%d: %s" % (kind, k, {a: "%.3g" % b for a, b in fig.items()}))
    for name, v in fig.items():
        assert v <= ELEM_TOL, (kind, k, name, v)


# ---- 6. GPMC ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gpmc_ref(kind, n, r):
    X, V, Y, params, mean = gr.make_case(kind, n, r)
    res = gr.grad(gr.rbf_spec(), X, V, Y, kind, params, mean, jitter=JITTER)
    res.update(X=X, V=V, Y=Y, params=params, mean=mean, tol=mo.solve_tol(res["K"]), cond=float(np.linalg.cond(res["K"])))
    return res


@pytest.mark.parametrize("kind", ["poisson", "student_t"])
@pytest.mark.parametrize("r", [17, 128])
def test_gpmc_lik_grad(handle, kind, r):
    """(N, R) = (129, 17) and (129, 128): one group of 16 columns plus one column, and eight groups, through tri_skinny and
    chol_seed inside gps_gpmc_lik_grad; gates of tests/test_gpu_gpmc.py"""
    c = _gpmc_ref(kind, 129, r)
    lik = _lik(kind, c["params"])
    prog = _rbf_prog(1.3, (0.5, 0.7))
    ll = handle.gpmc_lik(prog, c["X"], c["V"], c["Y"], JITTER, lik, mean=c["mean"])
    ll2, slots, glik, gV, gmean = handle.gpmc_lik_grad(prog, c["X"], c["V"], c["Y"], JITTER, lik, mean=c["mean"])
    assert ll == ll2
    got = dict(loglik=ll, slots=slots, glik=glik, gV=gV, gmean=gmean)
    fig = mo.check_solve(got, c, c["tol"], ("loglik", "slots", "glik", "gV", "gmean"), cond=c["cond"])
    print("gpmc %s R=%d: cond %.3g tol %.3g %s" % (kind, r, c["cond"], c["tol"], {a: "%.3g" % b for a, b in fig.items()}))
    again = handle.gpmc_lik_grad(prog, c["X"], c["V"], c["Y"], JITTER, lik, mean=c["mean"])
    assert again[0] == ll2 and np.array_equal(again[1], slots) and again[2] == glik and np.array_equal(again[3], gV)


# ---- 7. SGPMC --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", mo.SGPMC_KINDS)
@pytest.mark.parametrize("size", mo.SGPMC_SIZES, ids=lambda s: "M%d_N%d_R%d" % s)
def test_sgpmc_lik_and_grad(handle, size, kind):
    """R = 5 (skinny_xt_kernel<16> with a remainder of the 4-template), 16 (the template filled), 17 (16 + 1) and 128 (eight groups),
    chunk_rows 0 and 128, with everything tests/test_gpu_sgpmc.py::test_sgpmc_lik_and_grad asserts of one chunking"""
    m, n, r = size
    c = mo.sgpmc_case(kind, m, n, r)
    lik = _lik(kind, c["params"])
    prog = _rbf_prog(mo.SGPMC_KERN["variance"], mo.SGPMC_KERN["lengthscales"])
    args = (prog, c["Z"], c["X"], c["Y"], c["V"], JITTER, lik)
    for chunk in (0, 128):
        res = handle.sgpmc_lik_grad(*args, mean=c["mean"], chunk_rows=chunk, want_grad_Z=True)
        fig = mo.check_solve(dict(zip(mo.SGPMC_OUT, res)), c, c["tol"], mo.SGPMC_OUT, cond=c["cond"])
        print("sgpmc %s %s chunk %d: cond %.3g tol %.3g %s" % (kind, size, chunk, c["cond"], c["tol"], {a: "%.3g" % b for a, b in fig.items()}))
        # column by column: every column of grad_V and of d / d mean within the gate of its own size
        for name, i in (("gV", 3), ("gmean", 4)):
            for q in range(r):
                err = np.abs(res[i][:, q] - c[name][:, q]).max() / mo.scale(c[name][:, q])
                assert err <= c["tol"], (kind, size, chunk, name, q, err)
        assert handle.sgpmc_lik(*args, mean=c["mean"], chunk_rows=chunk) == res[0]
        again = handle.sgpmc_lik_grad(*args, mean=c["mean"], chunk_rows=chunk, want_grad_Z=True)
        assert again[0] == res[0] and again[2] == res[2] and all(np.array_equal(again[i], res[i]) for i in (1, 3, 4, 5))


# ---- 8. Bayesian GPLVM ---------------------------------------------------------------------------------------------------------------------
def _bgplvm_check(handle, c, prog, what):
    d = c["d"]
    bound, slots, gnoise, gZ, gmu, gS = handle.bgplvm_grad(prog, d["Z"], d["mu"], d["S"], d["Y"], JITTER, d["noise"])
    assert abs(bound - c["F"]) <= RTOL * abs(c["F"]), (bound, c["F"])
    value = handle.bgplvm(prog, d["Z"], d["mu"], d["S"], d["Y"], JITTER, d["noise"])[0]   # the value-only entry
    assert abs(value - bound) <= 1e-12 * abs(bound)
    if c["parts"] is None:
        got = {"variance": slots[:1], "lengthscales": slots[1:]}
    else:                                                            # (variance, lengthscales) part by part
        sizes = [len(p) for p in c["parts"]]
        offs = np.cumsum([0] + [1 + s for s in sizes])
        got = {"variance": np.array([slots[o] for o in offs[:-1]]),
               "lengthscales": np.concatenate([slots[o + 1:o + 1 + s] for o, s in zip(offs[:-1], sizes)])}
    got.update(noise=gnoise, Z=gZ, X_mean=gmu, X_var=gS)
    fig = mo.check_ld(got, c)
    print("bgplvm %s step %d: cond %.3g own %.3g ulp %.3g error / gate %s" % (what, c["step"], c["kuu_cond"], max(c["own"].values()),
                                                                              max(c["ulp"].values()), {k: "%.3g" % v for k, v in fig.items()}))


@pytest.mark.parametrize("shape", mo.BGPLVM_LD, ids=lambda s: "N%d_M%d_Q%d_R%d" % s)
def test_bgplvm_bound_and_gradient(handle, shape):
    """R = 4 (one full group of psi1_kernel<true>), 5 (a full group and a remainder), 128; Q = 9, 16 and 32 take the QT = 16 and
    QT = 32 instantiations of the four VJP kernels, M = 60 the B = 4 pair tile and M = 9 the B = 2 one"""
    c = mo.ld_case(*shape, False, None)
    d = c["d"]
    assert abs(pr.bound_ld(d["var"], d["ls"], d["noise"], d["Z"], d["mu"], d["S"], d["Y"])[0] - c["F"]) <= 1e-12 * abs(c["F"])
    _bgplvm_check(handle, c, _rbf_prog(d["var"], d["ls"]), shape)


def test_bgplvm_model_gradient_includes_the_kl_part(handle):
    """(65, 60, 9, 5) through models.BayesianGPLVM as _check_grads of tests/test_gpu_gplvm.py does: the gradient in X_mean and
    X_var with the KL term, chained to the unconstrained values, entry by entry at the gate of the long-double case"""
    gpf = _gpf()
    c = mo.ld_case(65, 60, 9, 5, False, None)
    d = c["d"]
    kern = gpf.ekernels.RBF(9, variance=d["var"], lengthscales=d["ls"], ARD=True)
    m = gpf.models.BayesianGPLVM(d["mu"], d["S"], d["Y"], kern, 60, Z=d["Z"], obs_var=d["noise"])
    kl = pr.kl(d["mu"], d["S"])
    assert abs(m.compute_log_likelihood() - (c["F"] - kl)) <= RTOL * abs(c["F"] - kl)
    _, grads = m.compute_log_likelihood_and_gradients()
    by = {id(p): g for p, g in grads}
    kl_mu, kl_S = pr.kl_grad(d["mu"], d["S"])
    got = {"variance": _con(by, m.kern._variance), "lengthscales": _con(by, m.kern._ls), "noise": _con(by, m.likelihood._variance),
           "Z": np.asarray(by[id(m._Z)]), "X_mean": np.asarray(by[id(m._X_mean)]) + kl_mu,
           "X_var": by[id(m._X_var)] / m._X_var.transform.forward_grad(m._X_var.vf_val) + kl_S}
    fig = mo.check_ld(got, c)
    print("bgplvm model: error / gate %s" % {k: "%.3g" % v for k, v in fig.items()})


def test_bgplvm_sum_of_rbf_gradient(handle):
    """two RBF parts of 6 latent dimensions each at (65, 60, 12, 5), against tests/_psi_sum_ref.py under the same admission rule"""
    be = _be()
    N, M, Q, R = mo.SUM_LD
    c = mo.ld_case(N, M, Q, R, False, mo.SUM_PARTS)
    nodes = []
    for i, p in enumerate(mo.sum_parts(c["d"], mo.SUM_PARTS)):
        nodes.append(be.primitive_node(be.K_RBF, float(p["var"]), dims=tuple(p["dims"]), lengthscales=tuple(float(v) for v in p["ls"])))
        if i:
            nodes.append(be.op_node(be.K_ADD))
    _bgplvm_check(handle, c, be.make_program(nodes), "sum " + str(mo.SUM_LD))


# ---- 9. at 129 ---------------------------------------------------------------------------------------------------------------------------
def test_capped_entry_points_refuse_129(handle):
    """every entry point with a cap raises with its "at most 128" message before any launch, and the handle works afterwards"""
    c = mo.ld_case(129, 40, 8, 9, True, None)
    d = c["d"]
    n, m_ = 129, 40
    prog = _rbf_prog(d["var"], d["ls"])
    Y = np.ones((n, 129))
    q_mu, q_diag = np.zeros((m_, 129)), np.ones((m_, 129))
    lik = _lik("poisson", [0.7])
    calls = {
        "gps_sgpr_grad": lambda: handle.sgpr_grad(prog, d["Z"], d["mu"], Y, JITTER, 0.3),
        "gps_fitc_grad": lambda: handle.sgpr_grad(prog, d["Z"], d["mu"], Y, JITTER, 0.3, fitc=True),
        "gps_svgp_elbo_grad": lambda: handle.svgp_elbo_grad(prog, d["Z"], d["mu"], Y, q_mu, q_diag, JITTER, 0.3),
        "gps_svgp_elbo_lik": lambda: handle.svgp_elbo_lik(prog, d["Z"], d["mu"], Y, q_mu, q_diag, JITTER, lik),
        "gps_svgp_elbo_lik_grad": lambda: handle.svgp_elbo_lik_grad(prog, d["Z"], d["mu"], Y, q_mu, q_diag, JITTER, lik),
        "gps_bgplvm": lambda: handle.bgplvm(prog, d["Z"], d["mu"], np.full((n, 8), 0.1), Y, JITTER, 0.3),
        "gps_bgplvm_grad": lambda: handle.bgplvm_grad(prog, d["Z"], d["mu"], np.full((n, 8), 0.1), Y, JITTER, 0.3),
        "gps_lik_varexp": lambda: handle.lik_varexp(lik, np.zeros((n, 129)), np.ones((n, 129)), Y),
        "gps_lik_logp": lambda: handle.lik_logp(lik, np.zeros((n, 129)), Y),
        "gps_gpmc_lik": lambda: handle.gpmc_lik(prog, d["mu"], np.zeros((n, 129)), Y, JITTER, lik),
        "gps_gpmc_lik_grad": lambda: handle.gpmc_lik_grad(prog, d["mu"], np.zeros((n, 129)), Y, JITTER, lik),
    }
    before = _launches(handle)
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match=name + ": at most 128 (outputs|latent functions)"):
            call()
    assert _launches(handle) == before
    bound = handle.sgpr_grad(prog, d["Z"], d["mu"], d["Y"], JITTER, d["noise"])[0]           # the handle is usable afterwards
    assert abs(bound - c["F"]) <= RTOL * abs(c["F"])


def _case_129(m_=40):
    rng = np.random.default_rng(129 + m_)
    n, d, r = 129, 8, 129
    X, Z = rng.standard_normal((n, d)), rng.standard_normal((m_, d))
    ls = rng.uniform(0.7, 2.0, d) * np.sqrt(d)
    Y = np.sin(X @ rng.standard_normal((d, r)) / np.sqrt(d)) + 0.1 * rng.standard_normal((n, r))
    return X, Z, Y, 1.7, ls


@pytest.mark.parametrize("fitc", [False, True], ids=["sgpr", "fitc"])
def test_sgpr_and_fitc_values_at_129(handle, fitc):
    """gps_sgpr / gps_fitc have no cap and need none: sparse_gpr_impl sizes everything by r (dAlpha 2 r max(np, mp), dTmp2 n r, dMean
    mp r + mp + n_new r + 2 n_new; rowdot_kernel, lml_reduce_kernel and the transposes loop over r; the substitutions take the
    right-hand sides two and four at a time with a remainder), and dG3 at (GPS_TILE + r) mp belongs to the gradients, which are
    capped.  So R = 129 is a case like any other: bound and prediction against the oracle, column by column."""
    X, Z, Y, var, ls = _case_129()
    spec = _orc_rbf(var, ls)
    Xs = np.random.default_rng(2).standard_normal((9, 8))
    bound, mu, v = handle.sgpr(_rbf_prog(var, ls), Z, X, Y, JITTER, 0.3, Xnew=Xs, fitc=fitc)
    Kuu = orc.K(spec, Z) + JITTER * np.eye(len(Z))
    assert np.linalg.cond(Kuu) <= 1e6                               # (8 dimensions: solve_tol is its floor, 1e-8)
    ref = (orc.fitc_lml if fitc else orc.sgpr_bound)(spec, X, Y, Z, 0.3)
    rmu, rv = (orc.fitc_predict if fitc else orc.sgpr_predict)(spec, X, Y, Z, 0.3, Xs)
    assert abs(bound - ref) <= RTOL * abs(ref), (bound, ref)
    assert mu.shape == (9, 129) and v.shape == (9,)                 # (the C entry returns the variance once: it is the same for every column)
    worst = max(np.abs(mu[:, q] - rmu[:, q]).max() / np.abs(rmu[:, q]).max() for q in range(129))
    print("%s R=129: bound rel %.3g, worst column of the mean %.3g" % ("fitc" if fitc else "sgpr", abs(bound - ref) / abs(ref), worst))
    assert worst <= RTOL and np.abs(v[:, None] - rv).max() <= RTOL * np.abs(rv).max()


@pytest.mark.parametrize("q", [None, 2, 3])
def test_conditional_at_129(handle, q):
    """gps_conditional has no cap and needs none: cond_solve / cond_mean / cond_base_var / cond_qsqrt_terms size dAlpha [k][mp], dTmp2
    max(n^2, m k), dMean n k + n and dVar n (k + 1) by k and take the q_sqrt terms latent by latent"""
    X, Z, Y, var, ls = _case_129()
    rng = np.random.default_rng(4)
    f = rng.standard_normal((40, 129)) * 0.3
    q_sqrt = None
    if q == 2:
        q_sqrt = np.abs(rng.standard_normal((40, 129))) * 0.4 + 0.2
    elif q == 3:
        q_sqrt = np.tril(rng.standard_normal((129, 40, 40)) * (0.5 / 40) + np.eye(40) * 0.5).transpose(1, 2, 0).copy()
    Xs = X[:17]
    fm, fv = handle.conditional(_rbf_prog(var, ls), Z, Xs, f, JITTER, q_sqrt=q_sqrt, white=True)
    rfm, rfv = orc.conditional(Xs, Z, _orc_rbf(var, ls), f, q_sqrt=q_sqrt, white=True)
    assert fm.shape == (17, 129) and fv.shape == (17, 129)
    worst = max(np.abs(fm[:, j] - rfm[:, j]).max() / max(1.0, np.abs(rfm[:, j]).max()) for j in range(129))
    assert worst <= RTOL and np.abs(fv - rfv).max() <= RTOL * max(1.0, np.abs(rfv).max()), (worst, np.abs(fv - rfv).max())


@pytest.mark.parametrize("q", [2, 3])
def test_gauss_kl_at_129_latents_and_128_inducing_points(handle, q):
    """gps_gauss_kl has no cap.  With a prior covariance it stages q_mu [m, k] in dTmp2, which was sized [mp, mp] for the L_q^T that
    follows: at m = 128 and k = 129, m k = 16512 > mp mp = 16384 doubles.  The buffer now takes the larger of the two, and this
    is that shape, against the oracle."""
    rng = np.random.default_rng(11)
    m_, k = 128, 129
    Z = rng.standard_normal((m_, 8))
    K = orc.K(_orc_rbf(1.7, np.full(8, 3.0)), Z) + JITTER * np.eye(m_)
    assert np.linalg.cond(K) <= 1e6
    q_mu = rng.standard_normal((m_, k)) * 0.3
    if q == 2:
        q_sqrt = np.abs(rng.standard_normal((m_, k))) * 0.4 + 0.2
    else:
        q_sqrt = np.tril(rng.standard_normal((k, m_, m_)) * (0.5 / m_) + np.eye(m_) * 0.5).transpose(1, 2, 0).copy()
    for Kp in (K, None):
        got, ref = handle.gauss_kl(q_mu, q_sqrt, Kp), orc.gauss_kl(q_mu, q_sqrt, Kp)
        assert abs(got - ref) <= RTOL * abs(ref), (q, Kp is None, got, ref)
