"""features.Multiscale on the device (csrc/multiscale.hip) against tests/_multiscale_ref.py: the entries of Kuu and Kuf, their
vector-Jacobian products, the models that take the feature (features.conditional, SVGP, SGPR, GPRFITC: bounds, predictions, every
gradient block), the one-shot state of the handle, the refusals at the C ABI, and a short training run."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _multiscale_ref as mr  # noqa: E402
import oracle.gp_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu
LD = np.longdouble
EPS = np.finfo(np.float64).eps
JIT = 1e-6

# (M, N, D, ard, d_all, dims, ls_factor)
ENTRY_CASES = {
    "one_point": (1, 1, 1, True, None, None, 1.0),
    "small_isotropic": (5, 7, 3, False, None, None, 1.0),
    "two_blocks_ard": (130, 129, 5, True, None, None, 1.0),
    "max_dims": (37, 33, 32, True, None, None, 1.0),
    "unordered_subset": (20, 300, 3, True, 6, [4, 0, 2], 1.0),
    "short_lengthscales": (130, 129, 5, True, None, None, 0.25),
}
VJP_CASES = dict(ENTRY_CASES, chunk_edge=(5, 129, 3, True, None, None, 1.0))


def _setup(case, table=ENTRY_CASES):
    """(kern, feat, X, the parameter values as the objects hold them)"""
    import gpflowSlim as gpf
    M, N, D, ard, d_all, dims, f = table[case]
    d = mr.inputs(M, N, D, seed=sorted(table).index(case), d_all=d_all, dims=dims, ls_factor=f, ard=ard)
    kern = gpf.kernels.RBF(D, variance=d["variance"], lengthscales=d["lengthscales"] if ard else float(d["lengthscales"][0]),
                           ARD=ard, active_dims=dims)
    feat = gpf.features.Multiscale(d["Z"], d["scales"])
    vals = dict(variance=float(np.squeeze(kern.variance)), lengthscales=np.atleast_1d(kern.lengthscales).astype(np.float64),
                Z=np.asarray(feat.Z), scales=np.asarray(feat.scales), X=d["X"], dims=dims)
    return kern, feat, d["X"], vals


# ---- 1. entries -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(ENTRY_CASES))
def test_entries_of_kuu_and_kuf(handle, case):
    """Entry by entry in relative error against the long-double evaluation: max(8 spread, 64 eps), the project's rule for
    kernel-matrix entries (the reference's own spread is at most 4e-14 on these cases; the smallest entry of
    short_lengthscales is 7e-84)."""
    kern, feat, X, v = _setup(case)
    ref = mr.matrices_with_spread(v["variance"], v["lengthscales"], v["Z"], v["scales"], X, v["dims"], JIT)
    Kuu, Kuf = feat.Kuu(kern, jitter=JIT), feat.Kuf(kern, X)
    M, N = len(v["Z"]), len(X)
    assert Kuu.shape == (M, M) and Kuf.shape == (M, N)
    for name, got in (("kuu", Kuu), ("kuf", Kuf)):
        tol = max(8 * ref[name + "_spread"], 64 * EPS)
        err = np.abs(got - ref[name]) / np.abs(ref[name])
        print(case, name, "spread %.2e tol %.2e err %.2e min entry %.2e" % (ref[name + "_spread"], tol, err.max(), np.abs(ref[name]).min()))
        assert tol <= 1e-12
        assert np.all(ref[name] > 0) and err.max() <= tol
    assert np.array_equal(Kuu, Kuu.T)
    K0 = feat.Kuu(kern, jitter=0.0)
    off = ~np.eye(M, dtype=bool)
    assert np.array_equal(K0[off], Kuu[off])
    assert np.abs((np.diag(Kuu) - np.diag(K0)) / JIT - 1).max() <= 1e-9          # (jitter added to O(1) values: 1e-16 / 1e-6)
    assert np.array_equal(feat.Kuu(kern, jitter=JIT), Kuu) and np.array_equal(feat.Kuf(kern, X), Kuf)


# ---- 2. VJPs -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(VJP_CASES))
def test_vjps_with_random_cotangents(handle, case):
    """Against the analytic VJPs in long double, relative to the sum of the absolute values of each output's terms: max(8 spread,
    64 eps) with the spread of the reference itself, capped at 1e-11."""
    from gpflowSlim import _backend as be
    kern, feat, X, v = _setup(case, VJP_CASES)
    M, N = len(v["Z"]), len(X)
    if case == "chunk_edge":
        chunk, nchunks = be.ms_chunking(N, M)
        assert N == 2 * chunk + 1 and nchunks == 3
    prog = kern._program(v["Z"].shape[1])
    rng = np.random.RandomState(7)
    for which in ("kuf", "kuu"):
        W = rng.randn(M, N if which == "kuf" else M)
        if which == "kuf":
            ref, scale, spread = mr.vjp_with_spread(mr.kuf_vjp, W, v["variance"], v["lengthscales"], v["Z"], v["scales"], X, v["dims"])
        else:
            ref, scale, spread = mr.vjp_with_spread(mr.kuu_vjp, W, v["variance"], v["lengthscales"], v["Z"], v["scales"], v["dims"])
        tol = max(8 * spread, 64 * EPS)
        assert tol <= 1e-11
        slots, gZ, gS = handle._ms_kmat_vjp(prog, v["Z"], v["scales"], W, X2=X if which == "kuf" else None)
        again = handle._ms_kmat_vjp(prog, v["Z"], v["scales"], W, X2=X if which == "kuf" else None)
        assert all(np.array_equal(a, b) for a, b in zip((slots, gZ, gS), again))
        nd = len(v["dims"]) if v["dims"] is not None else v["Z"].shape[1]      # (one slot per active dim, isotropic or not)
        assert slots.shape == (1 + nd,)
        got = {"variance": slots[0], "lengthscales": slots[1:], "Z": gZ, "scales": gS}
        for k in ("variance", "lengthscales", "Z", "scales"):
            err = np.abs(np.asarray(got[k]) - ref[k])
            act = np.asarray(scale[k]) > 0
            worst = float(np.max(err[act] / np.asarray(scale[k])[act])) if np.any(act) else 0.0
            print(case, which, k, "spread %.2e tol %.2e err %.2e" % (spread, tol, worst))
            assert worst <= tol, (which, k)
            assert np.all(np.asarray(got[k])[~act] == 0.0)             # (columns outside the active dims: exact zeros)
        if v["dims"] is not None:
            other = [j for j in range(v["Z"].shape[1]) if j not in v["dims"]]
            assert np.all(gZ[:, other] == 0.0) and np.all(gS[:, other] == 0.0)


# ---- 3. models -------------------------------------------------------------------------------------------------------------------------
SHAPES = {"n300_m37": (300, 37, 5), "n129_m130": (129, 130, 5)}


def _model_inputs(shape, R, seed=0):
    N, M, D = SHAPES[shape]
    d = mr.inputs(M, N, D, seed=50 + seed)
    rng = np.random.RandomState(90 + seed)
    Wt = rng.randn(D, R)
    F = np.sin(d["X"] @ Wt)
    d["Y"] = F + 0.1 * rng.randn(N, R)
    d["Yb"] = (F + 0.3 * rng.randn(N, R) > 0).astype(np.float64)
    d["Xs"] = rng.randn(23, D)
    d["q_mu"] = 0.3 * rng.randn(M, R)
    d["q_diag"] = 0.2 + 0.4 * np.abs(rng.randn(M, R))
    d["q_full"] = np.tril(rng.randn(R, M, M) * (0.5 / M) + 0.5 * np.eye(M)).transpose(1, 2, 0).copy()
    return d


def _kern_feat(d):
    import gpflowSlim as gpf
    kern = gpf.kernels.RBF(len(d["lengthscales"]), variance=d["variance"], lengthscales=d["lengthscales"], ARD=True)
    feat = gpf.features.Multiscale(d["Z"], d["scales"])
    return kern, feat


def _held(kern, feat, d, **more):
    """the parameter values as the objects hold them (the transforms round)"""
    p = dict(variance=float(np.squeeze(kern.variance)), lengthscales=np.atleast_1d(kern.lengthscales).astype(np.float64),
             Z=np.asarray(feat.Z), scales=np.asarray(feat.scales), X=d["X"], jitter=JIT, dims=None)
    p.update(more)
    return p


def _close(a, b, tol=1e-8):
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max())


@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("q", ["none", "diag", "full"])
@pytest.mark.parametrize("full_cov", [False, True])
@pytest.mark.parametrize("shape,R", [("n300_m37", 1), ("n129_m130", 3)])
def test_conditional(handle, shape, R, full_cov, q, white):
    """features.conditional against the reference's base_conditional on the reference's Kuu and Kuf, 1e-8 relative."""
    import gpflowSlim as gpf
    d = _model_inputs(shape, R)
    kern, feat = _kern_feat(d)
    p = _held(kern, feat, d)
    Xs = d["Xs"]
    Kmm = np.asarray(mr.kuu(p["variance"], p["lengthscales"], p["Z"], p["scales"], None, JIT, LD), dtype=np.float64)
    Kmn = np.asarray(mr.kuf(p["variance"], p["lengthscales"], p["Z"], p["scales"], Xs, None, LD), dtype=np.float64)
    Knn = mr.rbf(p["variance"], p["lengthscales"], Xs) if full_cov else np.full(len(Xs), p["variance"])
    q_sqrt = {"none": None, "diag": d["q_diag"], "full": d["q_full"]}[q]
    mu, var = gpf.features.conditional(feat, kern, Xs, d["q_mu"], full_cov=full_cov, q_sqrt=q_sqrt, white=white)
    rmu, rvar = orc.base_conditional(Kmn, Kmm, Knn, d["q_mu"], full_cov=full_cov, q_sqrt=q_sqrt, white=white)
    assert mu.shape == rmu.shape and var.shape == rvar.shape
    assert _close(mu, rmu) and _close(var, rvar)


def _svgp(d, lik, white, q, R):
    import gpflowSlim as gpf
    kern, feat = _kern_feat(d)
    like = gpf.likelihoods.Gaussian(0.3) if lik == "gaussian" else gpf.likelihoods.Bernoulli()
    Y = d["Y"] if lik == "gaussian" else d["Yb"]
    m = gpf.models.SVGP(d["X"], Y, kern, like, feat=feat, q_diag=(q == "diag"), whiten=white, train_inducing=True)
    m._q_mu.assign(d["q_mu"])
    m._q_sqrt.assign(d["q_diag"] if q == "diag" else d["q_full"])
    p = _held(kern, feat, d, Y=Y, q_mu=d["q_mu"], q_sqrt=np.asarray(m.q_sqrt), white=white, lik=lik)
    if lik == "gaussian":
        p["noise"] = float(np.squeeze(like.variance))
    return m, p


@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("lik", ["gaussian", "bernoulli"])
@pytest.mark.parametrize("shape,R,q", [("n300_m37", 1, "diag"), ("n300_m37", 3, "full"), ("n129_m130", 3, "diag"), ("n129_m130", 1, "full")])
def test_svgp_bound_and_predict(handle, shape, R, q, lik, white):
    d = _model_inputs(shape, R)
    m, p = _svgp(d, lik, white, q, R)
    ref = float(mr.model_bound("svgp", p, np.float64))
    got = m.compute_log_likelihood()
    assert abs(got - ref) <= 1e-8 * abs(ref), (got, ref)
    Kmm = mr.kuu(p["variance"], p["lengthscales"], p["Z"], p["scales"], None, JIT)
    Kmn = mr.kuf(p["variance"], p["lengthscales"], p["Z"], p["scales"], d["Xs"])
    rmu, rvar = orc.base_conditional(Kmn, Kmm, np.full(len(d["Xs"]), p["variance"]), p["q_mu"], q_sqrt=p["q_sqrt"], white=white)
    mu, var = m.predict_f(d["Xs"])
    assert _close(mu, rmu) and _close(var, rvar)


@pytest.mark.parametrize("kind", ["sgpr", "fitc"])
@pytest.mark.parametrize("shape,R", [("n300_m37", 1), ("n300_m37", 3), ("n129_m130", 1), ("n129_m130", 3)])
def test_collapsed_bounds_and_predict(handle, shape, R, kind):
    import gpflowSlim as gpf
    d = _model_inputs(shape, R)
    kern, feat = _kern_feat(d)
    m = (gpf.models.SGPR if kind == "sgpr" else gpf.models.GPRFITC)(d["X"], d["Y"], kern, feat=feat, obs_var=0.3)
    p = _held(kern, feat, d, Y=d["Y"], noise=float(np.squeeze(m.likelihood.variance)))
    ref = float(mr.model_bound(kind, p, np.float64))
    got = m.compute_log_likelihood()
    assert abs(got - ref) <= 1e-8 * abs(ref), (got, ref)
    if kind == "sgpr":
        Kj = mr.kuu(p["variance"], p["lengthscales"], p["Z"], p["scales"], None, JIT)
        rmu, rvar = mr.sgpr_predict(Kj, mr.kuf(p["variance"], p["lengthscales"], p["Z"], p["scales"], d["X"]),
                                    mr.kuf(p["variance"], p["lengthscales"], p["Z"], p["scales"], d["Xs"]), p["variance"], d["Y"], p["noise"])
        mu, var = m.predict_f(d["Xs"])
        assert _close(mu, rmu) and _close(var[:, 0], rvar)


# every gradient block against central differences of the long-double bound
GRAD_CASES = {
    "svgp_gauss_white_diag": ("svgp", "n300_m37", 1, dict(lik="gaussian", white=True, q="diag")),
    "svgp_gauss_plain_full": ("svgp", "n300_m37", 3, dict(lik="gaussian", white=False, q="full")),
    "svgp_bernoulli_white_diag": ("svgp", "n129_m130", 1, dict(lik="bernoulli", white=True, q="diag")),
    "sgpr_m37": ("sgpr", "n300_m37", 1, {}),
    "sgpr_m130": ("sgpr", "n129_m130", 3, {}),
    "fitc_m37": ("fitc", "n300_m37", 1, {}),
}


def _constrained(m, grads):
    """{id(parameter): d bound / d constrained value, shaped like the value}"""
    out = {}
    for prm, g in grads:
        if type(prm.transform).__name__ == "LowerTriangular":           # (its free vector is the constrained lower triangle)
            out[id(prm)] = np.asarray(g)
        else:
            out[id(prm)] = np.asarray(g) / np.atleast_1d(prm.transform.forward_grad(prm.vf_val)).reshape(np.shape(g))
    return out


@pytest.mark.parametrize("case", sorted(GRAD_CASES))
def test_every_gradient_block(handle, case):
    """Kernel variance, lengthscales, noise, q_mu, q_sqrt, Z, scales against central differences of the long-double bound,
    2e-6 max(1, |g|_inf).  The small blocks entry by entry, the large ones (Z, scales, q_mu, q_sqrt) at sampled entries (the
    reference costs one long-double Cholesky pair per entry).  First the reference itself: moving Z, X and scales by one ulp
    moves its gradient by at most a tenth of the tolerance."""
    import gpflowSlim as gpf
    kind, shape, R, opt = GRAD_CASES[case]
    d = _model_inputs(shape, R, seed=1)
    if kind == "svgp":
        m, p = _svgp(d, opt["lik"], opt["white"], opt["q"], R)
    else:
        kern, feat = _kern_feat(d)
        m = (gpf.models.SGPR if kind == "sgpr" else gpf.models.GPRFITC)(d["X"], d["Y"], kern, feat=feat, obs_var=0.3)
        p = _held(kern, feat, d, Y=d["Y"], noise=float(np.squeeze(m.likelihood.variance)))
    bound, grads = m.compute_log_likelihood_and_gradients()
    again = m.compute_log_likelihood_and_gradients()
    assert bound == again[0] and all(np.array_equal(a[1], b[1]) for a, b in zip(grads, again[1]))      # determinism, bit for bit
    ref = float(mr.model_bound(kind, p, LD))
    assert abs(bound - ref) <= 1e-8 * abs(ref)
    g = _constrained(m, grads)
    M = len(p["Z"])
    rng = np.random.RandomState(3)
    n_s = 12 if M < 100 else 6

    def sample(shape_):
        size = int(np.prod(shape_))
        flat = range(size) if size <= 8 else rng.choice(size, n_s, replace=False)
        return [np.unravel_index(i, shape_) for i in flat]

    blocks = [("variance", m.kern._variance, None), ("lengthscales", m.kern._ls, sample(p["lengthscales"].shape)),
              ("Z", m.feature._Z, sample(p["Z"].shape)), ("scales", m.feature._scales, sample(p["scales"].shape))]
    if "noise" in p:
        blocks.append(("noise", m.likelihood._variance, None))
    if kind == "svgp":
        blocks.append(("q_mu", m._q_mu, sample(p["q_mu"].shape)))
        if opt["q"] == "diag":
            blocks.append(("q_sqrt", m._q_sqrt, sample(p["q_sqrt"].shape)))
    p_ulp = dict(p, Z=np.nextafter(p["Z"], np.inf), X=np.nextafter(p["X"], np.inf), scales=np.nextafter(p["scales"], np.inf))
    for name, prm, where in blocks:
        got = np.asarray(g[id(prm)], dtype=np.float64).reshape(np.shape(p[name]))
        scale = max(1.0, float(np.abs(got).max()))
        tol = 2e-6 * scale
        for idx in (where if where is not None else [None]):
            fd = mr.fd_gradient(kind, p, name, idx)
            fd_ulp = mr.fd_gradient(kind, p_ulp, name, idx)
            assert abs(fd - fd_ulp) <= 0.1 * tol, (name, idx, fd, fd_ulp)
            val = float(got[idx]) if idx is not None else float(np.squeeze(got))
            assert abs(val - fd) <= tol, (name, idx, val, fd)
    if kind == "svgp" and opt["q"] == "full":
        # LowerTriangular: the free vector holds the lower triangles row-major per latent, already the constrained entries
        free = np.asarray(g[id(m._q_sqrt)]).reshape(R, -1)
        rows, cols = np.tril_indices(M, 0)
        scale = max(1.0, float(np.abs(free).max()))
        for t in rng.choice(len(rows), n_s, replace=False):
            for r in range(R):
                fd = mr.fd_gradient(kind, p, "q_sqrt", (rows[t], cols[t], r))
                assert abs(free[r, t] - fd) <= 2e-6 * scale, (t, r, free[r, t], fd)


@pytest.mark.parametrize("kind", ["svgp", "sgpr", "fitc"])
def test_tiny_scales_reproduce_inducing_points(handle, kind):
    """scales = 1e-9 against the plain inducing points of the same model, 1e-8 relative.  At the backend: the positive transform of
    features.Multiscale._scales has a floor of 1e-6, and widths of 1e-6 already move these bounds by 3e-7 relative (Kuu's
    diagonal loses 2 D s / l, which is 1 % of the jitter); the reference gives 3.5e-10 for 1e-9."""
    import gpflowSlim as gpf
    d = _model_inputs("n300_m37", 1)
    tiny = np.full_like(d["Z"], 1e-9)
    prog = gpf.kernels.RBF(5, variance=d["variance"], lengthscales=d["lengthscales"], ARD=True)._program(5)
    out = []
    for scales in (None, tiny):
        if kind == "svgp":
            out.append(handle.svgp_elbo(prog, d["Z"], d["X"], d["Y"], d["q_mu"], d["q_diag"], JIT, 0.3, white=True, scales=scales)[0])
        else:
            out.append(handle.sgpr(prog, d["Z"], d["X"], d["Y"], JIT, 0.3, fitc=(kind == "fitc"), scales=scales)[0])
    assert out[1] != out[0] and abs(out[1] - out[0]) <= 1e-8 * abs(out[0]), out


def test_the_one_shot_state_is_cleared(handle):
    """After a Multiscale call, and after one that the library refused, a plain call on the same handle returns the bytes it returns
    on a fresh handle."""
    import gpflowSlim as gpf
    from gpflowSlim import _backend as be
    d = _model_inputs("n129_m130", 1)
    kern, feat = _kern_feat(d)
    prog = kern._program(5)
    bad = gpf.kernels.Matern32(5)._program(5)
    args = (d["Z"], d["X"], d["Y"], d["q_mu"], d["q_diag"], JIT, 0.3)

    def plain(h):
        r = h.svgp_elbo_grad(prog, *args, white=False, want_grad_Z=True)
        return [np.atleast_1d(np.asarray(a)) for a in r]

    fresh = be.Handle()
    try:
        cold = plain(fresh)
    finally:
        fresh.close()
    r = handle.svgp_elbo_grad(prog, *args, white=False, want_grad_Z=True, scales=feat.scales)
    assert len(r) == len(cold) + 1 and r[-1].shape == d["Z"].shape and abs(r[0] - cold[0][0]) > 1e-3
    after = plain(handle)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(after, cold))
    with pytest.raises(RuntimeError, match=r"\(-4\).*Multiscale"):
        handle.svgp_elbo_grad(bad, *args, white=False, want_grad_Z=True, scales=feat.scales)
    after = plain(handle)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(after, cold))
    # ... and the conditional
    c0 = handle.conditional(prog, d["Z"], d["Xs"], d["q_mu"], JIT)
    handle.conditional(prog, d["Z"], d["Xs"], d["q_mu"], JIT, scales=feat.scales)
    c1 = handle.conditional(prog, d["Z"], d["Xs"], d["q_mu"], JIT)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(c0, c1))


# ---- 4. refusals at the C ABI ------------------------------------------------------------------------------------------------------------
def test_refusals_at_the_c_abi(handle):
    import gpflowSlim as gpf
    d = _model_inputs("n300_m37", 1)
    S = d["scales"]
    rbf = gpf.kernels.RBF(5)._program(5)
    for bad in (gpf.kernels.Matern32(5), gpf.kernels.RBF(5) + gpf.kernels.RBF(5)):
        prog = bad._program(5)
        with pytest.raises(RuntimeError, match=r"\(-4\).*Multiscale"):
            handle.svgp_elbo(prog, d["Z"], d["X"], d["Y"], d["q_mu"], d["q_diag"], JIT, 0.3, scales=S)
        with pytest.raises(RuntimeError, match=r"\(-4\).*Multiscale"):
            handle.sgpr(prog, d["Z"], d["X"], d["Y"], JIT, 0.3, scales=S)
        with pytest.raises(RuntimeError, match=r"\(-4\).*Multiscale"):
            handle.conditional(prog, d["Z"], d["Xs"], d["q_mu"], JIT, scales=S)
    # an entry that takes no inducing feature refuses while the scales are armed, and works again afterwards
    handle.gpr_set_data(d["X"], "multiscale-test")
    ok = handle.gpr_lml(rbf, 0.3, d["Y"])
    handle._arm_scales(S, d["Z"])
    with pytest.raises(RuntimeError, match=r"\(-4\).*Multiscale"):
        handle.gpr_lml(rbf, 0.3, d["Y"])
    assert handle.gpr_lml(rbf, 0.3, d["Y"]) == ok
    handle._arm_scales(S, d["Z"])
    with pytest.raises(RuntimeError, match=r"\(-4\).*Multiscale"):
        handle.sgpmc_lik(rbf, d["Z"], d["X"], d["Yb"], d["q_mu"], JIT, gpf._backend.make_lik(1, ()))
    # scales of another shape than Z never reach the library
    with pytest.raises(ValueError):
        handle.svgp_elbo(rbf, d["Z"], d["X"], d["Y"], d["q_mu"], d["q_diag"], JIT, 0.3, scales=S[:5])


# ---- 5. training ---------------------------------------------------------------------------------------------------------------------------
def test_training_moves_the_scales(handle):
    """The data of examples/svgp_multiscale.py with N = 500, M = 16: 100 Adam steps (learning rate 0.02) over all 286 parameters,
    inducing inputs and scales included.  The same loop on the CPU with tests/_multiscale_ref.py behind it (fp64 bound, central
    differences for the gradient) takes the objective from 10547.172 to 651.214 and moves the scales by up to 0.1609 (from 0.3
    to 0.139 .. 0.218); the device run prints the same three figures.  The thresholds are far inside that."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import svgp_multiscale as ex
    model, scales0 = ex.build(n=500, m=16, seed=0)
    start = model.objective
    final = model.optimize(max_iter=100, method="adam", learning_rate=2e-2)
    moved = float(np.abs(np.asarray(model.feature.scales) - scales0).max())
    print("training: objective %.3f -> %.3f, scales moved by up to %.4f" % (start, final, moved))
    assert np.isfinite(final) and final < start - 100.0, (start, final)
    assert moved > 0.05 and np.all(np.asarray(model.feature.scales) > 0), moved
