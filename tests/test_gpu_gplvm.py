"""GPU tests of the Bayesian GPLVM path: the RBF kernel expectations (csrc/psi.hip) entry by entry against tests/_psi_ref.py,
symmetry and bitwise determinism, the S = 0 limit against gps_sgpr, bound / KL / prediction / gradient against the 50-digit
fixture tests/golden/mp/bgplvm.npz and against _psi_ref, the ekernels.RBF surface, the refusals and one training run."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _psi_ref as pr  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def gpf():
    import gpflowSlim
    return gpflowSlim


def _kern(gpf, d):
    Q = d["mu"].shape[1]
    return gpf.ekernels.RBF(Q, variance=d["var"], lengthscales=d["ls"], ARD=np.ndim(d["ls"]) > 0)


def _chunk_shape():
    """N = k * chunk + 1 for the Psi2 kernel's own chunk length: M = 40 takes the 32-wide pair tile (3 lower-triangle tiles), and
    the chunk rule then cuts N = 193 into 4 chunks of 64 points: 193 = 3 * 64 + 1."""
    from gpflowSlim import _backend as be
    N, M = 193, 40
    tm, nt, chunk, nch = be.psi2_chunking(N, M)
    assert (tm, nt, chunk, nch) == (32, 3, 64, 4) and N == 3 * chunk + 1
    return (N, M, 2)


SHAPES = [(1, 1, 1), (7, 5, 1), (300, 37, 3), (129, 130, 5), (2050, 64, 8), (33, 9, 32), (193, 40, 2)]
_REF = {}


def _ref(shape, ard):
    key = (shape, ard)
    if key not in _REF:
        N, M, Q = shape
        d = pr.inputs(N, M, Q, seed=100 + N + M + Q, ard=ard)
        _REF[key] = (d, pr.psi_with_spread(d["var"], d["ls"], d["Z"], d["mu"], d["S"], want_psi2n=N * M * M <= 10 ** 6))
    return _REF[key]


def _tol(spread):
    tol = max(8 * spread, 64 * EPS)
    assert tol <= 1e-12, "the reference's own spread leaves no room under the hard cap"
    return tol


@pytest.mark.parametrize("ard", [True, False], ids=["ard", "iso"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d_M%d_Q%d" % s)
def test_psi_statistics_entrywise(gpf, shape, ard):
    if shape == (193, 40, 2):
        assert _chunk_shape() == shape
    d, ref = _ref(shape, ard)
    k = _kern(gpf, d)
    N, M, Q = shape
    p1 = k.eKxz(d["Z"], d["mu"], d["S"])
    p2 = k.eKzxKxz_sum(d["Z"], d["mu"], d["S"])
    assert p1.shape == (N, M) and p2.shape == (M, M)
    for name, got in (("psi1", p1), ("psi2", p2)):
        err = float(np.max(np.abs(got - ref[name]) / np.abs(ref[name])))
        print("%s %s ard=%s: rel err %.3g, spread %.3g" % (name, shape, ard, err, ref[name + "_spread"]))
        assert err <= _tol(ref[name + "_spread"]), (name, err, ref[name + "_spread"])
    assert np.array_equal(p2, p2.T)
    if "psi2n" in ref:
        p2n = k.eKzxKxz(d["Z"], d["mu"], d["S"])
        assert p2n.shape == (N, M, M)
        err = float(np.max(np.abs(p2n - ref["psi2n"]) / np.abs(ref["psi2n"])))
        print("psi2n %s ard=%s: rel err %.3g, spread %.3g" % (shape, ard, err, ref["psi2n_spread"]))
        assert err <= _tol(ref["psi2n_spread"])
    assert np.allclose(k.eKdiag(d["mu"], d["S"]), np.full(N, d["var"]), rtol=1e-14, atol=0)


# Seeds of the bound / prediction / gradient cases: 7 + N + R + 100 k with the first k at which the fp64 restatement of the
# reference's own algorithm (_psi_ref.bound, LAPACK) stays within 2e-9 of its long-double evaluation (_psi_ref.bound_ld) in the
# predicted mean and variance.  At k = 0, 1 of (300, 37, 3), R = 1 the draw of Z and the lengthscales gives cond(Kuu + 1e-6 I) =
# 1.5e7 and that restatement is itself 1.6e-8 and 2.5e-8 off (any fp64 run of gplvm.py:169-204 lands 0.7e-8 to 2.3e-8 from the
# long-double value there): a 1e-8 check of the device at such inputs checks nothing.  The test asserts the criterion.
# The gradient has its own criterion: the long-double reference gradient, evaluated at inputs moved by one ulp, may move by at most a
# tenth of the tolerance.  At k = 0 .. 3 of (129, 130, 5), R = 1 (cond(Kuu + 1e-6 I) about 1e8) it moves by 0.5 to 1.6 times the
# tolerance: no fp64 evaluation could be told from a wrong one there.
_SEED_STEP = {(300, 37, 3, 1): 2, (129, 130, 5, 1): 4}
REF_OWN_ERROR = 2e-9
REF_ONE_ULP_SHARE = 0.1


def _bg_case(N, M, Q, R):
    d = pr.inputs(N, M, Q, R=R, seed=7 + N + R + 100 * _SEED_STEP.get((N, M, Q, R), 0))
    d["noise"] = 0.3
    return d


def test_symmetry_and_determinism(gpf):
    d = _bg_case(300, 37, 3, 3)
    h = gpf.get_handle()
    prog = _kern(gpf, d)._psi_program(d["mu"])
    a = h.psi_stats(prog, d["Z"], d["mu"], d["S"], want_psi2=True)[1]
    b = h.psi_stats(prog, d["Z"], d["mu"], d["S"], want_psi2=True)[1]
    assert np.array_equal(a, a.T) and np.array_equal(a, b)
    g1 = h.bgplvm_grad(prog, d["Z"], d["mu"], d["S"], d["Y"], 1e-6, d["noise"])
    g2 = h.bgplvm_grad(prog, d["Z"], d["mu"], d["S"], d["Y"], 1e-6, d["noise"])
    for x, y in zip(g1, g2):
        assert np.array_equal(np.asarray(x), np.asarray(y))


def test_zero_variance_is_sgpr(gpf):
    """S = 0: Psi1 = K(X, Z), Psi2 = Kuf Kuf^T, so gps_bgplvm is gps_sgpr on (Z, X = mu, Y)."""
    d = _bg_case(300, 37, 3, 2)
    h = gpf.get_handle()
    k = _kern(gpf, d)
    prog = k._psi_program(d["mu"])
    Xs = np.random.default_rng(3).standard_normal((11, 3))
    F, mean, var = h.bgplvm(prog, d["Z"], d["mu"], np.zeros_like(d["S"]), d["Y"], 1e-6, d["noise"], Xnew=Xs)
    Fs, means, vars_ = h.sgpr(prog, d["Z"], d["mu"], d["Y"], 1e-6, d["noise"], Xnew=Xs)
    assert abs(F - Fs) <= 1e-8 * abs(Fs), (F, Fs)
    assert np.abs(mean - means).max() <= 1e-8 * np.abs(means).max()
    assert np.abs(var - vars_).max() <= 1e-8 * np.abs(vars_).max()
    p1 = k.eKxz(d["Z"], d["mu"], np.zeros_like(d["S"]))
    Kxz = k.K(d["mu"], d["Z"])
    assert np.abs(p1 - Kxz).max() <= 1e-13 * d["var"]


def _model(gpf, d):
    k = _kern(gpf, d)
    return gpf.models.BayesianGPLVM(d["mu"], d["S"], d["Y"], k, d["Z"].shape[0], Z=d["Z"], obs_var=d["noise"])


def _check_grads(m, ref_g, ref_kl_g):
    _, grads = m.compute_log_likelihood_and_gradients()
    want = {"variance": (m.kern._variance, ref_g["variance"]), "lengthscales": (m.kern._ls, ref_g["lengthscales"]),
            "noise": (m.likelihood._variance, ref_g["noise"]), "Z": (m._Z, ref_g["Z"]),
            "X_mean": (m._X_mean, ref_g["X_mean"] - ref_kl_g[0]), "X_var": (m._X_var, ref_g["X_var"] - ref_kl_g[1])}
    got = {id(p): g for p, g in grads}
    for name, (p, gc) in want.items():
        gc = np.asarray(gc, dtype=np.float64)
        if name in ("Z", "X_mean"):
            gu = gc                                                   # identity transform
        elif name == "lengthscales" and np.size(p.vf_val) == 1:
            gu = np.sum(gc) * pr.softplus_grad(p.vf_val)              # isotropic: the Q slots fold into one parameter
        else:
            gu = gc * pr.softplus_grad(p.vf_val)
        g = np.asarray(got[id(p)], dtype=np.float64)
        err = float(np.max(np.abs(g - gu.reshape(g.shape))))
        print("grad %s: abs err %.3g, |g|inf %.3g" % (name, err, float(np.max(np.abs(gu)))))
        assert err <= 2e-6 * max(1.0, float(np.max(np.abs(gu)))), (name, err)


def test_against_the_mpmath_fixture(gpf):
    g = np.load(os.path.join(ROOT, "tests", "golden", "mp", "bgplvm.npz"))
    d = {"var": float(g["variance"]), "ls": g["lengthscales"], "noise": float(g["noise"]), "Z": g["Z"], "mu": g["X_mean"],
         "S": g["X_var"], "Y": g["Y"]}
    k = _kern(gpf, d)
    assert np.abs(k.eKxz(d["Z"], d["mu"], d["S"]) / g["psi1"] - 1).max() <= 64 * EPS
    assert np.abs(k.eKzxKxz_sum(d["Z"], d["mu"], d["S"]) / g["psi2"] - 1).max() <= 64 * EPS
    m = _model(gpf, d)
    want = float(g["F"]) - float(g["KL"])
    assert abs(m._kl()[0] - float(g["KL"])) <= 1e-8 * abs(float(g["KL"]))
    assert abs(m.compute_log_likelihood() - want) <= 1e-8 * abs(want)
    mean, var = m.predict_f(g["Xnew"])
    assert np.abs(mean - g["mean"]).max() <= 1e-8 * np.abs(g["mean"]).max()
    assert var.shape == (3, 2) and np.abs(var[:, 0] - np.diag(g["cov"])).max() <= 1e-8 * np.abs(g["cov"]).max()
    mean2, cov = m.predict_f_full_cov(g["Xnew"])
    assert cov.shape == (3, 3, 2) and np.abs(cov[:, :, 1] - g["cov"]).max() <= 1e-8 * np.abs(g["cov"]).max()
    assert np.abs(mean2 - g["mean"]).max() <= 1e-8 * np.abs(g["mean"]).max()
    ref_g = {kk: g["grad_" + kk] for kk in ("variance", "lengthscales", "noise", "Z", "X_mean", "X_var")}
    _check_grads(m, ref_g, pr.kl_grad(d["mu"], d["S"]))


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("shape", [(300, 37, 3), (129, 130, 5)], ids=lambda s: "N%d_M%d_Q%d" % s)
def test_bound_predict_and_gradient_against_the_reference(gpf, shape, R):
    d = _bg_case(*shape, R)
    m = _model(gpf, d)
    Xs = np.random.default_rng(5).standard_normal((9, shape[2]))
    a = dict(var=d["var"], ls=d["ls"], noise=d["noise"], Z=d["Z"], mu=d["mu"], S=d["S"], Y=d["Y"])
    F, mean, var, cov = pr.bound_ld(**a, Xnew=Xs)
    _, mean64, var64 = pr.bound(**a, Xnew=Xs)
    own = max(np.abs(mean64 - mean).max() / np.abs(mean).max(), np.abs(var64 - var).max() / np.abs(var).max())
    print("the fp64 restatement's own error against long double: %.3g" % own)
    assert own <= REF_OWN_ERROR
    kl = pr.kl(d["mu"], d["S"])
    assert abs(m._kl()[0] - kl) <= 1e-8 * abs(kl)
    got = m.compute_log_likelihood()
    print("bound %s R=%d: %.12g vs %.12g" % (shape, R, got, F - kl))
    assert abs(got - (F - kl)) <= 1e-8 * abs(F - kl)
    gm, gv = m.predict_f(Xs)
    print("mean rel err %.3g, var rel err %.3g" % (np.abs(gm - mean).max() / np.abs(mean).max(), np.abs(gv[:, 0] - var).max() / np.abs(var).max()))
    assert np.abs(gm - mean).max() <= 1e-8 * np.abs(mean).max()
    assert gv.shape == (9, R) and np.abs(gv[:, 0] - var).max() <= 1e-8 * np.abs(var).max()
    _, gc = m.predict_f_full_cov(Xs)
    assert gc.shape == (9, 9, R) and np.abs(gc[:, :, 0] - cov).max() <= 1e-8 * np.abs(cov).max()
    b = dict(a)
    for kk in ("Z", "mu", "S"):
        b[kk] = a[kk] * (1 + EPS * np.where(np.arange(a[kk].size).reshape(a[kk].shape) % 2 == 0, 1.0, -1.0))
    _, moved = pr.bound_grad(**b, dtype=np.longdouble)
    Fg, ref_g = pr.bound_grad(**a, dtype=np.longdouble)      # (fp64: its explicit inverses lose up to 5e-3 of the Z gradient here)
    share = max(np.abs(np.asarray(moved[kk]) - np.asarray(ref_g[kk])).max() / (2e-6 * max(1.0, np.abs(np.asarray(ref_g[kk])).max()))
                for kk in ref_g)
    print("one-ulp movement of the reference gradient: %.3g of the tolerance" % share)
    assert share <= REF_ONE_ULP_SHARE
    _check_grads(m, ref_g, pr.kl_grad(d["mu"], d["S"]))


def test_isotropic_gradient_folds_the_lengthscale_slots(gpf):
    d = pr.inputs(129, 20, 3, R=2, seed=11, ard=False)
    d["noise"] = 0.3
    m = _model(gpf, d)
    a = dict(var=d["var"], ls=d["ls"], noise=d["noise"], Z=d["Z"], mu=d["mu"], S=d["S"], Y=d["Y"])
    _, ref_g = pr.bound_grad(**a, dtype=np.longdouble)
    _check_grads(m, ref_g, pr.kl_grad(d["mu"], d["S"]))


def test_ekernels_agree_with_the_c_entry_point(gpf):
    d = pr.inputs(33, 9, 4, seed=2)
    k = _kern(gpf, d)
    p1, p2, p2n = gpf.get_handle().psi_stats(k._psi_program(d["mu"]), d["Z"], d["mu"], d["S"], True, True, True)
    assert np.array_equal(k.eKxz(d["Z"], d["mu"], d["S"]), p1) and p1.shape == (33, 9)
    assert np.array_equal(k.eKzxKxz_sum(d["Z"], d["mu"], d["S"]), p2) and p2.shape == (9, 9)
    assert np.array_equal(k.eKzxKxz(d["Z"], d["mu"], d["S"]), p2n) and p2n.shape == (33, 9, 9)
    assert np.abs(p2n.sum(0) / p2 - 1).max() <= 64 * EPS
    assert k.eKdiag(d["mu"]).shape == (33,)


def test_refusals(gpf):
    from gpflowSlim import _backend as be
    d = pr.inputs(6, 4, 3, R=2, seed=4)
    h = gpf.get_handle()
    k = _kern(gpf, d)
    with pytest.raises(NotImplementedError, match="covariances"):
        k.eKxz(d["Z"], d["mu"], np.zeros((6, 3, 3)))
    with pytest.raises(NotImplementedError, match="active_dims"):
        gpf.ekernels.RBF(2, active_dims=[0, 2]).eKxz(d["Z"], d["mu"], d["S"])
    for name in ("Linear", "Sum", "Product"):
        with pytest.raises(NotImplementedError):
            getattr(gpf.ekernels, name)(3)
    # at the C ABI: GPS_ERR_UNSUPPORTED (-4) with a message that names the restriction
    mat = gpf.kernels.Matern32(3)._program(3)
    with pytest.raises(RuntimeError, match=r"\(-4\).*single RBF"):
        h.psi_stats(mat, d["Z"], d["mu"], d["S"], want_psi1=True)
    sub = be.make_program([be.primitive_node(be.K_RBF, 1.0, [0, 2], [1.0, 1.0])])
    with pytest.raises(RuntimeError, match=r"\(-4\).*latent dimensions"):
        h.bgplvm(sub, d["Z"], d["mu"], d["S"], d["Y"], 1e-6, 0.1)
    summed = (gpf.kernels.RBF(3) + gpf.kernels.RBF(3))._program(3)
    with pytest.raises(RuntimeError, match=r"\(-4\)"):
        h.bgplvm_grad(summed, d["Z"], d["mu"], d["S"], d["Y"], 1e-6, 0.1)


def test_training_separates_the_clusters(gpf):
    """N = 200, Q = 2, M = 15 on the example's synthetic generator: 150 Adam steps lower the objective and leave the latent
    means nearest-cluster-separable (the seed was first checked on the CPU with _psi_ref and scipy)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("example_gplvm", os.path.join(ROOT, "examples", "gplvm.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    Y, labels = example.synthetic(200, seed=3)
    Q, M = 2, 15
    X0 = gpf.models.PCA_reduce(Y, Q)
    Z0 = X0[np.random.default_rng(0).permutation(200)[:M]].copy()
    k = gpf.ekernels.RBF(Q, ARD=True)
    m = gpf.models.BayesianGPLVM(X0, 0.1 * np.ones((200, Q)), Y, k, M, Z=Z0)
    f0 = m.objective
    f1 = m.optimize(method="adam", learning_rate=0.05, max_iter=150)
    print("objective %.6g -> %.6g" % (f0, f1))
    assert f1 < f0
    X = m.X_mean
    D = np.sum((X[:, None, :] - X[None, :, :]) ** 2, axis=2) + 1e30 * np.eye(200)
    same = labels[np.argmin(D, axis=1)] == labels
    print("nearest neighbour shares the label: %.3f" % same.mean())
    assert same.mean() >= 0.95
