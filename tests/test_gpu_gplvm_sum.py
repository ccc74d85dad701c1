"""GPU tests of the Bayesian GPLVM with an ekernels.Sum of RBF kernels on separate latent dimensions (csrc/psi_sum.hip and the part
loops of csrc/gps_gplvm.hip): the expectations entry by entry against tests/_psi_sum_ref.py, symmetry and bitwise determinism,
the 50-digit fixture tests/golden/mp/bgplvm_sum.npz, bound / prediction / every gradient block against the long-double reference,
the S = 0 limit against SGPR, the combination of the single-RBF path's results, the refusals that remain, and one training run."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _psi_ref as pr  # noqa: E402
import _psi_sum_ref as ps  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def gpf():
    import gpflowSlim
    return gpflowSlim


def _as_slice(dims):
    return slice(dims[0], dims[-1] + 1) if list(dims) == list(range(dims[0], dims[-1] + 1)) else None


def _kern(gpf, parts, slices=False):
    """the ekernels.Sum of the parts; slices: contiguous parts are given as slice active_dims"""
    ks = []
    for p in parts:
        ad = _as_slice(p["dims"]) if slices else None
        ks.append(gpf.ekernels.RBF(len(p["dims"]), variance=p["var"], lengthscales=p["ls"],
                                   active_dims=p["dims"] if ad is None else ad, ARD=np.ndim(p["ls"]) > 0))
    return gpf.ekernels.Sum(ks)


# name -> (N, M, Q, columns of the parts, isotropic parts, slices, cross-term chunk (0: automatic))
CASES = {
    "one_point": (1, 1, 2, [[0], [1]], (), False, 0),
    "tiny": (7, 5, 3, [[0, 2], [1]], (), False, 0),
    "slices_ard_iso": (300, 37, 5, [[0, 1, 2], [3, 4]], (1,), True, 0),
    "three_parts_two_tiles": (129, 130, 5, [[0, 2], [1, 4], [3]], (), False, 0),       # M = 2 * 64 + 2, N = 2 * 64 + 1
    "psi2_chunk_edge": (193, 40, 4, [[0, 1], [2, 3]], (), False, 0),
    "every_register_length": (33, 9, 32, [[0], list(range(1, 6)), list(range(6, 15)), list(range(15, 32))], (2,), False, 0),
    "cross_chunk_edge": (129, 20, 3, [[0], [1, 2]], (), False, 64),                     # N = 2 * chunk + 1
    "unused_column": (50, 11, 5, [[0], [3, 1]], (), False, 0),                          # columns 2 and 4 belong to no part
}
_REF = {}


def _ref(name):
    if name not in _REF:
        N, M, Q, dl, iso, _, _ = CASES[name]
        d = pr.inputs(N, M, Q, seed=100 + N + M + Q)
        parts = ps.make_parts(d, dl, iso=iso)
        _REF[name] = (d, parts, ps.psi_with_spread(parts, d["Z"], d["mu"], d["S"], want_psi2n=N * M * M <= 10 ** 6))
    return _REF[name]


def _tol(spread):
    tol = max(8 * spread, 64 * EPS)
    assert tol <= 1e-12, "the reference's own spread leaves no room under the hard cap"
    return tol


@pytest.mark.parametrize("name", list(CASES))
def test_expectations_entrywise(gpf, name):
    from gpflowSlim import _backend as be
    N, M, Q, dl, iso, slices, chunk = CASES[name]
    if name == "psi2_chunk_edge":
        assert be.psi2_chunking(N, M) == (32, 3, 64, 4) and N == 3 * 64 + 1
    if name == "cross_chunk_edge":
        assert be.psi_sum_chunking(N, M, chunk) == (64, 3) and N == 2 * 64 + 1
    d, parts, ref = _ref(name)
    k = _kern(gpf, parts, slices)
    h = gpf.get_handle()
    h.psi_sum_set_chunk(chunk)
    try:
        p1 = k.eKxz(d["Z"], d["mu"], d["S"])
        p2 = k.eKzxKxz_sum(d["Z"], d["mu"], d["S"])
        p2_again = k.eKzxKxz_sum(d["Z"], d["mu"], d["S"])
        p2n = k.eKzxKxz(d["Z"], d["mu"], d["S"]) if "psi2n" in ref else None
    finally:
        h.psi_sum_set_chunk(0)
    assert p1.shape == (N, M) and p2.shape == (M, M)
    for what, got in (("psi1", p1), ("psi2", p2)) + ((("psi2n", p2n),) if p2n is not None else ()):
        err = float(np.max(np.abs(got - ref[what]) / np.abs(ref[what])))
        print("%s %s: rel err %.3g, spread %.3g" % (what, name, err, ref[what + "_spread"]))
        assert err <= _tol(ref[what + "_spread"]), (what, err, ref[what + "_spread"])
    assert np.array_equal(p2, p2.T)
    assert np.array_equal(p2, p2_again)
    if p2n is not None:
        assert p2n.shape == (N, M, M)
        assert np.abs(p2n.sum(0) / p2 - 1).max() <= 64 * EPS
    assert np.allclose(k.eKdiag(d["mu"], d["S"]), np.full(N, sum(p["var"] for p in parts)), rtol=1e-14, atol=0)


def _model(gpf, d, parts, slices=False):
    return gpf.models.BayesianGPLVM(d["mu"], d["S"], d["Y"], _kern(gpf, parts, slices), d["Z"].shape[0], Z=d["Z"], obs_var=d["noise"])


def _check_grads(m, parts, ref_g, ref_kl_g):
    """every gradient block against the reference, chained to the unconstrained values; per part in m.kern.kern_list[i]"""
    _, grads = m.compute_log_likelihood_and_gradients()
    got = {id(p): g for p, g in grads}
    want = [("noise", m.likelihood._variance, ref_g["noise"]), ("Z", m._Z, ref_g["Z"]),
            ("X_mean", m._X_mean, ref_g["X_mean"] - ref_kl_g[0]), ("X_var", m._X_var, ref_g["X_var"] - ref_kl_g[1])]
    for i, kp in enumerate(m.kern.kern_list):
        want.append(("variance[%d]" % i, kp._variance, ref_g["variance"][i]))
        want.append(("lengthscales[%d]" % i, kp._ls, ref_g["lengthscales"][i]))
    for name, p, gc in want:
        gc = np.asarray(gc, dtype=np.float64)
        if name in ("Z", "X_mean"):
            gu = gc
        elif name.startswith("lengthscales") and np.size(p.vf_val) == 1:
            gu = np.sum(gc) * pr.softplus_grad(p.vf_val)              # isotropic: the part's slots fold into one parameter
        else:
            gu = gc * pr.softplus_grad(p.vf_val)
        g = np.asarray(got[id(p)], dtype=np.float64)
        err = float(np.max(np.abs(g - gu.reshape(g.shape))))
        print("grad %s: abs err %.3g, |g|inf %.3g" % (name, err, float(np.max(np.abs(gu)))))
        assert err <= 2e-6 * max(1.0, float(np.max(np.abs(gu)))), (name, err)


def test_against_the_mpmath_fixture(gpf):
    g = np.load(os.path.join(ROOT, "tests", "golden", "mp", "bgplvm_sum.npz"))
    parts = [{"var": float(g["variance%d" % i]), "ls": g["lengthscales%d" % i], "dims": [int(c) for c in g["dims%d" % i]]} for i in (0, 1)]
    d = {"noise": float(g["noise"]), "Z": g["Z"], "mu": g["X_mean"], "S": g["X_var"], "Y": g["Y"]}
    k = _kern(gpf, parts)
    assert np.abs(k.eKxz(d["Z"], d["mu"], d["S"]) / g["psi1"] - 1).max() <= 64 * EPS
    assert np.abs(k.eKzxKxz_sum(d["Z"], d["mu"], d["S"]) / g["psi2"] - 1).max() <= 64 * EPS
    m = _model(gpf, d, parts)
    want = float(g["F"]) - float(g["KL"])
    assert abs(m._kl()[0] - float(g["KL"])) <= 1e-8 * abs(float(g["KL"]))
    assert abs(m.compute_log_likelihood() - want) <= 1e-8 * abs(want)
    mean, var = m.predict_f(g["Xnew"])
    assert np.abs(mean - g["mean"]).max() <= 1e-8 * np.abs(g["mean"]).max()
    assert var.shape == (3, 2) and np.abs(var[:, 0] - np.diag(g["cov"])).max() <= 1e-8 * np.abs(g["cov"]).max()
    mean2, cov = m.predict_f_full_cov(g["Xnew"])
    assert cov.shape == (3, 3, 2) and np.abs(cov[:, :, 1] - g["cov"]).max() <= 1e-8 * np.abs(g["cov"]).max()
    assert np.abs(mean2 - g["mean"]).max() <= 1e-8 * np.abs(g["mean"]).max()
    ref_g = {kk: g["grad_" + kk] for kk in ("noise", "Z", "X_mean", "X_var")}
    ref_g["variance"] = [float(g["grad_variance0"]), float(g["grad_variance1"])]
    ref_g["lengthscales"] = [g["grad_lengthscales0"], g["grad_lengthscales1"]]
    _check_grads(m, parts, ref_g, pr.kl_grad(d["mu"], d["S"]))


# The two criteria on the reference of tests/test_gpu_gplvm.py, asserted here too: the fp64 restatement of the reference's own
# algorithm (_psi_sum_ref.bound, LAPACK) within REF_OWN_ERROR of its long-double evaluation in the predicted mean and variance, and
# the long-double gradient moving by at most REF_ONE_ULP_SHARE of the tolerance when the inputs move by one ulp.  The cases are the
# ones checked on the CPU for both: M = 130 needs the lengthscales scaled by 0.25 (as drawn, cond(Kuu + 1e-6 I) is 3e8), and the
# three-part split is used at R = 3 only (at R = 1 the gradient moves by 0.29 of the tolerance).
REF_OWN_ERROR = 2e-9
REF_ONE_ULP_SHARE = 0.1
BOUND_CASES = {
    "N300_M37_slices_R1": (300, 37, [[0, 1, 2], [3, 4]], 1.0, 1, True),
    "N300_M37_slices_R3": (300, 37, [[0, 1, 2], [3, 4]], 1.0, 3, True),
    "N129_M130_lists_R1": (129, 130, [[0, 2, 4], [1, 3]], 0.25, 1, False),
    "N129_M130_lists_R3": (129, 130, [[0, 2, 4], [1, 3]], 0.25, 3, False),
    "N129_M130_three_parts_R3": (129, 130, [[0, 2], [1, 4], [3]], 0.25, 3, False),
}


def _flat(g):
    out = {kk: np.asarray(g[kk]) for kk in ("noise", "Z", "X_mean", "X_var")}
    out["variance"] = np.asarray(g["variance"])
    out["lengthscales"] = np.concatenate(g["lengthscales"])
    return out


@pytest.mark.parametrize("name", list(BOUND_CASES))
def test_bound_predict_and_gradient_against_the_reference(gpf, name):
    N, M, dl, scale, R, slices = BOUND_CASES[name]
    d = pr.inputs(N, M, 5, R=R, seed=7 + N + R)
    d["noise"] = 0.3
    parts = ps.make_parts(d, dl, scale)
    m = _model(gpf, d, parts, slices)
    Xs = np.random.default_rng(5).standard_normal((9, 5))
    a = dict(noise=d["noise"], Z=d["Z"], mu=d["mu"], S=d["S"], Y=d["Y"])
    F, mean, var, cov = ps.bound_ld(parts, Xnew=Xs, **a)
    _, mean64, var64 = ps.bound(parts, Xnew=Xs, **a)
    own = max(np.abs(mean64 - mean).max() / np.abs(mean).max(), np.abs(var64 - var).max() / np.abs(var).max())
    print("the fp64 restatement's own error against long double: %.3g" % own)
    assert own <= REF_OWN_ERROR
    kl = pr.kl(d["mu"], d["S"])
    assert abs(m._kl()[0] - kl) <= 1e-8 * abs(kl)
    got = m.compute_log_likelihood()
    print("bound %s: %.12g vs %.12g" % (name, got, F - kl))
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
    _, moved = ps.bound_grad(parts, dtype=np.longdouble, **b)
    _, ref_g = ps.bound_grad(parts, dtype=np.longdouble, **a)
    fm, fr = _flat(moved), _flat(ref_g)
    share = max(np.abs(fm[kk] - fr[kk]).max() / (2e-6 * max(1.0, np.abs(fr[kk]).max())) for kk in fr)
    print("one-ulp movement of the reference gradient: %.3g of the tolerance" % share)
    assert share <= REF_ONE_ULP_SHARE
    _check_grads(m, parts, ref_g, pr.kl_grad(d["mu"], d["S"]))


def _structure_case():
    d = pr.inputs(300, 37, 5, R=2, seed=7 + 300 + 2)
    d["noise"] = 0.3
    return d, ps.make_parts(d, [[0, 1, 2], [3, 4]])


def test_zero_variance_is_sgpr(gpf):
    """S = 0: Psi1 = K(X, Z) and Psi2 = Kuf Kuf^T of the summed kernel (the cross terms are what makes the second one hold), so
    gps_bgplvm is gps_sgpr with kernels.Sum of the same parts on (Z, X = mu, Y)."""
    d, parts = _structure_case()
    h = gpf.get_handle()
    k = _kern(gpf, parts)
    plain = gpf.kernels.Sum([gpf.kernels.RBF(len(p["dims"]), variance=p["var"], lengthscales=p["ls"], active_dims=p["dims"], ARD=True)
                             for p in parts])
    Xs = np.random.default_rng(3).standard_normal((11, 5))
    F, mean, var = h.bgplvm(k._psi_program(d["mu"]), d["Z"], d["mu"], np.zeros_like(d["S"]), d["Y"], 1e-6, d["noise"], Xnew=Xs)
    Fs, means, vars_ = h.sgpr(plain._program(5), d["Z"], d["mu"], d["Y"], 1e-6, d["noise"], Xnew=Xs)
    assert abs(F - Fs) <= 1e-8 * abs(Fs), (F, Fs)
    assert np.abs(mean - means).max() <= 1e-8 * np.abs(means).max()
    assert np.abs(var - vars_).max() <= 1e-8 * np.abs(vars_).max()
    p1 = k.eKxz(d["Z"], d["mu"], np.zeros_like(d["S"]))
    assert np.abs(p1 - plain.K(d["mu"], d["Z"])).max() <= 1e-13 * sum(p["var"] for p in parts)


def test_sum_is_the_single_rbf_path_combined_on_the_host(gpf):
    d, parts = _structure_case()
    k = _kern(gpf, parts)
    T, P2 = [], []
    for p in parts:
        c = p["dims"]
        kp = gpf.ekernels.RBF(len(c), variance=p["var"], lengthscales=p["ls"], ARD=True)
        Zp, mup, Sp = (np.ascontiguousarray(d[kk][:, c]) for kk in ("Z", "mu", "S"))
        T.append(kp.eKxz(Zp, mup, Sp)); P2.append(kp.eKzxKxz_sum(Zp, mup, Sp))
    want1 = T[0] + T[1]
    want2 = P2[0] + P2[1] + (T[0].T @ T[1] + T[1].T @ T[0])
    p1, p2 = k.eKxz(d["Z"], d["mu"], d["S"]), k.eKzxKxz_sum(d["Z"], d["mu"], d["S"])
    assert np.abs(p1 / want1 - 1).max() <= 1e-12
    assert np.abs(p2 / want2 - 1).max() <= 1e-12


def test_gradient_is_bitwise_reproducible(gpf):
    d, parts = _structure_case()
    h = gpf.get_handle()
    prog = _kern(gpf, parts)._psi_program(d["mu"])
    g1 = h.bgplvm_grad(prog, d["Z"], d["mu"], d["S"], d["Y"], 1e-6, d["noise"])
    g2 = h.bgplvm_grad(prog, d["Z"], d["mu"], d["S"], d["Y"], 1e-6, d["noise"])
    for x, y in zip(g1, g2):
        assert np.array_equal(np.asarray(x), np.asarray(y))


def test_refusals_that_remain(gpf):
    from gpflowSlim import _backend as be
    d = pr.inputs(6, 4, 3, R=2, seed=4)
    h = gpf.get_handle()
    E = gpf.ekernels
    with pytest.raises(NotImplementedError, match="Sum.*overlap"):
        E.Sum([E.RBF(2, active_dims=[0, 1]), E.RBF(2, active_dims=[1, 2])])
    with pytest.raises(NotImplementedError, match="Sum"):
        E.Sum([E.RBF(2, active_dims=[0, 1]), gpf.kernels.Matern32(1, active_dims=[2])])
    with pytest.raises(NotImplementedError, match="Sum"):
        E.Sum([E.RBF(3)])
    k = E.Sum([E.RBF(2, active_dims=[0, 2]), E.RBF(1, active_dims=[1])])
    with pytest.raises(NotImplementedError, match="covariances"):
        k.eKzxKxz_sum(d["Z"], d["mu"], np.zeros((6, 3, 3)))
    with pytest.raises(NotImplementedError, match="covariances"):
        gpf.models.BayesianGPLVM(d["mu"], np.zeros((6, 3, 3)), d["Y"], k, 4)
    with pytest.raises(NotImplementedError):
        k.exKxz(d["Z"], d["mu"], d["S"])
    with pytest.raises(NotImplementedError):
        k.exKxz_pairwise(d["Z"], d["mu"], d["S"])
    # at the C ABI: GPS_ERR_UNSUPPORTED (-4) for a Sum program with a Matern node, and for overlapping parts
    mat = (gpf.kernels.RBF(2, active_dims=[0, 2]) + gpf.kernels.Matern32(1, active_dims=[1]))._program(3)
    with pytest.raises(RuntimeError, match=r"\(-4\).*Sum of RBF"):
        h.psi_stats(mat, d["Z"], d["mu"], d["S"], want_psi1=True)
    over = be.make_program([be.primitive_node(be.K_RBF, 1.0, [0, 1], [1.0, 1.0]), be.primitive_node(be.K_RBF, 1.0, [1, 2], [1.0, 1.0]),
                            be.op_node(be.K_ADD)])
    with pytest.raises(RuntimeError, match=r"\(-4\).*disjoint"):
        h.bgplvm(over, d["Z"], d["mu"], d["S"], d["Y"], 1e-6, 0.1)


def test_training_with_the_reference_examples_kernel(gpf):
    """N = 200 on the example's generator with the reference's kernel at Q = 5 (RBF on 0:3 plus RBF on 3:5), M = 15: 150 Adam steps
    lower the objective and leave the latent means nearest-neighbour-separable in the two most sensitive dimensions.  The seed was
    first checked on the CPU, with _psi_sum_ref.bound_grad in place of the device behind the same Adam loop: objective 4070.8 ->
    -1134.3 in 150 steps, sensitivities (0.212, 0.206, 0.149 | 0.025, 0.025), agreement 1.000."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("example_gplvm", os.path.join(ROOT, "examples", "gplvm.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    Y, labels = example.synthetic(200, seed=3)
    Q, M = 5, 15
    X0 = gpf.models.PCA_reduce(Y, Q)
    Z0 = X0[np.random.default_rng(0).permutation(200)[:M]].copy()
    k = example.reference_kernel()
    m = gpf.models.BayesianGPLVM(X0, 0.1 * np.ones((200, Q)), Y, k, M, Z=Z0)
    f0 = m.objective
    f1 = m.optimize(method="adam", learning_rate=0.05, max_iter=150)
    print("objective %.6g -> %.6g" % (f0, f1))
    assert f1 < f0
    sens = example.sensitivities(m.kern, Q)
    assert len(m.kern.kern_list) == 2 and sens.shape == (5,)
    X = m.X_mean[:, np.argsort(sens)[::-1][:2]]
    D = np.sum((X[:, None, :] - X[None, :, :]) ** 2, axis=2) + 1e30 * np.eye(200)
    same = labels[np.argmin(D, axis=1)] == labels
    print("sensitivities %s; nearest neighbour shares the label: %.3f" % (np.array2string(sens, precision=3), same.mean()))
    assert same.mean() >= 0.95
