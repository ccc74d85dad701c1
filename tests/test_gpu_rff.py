"""GPU tests of the random-feature GPR branch (csrc/rff.hip, csrc/gps_rff.hip, gpflowSlim/kernel_kitchen_sink.py, the feature
branch of models/gpr.py and densities.multivariate_normal_feature) against tests/_rff_ref.py (tests/test_rff_ref_cpu.py checks
that restatement) and, where the shape matches, the 50-digit fixture tests/golden/mp/rff.npz.

Tolerances: 1e-12 for the entries of the feature map (|Phi| <= sqrt(2 var / F), arguments of the cosine below ~50: a few ulp),
1e-8 relative with scale max(1, |value|) for likelihoods, predictions and gradients, 1e-12 relative between two chunkings of the
same evaluation (they differ in summation order only), bitwise between two calls with the same chunking.  The one exception is
test_low_noise (s = 1e-5, cond(A) ~ 1e7): there the order in which A = Phi^T Phi is summed moves the results by 2e-11 with
every later step in long double (tests/test_rff_ref_cpu.py::test_what_the_order_of_summation_of_A_moves), and two chunkings
are held to rr.chunking_bound = eps cond(A) (3.9e-9 and 2.0e-9 on its two cases) instead of 1e-12."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _rff_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEATURE_SHAPES = [(1, 1, 1), (127, 3, 128), (129, 13, 130), (300, 4, 257)]
CASES = [(24, 3, 10, 2, True), (300, 13, 130, 3, False), (700, 1, 257, 2, True), (50, 4, 200, 1, True)]


def _rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def _gpf():
    import gpflowSlim as gpf
    return gpf


def _sampler(c):
    """An RBFSampler carrying the case's omega / offset."""
    ks = _gpf().kernel_kitchen_sink
    D, F = c["omega"].shape
    s = ks.RBFSampler(D, ls=c["ls"] if c["ls"].size > 1 else float(c["ls"][0]), var=c["var"], n_components=F,
                      rng=np.random.default_rng(0))
    s.omega, s.random_offset_ = c["omega"].copy(), c["offset"].copy()
    return s


def _case(N, D, F, R, ard):
    if (N, D, F, R) == (24, 3, 10, 2):
        g = np.load(os.path.join(ROOT, "tests", "golden", "mp", "rff.npz"))
        return dict(X=g["X"], Y=g["Y"], Xs=g["Xnew"], omega=g["omega"], offset=g["offset"], ls=g["ls"], var=float(g["variance"]),
                    s=float(g["noise"]), golden=g)
    return rr.case(N, D, F, R, ard, seed=N)


_REF = {}


def _reference(key):
    """(case, Phi, reference LML, mean, var, cov, gradients): computed once per case and shared."""
    if key not in _REF:
        c = _case(*key)
        Phi = rr.rbf_features(c["X"], c["omega"], c["offset"], c["ls"], c["var"])
        S = rr.rbf_sine_features(c["X"], c["omega"], c["offset"], c["ls"], c["var"])
        Pn = rr.rbf_features(c["Xs"], c["omega"], c["offset"], c["ls"], c["var"])
        mean, cov = rr.predict(Phi, c["Y"], c["s"], Pn, full_cov=True)
        _REF[key] = dict(c=c, Phi=Phi, lml=rr.lml(Phi, c["Y"], c["s"]), mean=mean, cov=cov, var=np.diag(cov).copy(),
                         grad=rr.lml_grad(Phi, c["Y"], c["s"], c["var"], S=S, X=c["X"], omega=c["omega"], ls=c["ls"]))
    return _REF[key]


# ---- the feature maps ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,F", FEATURE_SHAPES)
def test_feature_maps(handle, N, D, F):
    ks = _gpf().kernel_kitchen_sink
    c = rr.case(N, D, F, 1, D > 1, seed=11 * N + F, Ns=max(1, N // 3 + 2))
    X, X2 = c["X"], c["Xs"]
    maps = [(_sampler(c), lambda Z: rr.rbf_features(Z, c["omega"], c["offset"], c["ls"], c["var"])),
            (ks.LinearSampler(D, var=0.7, n_components=F), lambda Z: rr.linear_features(Z, 0.7, F)),
            (ks.ConstantSampler(D, var=1.9, n_components=F), lambda Z: rr.constant_features(Z, 1.9, F))]
    for sampler, ref in maps:
        Phi, Phi2 = ref(X), ref(X2)
        out = sampler.transform(X)
        assert out.shape == (N, F)
        assert np.abs(out - Phi).max() <= 1e-12, type(sampler).__name__
        k = ks.SamplerKernel(sampler)
        assert np.array_equal(k.features(X), out)                                  # bitwise between calls
        scale = max(1.0, np.abs(Phi @ Phi.T).max())
        assert np.abs(k.K(X) - Phi @ Phi.T).max() <= 1e-12 * scale
        K12 = k.K(X, X2)                                                           # non-square: padding must not leak
        assert K12.shape == (N, X2.shape[0])
        assert np.abs(K12 - Phi @ Phi2.T).max() <= 1e-12 * scale
        assert np.abs(k.Kdiag(X) - np.sum(Phi * Phi, axis=1)).max() <= 1e-12 * scale


def test_features_match_the_50_digit_fixture(handle):
    r = _reference(CASES[0])
    out = _sampler(r["c"]).transform(r["c"]["X"])
    assert np.abs(out - r["c"]["golden"]["Phi"]).max() <= 1e-12


# ---- likelihood, prediction, gradient --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,F,R,ard", CASES)
def test_lml_predict_gradient(handle, N, D, F, R, ard):
    r = _reference((N, D, F, R, ard))
    c = r["c"]
    desc, keep = _sampler(c)._descriptor()
    res = {}
    for chunk in (0, 256):
        lml = handle.rff_lml(desc, c["X"], c["s"], c["Y"], chunk_rows=chunk)
        mean, var = handle.rff_predict(desc, c["X"], c["s"], c["Y"], c["Xs"], chunk_rows=chunk)
        _, cov = handle.rff_predict(desc, c["X"], c["s"], c["Y"], c["Xs"], full_cov=True, chunk_rows=chunk)
        grad = handle.rff_lml_grad(desc, c["X"], c["s"], c["Y"], chunk_rows=chunk)
        print("chunk %d: lml %.3e mean %.3e var %.3e cov %.3e | grad lml %.3e var %.3e ls %.3e noise %.3e kinv %.3e" % (
            chunk, _rel(lml, r["lml"]), _rel(mean, r["mean"]), _rel(var, r["var"]), _rel(cov, r["cov"]), _rel(grad[0], r["lml"]),
            _rel(grad[1], r["grad"][0]), _rel(grad[2], r["grad"][1]), _rel(grad[3], r["grad"][2]), _rel(grad[4], r["grad"][3])))
        assert _rel(lml, r["lml"]) <= 1e-8 and _rel(grad[0], r["lml"]) <= 1e-8
        assert _rel(mean, r["mean"]) <= 1e-8 and _rel(var, r["var"]) <= 1e-8 and _rel(cov, r["cov"]) <= 1e-8
        assert _rel(grad[1], r["grad"][0]) <= 1e-8 and _rel(grad[2], r["grad"][1]) <= 1e-8
        assert _rel(grad[3], r["grad"][2]) <= 1e-8 and _rel(grad[4], r["grad"][3]) <= 1e-8
        # the same chunking again: bitwise
        assert handle.rff_lml(desc, c["X"], c["s"], c["Y"], chunk_rows=chunk) == lml
        again = handle.rff_lml_grad(desc, c["X"], c["s"], c["Y"], chunk_rows=chunk)
        assert again[0] == grad[0] and again[1] == grad[1] and again[3] == grad[3]
        assert np.array_equal(again[2], grad[2]) and np.array_equal(again[4], grad[4])
        res[chunk] = (lml, mean, var, cov) + grad[1:]
    for a, b in zip(res[0], res[256]):
        assert _rel(a, b) <= 1e-12
    if "golden" in c:
        g, (lml, mean, var, cov, gv, gl, gs, _) = c["golden"], res[0]
        assert _rel(lml, g["lml"]) <= 1e-8 and _rel(mean, g["mean"]) <= 1e-8 and _rel(cov, g["cov"]) <= 1e-8
        assert _rel(gv, g["grad_variance"]) <= 1e-8 and _rel(gl, g["grad_ls"]) <= 1e-8 and _rel(gs, g["grad_noise"]) <= 1e-8


def test_model_gradients_in_parameter_order(handle):
    """Through GPR with a Linear mean function and a scalar ls: the chain rule of the transforms and of the mean function,
    against central differences of the model's own likelihood (h = 1e-6 in the unconstrained values: 1e-6 relative)."""
    gpf = _gpf()
    c = rr.case(200, 3, 48, 2, False, seed=4)
    k = gpf.kernel_kitchen_sink.SamplerKernel(_sampler(c))
    m = gpf.models.GPR(c["X"], c["Y"], k, mean_function=gpf.mean_functions.Linear(np.zeros((3, 2)), np.zeros(2)), obs_var=c["s"])
    lml, grads = m.compute_log_likelihood_and_gradients()
    assert [p for p, _ in grads] == list(m.parameters)
    assert _rel(lml, m.compute_log_likelihood()) <= 1e-12
    for p, g in grads:
        flat = p.vf_val.reshape(-1).copy()
        for i in range(min(flat.size, 3)):
            vals = []
            for sgn in (1.0, -1.0):
                u = flat.copy()
                u[i] += sgn * 1e-6
                p.assign_unconstrained(u.reshape(p.vf_val.shape))
                vals.append(m.compute_log_likelihood())
            p.assign_unconstrained(flat.reshape(p.vf_val.shape))
            assert _rel(np.reshape(g, -1)[i], (vals[0] - vals[1]) / 2e-6) <= 1e-6, (p.name, i)


# ---- structural: the feature branch against the exact branch on K = Phi Phi^T ------------------------------------------------------
def test_feature_branch_equals_exact_branch_on_the_same_kernel_matrix(handle):
    """models/gpr.py:135-203 through the public API at N = 300, F = 40."""
    gpf = _gpf()
    c = rr.case(300, 4, 40, 2, True, seed=8, Ns=9)
    k = gpf.kernel_kitchen_sink.SamplerKernel(_sampler(c))
    m = gpf.models.GPR(c["X"], c["Y"], k, obs_var=c["s"])
    lml = m.compute_log_likelihood()
    mean, var = m.predict_f(c["Xs"])
    _, cov = m.predict_f_full_cov(c["Xs"])
    assert mean.shape == (9, 2) and var.shape == (9, 2) and cov.shape == (9, 9, 2)
    # the exact branch: L = chol(K + s I) by gps_potrf, the density and the solves by the host-matrix entries
    K, Kx, Kss = k.K(c["X"]), k.K(c["X"], c["Xs"]), k.K(c["Xs"])
    L = np.tril(handle.potrf(K + c["s"] * np.eye(300)))
    assert _rel(lml, gpf.densities.multivariate_normal(c["Y"], 0.0, L)) <= 1e-8
    A = handle.trsm_lower(L, Kx)
    V = handle.trsm_lower(L, c["Y"])
    assert _rel(mean, A.T @ V) <= 1e-8
    assert _rel(var[:, 0], np.diag(Kss) - np.sum(A * A, axis=0)) <= 1e-8 and np.array_equal(var[:, 0], var[:, 1])
    assert _rel(cov[:, :, 1], Kss - A.T @ A) <= 1e-8


@pytest.mark.parametrize("R", [1, 3])
def test_multivariate_normal_feature_equals_multivariate_normal(handle, R):
    """densities.py:159-174"""
    gpf = _gpf()
    rng = np.random.default_rng(R)
    C, x, mu, var = rng.normal(size=(20, 5)), rng.normal(size=(20, R)), rng.normal(size=(20, R)), 0.3
    L = np.tril(handle.potrf(C @ C.T + var * np.eye(20)))
    a = gpf.densities.multivariate_normal_feature(x, mu, C, var)
    assert _rel(a, gpf.densities.multivariate_normal(x, mu, L)) <= 1e-8
    assert _rel(a, rr.lml(C, x - mu, var)) <= 1e-8


# ---- reuse_factor ------------------------------------------------------------------------------------------------------------------
def test_warm_predict_is_bitwise_the_cold_one_and_follows_the_parameters(handle):
    gpf = _gpf()
    c = rr.case(300, 4, 40, 1, True, seed=9)
    s = _sampler(c)
    m = gpf.models.GPR(c["X"], c["Y"], gpf.kernel_kitchen_sink.SamplerKernel(s), obs_var=c["s"])
    cold = m.predict_f(c["Xs"])
    m.reuse_factor = True
    m.compute_log_likelihood()
    assert m._factor_key == m._state_key()
    warm = m.predict_f(c["Xs"])
    assert np.array_equal(cold[0], warm[0]) and np.array_equal(cold[1], warm[1])
    s._ls.assign(c["ls"] * 1.5)                                     # a changed ls invalidates the factor
    assert m._factor_key != m._state_key()
    moved = m.predict_f(c["Xs"])
    Phi = rr.rbf_features(c["X"], c["omega"], c["offset"], c["ls"] * 1.5, c["var"])
    Pn = rr.rbf_features(c["Xs"], c["omega"], c["offset"], c["ls"] * 1.5, c["var"])
    mean, var = rr.predict(Phi, c["Y"], c["s"], Pn)
    assert _rel(moved[0], mean) <= 1e-8 and _rel(moved[1][:, 0], var) <= 1e-8
    assert not np.array_equal(moved[0], warm[0])


# ---- fit ---------------------------------------------------------------------------------------------------------------------------------
def test_five_optimizer_steps_increase_the_likelihood(handle):
    gpf = _gpf()
    c = rr.case(500, 2, 64, 1, False, seed=12)
    s = _sampler(c)
    s._ls.assign(3.0)
    m = gpf.models.GPR(c["X"], c["Y"], gpf.kernel_kitchen_sink.SamplerKernel(s), obs_var=0.5)
    before, ls0 = m.compute_log_likelihood(), float(np.squeeze(s.ls))
    m.optimize(max_iter=5)
    after = m.compute_log_likelihood()
    assert after > before and abs(float(np.squeeze(s.ls)) - ls0) > 1e-6


# ---- what is not there, and failure --------------------------------------------------------------------------------------------------------
def test_unsupported_names_raise(handle):
    gpf = _gpf()
    ks = gpf.kernel_kitchen_sink
    a, b = ks.RBFSampler(2, n_components=4), ks.LinearSampler(2)
    with pytest.raises(NotImplementedError, match="RBFSampler, LinearSampler and ConstantSampler"):
        ks.EqApproxSumSampler([a, b], [0.5, 0.5], 4)
    with pytest.raises(NotImplementedError, match="RBFSampler, LinearSampler and ConstantSampler"):
        ks.SamplerKernel(a) + gpf.kernels.RBF(2)


def test_vanishing_noise_with_more_features_than_points_is_loud(handle):
    """s = 1e-300, F > N: A = Phi^T Phi + s I is singular to working precision.  Either the factorisation goes through and the
    value is finite, or NotPositiveDefiniteError is raised: never a silent NaN."""
    gpf = _gpf()
    c = rr.case(50, 4, 200, 1, True, seed=50)
    desc, keep = _sampler(c)._descriptor()
    try:
        lml = handle.rff_lml(desc, c["X"], 1e-300, c["Y"])
    except gpf.NotPositiveDefiniteError:
        return
    assert np.isfinite(lml)


# ---- the named problems of _rff_ref.CASES: every entry against the long-double form ---------------------------------------------------
# (tests/test_rff_ref_cpu.py: the fp64 restatement is within 1e-10 of that form on each of them, so 1e-8 here is the device's)
_NAMED = {}
_KEYS = ("lml", "mean", "var", "cov", "g_var", "g_ls", "g_s", "kinv")


def _named(name):
    """(case, long-double reference dict): computed once per name and shared."""
    if name not in _NAMED:
        c = rr.named_case(name)
        _NAMED[name] = (c, rr.reference_of(c, ld=True))
    return _NAMED[name]


def _desc(c):
    """The case's descriptor with the case's own numbers (no round trip through a Parameter's transform)."""
    be = _gpf()._backend
    D, F = c["X"].shape[1], c["F"]
    if c["kind"] == "explicit":
        return be.make_rff(be.RFF_EXPLICIT, F, F)
    if c["kind"] == "rbf":
        return be.make_rff(be.RFF_RBF, D, F, c["var"], ls=c["ls"], omega=c["omega"], offset=c["offset"])
    return be.make_rff(be.RFF_LINEAR if c["kind"] == "linear" else be.RFF_CONSTANT, D, F, c["var"])


def _io(c):
    """(X, Xnew) as the device entries take them: the points, or for explicit features the host feature matrices."""
    if c["kind"] == "explicit":
        return rr.features_of(c, c["X"]), rr.features_of(c, c["Xs"])
    return c["X"], c["Xs"]


def _run(handle, c, chunk, Y=None):
    """One cold pass through gps_rff_lml, _predict (both forms) and _lml_grad, keyed like the reference dict."""
    (desc, keep), (X, Xs), Y = _desc(c), _io(c), c["Y"] if Y is None else Y
    out = {"lml": handle.rff_lml(desc, X, c["s"], Y, chunk_rows=chunk)}
    out["mean"], out["var"] = handle.rff_predict(desc, X, c["s"], Y, Xs, chunk_rows=chunk)
    out["mean_full"], out["cov"] = handle.rff_predict(desc, X, c["s"], Y, Xs, full_cov=True, chunk_rows=chunk)
    out["lml_grad"], out["g_var"], out["g_ls"], out["g_s"], out["kinv"] = handle.rff_lml_grad(desc, X, c["s"], Y, chunk_rows=chunk)
    return out


def _between(a, b):
    """Worst _rel over the quantities of two runs (an empty gls has none)."""
    return max(_rel(a[k], b[k]) for k in a if np.size(a[k]))


def _deviations(out, ref):
    dev = {k: _rel(out[k], ref[k]) for k in _KEYS if k in ref}
    dev["lml_grad"], dev["mean_full"] = _rel(out["lml_grad"], ref["lml"]), _rel(out["mean_full"], ref["mean"])
    return dev


def _check(handle, name, chunks=(0, 128)):
    """Every returned quantity of the named case within 1e-8 of the long-double form under each chunking, diag(cov) within 1e-12 of
    the diagonal call, a repeated pass bitwise, the chunkings within 1e-12 of each other.  Returns the runs by chunking."""
    c, ref = _named(name)
    runs = {}
    for chunk in chunks:
        out = _run(handle, c, chunk)
        dev = _deviations(out, ref)
        diag = _rel(np.diag(out["cov"]), out["var"])
        print("%s chunk %d: %s | diag(cov) vs var %.2e" % (name, chunk, " ".join("%s %.2e" % kv for kv in dev.items()), diag))
        for k, v in dev.items():
            assert np.shape(out[k]) == np.shape(ref[{"lml_grad": "lml", "mean_full": "mean"}.get(k, k)]), (name, k)
            assert v <= 1e-8, (name, chunk, k, v)
        assert diag <= 1e-12, (name, chunk, diag)
        if c["kind"] != "rbf":
            assert out["g_ls"].size == 0
        if c["kind"] == "explicit":
            assert out["g_var"] == 0.0
        again = _run(handle, c, chunk)
        for k in out:
            assert np.array_equal(out[k], again[k]), (name, chunk, k)
        runs[chunk] = out
    worst = _between(runs[chunks[0]], runs[chunks[-1]])
    print("%s between chunkings: %.2e" % (name, worst))
    assert worst <= 1e-12, (name, worst)
    return runs


# ---- gap 1: the Linear and Constant samplers beyond the feature map -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["linear-5", "linear-13", "linear-d32", "constant-1", "constant-33"])
def test_linear_and_constant_samplers(handle, name):
    """Gap 1 (and, "linear-d32", gap 4: D = 32 staged by the Linear map).  gps_rff_lml, _predict (diagonal and full_cov) and
    _lml_grad with St, XT and Tm null: rff_grad_contract_kernel without a sine buffer, grad_var through the c1 of rff_upload_desc,
    kinv_resid and grad_noise; the returned gls is empty.  "linear-13": tiled duplicate columns, Phi^T Phi of rank 5;
    "linear-d32" / "constant-33": F across a 32-feature workgroup."""
    _check(handle, name)


@pytest.mark.parametrize("kind", ["linear", "constant"])
def test_sampler_model_equals_the_exact_kernel(handle, kind):
    """Gap 1, without tests/_rff_ref.py: tile(X) sqrt(var D / F) has Phi Phi^T = var X X^T whenever F is a multiple of D, and
    ones sqrt(var / F) has var 1 1^T, so GPR over the sampler (Woodbury branch) and GPR over kernels.Linear / kernels.Constant
    (exact branch, N = 200) are the same model: likelihood, both predictions, and the variance and noise gradients to 1e-8."""
    gpf = _gpf()
    ks = gpf.kernel_kitchen_sink
    D, var = 4, 0.7
    c = rr.case(200, D, 2 * D, 2, True, seed=21, Ns=9)
    if kind == "linear":
        sk, ek = ks.SamplerKernel(ks.LinearSampler(D, var, n_components=2 * D)), gpf.kernels.Linear(D, variance=var)
    else:
        sk, ek = ks.SamplerKernel(ks.ConstantSampler(D, var, n_components=2 * D)), gpf.kernels.Constant(D, variance=var)
    got, want = [], []
    for kern, res in ((sk, got), (ek, want)):
        m = gpf.models.GPR(c["X"], c["Y"], kern, obs_var=c["s"])
        assert m._has_features() == (kern is sk)
        res.append(m.compute_log_likelihood())
        res.extend(m.predict_f(c["Xs"]))
        res.append(m.predict_f_full_cov(c["Xs"])[1])
        lml, grads = m.compute_log_likelihood_and_gradients()
        assert [p.name for p, _ in grads] == ["variance", "variance"] and grads[1][0] is m.likelihood._variance
        res.extend([lml, np.asarray(grads[0][1]), np.asarray(grads[1][1])])
    dev = [_rel(a, b) for a, b in zip(got, want)]
    print("%s sampler vs exact kernel: lml %.2e mean %.2e var %.2e cov %.2e | grad lml %.2e variance %.2e noise %.2e" % ((kind,) + tuple(dev)))
    assert got[3].shape == (9, 9, 2) and max(dev) <= 1e-8, dev


# ---- gap 2: many outputs -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["r5", "r8", "r128", "r5-f130"])
def test_many_outputs(handle, name):
    """Gap 2: R > 4 takes the second body of rff_grad_contract_kernel (Et re-read from global memory, LDS of r * 32 doubles) and
    R = 128 fills all GPS_TILE rows of V, C, Xr and Et.  Column q of the R = 8 run equals the R = 1 run on that column (1e-12)."""
    runs = _check(handle, name)
    if name == "r8":
        c, _ = _named(name)
        worst = 0.0
        for chunk in (0, 128):
            for q in range(8):
                one = _run(handle, c, chunk, Y=np.ascontiguousarray(c["Y"][:, q:q + 1]))
                worst = max(worst, _rel(one["mean"][:, 0], runs[chunk]["mean"][:, q]), _rel(one["kinv"][:, 0], runs[chunk]["kinv"][:, q]))
        print("r8 column by column against R = 1, both chunkings: %.2e" % worst)
        assert worst <= 1e-12


def test_more_than_128_outputs_are_refused(handle):
    """Gap 2: R = 129 is refused by the host before any launch."""
    c, _ = _named("r5")
    desc, keep = _desc(c)
    Y = np.zeros((c["X"].shape[0], 129))
    launches = handle.profile_get("rff_features")["launches"]
    for call in (lambda: handle.rff_lml(desc, c["X"], c["s"], Y), lambda: handle.rff_lml_grad(desc, c["X"], c["s"], Y),
                 lambda: handle.rff_predict(desc, c["X"], c["s"], Y, c["Xs"])):
        with pytest.raises(RuntimeError, match="at most 128 outputs"):
            call()
    assert handle.profile_get("rff_features")["launches"] == launches


# ---- gaps 3 and 7: predictions wider than one tile or one chunk, warm after a gradient ----------------------------------------------------
def test_wide_predictions(handle):
    """Gap 3: (300, 4, 130, 2, ard) with up to 300 prediction points.  At chunk_rows = 128 the c0 += pc loop of rff_predict_tail
    makes 1, 2 (one-row last chunk) and 3 (partial last chunk) trips for Ns = 128, 129, 300 -- counted by the launches of the
    feature kernel on a warm call -- and full_cov extracts from a padded [256][256] and [384][384] product; diag(cov) against the
    diagonal call to 1e-12.  At s = 0.15 every diagonal block of the factor is classified well conditioned: the prediction's
    solve takes plain leaves only (classify_blocks after the factorisation in rff_forward).  The launch and leaf counts are
    assertions about the PATH taken, not about a value: the leaf counts rest on "leaf_plain_kappa" = 1000 and on the condition
    estimate of the two diagonal blocks of this case (cond(A) = 6e2, far below it); a retuning of either that makes a block of
    this case refined has to revisit them."""
    c, ref = _named("wide")
    desc, keep = _desc(c)
    X, Y, s = c["X"], c["Y"], c["s"]
    count = lambda k: handle.profile_get(k)["launches"]
    for chunk in (0, 128):
        for ns in (128, 129, 300):
            mean, var = handle.rff_predict(desc, X, s, Y, c["Xs"][:ns], chunk_rows=chunk)
            dm, dv = _rel(mean, ref["mean"][:ns]), _rel(var, ref["var"][:ns])
            line = "wide chunk %d Ns %d: mean %.2e var %.2e" % (chunk, ns, dm, dv)
            assert mean.shape == (ns, 2) and var.shape == (ns,) and dm <= 1e-8 and dv <= 1e-8, line
            f0, p0, r0 = count("rff_features"), count("leaves_plain"), count("leaves_refined")
            warm = handle.rff_predict(desc, X, s, Y, c["Xs"][:ns], refactor=False, chunk_rows=chunk)
            assert np.array_equal(warm[0], mean) and np.array_equal(warm[1], var)
            assert count("rff_features") - f0 == (-(-ns // 128) if chunk else 1), line
            assert count("leaves_plain") > p0 and count("leaves_refined") == r0, line
            if ns > 128:
                mean_f, cov = handle.rff_predict(desc, X, s, Y, c["Xs"][:ns], full_cov=True, chunk_rows=chunk)
                dc, dd = _rel(cov, ref["cov"][:ns, :ns]), _rel(np.diag(cov), var)
                line += " | full_cov mean %.2e cov %.2e diag(cov) vs var %.2e" % (_rel(mean_f, ref["mean"][:ns]), dc, dd)
                assert cov.shape == (ns, ns) and _rel(mean_f, ref["mean"][:ns]) <= 1e-8 and dc <= 1e-8 and dd <= 1e-12, line
                assert np.array_equal(cov, cov.T) or _rel(cov, cov.T) <= 1e-12
            print(line)


def test_warm_predict_after_a_gradient(handle):
    """Gap 7: rff_grad_body reuses dFeat, dB, dMean and dS1; the resident dK, dLinv and dAlpha survive it.  After rff_lml_grad,
    rff_predict(refactor=False) at Ns = 300, chunk_rows = 128 (three trips) is bitwise the cold call, in both forms; a descriptor
    of another F is refused ("no resident factor")."""
    c, ref = _named("wide")
    desc, keep = _desc(c)
    X, Y, s, Xs = c["X"], c["Y"], c["s"], c["Xs"]
    cold = handle.rff_predict(desc, X, s, Y, Xs, chunk_rows=128)
    cold_full = handle.rff_predict(desc, X, s, Y, Xs, full_cov=True, chunk_rows=128)
    grad = handle.rff_lml_grad(desc, X, s, Y, chunk_rows=128)
    warm = handle.rff_predict(desc, X, s, Y, Xs, refactor=False, chunk_rows=128)
    warm_full = handle.rff_predict(desc, X, s, Y, Xs, full_cov=True, refactor=False, chunk_rows=128)
    print("warm after gradient: lml %.2e mean %.2e var %.2e cov %.2e" % (
        _rel(grad[0], ref["lml"]), _rel(warm[0], ref["mean"]), _rel(warm[1], ref["var"]), _rel(warm_full[1], ref["cov"])))
    assert _rel(warm[0], ref["mean"]) <= 1e-8 and _rel(warm[1], ref["var"]) <= 1e-8 and _rel(warm_full[1], ref["cov"]) <= 1e-8
    assert np.array_equal(warm[0], cold[0]) and np.array_equal(warm[1], cold[1])
    assert np.array_equal(warm_full[0], cold_full[0]) and np.array_equal(warm_full[1], cold_full[1])
    be = _gpf()._backend
    other, keep2 = be.make_rff(be.RFF_RBF, 4, 129, c["var"], ls=c["ls"], omega=c["omega"][:, :129], offset=c["offset"][:129])
    with pytest.raises(RuntimeError, match="no resident factor"):
        handle.rff_predict(other, X, s, Y, Xs, refactor=False, chunk_rows=128)
    again = handle.rff_predict(desc, X, s, Y, Xs, refactor=False, chunk_rows=128)         # the refusal left the factor alone
    assert np.array_equal(again[0], cold[0]) and np.array_equal(again[1], cold[1])


# ---- gap 4: the input-dimension limit and the chunk edges ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d32", "n256", "n129", "n1"])
def test_limits_and_chunk_edges(handle, name):
    """Gap 4.  "d32": GPS_RFF_MAX_DIMS = 32 input dimensions, all 32 lengthscale slots, 41 KB of dynamic LDS in rff_feature_kernel;
    "n256": N an exact multiple of chunk_rows = 128 (no partial chunk); "n129": a one-row last chunk; "n1": a single point."""
    _check(handle, name)


def test_more_than_32_input_dimensions_are_refused(handle):
    """Gap 4: D = 33 is refused for the RBF and the Linear map, by every entry."""
    gpf = _gpf()
    be, ks = gpf._backend, gpf.kernel_kitchen_sink
    c = rr.case(40, 33, 8, 1, True, seed=33)
    rbf, keep = be.make_rff(be.RFF_RBF, 33, 8, c["var"], ls=c["ls"], omega=c["omega"], offset=c["offset"])
    lin, keep2 = be.make_rff(be.RFF_LINEAR, 33, 8, c["var"])
    for desc in (rbf, lin):
        for call in (lambda: handle.rff_lml(desc, c["X"], c["s"], c["Y"]), lambda: handle.rff_lml_grad(desc, c["X"], c["s"], c["Y"]),
                     lambda: handle.rff_predict(desc, c["X"], c["s"], c["Y"], c["Xs"]), lambda: handle.rff_features(desc, c["X"])):
            with pytest.raises(RuntimeError, match="at most 32 input dimensions"):
                call()
    with pytest.raises(RuntimeError, match="at most 32 input dimensions"):
        ks.LinearSampler(33).transform(c["X"])


# ---- gap 5: explicit features ----------------------------------------------------------------------------------------------------------
def test_explicit_features(handle):
    """Gap 5: make_rff(RFF_EXPLICIT, 37, 37) on host matrices C [300, 37] (F no multiple of 32; three chunks at chunk_rows = 128)
    and Cnew [130, 37]: rff_lml_grad (lml, grad_noise, kinv_resid; grad_var == 0.0), rff_predict in both forms."""
    _check(handle, "explicit")


def test_kernel_with_features_and_no_sampler(handle):
    """Gap 5: the fallback of models/gpr.py:_rff for a kernel that has ``features`` and no sampler -- the features go to the device
    as explicit host matrices.  Likelihood and prediction agree with the low-level calls; gradients are not available."""
    gpf = _gpf()
    c, ref = _named("explicit")

    class FeatureKernel(gpf.kernels.Kernel):
        def __init__(self):
            gpf.kernels.Kernel.__init__(self, input_dim=4)

        def features(self, X):
            return rr.features_of(c, np.asarray(X))

    m = gpf.models.GPR(c["X"], c["Y"], FeatureKernel(), obs_var=c["s"])
    assert m._has_features() and [p.name for p in m.parameters] == ["variance"]
    s = float(np.squeeze(m.likelihood.variance))                 # (the value after the round trip through the transform)
    (desc, keep), (C, Cnew) = _desc(c), _io(c)
    lml = m.compute_log_likelihood()
    mean, var = m.predict_f(c["Xs"])
    _, cov = m.predict_f_full_cov(c["Xs"])
    low_mean, low_var = handle.rff_predict(desc, C, s, c["Y"], Cnew)
    assert lml == handle.rff_lml(desc, C, s, c["Y"])
    assert np.array_equal(mean, low_mean) and var.shape == (130, 2) and np.array_equal(var[:, 0], low_var) and np.array_equal(var[:, 1], low_var)
    assert cov.shape == (130, 130, 2) and np.array_equal(cov[:, :, 1], handle.rff_predict(desc, C, s, c["Y"], Cnew, full_cov=True)[1])
    print("feature-only kernel: lml %.2e mean %.2e var %.2e cov %.2e" % (
        _rel(lml, ref["lml"]), _rel(mean, ref["mean"]), _rel(var[:, 0], ref["var"]), _rel(cov[:, :, 0], ref["cov"])))
    assert _rel(lml, ref["lml"]) <= 1e-8 and _rel(mean, ref["mean"]) <= 1e-8 and _rel(cov[:, :, 0], ref["cov"]) <= 1e-8
    with pytest.raises(NotImplementedError, match="kernel_kitchen_sink sampler"):
        m.compute_log_likelihood_and_gradients()


# ---- gap 6: low noise ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", [{}, {"leaf_plain_kappa": 0.0}, {"trsv_wave_refine": 0}], ids=["defaults", "every-leaf-refined", "recursive-trsv"])
@pytest.mark.parametrize("name", ["low-257", "low-300"])
def test_low_noise(handle, name, options):
    """Gap 6: s = 1e-5, cond(A) ~ 1e7 (Fp = 384: three diagonal blocks; Ns = 40).  Everything lml, predict and lml_grad return
    against the LONG-DOUBLE form at 1e-8 (the fp64 restatement is within 5.1e-11 of it), under the defaults (classify_blocks
    decides per block; the refined wavefront substitution at Fp >= 256), with every leaf refined ("leaf_plain_kappa" = 0: the
    refined leaves of the prediction's trsm_rec and of L^-T) and with the recursive substitution over refined leaves
    ("trsv_wave_refine" = 0).  After each pass a warm prediction (only the leaves of its trsm_rec are counted) is bitwise the
    cold one and shows the path: under the defaults classify_blocks finds an ill-conditioned diagonal block on both cases and
    the solve against it is refined (a path assertion: it rests on "leaf_plain_kappa" = 1000 and the condition estimate); with
    "leaf_plain_kappa" = 0 no leaf is plain.
    The two chunkings are held to rr.chunking_bound = eps cond(A) (3.9e-9 on "low-257", 2.0e-9 on "low-300"), not to the 1e-12 of
    the cases at s = 0.15: they sum A = Phi^T Phi in a different order, and that alone moves the answer by more than 1e-12
    here.  tests/test_rff_ref_cpu.py::test_what_the_order_of_summation_of_A_moves: A summed in fp64 in one product or in chunks
    of 128 rows (1.4e-15 |A| apart) and every later step in long double moves the mean by 2.2e-11 ("low-257") and 2.4e-11
    ("low-300"); the same experiment at s = 0.15 ("wide") gives 7.6e-15.  Measured on the device: 2.4e-11 and 4.2e-11."""
    c, ref = _named(name)
    defaults = {"leaf_plain_kappa": 1000.0, "trsv_wave_refine": 1}
    count = lambda k: handle.profile_get(k)["launches"]
    runs = {}
    try:
        for k, v in options.items():
            handle.set_option(k, v)
        for chunk in (0, 128):
            p0, r0 = count("leaves_plain"), count("leaves_refined")
            out = _run(handle, c, chunk)
            plain, refined = count("leaves_plain") - p0, count("leaves_refined") - r0
            dev = _deviations(out, ref)
            print("%s %s chunk %d: %s | leaves plain %d refined %d" % (name, options, chunk, " ".join("%s %.2e" % kv for kv in dev.items()),
                                                                     plain, refined))
            for k, v in dev.items():
                assert v <= 1e-8, (name, options, chunk, k, v)
            if "leaf_plain_kappa" in options:
                assert plain == 0 and refined > 0
            again = _run(handle, c, chunk)
            for k in out:
                assert np.array_equal(out[k], again[k]), (name, options, chunk, k)
            runs[chunk] = out
            # the factor of the gradient call is resident: a warm prediction runs the solve against it and nothing else
            (desc, keep), (X, Xs) = _desc(c), _io(c)
            p0, r0 = count("leaves_plain"), count("leaves_refined")
            warm = handle.rff_predict(desc, X, c["s"], c["Y"], Xs, refactor=False, chunk_rows=chunk)
            plain, refined = count("leaves_plain") - p0, count("leaves_refined") - r0
            print("%s %s chunk %d: warm prediction leaves plain %d refined %d" % (name, options, chunk, plain, refined))
            assert np.array_equal(warm[0], out["mean"]) and np.array_equal(warm[1], out["var"])
            assert refined > 0 and (plain == 0 or "leaf_plain_kappa" not in options)
        worst, bound = _between(runs[0], runs[128]), rr.chunking_bound(c)
        print("%s %s between chunkings: %.2e (bound %.1e)" % (name, options, worst, bound))
        assert worst <= bound, (name, options, worst, bound)
    finally:
        for k, v in defaults.items():
            handle.set_option(k, v)
