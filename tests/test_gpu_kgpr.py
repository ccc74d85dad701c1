"""GPU tests of Kronecker GP regression (csrc/kron.hip, csrc/gps_kgpr.hip, gpflowSlim/conjugate_gradient.py,
gpflowSlim/models/kgpr.py) against tests/_kgpr_ref.py (tests/test_kgpr_ref_cpu.py checks that restatement), the dense form where
N = m n <= 600, and the 50-digit fixture tests/golden/mp/kgpr.npz.

The CG iterate is ill conditioned with respect to rounding although the converged solution is not (test_kgpr_ref_cpu.py has the
figures), so parity is asserted on short runs (five iterations: the recurrence, 1e-10) and on converged runs (tol 1e-20, 400
iterations allowed: the project's usual 1e-8 max(1, |value|)); at the reference's defaults (tol 1e-6, 100 iterations) only the
structure of the result and a value gate drawn from the restatement's own spread are asserted.

Cases kr.CASES = (m, n, masked fraction, input span): the smallest that cross the 128-tile padding in either dimension
(129 x 130, 300 x 260, 257 x 3), have a degenerate dimension (1 x 1, 1 x 200, 257 x 3), have M = N (the unmasked 24 x 20) and
give spectra with negative eigenvalues (300 x 260, 1 x 200)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _kgpr_ref as kr  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TH = kr.THETA
EPS = np.finfo(float).eps
case_ids = lambda c: "%dx%d-%g" % c[:3]  # noqa: E731


def _rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def _gpf():
    import gpflowSlim as gpf
    return gpf


def _model(X1, X2, Y, mask, th=TH, **kw):
    gpf = _gpf()
    k1 = gpf.kernels.RBF(X1.shape[1], variance=th["var1"], lengthscales=th["ls1"])
    k2 = gpf.kernels.RBF(X2.shape[1], variance=th["var2"], lengthscales=th["ls2"])
    return gpf.models.KGPR(X1, X2, Y, k1, k2, mask, obs_var=th["s2"], **kw)


@functools.lru_cache(maxsize=None)
def _ref(case):
    """Everything the tests of one case share, computed once on the host and left unchanged."""
    X1, X2, Y, mask = kr.make_case(*case)
    K1, K2 = kr.kernels(X1, X2)
    C = kr.noise_of(mask, TH["s2"]) ** -0.5
    rs = np.random.RandomState(7)
    Xn1, Xn2 = rs.uniform(0, case[3], (5, 2)), rs.uniform(0, case[3], (4, 1))
    return dict(X1=X1, X2=X2, Y=Y, mask=mask, K1=K1, K2=K2, C=C, b=C * Y, Xn1=Xn1, Xn2=Xn2)


@functools.lru_cache(maxsize=None)
def _converged(case):
    c = _ref(case)
    res = kr.lml(c["K1"], c["K2"], c["Y"], c["mask"], TH["s2"], 400, 1e-20)
    res["grad"] = kr.gradient(c["X1"], c["X2"], c["Y"], c["mask"], TH, res)
    res["mean"] = kr.predict(res["alpha"], kr.rbf(c["X1"], c["Xn1"], TH["var1"], TH["ls1"]),
                             kr.rbf(c["X2"], c["Xn2"], TH["var2"], TH["ls2"]))
    return res


def _device_grad(model):
    """(dict of kgpr_lml, gradient dict over var1, ls1, var2, ls2, s2 in the constrained values) through the C entry."""
    h = _gpf().get_handle()
    p1, p2 = model._programs()
    e1, e2, sel, V1, V2 = model._spectra(p1, p2, True)
    res, s1, s2, gn = h.kgpr_lml_grad(p1, model.X1, p2, model.X2, model.Y, model.mask, TH["s2"], e1, e2, sel, V1, V2,
                                      max_iter=model.cg_max_iter, tol=model.cg_tol)
    return res, dict(var1=s1[0], ls1=np.sum(s1[1:]), var2=s2[0], ls2=np.sum(s2[1:]), s2=gn)


# ---- short runs: the recurrence --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", kr.CASES, ids=case_ids)
def test_five_iterations_match_the_restatement(case, handle):
    """max_iter = 5: x, iters and r^T r at 1e-10 relative (the two association orders of the restatement differ by 2.4e-15 or
    less there).  r^T r below (4 eps |b|)^2 is rounding alone (the 1 x 1 grid converges in one step) and is held to that."""
    c = _ref(case)
    x, k, rr, delta = handle.kron_cg(c["K1"], c["K2"], c["b"], c["C"], max_iter=5, tol=1e-6)
    xr, kr_, rrr, dr = kr.cgsolver(c["K1"], c["K2"], c["b"], c["C"], 5, 1e-6)
    print("five iterations", case, "x", _rel(x, xr), "rr", rr, rrr)
    assert k == kr_
    assert np.abs(x - xr).max() <= 1e-10 * np.abs(xr).max()
    assert abs(rr - rrr) <= 1e-10 * rrr + (4 * EPS) ** 2 * np.sum(c["b"] ** 2)
    assert abs(delta - dr) <= 1e-14 * dr


# ---- converged runs --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", kr.CASES, ids=case_ids)
def test_converged_solution(case, handle):
    """tol = 1e-20, 400 iterations allowed: stops before 400, |b - A x| / |b| recomputed on the host <= 1e-9, x at 1e-8 against
    the restatement and, N <= 600, the dense solve."""
    c = _ref(case)
    x, k, rr, delta = handle.kron_cg(c["K1"], c["K2"], c["b"], c["C"], max_iter=400, tol=1e-20)
    res = kr.rel_residual(c["K1"], c["K2"], c["C"], c["b"], x)[0]
    print("converged", case, "iters", k, "residual", res, "x", _rel(x, _converged(case)["x"]))
    assert k < 400
    assert res <= 1e-9
    assert _rel(x, _converged(case)["x"]) <= 1e-8
    if case[0] * case[1] <= 600:
        assert _rel(x, kr.dense_lml(c["X1"], c["X2"], c["Y"], c["mask"], TH)["x"]) <= 1e-8


@pytest.mark.parametrize("case", kr.CASES, ids=case_ids)
def test_converged_likelihood_gradient_prediction(case):
    """The model at tol = 1e-20: LML, its terms, every gradient entry and the prediction at 1e-8 max(1, |value|) against the
    restatement; N <= 600: the LML against the dense form and the gradient against five-point differences of the dense LML
    (their own error: 3.8e-11, tests/test_kgpr_ref_cpu.py)."""
    c = _ref(case)
    ref = _converged(case)
    model = _model(c["X1"], c["X2"], c["Y"], c["mask"], cg_max_iter=400, cg_tol=1e-20)
    res, grad = _device_grad(model)
    print("converged model", case, {k: res[k] for k in ("lml", "iters", "rr")}, "ref lml", ref["lml"])
    assert res["iters"] < 400
    for key in ("lml", "quadratic", "logdet"):
        assert _rel(res[key], ref[key]) <= 1e-8, key
    for key in grad:
        print("  grad", key, grad[key], ref["grad"][key])
        assert _rel(grad[key], ref["grad"][key]) <= 1e-8, key
    mean = model.predict_f(c["Xn1"], c["Xn2"])
    assert mean.shape == (5, 4)
    assert _rel(mean, ref["mean"]) <= 1e-8
    assert _rel(model.compute_log_likelihood(), ref["lml"]) <= 1e-8
    if case[0] * case[1] <= 600:
        assert _rel(res["lml"], kr.dense_lml(c["X1"], c["X2"], c["Y"], c["mask"], TH)["lml"]) <= 1e-8
        fd = kr.dense_gradient_fd(c["X1"], c["X2"], c["Y"], c["mask"], TH)
        for key in grad:
            assert _rel(grad[key], fd[key]) <= 1e-8, key


def test_against_the_mpmath_fixture():
    """m, n = 3, 2 with one masked cell against 50 digits: LML, its terms, the gradient (mpmath.diff of the whole evaluation) and
    the prediction at 1e-8."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "mp", "kgpr.npz"))
    th = dict(zip(["var1", "ls1", "var2", "ls2", "s2"], (float(v) for v in g["theta"])))
    model = _model(g["X1"], g["X2"], g["Y"], g["mask"], th, cg_max_iter=400, cg_tol=1e-30)
    h = _gpf().get_handle()
    p1, p2 = model._programs()
    e1, e2, sel, V1, V2 = model._spectra(p1, p2, True)
    res, s1, s2, gn = h.kgpr_lml_grad(p1, model.X1, p2, model.X2, model.Y, model.mask, th["s2"], e1, e2, sel, V1, V2, 400, 1e-30)
    for key in ("lml", "quadratic", "logdet"):
        assert _rel(res[key], g[key]) <= 1e-8, key
    assert _rel([s1[0], np.sum(s1[1:]), s2[0], np.sum(s2[1:]), gn], g["grad"]) <= 1e-8
    assert _rel(model.predict_f(g["Xnew1"], g["Xnew2"]), g["mean"]) <= 1e-8
    x, _, _, _ = h.kron_cg(g["K1"], g["K2"], g["Y"] / np.sqrt(th["s2"] + 1e6 * g["mask"]), 1.0 / np.sqrt(th["s2"] + 1e6 * g["mask"]),
                           400, 1e-30)
    assert _rel(x, g["x"]) <= 1e-8


# ---- the reference's defaults -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _default_variants(case):
    """The restatement at tol 1e-6, 100 iterations in both association orders, in long double too where N <= 20 000."""
    c = _ref(case)
    out = []
    for order in ("k1_sk2", "k1s_k2"):
        for dt in ([np.float64, np.longdouble] if case[0] * case[1] <= 20000 else [np.float64]):
            out.append(kr.lml(c["K1"], c["K2"], c["Y"], c["mask"], TH["s2"], 100, 1e-6, order, dt))
    return out


@pytest.mark.parametrize("case", kr.CASES, ids=case_ids)
def test_defaults(case, handle):
    """tol = 1e-6, max_iter = 100: at most 100 iterations; the stop rule holds for the returned r^T r and delta; the returned
    r^T r is the residual recomputed on the host from the returned x -- to 100 times the gap the restatement itself shows, floor
    1e-10 relative, plus the rounding floor (4 eps |b|)^2 of any recomputed residual.  That gap, measured on the restatement
    (it moves with the host's BLAS: 2.1e-13 to 2.6e-12 on 300 x 260 between two machines):
    1.0e-12 (5 x 3), 5.0e-12 and 1.1e-11 (24 x 20, masked and not), 4.5e-12 (129 x 130), 2.6e-12 (300 x 260), 1.3e-14 (257 x 3),
    3.7e-13 (1 x 200); r^T r is exactly 0 on the 1 x 1 grid.
    The LML lies within 10 times the largest spread among the restatement's own variants (measured: 0 on 1 x 1, 5 x 3 and
    257 x 3, 4.0e-5 and 3.9e-5 on the 24 x 20 grids, 2.2e-11 on 129 x 130, 1.3e-7 on 300 x 260, 8.5e-8 on 1 x 200; a case
    counts only while that spread is <= 1e-3) -- or within the converged runs' gate 1e-8 max(1, |LML|), whichever is wider:
    device and numpy kernel matrices differ in the last bits, so no closer agreement can be asked than of a converged run."""
    c = _ref(case)
    x, k, rr, delta = handle.kron_cg(c["K1"], c["K2"], c["b"], c["C"])
    assert k <= 100
    assert not (delta < rr and k < 100)
    variants = _default_variants(case)
    r0 = variants[0]
    floor = (4 * EPS) ** 2 * np.sum(c["b"] ** 2)
    gap = abs(kr.rel_residual(c["K1"], c["K2"], c["C"], c["b"], r0["x"])[1] - r0["rr"]) / max(r0["rr"], floor)
    rec = kr.rel_residual(c["K1"], c["K2"], c["C"], c["b"], x)[1]
    print("defaults", case, "iters", k, "rr", rr, "recomputed", rec, "restatement gap", gap)
    assert abs(rr - rec) <= max(100 * gap, 1e-10) * rr + floor
    lmls = [v["lml"] for v in variants]
    spread = max(lmls) - min(lmls)
    assert spread <= 1e-3
    model = _model(c["X1"], c["X2"], c["Y"], c["mask"])
    lml = model.compute_log_likelihood()
    print("  lml", lml, "restatement", lmls, "spread", spread, "iters", model.last_solve["iters"])
    assert model.last_solve["iters"] <= 100
    assert abs(lml - r0["lml"]) <= max(10 * spread, 1e-8 * max(1.0, abs(r0["lml"])))


# ---- control -------------------------------------------------------------------------------------------------------------------------
CTRL = (129, 130, 0.3, 40.0)


def test_two_calls_are_bitwise_equal(handle):
    c = _ref(CTRL)
    a = handle.kron_cg(c["K1"], c["K2"], c["b"], c["C"])
    b = handle.kron_cg(c["K1"], c["K2"], c["b"], c["C"])
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]


def test_result_does_not_depend_on_check_every(handle):
    c = _ref(CTRL)
    outs = []
    try:
        for every in (1, 8, 1000):
            handle.set_option("kron_cg_check_every", every)
            outs.append(handle.kron_cg(c["K1"], c["K2"], c["b"], c["C"]))
    finally:
        handle.set_option("kron_cg_check_every", 8)
    for o in outs[1:]:
        assert o[1] == outs[0][1] and o[2] == outs[0][2]
        assert np.array_equal(o[0], outs[0][0])


def test_zero_iterations_and_zero_right_hand_side(handle):
    c = _ref((24, 20, 0.25, 4.0))
    x, k, rr, delta = handle.kron_cg(c["K1"], c["K2"], c["b"], c["C"], max_iter=0)
    assert k == 0 and not x.any()
    assert abs(rr - np.sum(c["b"] ** 2)) <= 1e-13 * rr
    x, k, rr, delta = handle.kron_cg(c["K1"], c["K2"], np.zeros_like(c["b"]), c["C"])
    assert k == 0 and rr == 0.0 and delta == 0.0
    assert np.all(np.isfinite(x)) and not x.any()


def test_everything_masked():
    """M = 0: nothing is selected, the log-determinant is empty and the likelihood is the quadratic term alone."""
    X1, X2, Y, mask = kr.make_case(5, 3, 0.0, 4.0)
    model = _model(X1, X2, Y, np.ones_like(mask), cg_max_iter=400, cg_tol=1e-20)
    lml = model.compute_log_likelihood()
    K1, K2 = kr.kernels(X1, X2)
    ref = kr.lml(K1, K2, Y, np.ones_like(mask), TH["s2"], 400, 1e-20)
    assert ref["M"] == 0 and ref["logdet"] == 0.0
    assert np.isfinite(lml) and _rel(lml, ref["lml"]) <= 1e-8
    _, grads = model.compute_log_likelihood_and_gradients()
    assert all(np.all(np.isfinite(g)) for _, g in grads)


def test_cgsolver_on_column_vectors_equals_the_models_solve(handle):
    """cgsolver on the reference's [N, 1] column-major vectors is the [m, n] solve bit for bit, and is the solve inside the
    model: Y o alpha with alpha = C o x.  The model builds K1, K2 and C on the device, a few last bits from numpy's, and at the
    reference's defaults the iterate amplifies such bits to 1e-6 .. 4e-5 (measured here on this grid: 3e-8 in the quadratic
    term), so the two are compared where the module compares everything else: after five iterations at 1e-10 and converged
    (tol 1e-20) at 1e-8."""
    gpf = _gpf()
    cg = gpf.conjugate_gradient
    c = _ref((24, 20, 0.25, 4.0))
    m, n = c["Y"].shape
    xv = cg.cgsolver(c["K1"], c["K2"], cg.vec(c["b"]), cg.vec(c["C"]))
    assert xv.shape == (m * n, 1)
    x, _, _, _ = handle.kron_cg(c["K1"], c["K2"], c["b"], c["C"])
    assert np.array_equal(cg.unvec(xv, m, n), x)
    assert np.array_equal(cg.vec(x), xv)
    assert cg.dot(cg.vec(c["Y"]), cg.vec(c["C"]) * xv) == pytest.approx(np.sum(c["Y"] * c["C"] * x), rel=1e-14)
    for max_iter, tol, gate in ((5, 1e-6, 1e-10), (400, 1e-20, 1e-8)):
        xv = cg.cgsolver(c["K1"], c["K2"], cg.vec(c["b"]), cg.vec(c["C"]), max_iter=max_iter, tol=tol)
        quad = cg.dot(cg.vec(c["Y"]), cg.vec(c["C"]) * xv)
        model = _model(c["X1"], c["X2"], c["Y"], c["mask"], cg_max_iter=max_iter, cg_tol=tol)
        model.compute_log_likelihood()
        print("cgsolver against the model", max_iter, quad, model.last_solve["quadratic"])
        assert abs(model.last_solve["quadratic"] - quad) <= gate * max(1.0, abs(quad))


def test_predict_without_a_likelihood_call_and_after_a_parameter_change():
    c = _ref((24, 20, 0.25, 4.0))
    model = _model(c["X1"], c["X2"], c["Y"], c["mask"], cg_max_iter=400, cg_tol=1e-20)
    _gpf().get_handle().factor_key = None
    mean = model.predict_f(c["Xn1"], c["Xn2"])
    assert _rel(mean, _converged((24, 20, 0.25, 4.0))["mean"]) <= 1e-8
    model.likelihood._variance.assign(0.3)
    th = dict(TH, s2=0.3)
    res = kr.lml(c["K1"], c["K2"], c["Y"], c["mask"], 0.3, 400, 1e-20)
    ref = kr.predict(res["alpha"], kr.rbf(c["X1"], c["Xn1"], th["var1"], th["ls1"]), kr.rbf(c["X2"], c["Xn2"], th["var2"], th["ls2"]))
    assert _rel(model.predict_f(c["Xn1"], c["Xn2"]), ref) <= 1e-8
    assert model.predict_f(c["Xn1"][:0], c["Xn2"]).shape == (0, 4)


def test_predict_needs_a_resident_solution(handle):
    c = _ref((5, 3, 0.2, 4.0))
    model = _model(c["X1"], c["X2"], c["Y"], c["mask"])
    p1, p2 = model._programs()
    handle.kron_cg(c["K1"], c["K2"], c["b"], c["C"])          # (overwrites whatever solution was resident)
    with pytest.raises(RuntimeError, match="no resident solution"):
        handle.kgpr_predict(p1, c["X1"], c["Xn1"], p2, c["X2"], c["Xn2"])


def test_mean_function_other_than_zero_raises():
    gpf = _gpf()
    c = _ref((5, 3, 0.2, 4.0))
    k1, k2 = gpf.kernels.RBF(2), gpf.kernels.RBF(1)
    with pytest.raises(NotImplementedError):
        gpf.models.KGPR(c["X1"], c["X2"], c["Y"], k1, k2, c["mask"], mean_function=gpf.mean_functions.Constant(np.zeros(1)))
    model = gpf.models.KGPR(c["X1"], c["X2"], c["Y"], k1, k2, c["mask"], mean_function=gpf.mean_functions.Zero())
    names = [p for p in model.parameters]
    assert names == k1.parameters + k2.parameters + model.likelihood.parameters


def test_optimize_lowers_the_objective():
    c = _ref((24, 20, 0.25, 4.0))
    model = _model(c["X1"], c["X2"], c["Y"], c["mask"], dict(TH, ls1=1.5, ls2=1.2, var1=0.5, s2=0.5), cg_max_iter=400, cg_tol=1e-12)
    before = model.objective
    after = model.optimize(max_iter=12)
    print("optimize", before, "->", after)
    assert np.isfinite(after) and after < before - 1e-3


def test_shape_errors(handle):
    c = _ref((5, 3, 0.2, 4.0))
    gpf = _gpf()
    with pytest.raises(ValueError):
        handle.kron_cg(c["K1"], c["K2"], c["b"].T, c["C"])
    with pytest.raises(ValueError):
        handle.kron_cg(c["K1"][:, :2], c["K2"], c["b"], c["C"])
    with pytest.raises(ValueError):
        gpf.conjugate_gradient.cgsolver(c["K1"], c["K2"], np.zeros((7, 1)), np.ones((7, 1)))
    with pytest.raises(ValueError):
        _model(c["X1"], c["X2"], c["Y"].T, c["mask"])
    model = _model(c["X1"], c["X2"], c["Y"], c["mask"])
    p1, p2 = model._programs()
    e1, e2, sel, _, _ = model._spectra(p1, p2, False)
    with pytest.raises(ValueError):
        handle.kgpr_lml(p1, c["X1"], p2, c["X2"], c["Y"], c["mask"], 0.1, e1[:-1], e2, sel)
    with pytest.raises(RuntimeError, match="ranges"):            # ranges that do not hold M pairs: the library's own check
        handle.kgpr_lml(p1, c["X1"], p2, c["X2"], c["Y"], c["mask"], 0.1, e1, e2, np.zeros_like(sel))
    with pytest.raises(RuntimeError, match="bad argument"):
        handle.kgpr_lml(p1, c["X1"], p2, c["X2"], c["Y"], c["mask"], -1.0, e1, e2, sel)
    with pytest.raises(ValueError):
        model.predict_f(c["Xn1"][:, :1], c["Xn2"])
    x, k, rr, delta = handle.kron_cg(np.zeros((0, 0)), c["K2"], np.zeros((0, 3)), np.zeros((0, 3)))
    assert x.shape == (0, 3) and k == 0
