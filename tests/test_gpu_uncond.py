"""GPU tests of the conditional at Gaussian inputs (csrc/gps_uncond.hip, psi2_contract_kernel of csrc/psi.hip): the contraction of
eKzxKxz with weight matrices entry by entry against the long-double expectations, uncertain_conditional against the long-double
reference of tests/_uncond_ref.py under its conditioning rule (single RBF, both parametrisations, diagonal q_sqrt, full_cov_output,
a Sum of RBF parts across chunk edges), the limit of vanishing input variance against conditional(), a size at which eKzxKxz
could not be stored, and the Python surface."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _psi_ref as pr  # noqa: E402
import _uncond_ref as ur  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
LD = np.longdouble


@pytest.fixture(scope="module")
def gpf():
    import gpflowSlim
    return gpflowSlim


def _kern(gpf, parts):
    if len(parts) == 1:
        p = parts[0]
        return gpf.ekernels.RBF(len(p["dims"]), variance=p["var"], lengthscales=p["ls"], ARD=np.ndim(p["ls"]) > 0)
    return gpf.ekernels.Sum([gpf.ekernels.RBF(len(p["dims"]), variance=p["var"], lengthscales=p["ls"], active_dims=list(p["dims"]),
                                              ARD=np.ndim(p["ls"]) > 0) for p in parts])


# ---- 1. psi2_contract entry by entry ------------------------------------------------------------------------------------------
CONTRACT_SHAPES = [(1, 1, 1), (7, 5, 1), (300, 37, 3), (129, 130, 5), (33, 9, 32), (257, 40, 2)]


@pytest.mark.parametrize("ard", [True, False], ids=["ard", "iso"])
@pytest.mark.parametrize("shape", CONTRACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_psi2_contract_entrywise(gpf, shape, ard):
    N, M, Q = shape
    d = pr.inputs(N, M, Q, seed=200 + N + M + Q, ard=ard)
    k = gpf.ekernels.RBF(Q, variance=d["var"], lengthscales=d["ls"], ARD=ard)
    blk = max(1, int(4e6 // (M * M * Q)))
    p2l = np.concatenate([pr.psi2n(d["var"], d["ls"], d["Z"], d["mu"][i:i + blk], d["S"][i:i + blk], LD) for i in range(0, N, blk)])
    p2 = np.concatenate([pr.psi2n(d["var"], d["ls"], d["Z"], d["mu"][i:i + blk], d["S"][i:i + blk]) for i in range(0, N, blk)])
    spread = pr._rel(p2, p2l)
    factor = 8 * spread + 64 * EPS + M * M * EPS                    # the reference's own spread, the exponentials, any-order summation
    print("%s %s: spread %.3g factor %.3g" % (shape, "ard" if ard else "iso", spread, factor))
    assert factor <= 1e-11
    rng = np.random.default_rng(7 + N)
    for B in (1, 3, 9):
        W = rng.standard_normal((B, M, M))                         # random signs, not symmetric
        got = k.eKzxKxz_contract(d["Z"], d["mu"], d["S"], W)
        assert got.shape == (N, B)
        Wl = np.asarray(W, dtype=LD)
        ref = np.tensordot(p2l, Wl, axes=([1, 2], [1, 2]))
        scale = np.tensordot(np.abs(p2l), np.abs(Wl), axes=([1, 2], [1, 2]))
        ratio = float(np.max(np.abs(got - ref) / scale))
        print("  B = %d: max err / sum |psi2n| |W| = %.3g" % (B, ratio))
        assert ratio <= factor
        assert np.array_equal(got, k.eKzxKxz_contract(d["Z"], d["mu"], d["S"], W))                         # bitwise, run to run
        assert np.array_equal(got, k.eKzxKxz_contract(d["Z"], d["mu"], d["S"], 0.5 * (W + W.transpose(0, 2, 1))))
    one = k.eKzxKxz_contract(d["Z"], d["mu"], d["S"], W[0])
    assert one.shape == (N,) and np.array_equal(one, k.eKzxKxz_contract(d["Z"], d["mu"], d["S"], W[:1])[:, 0])     # one [M, M] matrix


# ---- 2. uncertain_conditional against the reference ---------------------------------------------------------------------------------
def _run(gpf, case, q_sqrt=None, **kw):
    x = case["x"]
    feat = gpf.features.InducingPoints(x["Z"])
    return gpf.conditionals.uncertain_conditional(x["mu"], x["S"], feat, _kern(gpf, x["parts"]), case["q_mu"],
                                                  case["q_sqrt"] if q_sqrt is None else q_sqrt, white=case["white"], **kw)


def _check(case, fm, fv, what=""):
    rows = case["rows"]
    if rows is not None:
        fm, fv = fm[rows], fv[rows]
    assert fm.shape == case["mean"].shape and fv.shape == case["var"].shape
    em, ev = ur.err(fm, case["mean"]), ur.err(fv, case["var"])
    print("%s lsf %.2f cond %.3g: mean err %.3g (own %.3g, tol %.3g), var err %.3g (own %.3g, tol %.3g)"
          % (what, case["x"]["lsf"], case["cond"], em, case["own_mean"], case["tol_mean"], ev, case["own_var"], case["tol_var"]))
    assert max(case["tol_mean"], case["tol_var"]) <= 1e-8
    assert em <= case["tol_mean"] and ev <= case["tol_var"]


@pytest.mark.parametrize("white", [True, False], ids=["white", "unwhite"])
@pytest.mark.parametrize("shape", ur.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_uncertain_conditional(gpf, shape, white):
    case = ur.case(shape, white)
    assert case is not None
    fm, fv = _run(gpf, case)
    _check(case, fm, fv, "%s %s" % (shape, "white" if white else "unwhite"))


def test_uncertain_conditional_diagonal_q_sqrt(gpf):
    case = ur.case((193, 40, 2, 4), False, False, True)
    assert case is not None
    q2 = np.stack([np.diag(case["q_sqrt"][:, :, d]) for d in range(4)], axis=1)                     # [M, D]
    fm, fv = _run(gpf, case, q_sqrt=q2)
    _check(case, fm, fv, "2-D q_sqrt")


@pytest.mark.parametrize("shape,white", [((65, 33, 3, 3), True), ((70, 65, 4, 5), False)], ids=["65x33x3x3", "70x65x4x5"])
def test_full_cov_output(gpf, shape, white):
    case, plain = ur.case(shape, white, True), ur.case(shape, white)
    assert case is not None and plain is not None and case["x"]["lsf"] == plain["x"]["lsf"]
    fm, fv = _run(gpf, case, full_cov_output=True)
    _check(case, fm, fv, "full_cov_output %s" % (shape,))
    assert np.array_equal(fv, fv.transpose(0, 2, 1))
    fm1, fv1 = _run(gpf, plain)
    d = np.arange(shape[3])
    assert np.array_equal(fm, fm1)
    assert ur.err(fv[:, d, d], fv1) <= plain["tol_var"]
    fm2, fv2 = _run(gpf, case, full_cov_output=True)
    assert np.array_equal(fm, fm2) and np.array_equal(fv, fv2)


# ---- 3. Sum of RBF parts -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("white", [True, False], ids=["white", "unwhite"])
@pytest.mark.parametrize("sc", ur.SUM_CASES, ids=["two_parts", "three_parts_chunk64"])
def test_uncertain_conditional_sum(gpf, sc, white):
    from gpflowSlim import _backend as be
    shape, dl, chunk = sc
    case = ur.case(shape, white, False, False, dl)
    assert case is not None
    if chunk:
        assert be.psi_sum_chunking(shape[0], shape[1], chunk) == (64, 2) and shape[0] == 64 + 6      # the chunk edge is crossed
    h = gpf.get_handle()
    h.psi_sum_set_chunk(chunk)
    try:
        fm, fv = _run(gpf, case)
        fm2, fv2 = _run(gpf, case)
    finally:
        h.psi_sum_set_chunk(0)
    _check(case, fm, fv, "Sum %s" % (dl,))
    assert np.array_equal(fm, fm2) and np.array_equal(fv, fv2)


# ---- 4. the limit of vanishing input variance ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("white", [True, False], ids=["white", "unwhite"])
def test_zero_variance_limit_is_conditional(gpf, white):
    case = ur.case((65, 33, 3, 3), white)
    x = case["x"]
    Sv = 1e-18
    ls = np.asarray(x["parts"][0]["ls"])
    dmax = np.abs(x["mu"][:, None, :] - x["Z"][None, :, :]).max(axis=(0, 1))
    premise = 4 * 3 * Sv * float(np.max(1 / ls ** 2 + dmax ** 2 / ls ** 4))      # relative change of Psi1 / psi2n entries from S
    assert premise <= 1e-12
    kern = _kern(gpf, x["parts"])
    feat = gpf.features.InducingPoints(x["Z"])
    fm, fv = gpf.conditionals.uncertain_conditional(x["mu"], np.full_like(x["S"], Sv), feat, kern, case["q_mu"], case["q_sqrt"],
                                                    white=white)
    cm, cv = gpf.conditionals.conditional(x["mu"], x["Z"], kern, case["q_mu"], q_sqrt=case["q_sqrt"], white=white)
    em, ev = ur.err(fm, cm), ur.err(fv, cv)
    print("S -> 0 (%s): mean %.3g var %.3g against 2 tol + 1e-12 = %.3g" % ("white" if white else "unwhite", em, ev,
                                                                           2 * case["tol_var"] + 1e-12))
    assert em <= 2 * case["tol_mean"] + 1e-12 and ev <= 2 * case["tol_var"] + 1e-12


# ---- 5. no [N, M, M] array ------------------------------------------------------------------------------------------------------------
def test_large_n_never_stores_psi2n(gpf):
    shape = (600000, 256, 4, 1)
    assert shape[0] * shape[1] ** 2 * 8 > 288e9                     # eKzxKxz would be 315 GB: more than the HBM
    case = ur.case(shape, False, n_rows=66)
    assert case is not None
    fm, fv = _run(gpf, case)
    assert fm.shape == (shape[0], 1) and fv.shape == (shape[0], 1) and np.all(np.isfinite(fm)) and np.all(np.isfinite(fv))
    _check(case, fm, fv, "N = 600000")


# ---- 6. the surface -----------------------------------------------------------------------------------------------------------------
def test_refusals(gpf):
    case = ur.case((7, 5, 1, 2), True)
    x = case["x"]
    kern, feat = _kern(gpf, x["parts"]), gpf.features.InducingPoints(x["Z"])
    uc = gpf.conditionals.uncertain_conditional
    with pytest.raises(NotImplementedError):
        uc(x["mu"], x["S"], feat, kern, case["q_mu"], case["q_sqrt"], full_cov=True)
    with pytest.raises(NotImplementedError):
        uc(x["mu"], x["S"], gpf.features.InducingFeature(), kern, case["q_mu"], case["q_sqrt"])
    with pytest.raises(NotImplementedError):
        uc(x["mu"], np.stack([np.diag(s) for s in x["S"]]), feat, kern, case["q_mu"], case["q_sqrt"])
    with pytest.raises(ValueError):
        uc(x["mu"], x["S"], feat, kern, case["q_mu"], None)
    with pytest.raises(NotImplementedError):
        uc(x["mu"], x["S"], feat, gpf.kernels.RBF(1), case["q_mu"], case["q_sqrt"])
    prog = kern._psi_program(x["mu"])
    with pytest.raises(RuntimeError, match="at most 16 outputs"):
        gpf.get_handle().uncertain_conditional(prog, x["Z"], x["mu"], x["S"], np.zeros((5, 17)), np.ones((5, 17)), 1e-6,
                                               full_cov_output=True)


@pytest.mark.parametrize("which", ["uncertain_conditional", "psi2_contract"])
def test_resident_gpr_factor_is_dropped(gpf, which):
    """both entries overwrite the buffers a resident GPR factor lives in: a model that reuses its factor must notice"""
    def model(reuse):
        g = np.random.default_rng(5)
        X = g.standard_normal((300, 2))
        m = gpf.models.GPR(X, np.sin(X[:, :1]), gpf.kernels.RBF(2, variance=1.2, lengthscales=[0.9, 1.4], ARD=True), obs_var=0.1)
        m.reuse_factor = reuse
        return m, g.standard_normal((9, 2))
    m0, Xs = model(False)
    m0.compute_log_likelihood()
    mu0, var0 = m0.predict_f(Xs)
    m, _ = model(True)
    m.compute_log_likelihood()
    assert gpf.get_handle().factor_key is not None
    case = ur.case((65, 33, 3, 3), True)
    x = case["x"]
    if which == "uncertain_conditional":
        _run(gpf, case)
    else:
        _kern(gpf, x["parts"]).eKzxKxz_contract(x["Z"], x["mu"], x["S"], np.eye(33))
    assert gpf.get_handle().factor_key is None
    mu, var = m.predict_f(Xs)
    assert np.array_equal(mu, mu0) and np.array_equal(var, var0)


def test_feature_expectations_shapes(gpf):
    case = ur.case((7, 5, 1, 2), True)
    x = case["x"]
    kern, feat = _kern(gpf, x["parts"]), gpf.features.InducingPoints(x["Z"])
    a, b = feat.eKfu(kern, x["mu"], x["S"]), feat.eKufKfu(kern, x["mu"], x["S"])
    assert a.shape == (7, 5) and b.shape == (7, 5, 5)
    assert np.array_equal(a, kern.eKxz(x["Z"], x["mu"], x["S"])) and np.array_equal(b, kern.eKzxKxz(x["Z"], x["mu"], x["S"]))


@pytest.mark.parametrize("whiten", [True, False], ids=["white", "unwhite"])
def test_svgp_predict_f_uncertain(gpf, whiten):
    case = ur.case((65, 33, 3, 3), whiten)
    x = case["x"]
    rng = np.random.default_rng(3)
    X, Y = rng.standard_normal((40, 3)), rng.standard_normal((40, 3))
    m = gpf.models.SVGP(X, Y, _kern(gpf, x["parts"]), gpf.likelihoods.Gaussian(0.1), Z=x["Z"], whiten=whiten)
    m._q_mu.assign(case["q_mu"])
    m._q_sqrt.assign(np.stack([np.tril(case["q_sqrt"][:, :, d]) for d in range(3)], axis=2))
    fm, fv = m.predict_f_uncertain(x["mu"], x["S"])
    rm, rv = gpf.conditionals.uncertain_conditional(x["mu"], x["S"], m.feature, m.kern, m.q_mu, m.q_sqrt, white=whiten)
    assert np.array_equal(fm, rm) and np.array_equal(fv, rv)
    _check(case, fm, fv, "SVGP.predict_f_uncertain")
    assert m.predict_f_uncertain(x["mu"], x["S"], full_cov_output=True)[1].shape == (65, 3, 3)
    mc = gpf.models.SVGP(X, Y, _kern(gpf, x["parts"]), gpf.likelihoods.Gaussian(0.1), Z=x["Z"],
                         mean_function=gpf.mean_functions.Constant(np.zeros(3)))
    with pytest.raises(NotImplementedError):
        mc.predict_f_uncertain(x["mu"], x["S"])
