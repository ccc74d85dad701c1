"""The reference side of tests/test_gpu_many_outputs.py, without a GPU: every long-double case is admitted at its recorded seed
step and at no earlier one, every solve_tol case stays below cond_2 = 1e9 with finite outputs, and the comparison helpers of
tests/_many_outputs.py -- the functions the GPU tests apply their gates with -- reject a result whose last output column is
mishandled.  A case that is not admissible fails here, not on the GPU machine."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gpmc_ref as gr  # noqa: E402
import _many_outputs as mo  # noqa: E402
import _sgpmc_ref as sr  # noqa: E402

LD_CASES = [s + (True, None) for s in mo.SGPR_LD] + [s + (False, None) for s in mo.BGPLVM_LD] + [mo.SUM_LD + (False, mo.SUM_PARTS)]


def _id(c):
    return "N%d_M%d_Q%d_R%d_%s%s" % (c[0], c[1], c[2], c[3], "sgpr" if c[4] else "bgplvm", "_sum" if c[5] else "")


def test_every_long_double_case_has_a_recorded_step():
    assert set(LD_CASES) == set(mo.SEED_STEP)


@pytest.mark.parametrize("case", LD_CASES, ids=_id)
def test_long_double_case_is_admitted_at_its_step_and_not_before(case):
    """tol = max(1e-10, 10 own) <= 1e-8 and the one-ulp movement <= 0.1 tol, for every output array; the steps below the recorded
    one are refused (M = 130: the one before it only -- 10 s a step; the others are recorded in tests/_many_outputs.py)."""
    c = mo.ld_case(*case)
    ok, why = mo.admitted(c, c["zero_S"])
    print("%s step %d: cond(Kuu) %.3g own %.3g one-ulp %.3g" % (_id(case), c["step"], c["kuu_cond"], max(c["own"][k] for k in c["names"]),
                                                              max(c["ulp"][k] for k in c["names"])))
    assert ok, why
    for k in c["names"]:
        assert c["tol"][k] <= mo.LD_CAP and c["ulp"][k] <= mo.REF_ONE_ULP_SHARE * c["tol"][k] and np.all(np.isfinite(c["ref"][k]))
    N, M, Q, R, zero_S, parts = case
    for step in range(max(0, c["step"] - 1) if M == 130 else 0, c["step"]):
        refused = mo.admitted(mo.ld_figures(mo.ld_inputs(N, M, Q, R, zero_S, step), parts), zero_S)
        assert not refused[0], (case, step)
    assert mo.check_ld(c["ref"], c) == {k: 0.0 for k in c["names"]}          # the reference passes its own comparison


def test_the_long_double_bound_with_zero_variances_is_the_sgpr_bound():
    import oracle.gp_oracle as orc
    c = mo.ld_case(129, 40, 8, 9, True, None)
    d = c["d"]
    spec = {"type": "rbf", "variance": d["var"], "lengthscales": d["ls"], "input_dim": 8}
    ref = orc.sgpr_bound(spec, d["mu"], d["Y"], d["Z"], d["noise"])
    assert abs(ref - c["F"]) <= 1e-13 * abs(ref)


# ---- the comparison must be able to fail ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["swap", "scale"])
@pytest.mark.parametrize("case", [(129, 40, 8, 9, True, None), (65, 60, 9, 5, False, None)], ids=_id)
def test_check_ld_rejects_a_mishandled_last_column(case, mode):
    """SGPR at R = 9 and the Bayesian GPLVM at R = 5: column 0 read where the last one was meant, and the last column's
    contribution scaled by 1 + 1e-6 (tests/_many_outputs.py: ld_wrong_last_column)"""
    c = mo.ld_case(*case)
    wrong = mo.ld_wrong_last_column(c, mode)
    worst = max(float(np.max(np.abs(wrong[k] - c["ref"][k]))) / mo.scale(c["ref"][k]) / c["tol"][k] for k in c["names"])
    print("%s %s: the wrong result is %.3g gates away" % (_id(case), mode, worst))
    with pytest.raises(AssertionError):
        mo.check_ld(wrong, c)
    # ... and every array that depends on Y is rejected on its own (the kernel variance's gradient does not depend on Y when S = 0
    # only through Psi2: it is left to the others)
    rejected = []
    for k in c["names"]:
        only = dict(c["ref"]); only[k] = wrong[k]
        try:
            mo.check_ld(only, c)
        except AssertionError:
            rejected.append(k)
    print("rejected on their own: %s" % rejected)
    assert "Z" in rejected and "lengthscales" in rejected and "noise" in rejected


@pytest.mark.parametrize("mode", ["swap", "scale"])
@pytest.mark.parametrize("kind", mo.SGPMC_KINDS)
def test_check_solve_rejects_a_mishandled_last_column(kind, mode):
    """SGPMC at (M, N, R) = (40, 129, 9): the last column of grad_V and of d / d mean swapped with column 0, and scaled by 1 + 1e-6"""
    c = mo.sgpmc_case(kind, 40, 129, 9)
    assert mo.check_solve(c, c, c["tol"], mo.SGPMC_OUT, cond=c["cond"]) == {k: 0.0 for k in mo.SGPMC_OUT}
    for name in ("gV", "gmean"):
        wrong = mo.columns_wrong_last(c, (name,), mode)
        with pytest.raises(AssertionError):
            mo.check_solve(wrong, c, c["tol"], mo.SGPMC_OUT, cond=c["cond"])


def test_check_solve_rejects_an_ill_conditioned_case():
    c = mo.sgpmc_case("poisson", 40, 129, 9)
    with pytest.raises(AssertionError):
        mo.check_solve(c, c, c["tol"], mo.SGPMC_OUT, cond=2e9)


# ---- the solve_tol cases ------------------------------------------------------------------------------------------------------------------
def test_solve_tol_is_the_projects():
    K = np.diag([1.0, 1e-10])
    assert mo.solve_tol(K) == max(1e-8, 2.0 * np.finfo(float).eps * 1e10) and mo.solve_tol(np.eye(3)) == 1e-8


@pytest.mark.parametrize("kind", mo.SGPMC_KINDS)
@pytest.mark.parametrize("size", mo.SGPMC_SIZES, ids=lambda s: "M%d_N%d_R%d" % s)
def test_sgpmc_case_is_admissible(size, kind):
    c = mo.sgpmc_case(kind, *size)
    print("sgpmc %s %s: cond %.3g tol %.3g" % (kind, size, c["cond"], c["tol"]))
    assert c["cond"] <= mo.COND_CAP
    assert all(np.all(np.isfinite(np.asarray(c[k], dtype=float))) for k in mo.SGPMC_OUT)
    # every column of the two per-column outputs carries something to compare
    assert np.all(np.abs(c["gV"]).max(0) > 0) and np.all(np.abs(c["gmean"]).max(0) > 0)


SVGP_LIK = [(kind, k, qd) for kind, k in (("bernoulli", 9), ("student_t", 9), ("poisson", 17), ("multiclass", 17)) for qd in (False, True)]
SVGP_LIK.append(("poisson", 128, True))


@pytest.mark.parametrize("kind,k,q_diag", SVGP_LIK)
def test_svgp_lik_case_is_admissible(kind, k, q_diag):
    """the problems of tests/test_gpu_lik.py at n = 129, m = 30 (the models are built on the host; nothing is evaluated on a device)"""
    import oracle.gp_oracle as orc
    import test_gpu_lik as tl
    m, P = tl._problem(kind, k, True, q_diag, n=129, m_=30, mean=(kind == "student_t"), train_inducing=True)
    Kuu = orc.K(P["spec"](P["theta"]), P["Z"]) + orc.JITTER * np.eye(30)
    cond = float(np.linalg.cond(Kuu))
    print("svgp %s k=%d q_diag=%s: cond %.3g tol %.3g" % (kind, k, q_diag, cond, mo.solve_tol(Kuu)))
    assert cond <= mo.COND_CAP and np.isfinite(tl._ref_bound(P))


@pytest.mark.parametrize("kind", ["poisson", "student_t"])
@pytest.mark.parametrize("r", [17, 128])
def test_gpmc_case_is_admissible(kind, r):
    X, V, Y, params, mean = gr.make_case(kind, 129, r)
    res = gr.grad(gr.rbf_spec(), X, V, Y, kind, params, mean, jitter=mo.JITTER)
    cond = float(np.linalg.cond(res["K"]))
    print("gpmc %s R=%d: cond %.3g tol %.3g" % (kind, r, cond, mo.solve_tol(res["K"])))
    assert cond <= mo.COND_CAP
    assert all(np.all(np.isfinite(np.asarray(res[k], dtype=float))) for k in ("loglik", "slots", "glik", "gV", "gmean"))
