"""CPU checks of tests/_uncond_ref.py, the reference of the conditional at Gaussian inputs: the line-by-line restatement ``uc``
agrees with the weight form ``uc_w`` the device uses, and every case of tests/test_gpu_uncond.py meets the conditioning rule its
tolerance rests on (tol = 4 max(own, eps cond) <= 1e-8 at the first lengthscale factor of the list that allows it)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _uncond_ref as ur  # noqa: E402

# (shape, white, full_cov_output, diagonal q_sqrt, parts): what the GPU tests run
GPU_CASES = ([(s, w, False, False, None) for s in ur.SHAPES for w in (True, False)]
             + [((65, 33, 3, 3), True, True, False, None), ((70, 65, 4, 5), False, True, False, None),
                ((193, 40, 2, 4), False, False, True, None)]
             + [(s, w, False, False, dl) for s, dl, _ in ur.SUM_CASES for w in (True, False)])


def _id(c):
    s, w, full, diag, dl = c
    return "%s-%s%s%s%s" % ("x".join(map(str, s)), "white" if w else "unwhite", "-full" if full else "", "-diag" if diag else "",
                            "-sum%d" % len(dl) if dl else "")


@pytest.mark.parametrize("c", GPU_CASES, ids=_id)
def test_rule_and_forms_agree(c):
    shape, white, full, diag, dl = c
    case = ur.case(shape, white, full, diag, dl)
    assert case is not None, "no lengthscale factor of the list meets cond <= 1.1e7 and own <= 2.5e-9"
    print("%s: lsf %.2f cond %.3g own mean %.3g var %.3g tol mean %.3g var %.3g"
          % (_id(c), case["x"]["lsf"], case["cond"], case["own_mean"], case["own_var"], case["tol_mean"], case["tol_var"]))
    assert case["cond"] <= 1.1e7 and max(case["own_mean"], case["own_var"]) <= 2.5e-9
    assert max(case["tol_mean"], case["tol_var"]) <= 1e-8
    x = case["x"]
    m64, v64 = ur.uc_w(x["parts"], x["Z"], x["mu"], x["S"], case["q_mu"], case["q_sqrt"], white, full)
    assert m64.shape == case["uc"][0].shape and v64.shape == case["uc"][1].shape
    assert ur.err(case["uc"][0], m64) <= case["tol_mean"] and ur.err(case["uc"][1], v64) <= case["tol_var"]
    assert ur.err(m64, case["mean"]) <= case["tol_mean"] and ur.err(v64, case["var"]) <= case["tol_var"]
    if full:                                                        # the diagonal of the [N, D, D] result is the [N, D] result
        plain = ur.case(shape, white, False, diag, dl)
        assert plain["x"]["lsf"] == x["lsf"]
        d = np.arange(shape[3])
        assert ur.err(case["var"][:, d, d], plain["var"]) <= 4 * np.finfo(np.float64).eps


def test_both_parametrisations_describe_one_posterior():
    """(v, s) whitened and (L v, L s) unwhitened give the same moments"""
    a, b = ur.case((65, 33, 3, 3), True), ur.case((65, 33, 3, 3), False)
    assert ur.err(a["mean"], b["mean"]) <= a["tol_mean"] and ur.err(a["var"], b["var"]) <= a["tol_var"]


def test_zero_input_variance_is_the_plain_conditional():
    """S -> 0: Psi1 -> Kfu, psi2n -> Kuf Kfu, and the moments become those of conditional() at the means"""
    import scipy.linalg as sla
    import _psi_sum_ref as ps
    x = ur.case((65, 33, 3, 3), False)["x"]
    q_mu, q_sqrt = ur.posterior(x, False)
    S0 = np.full_like(x["S"], 1e-18)
    fm, fv = ur.uc_w(x["parts"], x["Z"], x["mu"], S0, q_mu, q_sqrt, False, dtype=np.longdouble)
    L = np.linalg.cholesky(ps.K(x["parts"], x["Z"]) + ur.JITTER * np.eye(33))
    A = sla.solve_triangular(L, ps.K(x["parts"], x["Z"], x["mu"]), lower=True)
    A2 = sla.solve_triangular(L.T, A, lower=False)
    mean = A2.T @ q_mu
    var = np.stack([x["parts"][0]["var"] - np.sum(A * A, 0) + np.sum((np.tril(q_sqrt[:, :, d]).T @ A2) ** 2, 0) for d in range(3)], 1)
    u = 4 * np.finfo(np.float64).eps * x["cond"]
    assert ur.err(mean, fm) <= u + 1e-12 and ur.err(var, fv) <= u + 1e-12
