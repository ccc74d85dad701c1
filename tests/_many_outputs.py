"""Cases, gates and the comparison helpers of tests/test_gpu_many_outputs.py (the device at 5 to 129 output columns) and of
tests/test_many_outputs_ref_cpu.py (the reference side of the same cases, without a GPU).  Nothing here touches the device.

Gates.  Every gate is taken from the project or from the reference, never from a device result.

* ``check_ld``: entry-by-entry gradients against a long-double reference (tests/_psi_ref.py, tests/_psi_sum_ref.py).  For every
  output array  tol = max(1e-10, 10 own) max(1, max |reference|) : ``own`` is the distance of the fp64 evaluation of the same
  restatement from the long-double one relative to that scale, 1e-10 is the entry bound of tests/test_gpu_kmat_vjp.py, and the
  factor 10 is there because the device is another fp64 evaluation in another operation order.  A case is admitted only if
  tol <= 1e-8 max(1, max |reference|) (the project's 1e-8 north star) and if the long-double gradient moves by at most
  REF_ONE_ULP_SHARE = 0.1 of tol when Z, the inputs and their variances move by one ulp (tests/test_gpu_gplvm.py).  The seed of a
  case is 7 + N + R + 100 step with the first step at which the case is admitted (``first_admitted_step``); the steps are
  written next to the cases below and tests/test_many_outputs_ref_cpu.py asserts them.
* ``check_solve``: everything that goes through the factor of Kuu + 1e-6 I: solve_tol = max(1e-8, 2 eps cond_2) of
  tests/test_gpu_sgpmc.py relative to max(1, max |reference|) of each output; cond_2 <= 1e9 is asserted.
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _psi_ref as pr  # noqa: E402
import _psi_sum_ref as ps  # noqa: E402

EPS = np.finfo(np.float64).eps
JITTER = 1e-6
NOISE = 0.3
LD_FLOOR = 1e-10                # tests/test_gpu_kmat_vjp.py: the entry bound
LD_OWN_FACTOR = 10.0            # the device is another fp64 evaluation in another operation order
LD_CAP = 1e-8                   # the north star
REF_ONE_ULP_SHARE = 0.1         # tests/test_gpu_gplvm.py
COND_CAP = 1e9
LD_NAMES = ("variance", "lengthscales", "noise", "Z", "X_mean", "X_var")


def scale(ref):
    return max(1.0, float(np.max(np.abs(np.asarray(ref, dtype=np.float64)))))


def solve_tol(K):
    """tests/test_gpu_sgpmc.py: two backward-stable fp64 solves differ by at most 2 eps cond_2(K), never gated below 1e-8"""
    return max(1e-8, 2.0 * EPS * float(np.linalg.cond(K)))


# ---- long-double cases: SGPR (zero_S) and the Bayesian GPLVM -----------------------------------------------------------------------
# (N, M, Q, R, zero_S, parts) -> seed step.  `parts`: None for one RBF-ARD kernel over all Q dimensions, or a tuple of tuples of
# columns for a Sum of RBF parts.  Each step is the first one admitted (tests/test_many_outputs_ref_cpu.py asserts exactly that), and
# the reason a lower step is refused is the figure written here, measured with first_admitted_step on the CPU.
SGPR_LD = [(129, 40, 8, 5), (129, 40, 8, 9), (129, 40, 8, 17), (129, 40, 8, 128), (130, 130, 8, 9)]
BGPLVM_LD = [(65, 60, 9, 4), (65, 60, 9, 5), (65, 60, 16, 5), (33, 9, 32, 5), (65, 60, 9, 128)]
SUM_PARTS = (tuple(range(6)), tuple(range(6, 12)))
SUM_LD = (65, 60, 12, 5)
# _psi_ref.inputs draws the lengthscales as U(0.7, 2) sqrt(Q) with Q = 12, but each part of the Sum sees 6 dimensions only: the
# parts take U(0.7, 2) sqrt(6).  With the factor 1 the case is refused at the steps 0 .. 10 (Z: 10 x own = 2.1e-8 .. 2.2e-6,
# cond(Kuu) 2.6e4 .. 1.8e5); with sqrt(6 / 12) step 0 is admitted (own 1.8e-10, cond(Kuu) 8.4e3).
SUM_LS_SCALE = float(np.sqrt(0.5))
SEED_STEP = {
    (129, 40, 8, 5, True, None): 0,
    (129, 40, 8, 9, True, None): 0,
    (129, 40, 8, 17, True, None): 1,        # step 0: Z: 10 x own = 1.34e-8 > 1e-8 (cond(Kuu) 2.2e4)
    (129, 40, 8, 128, True, None): 1,       # step 0: Z: 10 x own = 2.29e-8 > 1e-8
    # M = 130 at 8 dimensions: the steps 0 .. 42 are all refused on `own` (10 x own between 1.0e-8 and 2.4e-6 in Z, the
    # lengthscales or the variance, at cond(Kuu) 3.9e4 .. 1.1e6); step 43 (cond(Kuu) 1.4e4) is the first one admitted.  The search
    # takes 10 s a step, so tests/test_many_outputs_ref_cpu.py asserts the admission of step 43 and the refusal of step 42 only.
    (130, 130, 8, 9, True, None): 43,
    (65, 60, 9, 4, False, None): 0,
    (65, 60, 9, 5, False, None): 0,
    (65, 60, 16, 5, False, None): 0,
    (33, 9, 32, 5, False, None): 0,
    (65, 60, 9, 128, False, None): 0,
    SUM_LD + (False, SUM_PARTS): 0,
}


def sum_parts(d, parts):
    """the parts of the Sum case over the inputs d (tests/_psi_sum_ref.py: make_parts)"""
    return ps.make_parts(d, [list(p) for p in parts], SUM_LS_SCALE)


def _flat(g):
    """the gradient dictionaries of _psi_ref / _psi_sum_ref as {name: fp64 array}, the slots of a Sum part by part"""
    out = {}
    for name in LD_NAMES:
        v = g[name]
        if isinstance(v, list):
            v = np.concatenate([np.atleast_1d(np.asarray(x, dtype=np.float64)) for x in v])
        out[name] = np.atleast_1d(np.asarray(v, dtype=np.float64))
    return out


def _move_one_ulp(a):
    return a * (1 + EPS * np.where(np.arange(a.size).reshape(a.shape) % 2 == 0, 1.0, -1.0))


def ld_inputs(N, M, Q, R, zero_S, step):
    d = pr.inputs(N, M, Q, R=R, seed=7 + N + R + 100 * step)
    d["noise"] = NOISE
    if zero_S:
        d["S"] = np.zeros_like(d["S"])
    return d


def ld_grad(d, parts=None, dtype=np.longdouble, Y=None):
    """(F, {name: array}) of the bound without the KL term at the inputs d"""
    a = dict(noise=d["noise"], Z=d["Z"], mu=d["mu"], S=d["S"], Y=d["Y"] if Y is None else Y)
    if parts is None:
        F, g = pr.bound_grad(d["var"], d["ls"], dtype=dtype, **a)
    else:
        F, g = ps.bound_grad(sum_parts(d, parts), dtype=dtype, **a)
    return F, _flat(g)


def ld_figures(d, parts=None):
    """dict(F, ref, own, ulp, tol, kuu_cond): the long-double gradient, per output the fp64 restatement's distance from it (own), its
    movement under one ulp on Z, mu and S (ulp) and the gate (tol), all three relative to max(1, max |reference|)"""
    F, ref = ld_grad(d, parts)
    _, g64 = ld_grad(d, parts, dtype=np.float64)
    b = dict(d)
    for kk in ("Z", "mu", "S"):
        b[kk] = _move_one_ulp(d[kk])
    _, moved = ld_grad(b, parts)
    own = {k: float(np.max(np.abs(g64[k] - ref[k]))) / scale(ref[k]) for k in ref}
    ulp = {k: float(np.max(np.abs(moved[k] - ref[k]))) / scale(ref[k]) for k in ref}
    tol = {k: max(LD_FLOOR, LD_OWN_FACTOR * own[k]) for k in ref}
    if parts is None:
        Kuu = pr.rbf_K(d["var"], d["ls"], d["Z"])
    else:
        Kuu = ps.K(sum_parts(d, parts), d["Z"])
    return dict(F=F, ref=ref, own=own, ulp=ulp, tol=tol, kuu_cond=float(np.linalg.cond(Kuu + JITTER * np.eye(len(Kuu)))))


def admitted(c, zero_S=False):
    """(admitted, reason) of the figures of one case; with S = 0 the gradients in X_mean and X_var are no output of SGPR"""
    for k in c["ref"]:
        if zero_S and k in ("X_mean", "X_var"):
            continue
        if c["tol"][k] > LD_CAP:
            return False, "%s: 10 x own = %.3g > 1e-8" % (k, c["tol"][k])
        if c["ulp"][k] > REF_ONE_ULP_SHARE * c["tol"][k]:
            return False, "%s: one ulp moves the reference by %.3g > 0.1 x tol = %.3g" % (k, c["ulp"][k], 0.1 * c["tol"][k])
    return True, ""


@functools.lru_cache(maxsize=None)
def ld_case(N, M, Q, R, zero_S=False, parts=None, step=None):
    """the inputs and figures of one case at its recorded seed step, computed once and left unchanged"""
    if step is None:
        step = SEED_STEP[(N, M, Q, R, zero_S, parts)]
    d = ld_inputs(N, M, Q, R, zero_S, step)
    c = ld_figures(d, parts)
    c.update(d=d, zero_S=zero_S, parts=parts, step=step, names=tuple(k for k in LD_NAMES if not (zero_S and k in ("X_mean", "X_var"))))
    return c


def first_admitted_step(N, M, Q, R, zero_S=False, parts=None, limit=8):
    """(step, [reason of every refused step]) as _SEED_STEP of tests/test_gpu_gplvm.py is chosen"""
    reasons = []
    for step in range(limit):
        ok, why = admitted(ld_figures(ld_inputs(N, M, Q, R, zero_S, step), parts), zero_S)
        if ok:
            return step, reasons
        reasons.append(why)
    raise AssertionError("no admitted seed step below %d: %s" % (limit, reasons))


def check_ld(got, c):
    """The comparison of the long-double cases: got {name: array} against the case c; {name: error / tol}, AssertionError where an
    entry misses its gate or the case is not admitted."""
    ok, why = admitted(c, c["zero_S"])
    assert ok, why
    out = {}
    for k in c["names"]:
        g, ref = np.atleast_1d(np.asarray(got[k], dtype=np.float64)), c["ref"][k]
        assert g.shape == ref.shape, (k, g.shape, ref.shape)
        err = float(np.max(np.abs(g - ref))) / scale(ref)
        out[k] = err / c["tol"][k]
        assert np.all(np.isfinite(g)) and err <= c["tol"][k], (k, err, c["tol"][k], c["own"][k])
    return out


def ld_wrong_last_column(c, mode):
    """What a device that mishandles the last output column would return, from the reference itself.  The bound is
    R x (a term without Y) + sum over the columns of a term of one column, and so is every gradient: the last column's contribution
    is gradient(Y) - gradient(Y with the last column zeroed).  mode "swap": column 0 is read where the last one was meant (its
    contribution counted twice, the last one's dropped) ; "scale": the last column's contribution times 1 + 1e-6."""
    d = c["d"]
    Y = d["Y"].copy()
    if mode == "swap":
        Y[:, -1] = Y[:, 0]
        return ld_grad(d, c["parts"], Y=Y)[1]
    Y[:, -1] = 0.0
    without = ld_grad(d, c["parts"], Y=Y)[1]
    return {k: c["ref"][k] + 1e-6 * (c["ref"][k] - without[k]) for k in c["ref"]}


# ---- cases through the factor of Kuu + 1e-6 I ------------------------------------------------------------------------------------------
SGPMC_SIZES = [(40, 129, 5), (40, 129, 16), (130, 300, 17), (40, 129, 128)]
SGPMC_KINDS = ("poisson", "student_t", "multiclass")
SGPMC_OUT = ("loglik", "slots", "glik", "gV", "gmean", "gZ")
SGPMC_KERN = dict(variance=1.3, lengthscales=(0.5, 0.7))         # the RBF of tests/test_gpu_sgpmc.py


@functools.lru_cache(maxsize=None)
def sgpmc_case(kind, m, n, r):
    import _sgpmc_ref as sr
    spec = {"type": "rbf", "dims": [0, 1], "variance": SGPMC_KERN["variance"], "lengthscales": np.array(SGPMC_KERN["lengthscales"])}
    Z, X, V, Y, params, mean = sr.make_case(kind, m, n, r)
    res = sr.grad(spec, Z, X, V, Y, kind, params, mean, jitter=JITTER)
    res.update(Z=Z, X=X, V=V, Y=Y, params=params, mean=mean, tol=solve_tol(res["Kuu"]), cond=float(np.linalg.cond(res["Kuu"])), spec=spec)
    return res


def check_solve(got, ref, tol, names, cond=None):
    """The comparison of the solve_tol cases: got and ref {name: value}; {name: error relative to max(1, max |reference|)},
    AssertionError where one exceeds tol or the conditioning leaves no room (cond_2 > 1e9)."""
    if cond is not None:
        assert cond <= COND_CAP, cond
    out = {}
    for k in names:
        g, r = np.atleast_1d(np.asarray(got[k], dtype=np.float64)), np.atleast_1d(np.asarray(ref[k], dtype=np.float64))
        assert g.shape == r.shape, (k, g.shape, r.shape)
        out[k] = float(np.max(np.abs(g - r))) / scale(r)
        assert np.all(np.isfinite(g)) and out[k] <= tol, (k, out[k], tol)
    return out


def columns_wrong_last(ref, names, mode):
    """the per-column outputs `names` ([*, R] arrays) of ref with the last column swapped with column 0, or scaled by 1 + 1e-6"""
    out = dict(ref)
    for k in names:
        a = np.array(ref[k], dtype=np.float64)
        if mode == "swap":
            a[:, [0, -1]] = a[:, [-1, 0]]
        else:
            a[:, -1] *= 1 + 1e-6
        out[k] = a
    return out
