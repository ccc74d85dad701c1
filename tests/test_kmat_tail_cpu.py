"""The host side of tests/test_gpu_kmat_tail.py (tests/_kmat_tail.py): the fixture is what its generator writes, the arguments of
the exponential are exact where the design says so, the domains around a = -708 are populated, `own` of every kind is measured
and bounded, and the comparison itself fails on the two defects it is there for.  No GPU."""
import importlib.util
import os
import sys

import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _kmat_tail as kt  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SIZE_CAP = 252 * 1024            # what tests/golden/mp held before this fixture


def _generator():
    spec = importlib.util.spec_from_file_location("make_kmat_tail_golden", os.path.join(HERE, "golden", "mp", "make_kmat_tail_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_is_what_the_generator_writes():
    """every array of tests/golden/mp/kmat_tail.npz byte for byte (the file itself is a zip archive with a time stamp)"""
    new, old = _generator().build(), kt.fixture()
    assert sorted(new) == sorted(old)
    for k in sorted(new):
        a, b = np.asarray(new[k]), old[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    assert os.path.getsize(kt.FIXTURE) < SIZE_CAP


def _exact(x):
    return mp.mpf(float(x))


def test_arguments_are_exact():
    """S^2 + T^2 in fp64 is the exact number for every entry of every stationary grid, the coordinates are multiples of 2^-10 within
    [-40, 40] and the lengthscales powers of two"""
    mp.mp.dps = 50
    for kind in kt.STATIONARY:
        g = kt.grid(kind)
        for v in (g["s"], g["t"]):
            assert np.all(v * 1024 == np.round(v * 1024)) and np.abs(v).max() <= 40.0
        assert g["s"][0] == 0.0 and g["t"][0] == 0.0 and g["r2"][0, 0] == 0.0
        S2, T2 = [_exact(v) * _exact(v) for v in g["S"]], [_exact(v) * _exact(v) for v in g["T"]]
        for i in range(kt.N):
            for j in range(kt.N):
                assert _exact(g["r2"][i, j]) == S2[i] + T2[j], (kind, i, j)


@pytest.mark.parametrize("D", kt.DIMS)
def test_dimension_cases_are_exact(D):
    """with the common offsets: the features x / l, both squared norms and every dot product are exact (the dot product is the same
    W for every entry), and -2 dot + (ni + nj) is the grid's S^2 + T^2 to the bit, in the VALU order and in fma(-2, dot, ni + nj)"""
    mp.mp.dps = 50
    for kind in ("rbf", "matern52"):
        g = kt.grid(kind)
        for which in range(3):
            X, X2, ls, p, q = kt.dim_case(kind, D, which)
            assert p != q and 0 <= p < D and 0 <= q < D
            assert np.all(np.log2(ls) == np.round(np.log2(ls)))
            assert np.all(X[:, q] == 0.0) and np.all(X2[:, p] == 0.0)
            other = [c for c in range(D) if c not in (p, q)]
            assert np.all(X[:, other] != 0.0) and np.all(X[:, other] == X2[:, other]) and np.all(X[:, other] == X[0, other])
            assert np.all(X[:, other] * 8 == np.round(X[:, other] * 8))
            F, G = X / ls, X2 / ls
            assert np.all(F * ls == X) and np.all(G * ls == X2) and np.all(F[:, p] == g["S"]) and np.all(G[:, q] == g["T"])
            r2, ni, nj, dot = kt.gemm_r2(X, X2, ls)
            W = sum((_exact(X[0, c]) / _exact(ls[c])) ** 2 for c in other)
            assert np.all(dot == dot[0, 0]) and _exact(dot[0, 0]) == W
            for i in range(kt.N):
                assert _exact(ni[i]) == W + _exact(g["S"][i]) ** 2 and _exact(nj[i]) == W + _exact(g["T"][i]) ** 2
            nsum = ni[:, None] + nj[None, :]
            for i in (0, 1, kt.N - 1):
                for j in range(kt.N):
                    assert _exact(nsum[i, j]) == _exact(ni[i]) + _exact(nj[j])
            assert np.array_equal(r2, g["r2"])
    if D == 32:
        for which in range(3):
            X, X2, ls, p, q = kt.dim_case("periodic", D, which)
            other = [c for c in range(D) if c not in (p, q)]
            assert np.all(X[:, other] == X2[:, other]) and np.all(X[:, other] != 0.0)
            assert np.all(X[:, p] == kt.periodic_grid(ls)["s"]) and np.all(X2[:, q] == kt.periodic_grid(ls)["t"])


def _run_counts(a_run):
    return int(((a_run >= kt.A_EDGE) & (a_run < -707.3)).sum()), int((a_run < -708.1).sum())


def test_domains_are_populated():
    """per kind the run holds at least five arguments in [-708, -707.3) and five below -708.1 (a flush threshold moved by one
    changes entries of the first set), the singles are where they are meant to be, and both domains have entries"""
    cases = [(k, kt.grid(k), 0) for k in kt.STATIONARY] + [("periodic", kt.periodic_grid(kt.PERIODIC_LS[1]), 1)]
    for kind, g, row in cases:
        a = g["a"]
        near, below = _run_counts(a[row, 1:1 + kt.RUN_LEN])
        assert near >= 5 and below >= 5, (kind, near, below)
        singles = a[row, 1 + kt.RUN_LEN:1 + kt.RUN_LEN + len(kt.SINGLES)]
        assert np.all(np.abs(singles - np.array(kt.SINGLES)) < 0.05), (kind, singles)
        rel = a >= kt.A_EDGE
        assert rel.sum() >= 500 and (~rel).sum() >= 250, (kind, rel.sum())
        assert ((np.abs(a) < 1.0).sum() >= 10 or kind == "periodic") and a.min() < -800.0, kind      # (Periodic near 0: its grid at l = 1)
        # the reference goes through the denormals and reaches 0
        assert np.any((g["ref"] > 0.0) & (g["ref"] < 2.0 ** -1022)) and np.any(g["ref"] == 0.0), kind
    assert np.all(kt.periodic_grid(kt.PERIODIC_LS[0])["a"] >= -1.0)


def test_own_is_measured_and_small(capsys):
    """own(kind): printed, positive, and for the exact-argument kinds at most 3 units (two roundings of eps / 2 on the argument
    path, four on the value path)"""
    with capsys.disabled():
        for kind in kt.STATIONARY:
            g = kt.grid(kind)
            raw, ref = kt.own_raw(g), kt.own_reference(g)
            print("own(%s): restatement %.3g, fixture rounding %.3g -> %.3g" % (kind, raw, ref, kt.own_grid(kind)))
            assert 0.0 < raw <= 3.0 and 0.0 < kt.own_grid(kind) <= 3.0, (kind, raw)
        print("own(product of two rbf): %.3g" % kt.own_grid("product"))
        assert 0.0 < kt.own_grid("product") <= 3.0
        for ls in kt.PERIODIC_LS:
            g = kt.periodic_grid(ls)
            print("own(periodic, l = %g): restatement %.3g, fixture rounding %.3g; largest E / eps %.3g"
                  % (ls, kt.own_raw(g), kt.own_reference(g), float((g["E"] / kt.EPS).max())))
            assert 0.0 < kt.own_grid("periodic", ls) <= 3.0
        for D in kt.GENERAL_DIMS:
            for kind in ("rbf", "matern52"):
                g = kt.general_case(kind, D)
                print("own(general %s, D = %d): %.3g (r2 up to %.6g)" % (kind, D, kt.own_of(g), g["r2"].max()))
                assert kt.own_of(g) > 0.0 and abs(g["r2"].max() - kt.GENERAL_R2_MAX) < 1e-6 and np.all(g["a"] >= kt.A_EDGE)
        for which in range(3):
            c = kt.periodic_dim_case(32, which)
            print("own(periodic, D = 32, case %d): %.3g" % (which, kt.own_of(c)))
            assert kt.own_of(c) > 0.0


# ---- the comparison can fail: the two defects of csrc/kmat.hip it is there for, restated on the host ----------------------------------
LOG2E, LN2_LO = 1.4426950408889634, 1.90821492927058770002e-10


def _device_like(kind, defect):
    """the restatement of a stationary kind with the exponential of gps_exp_nonpos in one of two defective forms: "ln2_low": the low
    word of ln 2 dropped from the argument reduction (the result is off by the factor exp(k ln2_low)); "flush": the flush test at
    ki < -1020 instead of ki < -1021"""
    g = kt.grid(kind)
    k = np.round(g["a"] * LOG2E)
    if defect == "ln2_low":
        e = kt._exp(g["a"]) * np.exp(k * LN2_LO)
    else:
        e = np.where(k < -1020, 0.0, kt._exp(g["a"]))
    return g["pre"] * np.where(k < -1021, 0.0, e)


@pytest.mark.parametrize("kind", kt.STATIONARY)
def test_comparison_passes_the_restatement_and_fails_the_defects(kind, capsys):
    g = kt.grid(kind)
    own = kt.own_grid(kind)
    with capsys.disabled():
        kt.check(g["val"], g, own, what="restatement " + kind)
        # a device that flushes where it may: passes
        kt.check(np.where(np.round(g["a"] * LOG2E) < -1021, 0.0, g["val"]), g, own, what="restatement with the flush " + kind)
    for defect in ("ln2_low", "flush"):
        with pytest.raises(AssertionError):
            kt.check(_device_like(kind, defect), g, own, what="%s %s" % (defect, kind))
    # one entry far out wrong by a factor of two, invisible to a gate on max |K|
    bad = g["val"].copy()
    i, j = np.argwhere((g["a"] < -90.0) & (g["a"] >= kt.A_EDGE))[0]
    bad[i, j] *= 2.0
    assert abs(bad[i, j] - g["ref"][i, j]) < 1e-30
    with pytest.raises(AssertionError):
        kt.check(bad, g, own, what="factor two " + kind)
    # a tail entry that is not small, and a negative one
    for v in (2.0 ** -1019, -(2.0 ** -1060)):
        bad = g["val"].copy()
        i, j = np.argwhere(g["a"] < -720.0)[0]
        bad[i, j] = v * g["pre"][i, j]
        with pytest.raises(AssertionError):
            kt.check(bad, g, own, what="tail " + kind)
