"""The numpy reference of the Sum-of-RBF kernel expectations (tests/_psi_sum_ref.py) checked against itself on the CPU: its
gradient against central differences of its own long-double bound, its cross terms against their absence, and the one-part case
against tests/_psi_ref.py.  No GPU, no product code."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _psi_ref as pr  # noqa: E402
import _psi_sum_ref as ps  # noqa: E402

LD = np.longdouble
DIMS = [[0, 3], [1], [4, 2]]


def _case():
    d = pr.inputs(11, 6, 5, R=2, seed=21)
    parts = ps.make_parts(d, DIMS)
    return d, parts


def test_gradient_against_central_differences_in_long_double():
    """h = 1e-5 relative to O(1) inputs: truncation h^2 f''' / 6 ~ 1e-10, rounding eps_ld |F| / h ~ 1e-12 in long double: every
    block must agree to 1e-7 of its largest entry (at least 1e-7 absolute)."""
    d, parts = _case()
    noise = 0.3
    _, g = ps.bound_grad(parts, noise, d["Z"], d["mu"], d["S"], d["Y"], dtype=LD)
    h = LD(1e-5)

    def F(parts_=parts, noise_=noise, Z=d["Z"], mu=d["mu"], S=d["S"]):
        return ps.bound_ld(parts_, noise_, Z, mu, S, d["Y"], raw=True)

    def check(name, got, fd):
        got, fd = np.asarray(got, dtype=LD), np.asarray(fd, dtype=LD)
        err = float(np.max(np.abs(got - fd)))
        scale = max(1.0, float(np.max(np.abs(fd))))
        print("%s: err %.3g of |g|inf %.3g" % (name, err, scale))
        assert err <= 1e-7 * scale, (name, err)

    def with_part(i, key, val):
        out = [dict(p) for p in parts]
        out[i][key] = val
        return out

    for i, p in enumerate(parts):
        v = LD(p["var"])
        check("variance[%d]" % i, g["variance"][i], (F(parts_=with_part(i, "var", v + h)) - F(parts_=with_part(i, "var", v - h))) / (2 * h))
        fd = []
        for k in range(len(p["dims"])):
            lp, lm = np.asarray(p["ls"], dtype=LD).copy(), np.asarray(p["ls"], dtype=LD).copy()
            lp[k] += h; lm[k] -= h
            fd.append((F(parts_=with_part(i, "ls", lp)) - F(parts_=with_part(i, "ls", lm))) / (2 * h))
        check("lengthscales[%d]" % i, g["lengthscales"][i], fd)
    check("noise", g["noise"], (F(noise_=LD(noise) + h) - F(noise_=LD(noise) - h)) / (2 * h))
    for name, key in (("Z", "Z"), ("X_mean", "mu"), ("X_var", "S")):
        base = np.asarray(d[key], dtype=LD)
        fd = np.zeros(base.shape, dtype=LD)
        for idx in np.ndindex(*base.shape):
            a, b = base.copy(), base.copy()
            a[idx] += h; b[idx] -= h
            fd[idx] = (F(**{key: a}) - F(**{key: b})) / (2 * h)
        check(name, g[name], fd)


def test_cross_terms_matter():
    d, parts = _case()
    full = ps.psi2n(parts, d["Z"], d["mu"], d["S"]).sum(0)
    bare = ps.psi2n(parts, d["Z"], d["mu"], d["S"], cross=False).sum(0)
    assert np.max(np.abs(full - bare) / np.abs(full)) > 0.1
    # ... and they are what the definition says: E[k(z, x) k(x, z')] of the summed kernel factorises over disjoint columns
    T = ps.part_psi1(parts, d["Z"], d["mu"], d["S"])
    want = bare + sum(T[i].T @ T[j] + T[j].T @ T[i] for i in range(3) for j in range(i + 1, 3))
    assert np.max(np.abs(full - want) / np.abs(want)) <= 64 * np.finfo(float).eps


def test_one_part_over_all_dimensions_is_the_single_rbf():
    d = pr.inputs(11, 6, 5, R=2, seed=21)
    parts = [{"var": d["var"], "ls": d["ls"], "dims": list(range(5))}]
    assert np.array_equal(ps.psi1(parts, d["Z"], d["mu"], d["S"]), pr.psi1(d["var"], d["ls"], d["Z"], d["mu"], d["S"]))
    assert np.array_equal(ps.psi2n(parts, d["Z"], d["mu"], d["S"], cross=False),
                          pr.psi2n(d["var"], d["ls"], d["Z"], d["mu"], d["S"]))
    a = dict(noise=0.3, Z=d["Z"], mu=d["mu"], S=d["S"], Y=d["Y"])
    Xs = np.random.default_rng(5).standard_normal((4, 5))
    one = pr.bound_ld(var=d["var"], ls=d["ls"], Xnew=Xs, **a)
    many = ps.bound_ld(parts, Xnew=Xs, **a)
    for x, y in zip(one, many):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    F1, g1 = pr.bound_grad(var=d["var"], ls=d["ls"], dtype=LD, **a)
    F2, g2 = ps.bound_grad(parts, dtype=LD, **a)
    # the gradient adds the same long-double terms in another order (part by part): equal up to the final rounding to fp64
    assert F1 == F2
    g2 = dict(g2, variance=g2["variance"][0], lengthscales=g2["lengthscales"][0])
    for kk in g1:
        a_, b_ = np.asarray(g1[kk]), np.asarray(g2[kk])
        assert np.max(np.abs(a_ - b_)) <= 2 * np.finfo(float).eps * np.max(np.abs(a_)), kk
