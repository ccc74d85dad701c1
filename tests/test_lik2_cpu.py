"""Gamma, Beta and Ordinal of gpflowSlim.likelihoods (host numpy) against the restatement of the reference in tests/_lik_ref2.py,
and the restatement itself pinned independently: mpmath integrals at 50 digits and central differences of its analytic
derivatives (what the device kernels are then compared with, tests/test_gpu_lik2.py), as tests/test_lik_cpu.py does for the
other kinds and with its gates.  Also what the Python layer refuses before any device call, and the layout of the descriptor
struct against the header.  No GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _lik_ref2 as ref  # noqa: E402

ULP = 64 * np.finfo(float).eps          # tests/test_lik_cpu.py: same formulas, same nodes; sums of 20 terms of mixed sign


@pytest.fixture(scope="module")
def lk():
    from gpflowSlim import likelihoods
    return likelihoods


def _make(lk, kind, params):
    if kind == "gamma":
        m = lk.Gamma()
        m._shape.assign(params[0])
    elif kind == "beta":
        m = lk.Beta(scale=params[0])
    else:
        m = lk.Ordinal(params[1])
        m._sigma.assign(params[0])
    return m


def _close(a, b, tol=ULP):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))
    assert err <= tol, err


@pytest.mark.parametrize("kind", ref.KINDS)
def test_classes_match_restatement(lk, kind):
    rng = np.random.default_rng(12)
    k = 2
    mu, var, Y, params = ref.sample_inputs(kind, 60, k, rng, var_hi=4.0)
    like = _make(lk, kind, params)
    assert like.num_gauss_hermite_points == 20 and len(like.parameters) == 1
    assert abs(float(np.squeeze(like.parameters[0].value)) - params[0]) <= 8 * np.finfo(float).eps * params[0]   # (through the transform)
    F = rng.standard_normal((60, k)) * (3.0 if kind == "ordinal" else 1.0)
    _close(like.logp(F, Y), ref.logp(kind, params, F, Y))
    _close(like.variational_expectations(mu, var, Y), ref.varexp(kind, params, mu, var, Y))
    cm, cv = ref.cond_mean_var(kind, params, F)
    _close(like.conditional_mean(F), cm); _close(like.conditional_variance(F), cv)
    _close(like.predict_density(mu, var, Y), ref.predict_density(kind, params, mu, var, Y))
    m1, v1 = like.predict_mean_and_var(mu, var)                  # the generic host quadrature of the base class
    x, w = ref.gh(20)
    X = x[None, :] * np.sqrt(2.0 * var.reshape(-1, 1)) + mu.reshape(-1, 1)
    cmX, cvX = ref.cond_mean_var(kind, params, X)
    E = (cmX @ w).reshape(mu.shape)
    _close(m1, E, 1e-12); _close(v1, ((cvX + cmX ** 2) @ w).reshape(mu.shape) - E ** 2, 1e-9)   # (E[y^2] - E[y]^2 cancels)
    if kind == "ordinal":
        phi = like._make_phi(F)
        assert phi.shape == (F.size, len(params[1]) + 1)
        _close(phi.sum(1), np.full(F.size, 1 - 2e-3), 1e-14)     # (the squashed probit telescopes to probit(inf) - probit(-inf))
        _close(np.log(phi[np.arange(F.size), Y.astype(int).ravel()] + 1e-6).reshape(F.shape), like.logp(F, Y), 1e-9)


def test_device_spec_and_links(lk):
    g, b, o = lk.Gamma(), lk.Beta(scale=2.5), lk.Ordinal(np.array([-1.0, 0.0, 2.0]))
    assert g._device_spec()[:2] == (6, [1.0]) and g._device_spec()[2] is g._shape
    assert b._device_spec()[:2] == (7, [2.5]) and b._device_spec()[2] is b._scale
    kind, params, trainable, edges = o._device_spec()
    assert (kind, params) == (8, [1.0]) and trainable is o._sigma and np.array_equal(edges, [-1.0, 0.0, 2.0])
    assert o.num_bins == 4
    assert lk.Gamma(invlink=np.square)._device_spec() is None          # another link keeps the host fallback
    assert lk.Beta(invlink=lambda f: 1 / (1 + np.exp(-f)))._device_spec() is None
    for like in (g, b, o):
        assert like.parameters[0].transform is not None and float(np.squeeze(like.parameters[0].value)) > 0


def test_value_errors_before_any_device_call(lk):
    from gpflowSlim import _abi, _backend as be
    edges = np.array([-1.0, 0.5, 2.0])
    with pytest.raises(ValueError, match="bin edges"):
        _abi.make_lik(8, [1.0], 20, edges=np.linspace(-3, 3, 33))
    with pytest.raises(ValueError, match="bin edges"):
        _abi.make_lik(8, [1.0], 20, edges=np.zeros(0))
    with pytest.raises(ValueError, match="bin edges"):
        _abi.make_lik(8, [1.0], 20)
    desc, keep = _abi.make_lik(8, [0.7], 20, edges=edges)
    assert desc.n_edges == 3 and [desc.edges[j] for j in range(3)] == list(edges) and keep[2] is not None
    desc0, keep0 = _abi.make_lik(7, [2.0], 20)
    assert desc0.n_edges == 0 and not desc0.edges and len(keep0) == 2
    for bad in ([[0.0], [4.0]], [[1.5], [2.0]], [[-1.0], [0.0]], [[np.nan], [1.0]]):
        with pytest.raises(ValueError, match="Ordinal labels"):
            be._need_ordinal_labels(desc, np.array(bad))
        with pytest.raises(ValueError, match="Ordinal labels"):
            lk.Ordinal(edges).logp(np.zeros((2, 1)), np.array(bad))
    be._need_ordinal_labels(desc, np.array([[0.0], [3.0]]))
    be._need_ordinal_labels(desc0, np.array([[0.5], [7.0]]))               # (only Ordinal has labels)
    # a model hands a table that is too long to make_lik, which refuses it
    import gpflowSlim as gpf
    X = np.linspace(0, 1, 12)[:, None]; Y = np.floor(X * 3.99)
    m = gpf.models.SVGP(X, Y, gpf.kernels.RBF(1), lk.Ordinal(np.linspace(-3, 3, 40)), Z=X[:4].copy())
    with pytest.raises(ValueError, match="bin edges"):
        m._device_lik()
    (d2, _), trainable = gpf.models.SVGP(X, Y, gpf.kernels.RBF(1), lk.Ordinal(edges), Z=X[:4].copy())._device_lik()
    assert d2.kind == 8 and d2.n_edges == 3 and d2.n_gh == 20 and trainable is not None


def test_lik_desc_layout_matches_header(tmp_path):
    """sizeof and the offsets of every field of gps_lik_t as a C++ compiler sees the header, against the ctypes mirror"""
    from gpflowSlim._abi import LikDesc
    root = os.path.dirname(HERE)
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "gpflowslim_hip.h"\n'
                   'int main() { std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d\\n", sizeof(gps_lik_t), offsetof(gps_lik_t, kind), '
                   'offsetof(gps_lik_t, n_gh), offsetof(gps_lik_t, param), offsetof(gps_lik_t, gh_x), offsetof(gps_lik_t, gh_w), '
                   'offsetof(gps_lik_t, n_edges), offsetof(gps_lik_t, edges), (int)GPS_LIK_GAMMA, (int)GPS_LIK_BETA, '
                   '(int)GPS_LIK_ORDINAL, (int)GPS_LIK_MAX_EDGES); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["g++", "-O0", "-I", os.path.join(root, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    mine = [ctypes.sizeof(LikDesc)] + [getattr(LikDesc, f).offset for f in ("kind", "n_gh", "param", "gh_x", "gh_w", "n_edges", "edges")]
    assert got[:8] == mine == [72, 0, 4, 8, 40, 48, 56, 64]
    from gpflowSlim import _abi, likelihoods
    assert got[8:] == [likelihoods.LIK_GAMMA, likelihoods.LIK_BETA, likelihoods.LIK_ORDINAL, _abi.LIK_MAX_EDGES] == [6, 7, 8, 32]
    assert [likelihoods.LIK_GAUSSIAN, likelihoods.LIK_BERNOULLI, likelihoods.LIK_POISSON, likelihoods.LIK_EXPONENTIAL,
            likelihoods.LIK_STUDENT_T, likelihoods.LIK_MULTICLASS] == list(range(6))


# ---- the restatement itself ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ref.KINDS)
def test_restatement_against_mpmath(kind):
    """The 100-node rule (Gamma: the closed form) against 50-digit integrals of log p(y | f) N(f; mu, var).  Gate 1e-4 as in
    tests/test_lik_cpu.py: what this pins is the integrand (link, squash, floor, density constants), not the rule's convergence,
    which on the squashed probit is algebraic."""
    import mpmath as mp
    mp.mp.dps = 50
    c = 1 - mp.mpf("2e-3")
    pr = lambda f: (1 + mp.erf(f / mp.sqrt(2))) / 2 * c + mp.mpf("1e-3")
    edges = [-1.0, 0.25, 1.5]
    cases = {"gamma": [(0.3, 0.5, 1.3, 0.5), (-1.2, 2.0, 0.2, 1.0), (0.0, 0.05, 4.0, 3.0)],
             "beta": [(0.3, 0.5, 0.2, 3.0), (-1.2, 2.0, 0.9, 0.05), (0.4, 0.05, 0.0, 200.0), (1.0, 1.0, 1.0, 0.7)],
             "ordinal": [(0.3, 0.5, 0, 0.7), (-1.2, 2.0, 3, 1.0), (0.0, 0.05, 1, 0.4), (2.0, 1.0, 2, 2.0), (6.0, 0.3, 0, 0.5)]}[kind]
    for mu, var, y, par in cases:
        if kind == "gamma":
            params = [par]
            lp = lambda f: -par * f - mp.loggamma(par) + (par - 1) * mp.log(y) - y * mp.exp(-f)
        elif kind == "beta":
            params = [par]
            yc = min(max(mp.mpf(y), mp.mpf("1e-6")), 1 - mp.mpf("1e-6"))

            def lp(f):
                a = pr(f) * par
                b = par - a
                return (a - 1) * mp.log(yc) + (b - 1) * mp.log(1 - yc) + mp.loggamma(par) - mp.loggamma(a) - mp.loggamma(b)
        else:
            params = [par, np.array(edges)]
            hi = pr(mp.inf) if y == len(edges) else None
            lo = pr(-mp.inf) if y == 0 else None
            lp = lambda f: mp.log((hi if hi is not None else pr((edges[y] - f) / par))
                                  - (lo if lo is not None else pr((edges[y - 1] - f) / par)) + mp.mpf("1e-6"))
        sd = mp.sqrt(var)
        exact = mp.quad(lambda f: lp(f) * mp.npdf(f, mu, sd), [mu - 12 * sd, mu - 3 * sd, mu, mu + 3 * sd, mu + 12 * sd])
        got = ref.varexp(kind, params, np.array([[mu]]), np.array([[var]]), np.array([[float(y)]]), n_gh=100)[0, 0]
        assert abs(got - float(exact)) <= 1e-4 * max(1.0, abs(float(exact))), (kind, mu, var, y, par, got, float(exact))


def _mp_logp(kind, params, f, y):
    """tests/_lik_ref2.logp of one point at mpmath's working precision (the constants are the doubles the restatement uses)"""
    import mpmath as mp
    if kind != "ordinal":
        return mp.mpf(float(ref.logp(kind, params, np.array([[float(f)]]), np.array([[y]]))[0, 0]))
    sigma, edges, y = mp.mpf(params[0]), params[1], int(y)
    pr = lambda z: (1 + mp.erf(z / mp.sqrt(2))) / 2 * (1 - mp.mpf(2e-3)) + mp.mpf(1e-3)
    hi = pr(mp.inf) if y == len(edges) else pr(mp.mpf(float(edges[y])) / sigma - f / sigma)
    lo = pr(-mp.inf) if y == 0 else pr(mp.mpf(float(edges[y - 1])) / sigma - f / sigma)
    return mp.log(hi - lo + mp.mpf(1e-6))


def _mp_varexp(kind, params, mu, var, y, n_gh=20):
    """the 20-node rule of one point summed at mpmath's working precision over the double nodes and weights"""
    import mpmath as mp
    x, w = ref.gh(n_gh)
    sd = mp.sqrt(2 * mp.mpf(var))
    return mp.fsum(mp.mpf(float(wh)) * _mp_logp(kind, params, mp.mpf(mu) + sd * mp.mpf(float(xh)), y) for xh, wh in zip(x, w))


@pytest.mark.parametrize("kind,param,n_edges", [("gamma", 0.5, 0), ("gamma", 3.0, 0), ("beta", 0.05, 0), ("beta", 3.0, 0),
                                                 ("beta", 200.0, 0), ("ordinal", 0.7, 1), ("ordinal", 0.7, 3), ("ordinal", 1.3, 32)])
def test_analytic_derivatives_against_central_differences(kind, param, n_edges):
    """Step and gate of tests/test_lik_cpu.py; the parameter derivative for all three kinds.  Two departures in how the
    differences are TAKEN, neither in what they are held to.  They are taken of the point's own term: differencing the sum over
    all 24 points instead adds eps |sum| / h of rounding, which at h = 1e-6 var = 1e-8 and Gamma's terms of exp(var / 2) = e^5 is
    as large as the gate.  And Ordinal's are taken at 50 digits (same formula, same double nodes and weights): in a bin's far
    tail log(P + 1e-6) amplifies the rounding of the two probits by 1e6, to 1e-10 in log p, and a difference of that over a
    step of 1e-8 is noise of 1e-2 -- the analytic derivative has no such amplification, so in double the check would measure
    the difference quotient, not the derivative."""
    import mpmath as mp
    mp.mp.dps = 50
    rng = np.random.default_rng(22)
    k = 2
    mu, var, Y, params = ref.sample_inputs(kind, 12, k, rng, var_lo=1e-2, var_hi=10.0, param=param, n_edges=n_edges)
    ve, dmu, dvar, dpar = ref.varexp_grad(kind, params, mu, var, Y)
    _close(ve, ref.varexp(kind, params, mu, var, Y), 0.0)
    assert np.all(np.isfinite(ve)) and np.all(np.isfinite(dmu)) and np.all(np.isfinite(dvar)) and np.isfinite(dpar)
    h = 1e-6 * params[0]
    p_hi, p_lo = [params[0] + h] + params[1:], [params[0] - h] + params[1:]

    def one(i, q, m, v, p=params):
        if kind == "ordinal":
            return _mp_varexp(kind, p, m, v, Y[i, q])
        return ref.varexp(kind, p, np.array([[m]]), np.array([[v]]), Y[i:i + 1, q:q + 1])[0, 0]

    def point(i, q, f, p=params):
        return _mp_logp(kind, p, mp.mpf(f), Y[i, q])

    g, gp = ref._dlogp(kind, params, mu, Y)                       # the pointwise derivatives (what gps_lik_logp is compared with)
    fd_par = 0.0
    for i in range(mu.shape[0]):
        for q in range(k):
            m0, v0 = mu[i, q], var[i, q]
            hm = 1e-6 * max(1.0, abs(m0)); hv = 1e-6 * v0
            fd = float((one(i, q, m0 + hm, v0) - one(i, q, m0 - hm, v0)) / (2 * hm))
            assert abs(dmu[i, q] - fd) <= 2e-6 * max(1.0, abs(fd)), ("dmu", i, q, dmu[i, q], fd)
            fd = float((one(i, q, m0, v0 + hv) - one(i, q, m0, v0 - hv)) / (2 * hv))
            assert abs(dvar[i, q] - fd) <= 2e-6 * max(1.0, abs(fd)), ("dvar", i, q, dvar[i, q], fd)
            fd_par += float((one(i, q, m0, v0, p_hi) - one(i, q, m0, v0, p_lo)) / (2 * h))
            fd = float((point(i, q, m0 + hm) - point(i, q, m0 - hm)) / (2 * hm))
            assert abs(g[i, q] - fd) <= 2e-6 * max(1.0, abs(fd)), ("dlogp/df", i, q, g[i, q], fd)
            fd = float((point(i, q, m0, p_hi) - point(i, q, m0, p_lo)) / (2 * h))
            assert abs(gp[i, q] - fd) <= 2e-6 * max(1.0, abs(fd)), ("dlogp/dparam", i, q, gp[i, q], fd)
    assert abs(dpar - fd_par) <= 2e-6 * max(1.0, abs(fd_par)), (dpar, fd_par)
