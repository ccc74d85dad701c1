"""Analytic fp64 reference (numpy / scipy / LAPACK) for the gradient of the exact-GP log-marginal likelihood, for the tests of
gps_gpr_lml_grad above the sizes the oracle's central differences reach (tests/test_gpu_grad_large.py) and, first, for its
own tests (tests/test_grad_ref_cpu.py).

    d LML / d theta = 1/2 sum((a a^T - R K_y^-1) o dK/dtheta),   a = K_y^-1 Y,   K_y = K + s2 I

K is the oracle's (oracle/gp_oracle.py::K, the reference's op order); K_y^-1 comes from LAPACK's Cholesky factor (cho_factor;
a by cho_solve, the full inverse by dpotri on the same factor -- a third of the flop of cho_solve against the identity).
dK/dtheta is ANALYTIC and differentiates exactly what orc.K computes: the clamp of r2 at 0 (kernels.py:421), r = sqrt(r2 +
1e-12) of the Matern / Exponential kinds (:424-426), Periodic's sum_d sin^2(pi (x_d - x'_d) / p) / l_d^2 (:813-819), the
left folds of Sum and Product (:1071-1084), White and Constant.  One parameter at a time: the peak is a handful of N x N
arrays (N = 12288: 1.2 GB each).

Which entry of theta drives which field of which primitive is found by probing spec_fn (one entry changed, the two spec trees
compared), so that the same spec_fn / theta pairs the oracle's gpr_lml_grad takes are taken here.

The reference reports its own spread, in units of max(1, |g|_inf): every slot sum contracted in fp64 and again with a
np.longdouble accumulator (up to N = 4608 the products are long double as well; above that they are fp64 products summed in long
double), and for N <= 3072 the whole gradient once more with K_y^-1 = Q diag(1 / lambda) Q^T from eigh instead of Cholesky.
"""
import collections
import os
import sys

import numpy as np
import scipy.linalg as sl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import oracle.gp_oracle as orc  # noqa: E402

GradRef = collections.namedtuple("GradRef", "lml g g_noise a spread")
EIGH_MAX_N = 3072
LONGDOUBLE_PRODUCT_MAX_N = 4608
_STATIONARY = ("rbf", "matern12", "matern32", "matern52", "exponential")


# ---------------------------------------------------------------------------------------------------------------------------
# which theta entry drives which leaf field
def _walk(spec, path=()):
    """(path, leaf spec) of every primitive of a spec tree; numeric children of Sum / Product are not parameters here"""
    if isinstance(spec, (int, float)):
        return
    if spec["type"] == "nkn":
        raise NotImplementedError("no analytic form for a Neural Kernel Network: use orc.gpr_lml_grad")
    if spec["type"] in ("sum", "product"):
        for i, ch in enumerate(spec["children"]):
            for item in _walk(ch, path + (i,)):
                yield item
        return
    yield path, spec


def _fields(leaf):
    """{(field, index or None): value} of a primitive"""
    out = {("variance", None): float(leaf["variance"])}
    if "lengthscales" in leaf:
        ls = np.asarray(leaf["lengthscales"], dtype=np.float64)
        if ls.ndim == 0:
            out[("lengthscales", None)] = float(ls)
        else:
            for q in range(ls.size):
                out[("lengthscales", q)] = float(ls[q])
    if "period" in leaf:
        out[("period", None)] = float(leaf["period"])
    return out


def theta_map(spec_fn, theta):
    """{(path, field, index): [theta entries]}: entry p is changed alone and the two spec trees are compared"""
    theta = np.asarray(theta, dtype=np.float64)
    base = {path: _fields(leaf) for path, leaf in _walk(spec_fn(theta))}
    out = {}
    for p in range(theta.size):
        t = theta.copy()
        t[p] = 1.5 * t[p] + 0.25
        hit = 0
        for path, leaf in _walk(spec_fn(t)):
            for key, val in _fields(leaf).items():
                if val != base[path][key]:
                    out.setdefault((path,) + key, []).append(p)
                    hit += 1
        if not hit:
            raise ValueError("theta[%d] drives no primitive parameter of the spec" % p)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# dK / d(field) of one primitive, one parameter at a time
def _leaf_derivatives(leaf, X):
    """yields ((field, index), dK_leaf / d field[index]) -- N x N each, formed when asked for"""
    n = X.shape[0]
    t, v = leaf["type"], float(leaf["variance"])
    if t == "white":
        yield ("variance", None), np.eye(n)
        return
    if t == "constant":
        yield ("variance", None), np.ones((n, n))
        return
    Kl = orc.K(leaf, X)
    yield ("variance", None), Kl / v
    Xs, _ = orc._slice(leaf, X, None)
    ls = np.asarray(leaf["lengthscales"], dtype=np.float64)
    if t == "periodic":
        p = float(leaf["period"])
        lsd = np.broadcast_to(ls, (Xs.shape[1],))
        if ls.ndim == 0:
            S = np.zeros((n, n))
            for q in range(Xs.shape[1]):
                S += np.square(np.sin(np.pi * (Xs[:, q:q + 1] - Xs[:, q:q + 1].T) / p) / lsd[q])
            yield ("lengthscales", None), Kl * S / float(ls)
            del S
        else:
            for q in range(ls.size):
                sq = np.square(np.sin(np.pi * (Xs[:, q:q + 1] - Xs[:, q:q + 1].T) / p))
                if ls.size == 1 and Xs.shape[1] > 1:
                    for q2 in range(1, Xs.shape[1]):
                        sq += np.square(np.sin(np.pi * (Xs[:, q2:q2 + 1] - Xs[:, q2:q2 + 1].T) / p))
                yield ("lengthscales", q), Kl * sq / lsd[q] ** 3
        # d/dp of -1/2 sum_q sin^2(arg_q) / l_q^2 with arg_q = pi (x_q - x'_q) / p: d arg / dp = -arg / p
        T = np.zeros((n, n))
        for q in range(Xs.shape[1]):
            arg = np.pi * (Xs[:, q:q + 1] - Xs[:, q:q + 1].T) / p
            T += np.sin(2.0 * arg) * arg / (2.0 * p * lsd[q] ** 2)
        yield ("period", None), Kl * T
        return
    if t not in _STATIONARY:
        raise ValueError("unknown kernel type %r" % t)
    r2 = orc.square_dist(Xs, None, ls)                       # the GEMM form, clamped at 0: what K() itself used
    if t == "rbf":
        base = -0.5 * Kl                                     # dK / d r2
    else:
        r = np.sqrt(r2 + 1e-12)
        if t == "matern12":
            dKdr = -Kl
        elif t == "exponential":
            dKdr = -0.5 * Kl
        elif t == "matern32":
            dKdr = -3.0 * v * r * np.exp(-np.sqrt(3.) * r)
        else:
            dKdr = -(5. / 3.) * v * r * (1.0 + np.sqrt(5.) * r) * np.exp(-np.sqrt(5.) * r)
        base = dKdr / (2.0 * r)                              # dK / d r2 through r = sqrt(r2 + 1e-12)
        del r, dKdr
    del Kl
    if ls.size == 1:
        # r2 = |x - x'|^2 / l^2 (clamped: the derivative of the clamped value is that of r2 where r2 > 0 and 0 where it is 0)
        yield ("lengthscales", None if ls.ndim == 0 else 0), base * (r2 * (-2.0 / float(ls.reshape(-1)[0])))
        return
    base *= (r2 > 0.0)                                       # clamp active: r2 is the constant 0 there
    del r2
    for q in range(ls.size):
        yield ("lengthscales", q), base * (np.square(Xs[:, q:q + 1] - Xs[:, q:q + 1].T) * (-2.0 / ls[q] ** 3))


def _leaves_with_cofactors(spec, X, path=(), cof=None):
    """(path, leaf, cofactor): d K_total / d K_leaf, entry by entry -- the product of the siblings under every Product on the
    way down (None: 1)"""
    if isinstance(spec, (int, float)):
        return
    if spec["type"] == "sum":
        for i, ch in enumerate(spec["children"]):
            for item in _leaves_with_cofactors(ch, X, path + (i,), cof):
                yield item
        return
    if spec["type"] == "product":
        for i, ch in enumerate(spec["children"]):
            if isinstance(ch, (int, float)):
                continue
            c = cof
            for j, other in enumerate(spec["children"]):
                if j != i:
                    Kj = orc.K(other, X)
                    c = Kj if c is None else c * Kj
            for item in _leaves_with_cofactors(ch, X, path + (i,), c):
                yield item
        return
    yield path, spec, cof


def _contract(M, dK, long_products):
    """sum(M o dK) with an fp64 (pairwise) and with a long double accumulator"""
    if not long_products:
        P = M * dK
        return float(P.sum()), float(P.sum(dtype=np.longdouble))
    s64, sld = float((M * dK).sum()), np.longdouble(0)
    for s in range(0, M.shape[0], 256):
        sld += (M[s:s + 256].astype(np.longdouble) * dK[s:s + 256].astype(np.longdouble)).sum()
    return s64, float(sld)


def _slot_sums(spec, X, W, tmap, n_theta):
    """1/2 sum(W o dK/dtheta_p) for every p, twice (fp64 / long double accumulation)"""
    g64, gld = np.zeros(n_theta), np.zeros(n_theta)
    long_products = X.shape[0] <= LONGDOUBLE_PRODUCT_MAX_N
    for path, leaf, cof in _leaves_with_cofactors(spec, X):
        M = W if cof is None else W * cof
        for (field, idx), dK in _leaf_derivatives(leaf, X):
            targets = tmap.get((path, field, idx))
            if not targets:
                continue                                     # a field no theta entry drives
            a, b = _contract(M, dK, long_products)
            del dK
            for p in targets:
                g64[p] += 0.5 * a
                gld[p] += 0.5 * b
    return g64, gld


# ---------------------------------------------------------------------------------------------------------------------------
def lml_grad_ref(spec_fn, theta, X, Y, noise, inverse_route=None):
    """GradRef(lml, g [theta.size], g_noise, a [N, R], spread): the log-marginal likelihood of models/gpr.py:69-72, its
    gradient with respect to the constrained kernel parameters theta (as spec_fn(theta) -> spec consumes them) and to the noise
    variance, and a = K_y^-1 Y.  spread: {"contraction", "inverse_route" (None above EIGH_MAX_N rows unless asked for),
    "cond" (of K_y, from the same eigenvalues, or None)}."""
    theta = np.asarray(theta, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64); Y = np.asarray(Y, dtype=np.float64)
    n, R = Y.shape
    noise = float(noise)
    spec = spec_fn(theta)
    tmap = theta_map(spec_fn, theta)
    if inverse_route is None:
        inverse_route = n <= EIGH_MAX_N
    Ky = orc.K(spec, X)
    Ky[np.diag_indices(n)] += noise
    ev = Q = None
    if inverse_route:
        ev, Q = np.linalg.eigh(Ky)
    c, low = sl.cho_factor(Ky, lower=True, overwrite_a=True, check_finite=False)
    del Ky
    a = sl.cho_solve((c, low), Y, check_finite=False)
    lml = -0.5 * n * R * np.log(2 * np.pi) - R * float(np.sum(np.log(np.diag(c)))) - 0.5 * float(np.sum(Y * a))
    W, info = sl.lapack.dpotri(c, lower=1, overwrite_c=1)
    if info != 0:
        raise np.linalg.LinAlgError("dpotri: info = %d" % info)
    del c
    W = np.tril(W)
    W += np.tril(W, -1).T                                    # K_y^-1, both triangles
    W *= -float(R)
    W += a @ a.T                                             # a a^T - R K_y^-1
    gn64, gnld = 0.5 * float(np.trace(W)), 0.5 * float(np.sum(np.diag(W), dtype=np.longdouble))
    g64, gld = _slot_sums(spec, X, W, tmap, theta.size)
    del W
    scale = max(1.0, float(np.abs(g64).max()) if g64.size else 0.0)
    nscale = max(1.0, abs(gn64))                             # (the noise slot in units of its own size, as it is gated)
    spread = {"contraction": max((float(np.abs(g64 - gld).max()) if g64.size else 0.0) / scale, abs(gn64 - gnld) / nscale),
              "inverse_route": None, "cond": None}
    if inverse_route:
        Qs = Q / ev
        We = Qs @ Q.T
        ae = Qs @ (Q.T @ Y)
        del Qs, Q
        We *= -float(R)
        We += ae @ ae.T
        ge, _ = _slot_sums(spec, X, We, tmap, theta.size)
        gne = 0.5 * float(np.trace(We))
        del We
        spread["inverse_route"] = max((float(np.abs(g64 - ge).max()) if g64.size else 0.0) / scale, abs(gn64 - gne) / nscale)
        spread["cond"] = float(ev[-1] / ev[0])
    return GradRef(lml, g64, gn64, a, spread)


_CACHE = {}


def cached(key, make):
    """Module-level cache (as _CONC_REF in test_gpu_kernels.py): the schedule variants of one problem share one CPU factorisation."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------------------------------
# cases shared by tests/test_grad_ref_cpu.py and tests/test_gpu_grad_large.py, next to those of test_gpu_grad.py::_cases
def six_case(gpf, d=3):
    """(kernel, theta, spec_fn) of test_gpu_grad.py::test_gradient_six_primitive_sum_product"""
    c = orc.constrained
    k = gpf.kernels
    ls = np.linspace(0.8, 1.7, d)
    kern = (k.RBF(d, variance=1.3, lengthscales=ls, ARD=True) * k.Periodic(d, period=2.5, variance=0.8, lengthscales=1.2)
            + k.Matern52(d, variance=0.9, lengthscales=1.4) * k.Matern12(1, variance=0.7, lengthscales=2.0, active_dims=[1])
            + k.Matern32(d, variance=1.1, lengthscales=1.3) + k.White(d, variance=0.2))
    theta = np.concatenate([[c(1.3)], c(ls), [c(0.8), c(1.2), c(2.5)], [c(0.9), c(1.4)], [c(0.7), c(2.0)], [c(1.1), c(1.3)], [c(0.2)]])

    def fn(t):
        return {"type": "sum", "children": [
            {"type": "product", "children": [{"type": "rbf", "variance": t[0], "lengthscales": t[1:1 + d], "input_dim": d},
                                             {"type": "periodic", "variance": t[1 + d], "lengthscales": t[2 + d], "period": t[3 + d], "input_dim": d}]},
            {"type": "product", "children": [{"type": "matern52", "variance": t[4 + d], "lengthscales": t[5 + d], "input_dim": d},
                                             {"type": "matern12", "variance": t[6 + d], "lengthscales": t[7 + d], "input_dim": 1, "active_dims": [1]}]},
            {"type": "matern32", "variance": t[8 + d], "lengthscales": t[9 + d], "input_dim": d},
            {"type": "white", "variance": t[10 + d]}]}
    return kern, theta, fn


def rbf_ard_case(gpf, d, variance=1.1, scale=1.0):
    """RBF ARD with the length-scales of the benchmark's workload (sqrt(d) times 0.8 .. 1.2)"""
    c = orc.constrained
    ls = scale * np.sqrt(d) * np.linspace(0.8, 1.2, d)
    kern = gpf.kernels.RBF(d, variance=variance, lengthscales=ls, ARD=True)
    theta = np.concatenate([[c(variance)], c(ls)])
    return kern, theta, lambda t: {"type": "rbf", "variance": t[0], "lengthscales": t[1:], "input_dim": d}


def case(gpf, name, d):
    """(kernel, theta, spec_fn) by name: test_gpu_grad.py::KINDS, "six", "rbf_ard_bench" """
    if name == "six":
        return six_case(gpf, d)
    if name == "rbf_ard_bench":
        return rbf_ard_case(gpf, d)
    from test_gpu_grad import _cases
    kern, theta, fn, _ = _cases(gpf, d)[name]()
    return kern, theta, fn


def block_separable(nc, per, d, seed, r=1):
    """nc clusters of `per` points 60 length-scales apart on a 4 x 4 x 4 grid, interleaved in memory, as
    test_gpu_parity.py::test_full_size_block_separable lays them out: every cross-cluster RBF covariance is exactly 0.
    Returns (X, Y, order, Xc, Yc, ls, shift): cluster k sits at Xc[k] + shift(k)."""
    rng = np.random.default_rng(seed)
    ls = np.sqrt(d) * np.ones(d)
    Xc = [rng.standard_normal((per, d)) for _ in range(nc)]
    w = rng.standard_normal((d, r)) / np.sqrt(d)
    Yc = [np.sin(x @ w) + 0.1 * rng.standard_normal((per, r)) for x in Xc]

    def shift(k):
        o = np.zeros((1, d))
        o[0, 0], o[0, 1], o[0, 2] = 60.0 * ls[0] * (k % 4), 60.0 * ls[1] * ((k // 4) % 4), 60.0 * ls[2] * (k // 16)
        return o
    order = rng.permutation(nc * per)
    X = np.concatenate([x + shift(k) for k, x in enumerate(Xc)])[order]
    Y = np.concatenate(Yc)[order]
    return X, Y, order, Xc, Yc, ls, shift


def data(n, d, r, seed):
    """seeded inputs and r DISTINCT output columns (a dropped or repeated column changes every slot)"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    Y = np.sin(X @ rng.standard_normal((d, r)) / np.sqrt(d) * 1.5) + 0.1 * rng.standard_normal((n, r)) + 0.05 * np.arange(r)
    return X, Y


def low_noise_data(n, ratio, var=1.3):
    """two-dimensional inputs at noise / variance = ratio, laid out as test_gpu_parity.py::test_gpr_low_noise_sweep"""
    rng = np.random.default_rng(int(n + 1e7 * ratio))
    X = rng.uniform(-3.0, 3.0, (n, 2))
    noise = float(orc.constrained(ratio * var))
    Y = np.sin(X[:, :1]) * np.cos(0.5 * X[:, 1:2]) + np.sqrt(noise) * rng.standard_normal((n, 1))
    return X, Y, noise


NOISE = float(orc.constrained(0.1))
# (case name, N, D, R) of the cases of tests/test_gpu_grad_large.py up to EIGH_MAX_N rows (sections a, b, c and e of its docstring):
# tests/test_grad_ref_cpu.py asserts the reference's own spread on each
SMALL_CASES = ([("rbf_ard_bench", 2049, 8, 1), ("rbf_ard_bench", 2500, 8, 1), ("rbf_ard_bench", 640, 8, 1)]
               + [(k, 2500, 3, 1) for k in ("m52_plus_periodic", "m32_ard", "rbf_times_periodic_plus_white", "six")]
               + [("rbf_ard_bench", 2500, 8, 3), ("rbf_ard_bench", 2500, 8, 17), ("rbf_ard_bench", 2500, 8, 130), ("rbf_ard_bench", 1000, 8, 17)])


def problem(gpf, name, n, d, r, inverse_route=False):
    """(kernel, theta, spec_fn, X, Y, GradRef) of a named case at noise NOISE; the reference is cached"""
    kern, theta, fn = case(gpf, name, d)
    X, Y = data(n, d, r, seed=1000 * d + n + r)
    ref = cached((name, n, d, r, bool(inverse_route)), lambda: lml_grad_ref(fn, theta, X, Y, NOISE, inverse_route=inverse_route))
    return kern, theta, fn, X, Y, ref


# ---------------------------------------------------------------------------------------------------------------------------
# Neural Kernel Network: no analytic form; the oracle's own central differences, affordably
def nkn_theta(spec):
    """(theta, spec_fn) of an NKN spec in kern.parameters order -- every Linear layer's weights (row-major) and bias, then every
    primitive's variance, length-scales and period -- as test_gpu_grad.py::test_nkn_gradient_matches_oracle_and_finite_differences
    lays them out for orc.gpr_lml_grad"""
    import copy
    where = []
    for li, ly in enumerate(spec["layers"]):
        if ly[0] == "linear":
            where += [("W", li, idx) for idx in np.ndindex(np.shape(ly[1]))] + [("b", li, (o,)) for o in range(np.size(ly[2]))]
    for pi, ps in enumerate(spec["primitives"]):
        where.append(("variance", pi, None))
        if "lengthscales" in ps:
            where += [("lengthscales", pi, q) for q in range(np.atleast_1d(ps["lengthscales"]).size)]
        if "period" in ps:
            where.append(("period", pi, None))

    def get(sp, kind, i, idx):
        if kind == "W": return sp["layers"][i][1][idx]
        if kind == "b": return sp["layers"][i][2][idx]
        if kind == "lengthscales": return np.atleast_1d(sp["primitives"][i]["lengthscales"])[idx]
        return sp["primitives"][i][kind]

    def put(sp, kind, i, idx, v):
        if kind in ("W", "b"):
            ly = list(sp["layers"][i])
            k = 1 if kind == "W" else 2
            ly[k] = np.array(ly[k], dtype=np.float64); ly[k][idx] = v
            sp["layers"][i] = tuple(ly)
        elif kind == "lengthscales":
            ls = np.array(np.atleast_1d(sp["primitives"][i]["lengthscales"]), dtype=np.float64); ls[idx] = v
            sp["primitives"][i]["lengthscales"] = ls if ls.size > 1 else float(ls[0])
        else:
            sp["primitives"][i][kind] = v

    theta = np.array([get(spec, *w) for w in where], dtype=np.float64)

    def fn(t):
        sp = copy.deepcopy(spec)
        sp["layers"] = list(sp["layers"])
        for w, v in zip(where, t):
            put(sp, w[0], w[1], w[2], float(v))
        return sp
    fn.where, fn.put = where, put
    return theta, fn


def nkn_grad_oracle(spec, X, Y, noise, rel_step=1e-6):
    """orc.gpr_lml_grad for an NKN spec: the same formula, the same steps and central differences of the oracle's own network
    forward (orc.K per primitive, orc.nkn_forward; distances as differences, as orc.gpr_lml_grad forms them) -- made affordable at
    thousands of rows, where 2 x 83 whole kernel matrices are minutes: only the lower triangle of the symmetric K goes through
    the network; a perturbed primitive parameter rebuilds that primitive's K alone; a perturbed Linear entry changes ONE output
    column of its layer (and one of a Product layer behind it), which is set directly before orc.nkn_forward runs the remaining
    layers.  The differences therefore differ from orc.gpr_lml_grad's in rounding only (eps |K| / h ~ 1e-10 per entry):
    tests/test_grad_ref_cpu.py holds the two together at N = 160.  Returns (theta, g, g_noise, a)."""
    import copy
    theta, fn = nkn_theta(spec)
    n, R = Y.shape
    layers = list(spec["layers"])
    tri = np.tril_indices(n)
    saved, orc.SQUARE_DIST_MODE = orc.SQUARE_DIST_MODE, "diff"
    try:
        stacked = np.stack([np.asarray(orc.K(s, X), dtype=np.float64)[tri] for s in spec["primitives"]], 1)
        acts = [stacked]
        for ly in layers:
            acts.append(orc.nkn_forward([ly], acts[-1]))
        Ky = np.zeros((n, n))
        Ky[tri] = acts[-1][:, 0]
        Ky = Ky + np.tril(Ky, -1).T + np.eye(n) * noise
        Kinv = np.linalg.inv(Ky)
        del Ky
        a = Kinv @ Y
        W = a @ a.T - R * Kinv
        gn = 0.5 * np.trace(W)
        del Kinv
        Wf = 2.0 * W[tri]                                    # sum over both triangles of symmetric W o dK ...
        Wf[tri[0] == tri[1]] *= 0.5                          # ... the diagonal once
        del W
        g = np.zeros_like(theta)
        for p, (kind, i, idx) in enumerate(fn.where):
            h = rel_step * max(1.0, abs(theta[p]))
            out = []
            for sgn in (1.0, -1.0):
                if kind in ("W", "b"):
                    o = idx[0]
                    col = acts[i + 1][:, o] + (sgn * h) * (acts[i][:, idx[1]] if kind == "W" else 1.0)
                    nxt, c, rest = acts[i + 1], o, layers[i + 1:]
                    if rest and rest[0][0] == "product":
                        step = rest[0][1]
                        for o2 in range((o // step) * step, (o // step + 1) * step):
                            if o2 != o:
                                col = col * acts[i + 1][:, o2]
                        nxt, c, rest = acts[i + 2], o // step, rest[1:]
                    keep = nxt[:, c].copy()
                    nxt[:, c] = col
                    out.append(orc.nkn_forward(rest, nxt).reshape(-1).copy())
                    nxt[:, c] = keep
                else:
                    sp = {"primitives": [copy.deepcopy(s) for s in spec["primitives"]]}
                    fn.put(sp, kind, i, idx, theta[p] + sgn * h)
                    keep = stacked[:, i].copy()
                    stacked[:, i] = np.asarray(orc.K(sp["primitives"][i], X), dtype=np.float64)[tri]
                    out.append(orc.nkn_forward(layers, stacked).reshape(-1))
                    stacked[:, i] = keep
            g[p] = 0.5 * float(np.dot(Wf, (out[0] - out[1]) / (2 * h)))
        return theta, g, gn, a
    finally:
        orc.SQUARE_DIST_MODE = saved


# Handle.set_option has no getter: tests that switch schedules restore these, the defaults of csrc/gps_common.hpp (option name ->
# (member of gps_handle_s, default)); tests/test_grad_ref_cpu.py reads the header and fails the day one of them moves.
OPTION_DEFAULTS = {"trsv_wave": ("trsv_wave", 1), "potrf_lookahead": ("potrf_lookahead", 1), "potrf_rl_max": ("potrf_rl_max", 4096),
                   "gpr_aug_rows": ("gpr_aug_rows", -1), "trsm_panel": ("trsm_panel", 1), "gemm_force_tile": ("gemm_force_tb", 0),
                   "leaf_refine": ("leaf_refine", -1), "leaf_plain_kappa": ("leaf_plain_kappa", 1000.0),
                   "trsv_wave_refine": ("trsv_wave_refine", 1)}


def low_noise_problem(n, ratio, var=1.3):
    """(theta, spec_fn, GradRef with the inverse-route spread and cond) of the isotropic RBF on low_noise_data; cached"""
    X, Y, noise = low_noise_data(n, ratio, var)
    theta = np.array([orc.constrained(var), orc.constrained(0.8)])
    fn = lambda t: {"type": "rbf", "variance": t[0], "lengthscales": t[1], "input_dim": 2}
    return theta, fn, cached(("low_noise", n, ratio), lambda: lml_grad_ref(fn, theta, X, Y, noise, inverse_route=True))
