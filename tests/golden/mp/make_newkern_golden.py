"""50-digit pins of the Cosine and ArcCosine kernels, independent of tests/_kern_ref2.py (imports numpy and mpmath only).

The formulas of the reference's kernels.py:617-646 (Cosine; the active columns are sliced before they are divided by the
lengthscales) and :722-758 (ArcCosine, orders 0, 1, 2), and densities.py:81-94 for the GPR log-marginal likelihood, evaluated
with mpmath at 50 digits on n = 6 seeded points in d = 2 dimensions: K(X), K(X, X2), the likelihood, and its gradient in every
(constrained) parameter element and the noise by 1e-25 central differences of the 60-digit likelihood.  The jitter is the fp64
number 1e-15 and 1 - 2 jitter is exact.  The fp64 parameter values stored in the fixture are the ones the formulas were
evaluated with.
    python tests/golden/mp/make_newkern_golden.py        # rewrites tests/golden/mp/newkern.npz
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N, M, D = 6, 4, 2
NOISE = 0.3

# plain dicts of fp64 values; the parameter elements in kern.parameters order are PARAMS[type]
CASES = {
    "cosine_ard": {"type": "cosine", "dims": [0, 1], "variance": 1.3, "lengthscales": [0.7, 1.3], "weights": [0.9, -1.4]},
    "cosine_iso": {"type": "cosine", "dims": [0, 1], "variance": 0.8, "lengthscales": 1.2, "weights": [0.5, 1.1]},
    "cosine_sub": {"type": "cosine", "dims": [1], "variance": 1.1, "lengthscales": 0.9, "weights": [1.7]},
    "arc0_ard": {"type": "arccosine", "order": 0, "dims": [0, 1], "variance": 1.2, "bias_variance": 0.7, "weight_variances": [0.6, 1.5]},
    "arc1_ard": {"type": "arccosine", "order": 1, "dims": [0, 1], "variance": 0.9, "bias_variance": 1.1, "weight_variances": [1.4, 0.5]},
    "arc2_ard": {"type": "arccosine", "order": 2, "dims": [0, 1], "variance": 0.4, "bias_variance": 0.8, "weight_variances": [0.7, 0.9]},
    "arc0_iso": {"type": "arccosine", "order": 0, "dims": [0, 1], "variance": 0.7, "bias_variance": 1.3, "weight_variances": 0.8},
    "arc1_iso": {"type": "arccosine", "order": 1, "dims": [0, 1], "variance": 1.1, "bias_variance": 0.6, "weight_variances": 1.2},
    "arc2_iso": {"type": "arccosine", "order": 2, "dims": [0, 1], "variance": 0.5, "bias_variance": 0.9, "weight_variances": 0.6},
    "arc1_sub": {"type": "arccosine", "order": 1, "dims": [1], "variance": 1.0, "bias_variance": 0.5, "weight_variances": 1.3},
}
PARAMS = {"cosine": ("variance", "lengthscales", "weights"), "arccosine": ("variance", "bias_variance", "weight_variances")}


def _vec(mp, v, nd):
    v = list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v] * nd
    return [x if isinstance(x, mp.mpf) else mp.mpf(float(x)) for x in v]


def mp_kernel(mp, spec, x, y):
    nd = len(spec["dims"])
    xs = [mp.mpf(float(x[d])) for d in spec["dims"]]; ys = [mp.mpf(float(y[d])) for d in spec["dims"]]
    v = _vec(mp, spec["variance"], 1)[0]
    if spec["type"] == "cosine":                          # kernels.py:633-646, sliced first
        ls = _vec(mp, spec["lengthscales"], nd); w = _vec(mp, spec["weights"], nd)
        a = sum(p * q / l for p, q, l in zip(xs, w, ls)); b = sum(p * q / l for p, q, l in zip(ys, w, ls))
        return v * mp.cos(a - b)
    w = _vec(mp, spec["weight_variances"], nd); bias = _vec(mp, spec["bias_variance"], 1)[0]
    P = sum(q * p * r for q, p, r in zip(w, xs, ys)) + bias                                   # :722-725
    ni = sum(q * p * p for q, p in zip(w, xs)) + bias; nj = sum(q * r * r for q, r in zip(w, ys)) + bias
    jitter = mp.mpf(1e-15)
    theta = mp.acos(jitter + (1 - 2 * jitter) * P / mp.sqrt(ni) / mp.sqrt(nj))                # :752-754
    o = spec["order"]
    if o == 0:
        J = mp.pi - theta
    elif o == 1:
        J = mp.sin(theta) + (mp.pi - theta) * mp.cos(theta)
    else:
        J = 3 * mp.sin(theta) * mp.cos(theta) + (mp.pi - theta) * (1 + 2 * mp.cos(theta) ** 2)
    return v / mp.pi * J * mp.sqrt(ni) ** o * mp.sqrt(nj) ** o                                # :756-758


def mp_lml(mp, spec, X, Y, s2):
    """densities.py:81-94 as an mpmath number; spec and s2 may hold mpmath values"""
    n, r = Y.shape
    Km = mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            Km[i, j] = mp_kernel(mp, spec, X[i], X[j]) + (s2 if i == j else 0)
    L = mp.cholesky(Km)
    out = -mp.mpf(n * r) / 2 * mp.log(2 * mp.pi) - r * sum(mp.log(L[i, i]) for i in range(n))
    for q in range(r):
        alpha = mp.lu_solve(L, mp.matrix([float(v) for v in Y[:, q]]))
        out -= sum(a * a for a in alpha) / 2
    return out


def _elements(spec):
    """(name, index or None) of every parameter element, in kern.parameters order"""
    out = []
    for name in PARAMS[spec["type"]]:
        v = spec[name]
        out += [(name, i) for i in range(len(v))] if isinstance(v, list) else [(name, None)]
    return out


def _shifted(mp, spec, name, idx, delta):
    s = dict(spec)
    if idx is None:
        s[name] = mp.mpf(float(spec[name])) + delta
    else:
        s[name] = [mp.mpf(float(x)) + (delta if i == idx else 0) for i, x in enumerate(spec[name])]
    return s


def main():
    import mpmath as mp
    rng = np.random.default_rng(20251)
    X = rng.standard_normal((N, D)); X2 = rng.standard_normal((M, D))
    Y = np.sin(X @ rng.standard_normal((D, 2))) + 0.1 * rng.standard_normal((N, 2))
    out = {"X": X, "X2": X2, "Y": Y, "noise": np.float64(NOISE), "names": np.array(sorted(CASES))}
    for name in sorted(CASES):
        spec = CASES[name]
        mp.mp.dps = 50
        out[name + "/K"] = np.array([[float(mp_kernel(mp, spec, X[i], X[j])) for j in range(N)] for i in range(N)])
        out[name + "/K2"] = np.array([[float(mp_kernel(mp, spec, X[i], X2[j])) for j in range(M)] for i in range(N)])
        mp.mp.dps = 60
        s2 = mp.mpf(NOISE)
        out[name + "/lml"] = np.float64(float(mp_lml(mp, spec, X, Y, s2)))
        h = mp.mpf("1e-25")
        g = [float((mp_lml(mp, _shifted(mp, spec, nm, i, h), X, Y, s2) - mp_lml(mp, _shifted(mp, spec, nm, i, -h), X, Y, s2)) / (2 * h))
             for nm, i in _elements(spec)]
        out[name + "/grad"] = np.array(g)
        out[name + "/grad_noise"] = np.float64(float((mp_lml(mp, spec, X, Y, s2 + h) - mp_lml(mp, spec, X, Y, s2 - h)) / (2 * h)))
        for key, v in spec.items():
            if key not in ("type", "dims"):
                out[name + "/" + key] = np.asarray(v, dtype=np.float64)
        out[name + "/dims"] = np.asarray(spec["dims"], dtype=np.int64)
        out[name + "/type"] = np.array(spec["type"])
    np.savez(os.path.join(HERE, "newkern.npz"), **out)


if __name__ == "__main__":
    main()
