"""Plain reference of the matrix-free path (csrc/kmvm.hip, csrc/gps_kmvm.hip) for tests/test_gpu_kmvm.py: the kernel matrix by
tests/_kern_ref.py's formulas, then products and solves in numpy.longdouble.  Host only.

The fp64 evaluation is _kern_ref.K itself; the long-double one repeats its square_dist (kernels.py:408-421, the expanded form and
the clamp) on long-double inputs and hands r2 to the same _kern_ref._stationary.  numpy.linalg has no long-double solve: ``solve``
is numpy.linalg.solve refined three times with long-double residuals, which at the condition numbers used here (<= 1e3) is
accurate to the long-double rounding.
"""
import numpy as np

import _kern_ref as kr

LD = np.longdouble


def leaf(kind, dims, seed):
    """an ARD stationary leaf with lengthscales in [0.7, 1.3] and variance 1.3"""
    rng = np.random.default_rng(seed)
    out = {"type": kind, "dims": list(dims), "variance": 1.3, "lengthscales": rng.uniform(0.7, 1.3, len(dims))}
    if kind == "ratquad":
        out["alpha"] = 1.7
    return out


def K_ld(lf, X, X2=None):
    ls = kr._per_dim(lf["lengthscales"], len(lf["dims"])).astype(LD)
    A = np.asarray(X, dtype=LD)[:, lf["dims"]] / ls
    B = A if X2 is None else np.asarray(X2, dtype=LD)[:, lf["dims"]] / ls
    r2 = -2.0 * (A @ B.T) + (np.sum(np.square(A), 1)[:, None] + np.sum(np.square(B), 1)[None, :])
    return kr._stationary(lf, np.maximum(r2, LD(0)))[0]


def product(lf, X, V, X2=None, diag_add=0.0):
    """(the product in long double, the scale sum_p |K_ip| |V_pt| of its entries, the spread of the fp64 evaluation)"""
    Kl, K64 = K_ld(lf, X, X2), kr.K(lf, X, X2)
    Vl = np.asarray(V, dtype=LD)
    ref, r64 = Kl @ Vl, K64 @ V
    if X2 is None:
        ref, r64 = ref + LD(diag_add) * Vl, r64 + diag_add * V
    scale = np.abs(Kl) @ np.abs(Vl)
    return ref, scale, float(np.max(np.abs(r64 - ref) / scale))


def solve(A, B):
    A64 = np.asarray(A, dtype=np.float64)
    x = np.linalg.solve(A64, np.asarray(B, dtype=np.float64)).astype(LD)
    for _ in range(3):
        x = x + np.linalg.solve(A64, np.asarray(B - A @ x, dtype=np.float64)).astype(LD)
    return x


def dense(lf, X, noise):
    """(K + noise I in long double, its 2-norm condition number)"""
    A = K_ld(lf, X) + LD(noise) * np.eye(X.shape[0], dtype=LD)
    w = np.linalg.eigvalsh(np.asarray(A, dtype=np.float64))
    return A, float(w[-1] / w[0])
