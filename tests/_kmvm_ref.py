"""Plain reference of the matrix-free path (csrc/kmvm.hip, csrc/gps_kmvm.hip) for tests/test_gpu_kmvm.py: the kernel matrix by
tests/_kern_ref.py's formulas, then products and solves in numpy.longdouble.  Host only.  For tests/test_gpu_kmvm_large.py, where
a dense long-double K is out of reach: the same product on sampled rows (K_rows, product_rows, sample_rows) and the pivoted factor
from its k columns (factor_columns); tests/test_kmvm_ref_cpu.py proves them against the dense ones.

The fp64 evaluation is _kern_ref.K itself; the long-double one repeats its square_dist (kernels.py:408-421, the expanded form and
the clamp) on long-double inputs and hands r2 to the same _kern_ref._stationary.  numpy.linalg has no long-double solve: ``solve``
is numpy.linalg.solve refined three times with long-double residuals, which at the condition numbers used here (<= 1e5) is
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


def _block(lf, A, B, dtype, same):
    """k of the scaled points A [a, nd] against B [b, nd] in `dtype` by the expanded, clamped r2; same [a] (or None): the column of
    each row that is the row's own point, where r2 is set to 0"""
    A, B = np.asarray(A, dtype=dtype), np.asarray(B, dtype=dtype)
    r2 = np.maximum(-2.0 * (A @ B.T) + (np.sum(np.square(A), 1)[:, None] + np.sum(np.square(B), 1)[None, :]), dtype(0))
    if same is not None:
        r2[np.arange(len(A)), same] = 0
    return kr._stationary(lf, r2)[0]


def _scaled(lf, X, dtype):
    return np.asarray(X, dtype=dtype)[:, lf["dims"]] / kr._per_dim(lf["lengthscales"], len(lf["dims"])).astype(dtype)


def K_rows(lf, X, rows, dtype=LD):
    """K(X[rows], X) in `dtype` with r2 = 0 on the entries (i, rows[i]): product_rows' convention"""
    rows = np.asarray(rows, dtype=np.int64)
    F = _scaled(lf, X, dtype)
    return _block(lf, F[rows], F, dtype, rows)


def product_rows(lf, X, V, rows, diag_add=0.0):
    """``product`` for K(X, X) restricted to `rows`: (K(X[rows], X) V + diag_add V[rows] in long double, the scale
    sum_p |K_ip| |V_pt|, the spread of the fp64 evaluation), O(len(rows) n) memory -- no n x n matrix.

    Convention of the diagonal: entry (i, rows[i]) is a point against itself and has r2 = 0 exactly, the true distance and what the
    device's patched diagonal block has (``dense_form`` of tests/test_gpu_kmvm_train.py does the same); everywhere else r2 is the
    expanded form clamped at 0, as in ``K_ld``.  Against ``product`` that moves a diagonal entry by the 1e-19 |a|^2 (long double)
    the expanded form leaves there: nothing for a kernel that is flat at r = 0, 5e-13 of a Matern12 / Exponential value."""
    rows = np.asarray(rows, dtype=np.int64)
    Vl, V64 = np.asarray(V, dtype=LD), np.asarray(V, dtype=np.float64)
    Kl, K64 = K_rows(lf, X, rows), K_rows(lf, X, rows, np.float64)
    ref, r64 = Kl @ Vl + LD(diag_add) * Vl[rows], K64 @ V64 + diag_add * V64[rows]
    scale = np.abs(Kl) @ np.abs(Vl)
    return ref, scale, float(np.max(np.abs(r64 - ref) / scale))


def factor_columns(lf, X, piv, dtype):
    """(L, residual diagonal, d_p of every step, the largest residual diagonal entry before every step) of the pivoted partial
    Cholesky of K(X, X) with the given pivots, in `dtype`: what ``_factor`` of tests/test_gpu_pchol.py returns, from the n x k block
    K(X, X[piv]) and a constant diagonal alone -- O(n k^2) work, no n x n matrix.  The diagonal, and entry (piv[m], m) of the block,
    is the kernel at r2 = 0 (product_rows' convention): `variance`, or for the Matern family and Exponential what sqrt(r2 + 1e-12)
    leaves of it (Matern32: variance (1 - 1.5e-12)), as the device's factor starts from."""
    piv = np.asarray(piv, dtype=np.int64)
    F = _scaled(lf, X, dtype)
    Kc = _block(lf, F[piv], F, dtype, piv).T                   # [n, k]
    n, d = F.shape[0], np.full(F.shape[0], kr._stationary(lf, np.zeros(1, dtype=dtype))[0][0], dtype=dtype)
    L, dp, dmax = np.zeros((n, len(piv)), dtype=dtype), [], []
    for m, p in enumerate(piv):
        dp.append(d[p]); dmax.append(d.max())
        L[:, m] = (Kc[:, m] - L[:, :m] @ L[p, :m]) / np.sqrt(d[p])
        d = np.maximum(d - np.square(L[:, m]), 0)
        d[p] = 0
    return L, d, np.array(dp, dtype=dtype), np.array(dmax, dtype=dtype)


def sample_rows(n):
    """The rows on which the large cases are compared, about 300 at most: the first tile of 64; the last 64 rows; the tile from row
    4096 (n > 4160: the first tile past 64 row tiles); every row from 8160 on (n > 8192: the end of the first pass of a 512-workgroup
    row loop, 16 rows a workgroup, and its second pass), cut to the first and last 86 of them when there are more than 172.
    Every row of A x - b sees all of x, so an error in the stride tail of any vector shows in every sampled row."""
    rows = set(range(min(n, 64))) | set(range(max(n - 64, 0), n))
    if n > 4160:
        rows |= set(range(4096, 4160))
    if n > 8192:
        tail = list(range(8160, n))
        rows |= set(tail if len(tail) <= 172 else tail[:86] + tail[-86:])
    return np.array(sorted(rows), dtype=np.int64)


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
