"""Conjugate gradients on a Kronecker-structured system (mirrors gpflowSlim/conjugate_gradient.py:18-55).

``cgsolver`` solves (I + C o (K1 (C o .) K2)) x = b by plain CG from x = 0; the loop runs on the device
(gps_kron_cg: two fp64 GEMMs and three fused vector kernels per iteration, the loop's state in device memory).
Vectors are the reference's [N, 1] columns, ``vec`` column-major; the device keeps each as the [m, n] matrix it is.
"""
import numpy as np

from . import _backend as be
from ._settings import settings


def dot(a, b):
    """conjugate_gradient.py:18-20"""
    return np.sum(np.asarray(a) * np.asarray(b))


def vec(X):
    """conjugate_gradient.py:22-25: the columns of X stacked, [N, 1]."""
    return np.reshape(np.transpose(np.asarray(X)), [-1, 1])


def unvec(v, m, n):
    """The [m, n] matrix whose ``vec`` is v."""
    return np.ascontiguousarray(np.reshape(np.asarray(v), [n, m]).T)


def cgsolver(K1, K2, b, C, max_iter=100, tol=1e-6):
    """conjugate_gradient.py:28-55.  K1 [m, m], K2 [n, n]; b, C [N, 1] with N = m n.  Returns x [N, 1].  The stop rule
    compares tol * |b| with the SQUARED residual norm, as the reference does."""
    K1 = np.asarray(K1, dtype=settings.float_type)
    K2 = np.asarray(K2, dtype=settings.float_type)
    if K1.ndim != 2 or K2.ndim != 2:
        raise ValueError("K1 and K2 must be square")
    m, n = K1.shape[0], K2.shape[0]
    b = np.asarray(b, dtype=settings.float_type)
    C = np.broadcast_to(np.asarray(C, dtype=settings.float_type), b.shape) if np.ndim(C) else np.full(b.shape, float(C))
    if b.size != m * n:
        raise ValueError("b must have %d entries" % (m * n))
    x, _, _, _ = be.get_handle().kron_cg(K1, K2, unvec(b, m, n), unvec(C, m, n), max_iter=max_iter, tol=tol)
    return vec(x)


# ---- exact GPs without the N x N matrix (not in the reference) -------------------------------------------------------------------
# kernel_matmul is (K(X, X2) + c I) V with K generated tile by tile on the device and never stored; kernel_cgsolver solves
# (K(X, X) + s I) x = B on it, all columns of B at once (gps_kmvm, gps_kernel_cg: csrc/kmvm.hip).
MATRIX_FREE_SCOPE = "one stationary kernel: RBF, Matern12, Matern32, Matern52, Exponential or RatQuad"


def _matrix_free_program(kern, d_all):
    """The kernel's program if the matrix-free path takes it, else NotImplementedError -- before anything touches the device."""
    from . import kernels
    if not isinstance(kern, (kernels.RBF, kernels.Matern12, kernels.Matern32, kernels.Matern52, kernels.Exponential,
                             kernels.RatQuad)):
        raise NotImplementedError("the matrix-free path takes %s; got %s" % (MATRIX_FREE_SCOPE, type(kern).__name__))
    return kern._program(d_all)


def kernel_matmul(kern, X, V, X2=None, diag_add=0.0):
    """K(X, X2) V [n, T], or (K(X, X) + diag_add I) V without an X2; memory O(n (D + T))."""
    X = np.ascontiguousarray(X, dtype=settings.float_type)
    prog = _matrix_free_program(kern, X.shape[1])
    kern._check_inputs(*([X] if X2 is None else [X, X2]))
    return be.kmvm(be.get_handle(), prog, X, V, X2=X2, diag_add=diag_add)


def kernel_cgsolver(kern, X, B, noise_var, max_iter=1000, tol=1e-8):
    """(K(X, X) + noise_var I) x = B by plain conjugate gradients from x = 0, the T columns of B at once.  A column stops when
    |r| <= tol |b| -- the unsquared norms; ``cgsolver`` above keeps the reference's rule, tol |b| against r^T r.  Returns
    (x [n, T], info) with info['iterations'] [T], info['relative_residual'] [T] (of the recurrence) and info['converged'] [T];
    a column that did not converge within max_iter is reported by a warning, not an error."""
    import warnings
    X = np.ascontiguousarray(X, dtype=settings.float_type)
    prog = _matrix_free_program(kern, X.shape[1])
    kern._check_inputs(X)
    x, iters, rel, conv = be.kernel_cg(be.get_handle(), prog, X, B, noise_var, max_iter=max_iter, tol=tol)
    info = {"iterations": iters, "relative_residual": rel, "converged": conv}
    if not np.all(info["converged"]):
        warnings.warn("kernel_cgsolver: %d of %d columns did not reach tol = %g in %d iterations (largest |r| / |b| = %.3g)"
                      % (int(np.sum(~info["converged"])), rel.size, tol, max_iter, float(np.max(rel))))
    return x, info
