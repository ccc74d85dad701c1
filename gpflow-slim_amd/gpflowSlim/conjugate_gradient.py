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
