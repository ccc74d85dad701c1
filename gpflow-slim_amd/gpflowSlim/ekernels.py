"""Kernels with expectations under a Gaussian q(x) (the reference's ekernels.py).

Implemented: ``RBF`` (ARD or isotropic, over all input dimensions in order) with diagonal covariances given as ``[N, Q]`` --
ekernels.py:13-47, 120-149 restricted to diagonal ``Xcov``.  The expectations run on the GPU (csrc/psi.hip, gps_psi_stats);
Psi2 = sum_n eKzxKxz is evaluated without the reference's [N, Q, M, M] temporary (``eKzxKxz_sum``).  Full ``[N, Q, Q]``
covariances, ``active_dims`` subsets, ``Linear`` / ``Sum`` / ``Product`` kernels with their cross terms and the quadrature
fall-back, and ``exKxz*`` raise ``NotImplementedError``.
"""
import numpy as np

from . import kernels
from . import _backend as be
from ._settings import settings


def _diag_cov(Xcov):
    Xcov = np.asarray(Xcov, dtype=settings.float_type)
    if Xcov.ndim == 3:
        raise NotImplementedError("full [N, Q, Q] covariances of q(x) are not implemented: pass the diagonals as [N, Q]")
    if Xcov.ndim != 2:
        raise ValueError("Xcov must be [N, Q]")
    return Xcov


class RBF(kernels.RBF):
    def _psi_program(self, Xmu):
        """The one-node program gps_psi_stats takes: this kernel over the columns 0 .. Q-1 of Xmu, in order."""
        q = np.shape(Xmu)[1]
        if self._dims(False, q) != list(range(q)):
            raise NotImplementedError("kernel expectations are implemented for an RBF over all latent dimensions, in order "
                                      "(no active_dims subset)")
        return self._program(q)

    def _psi(self, Z, Xmu, Xcov, **want):
        prog, Xvar = self._psi_program(Xmu), _diag_cov(Xcov)         # (the refusals come before anything touches the device)
        return be.get_handle().psi_stats(prog, Z, Xmu, Xvar, **want)

    def eKdiag(self, X, Xcov=None):
        """psi0 per point, [N]  (ekernels.py:14-20)"""
        return self.Kdiag(X)

    def eKxz(self, Z, Xmu, Xcov):
        """Psi1 = <K(x, Z)>_q(x), [N, M]  (ekernels.py:22-47)"""
        return self._psi(Z, Xmu, Xcov, want_psi1=True)[0]

    def eKzxKxz(self, Z, Xmu, Xcov):
        """<K(Z, x) K(x, Z)>_q(x) point by point, [N, M, M]  (ekernels.py:120-149).  O(N M^2) memory: small sizes; models use
        eKzxKxz_sum."""
        return self._psi(Z, Xmu, Xcov, want_psi2n=True)[2]

    def eKzxKxz_sum(self, Z, Xmu, Xcov):
        """Psi2 = sum_n eKzxKxz, [M, M], in O(M^2) device memory; exactly symmetric and bitwise reproducible."""
        return self._psi(Z, Xmu, Xcov, want_psi2=True)[1]

    def exKxz(self, Z, Xmu, Xcov):
        raise NotImplementedError("exKxz is not implemented")

    def exKxz_pairwise(self, Z, Xmu, Xcov):
        raise NotImplementedError("exKxz_pairwise is not implemented")


def _unsupported(name):
    class _Unsupported(object):
        def __init__(self, *args, **kwargs):
            raise NotImplementedError("ekernels.%s is not implemented: the kernel expectations cover a single RBF kernel" % name)
    _Unsupported.__name__ = name
    return _Unsupported


Linear = _unsupported("Linear")
Sum = _unsupported("Sum")
Product = _unsupported("Product")
