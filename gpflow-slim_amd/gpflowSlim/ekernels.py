"""Kernels with expectations under a Gaussian q(x) (the reference's ekernels.py).

Implemented: ``RBF`` (ARD or isotropic, over all input dimensions in order) and ``Sum`` of two or more such ``RBF`` kernels on
pairwise disjoint ``active_dims`` (slices or index lists), with diagonal covariances given as ``[N, Q]`` -- ekernels.py:13-47,
120-149 and the separate-dimensions branch 224-249, restricted to diagonal ``Xcov``.  The expectations run on the GPU (csrc/psi.hip,
csrc/psi_sum.hip, gps_psi_stats); Psi2 = sum_n eKzxKxz is evaluated without the reference's [N, Q, M, M] temporary, and for a Sum
without any [N, M] array (``eKzxKxz_sum``); ``eKzxKxz_contract`` contracts eKzxKxz with weight matrices point by point without
storing it (gps_psi2_contract: what conditionals.uncertain_conditional rests on).  Full ``[N, Q, Q]`` covariances, a stand-alone ``RBF`` on an ``active_dims`` subset,
``Linear`` / ``Product`` kernels, sums with overlapping parts (the quadrature fall-back), and ``exKxz*`` raise
``NotImplementedError``.
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

    def eKzxKxz_contract(self, Z, Xmu, Xcov, W):
        """sum_{m, m'} eKzxKxz[n, m, m'] W[b, m, m'], [N, B] for W [B, M, M] ([N] for one [M, M] matrix), without forming
        eKzxKxz; only the symmetric part of each W counts.  Bitwise reproducible."""
        prog, Xvar = self._psi_program(Xmu), _diag_cov(Xcov)
        return be.get_handle().psi2_contract(prog, Z, Xmu, Xvar, W)

    def exKxz(self, Z, Xmu, Xcov):
        raise NotImplementedError("exKxz is not implemented")

    def exKxz_pairwise(self, Z, Xmu, Xcov):
        raise NotImplementedError("exKxz_pairwise is not implemented")


def _unsupported(name):
    class _Unsupported(object):
        def __init__(self, *args, **kwargs):
            raise NotImplementedError("ekernels.%s is not implemented: the kernel expectations cover an RBF kernel and a Sum of RBF "
                                      "kernels on separate dimensions" % name)
    _Unsupported.__name__ = name
    return _Unsupported


_SUM_SCOPE = ("ekernels.Sum is implemented for a list of at least two ekernels.RBF kernels that act on pairwise disjoint "
              "active_dims (no overlapping parts, no other kernel types, no scalars)")


def _part_dims(k, d_all=None):
    """The columns an RBF part reads; without the input width an open-ended slice counts input_dim columns from its start."""
    if d_all is not None or not isinstance(k.active_dims, slice):
        return k._dims(False, d_all)
    a = k.active_dims
    start, step = a.start or 0, a.step or 1
    return list(range(start, start + step * k.input_dim, step)) if a.stop is None else list(range(start, a.stop, step))


class Sum(kernels.Sum):
    """ekernels.py:224-249, the branch ``on_separate_dimensions``: Psi1 is the sum of the parts' Psi1, Psi2 the sum of the parts'
    Psi2 plus the cross terms eKxz_p^T eKxz_p' + eKxz_p'^T eKxz_p (csrc/psi_sum.hip)."""

    def __init__(self, kern_list, name='kernel'):
        if not isinstance(kern_list, (list, tuple)) or len(kern_list) < 2 or not all(type(k) is RBF for k in kern_list):
            raise NotImplementedError(_SUM_SCOPE)
        kernels.Sum.__init__(self, list(kern_list), name=name)
        self._check_separate(None)

    def _check_separate(self, d_all):
        seen = set()
        for k in self.kern_list:
            dims = _part_dims(k, d_all)
            if len(dims) != k.input_dim:
                raise ValueError("active_dims of a part do not match its input_dim")
            if seen.intersection(dims):
                raise NotImplementedError(_SUM_SCOPE + ": the parts overlap")
            seen.update(dims)

    @property
    def on_separate_dimensions(self):
        """True by construction (also for slices, which the reference's property does not look into)."""
        return True

    def _psi_program(self, Xmu):
        q = np.shape(Xmu)[1]
        self._check_separate(q)
        if any(d < 0 or d >= q for k in self.kern_list for d in k._dims(False, q)):
            raise NotImplementedError(_SUM_SCOPE + ": active_dims outside the latent dimensions")
        return self._program(q)

    _psi = RBF._psi

    def eKdiag(self, X, Xcov=None):
        """psi0 per point, [N]: the sum of the parts' variances"""
        return self.Kdiag(X)

    eKxz = RBF.eKxz
    eKzxKxz = RBF.eKzxKxz
    eKzxKxz_sum = RBF.eKzxKxz_sum
    eKzxKxz_contract = RBF.eKzxKxz_contract
    exKxz = RBF.exKxz
    exKxz_pairwise = RBF.exKxz_pairwise


Linear = _unsupported("Linear")
Product = _unsupported("Product")
