"""GP conditionals on the GPU.

Mirrors gpflowSlim/conditionals.py: conditional :24-66, feature_conditional :69-77,
base_conditional :80-121.  ``conditional`` / ``feature_conditional`` build Kmm (+jitter), Kmn and
Knn on the device and never move them over PCIe; ``base_conditional`` accepts host matrices.
``uncertain_conditional`` (:125-203) is the conditional at Gaussian inputs with diagonal covariances, for the kernels of
``ekernels``; the reference's ``[N, M, M]`` expectation is contracted as it is evaluated and never stored.
"""
import numpy as np

from . import _backend as be
from ._settings import settings


def conditional(Xnew, X, kern, f, *, full_cov=False, q_sqrt=None, white=False):
    """conditionals.py:24-66"""
    Xnew = np.asarray(Xnew, dtype=settings.float_type)
    X = np.asarray(X, dtype=settings.float_type)
    kern._check_inputs(X, Xnew)
    prog = kern._program(X.shape[1])
    return be.get_handle().conditional(prog, X, Xnew, f, settings.numerics.jitter_level,
                                       q_sqrt=q_sqrt, white=white, full_cov=full_cov)


def feature_conditional(Xnew, feat, kern, f, *, full_cov=False, q_sqrt=None, white=False):
    """conditionals.py:69-77 with the feature's Kuu / Kuf: features.InducingPoints (features.py:74-81) or, when the feature has
    ``scales``, features.Multiscale (features.py:123-147) -- both built inside the one device call."""
    scales = getattr(feat, "scales", None)
    if scales is None:
        return conditional(Xnew, feat.Z, kern, f, full_cov=full_cov, q_sqrt=q_sqrt, white=white)
    feat._check_kern(kern)
    Xnew = np.asarray(Xnew, dtype=settings.float_type)
    Z = np.asarray(feat.Z, dtype=settings.float_type)
    kern._check_inputs(Z, Xnew)
    return be.get_handle().conditional(kern._program(Z.shape[1]), Z, Xnew, f, settings.numerics.jitter_level,
                                       q_sqrt=q_sqrt, white=white, full_cov=full_cov, scales=scales)


def uncertain_conditional(Xnew_mu, Xnew_var, feat, kern, q_mu, q_sqrt, *, full_cov_output=False, full_cov=False, white=False):
    """conditionals.py:125-203: mean [N, D] and variance ([N, D], or [N, D, D] with full_cov_output) of f(x_n) for
    x_n ~ N(Xnew_mu_n, diag Xnew_var_n) under q(u) = N(q_mu, q_sqrt q_sqrt^T) at the inducing points.  ``kern`` is an
    ekernels.RBF or ekernels.Sum; ``Xnew_var`` holds the diagonals, [N, Din].  One device call (gps_uncertain_conditional): the
    [N, M, M] array eKufKfu of the reference is never formed."""
    from .features import InducingPoints, refuse_multiscale          # (features imports this module)
    refuse_multiscale(feat, "uncertain_conditional")
    if not isinstance(feat, InducingPoints):
        raise NotImplementedError("uncertain_conditional is implemented for InducingPoints only")
    if full_cov:
        raise NotImplementedError("uncertain_conditional: full_cov=True is not implemented (nor is it in the reference)")
    Xnew_mu = np.asarray(Xnew_mu, dtype=settings.float_type)
    Xnew_var = np.asarray(Xnew_var, dtype=settings.float_type)
    if Xnew_var.ndim == 3:
        raise NotImplementedError("full [N, Din, Din] input covariances are not implemented: pass the diagonals as [N, Din]")
    if q_sqrt is None:
        raise ValueError("uncertain_conditional needs q_sqrt")
    if not hasattr(kern, "_psi_program"):
        raise NotImplementedError("uncertain_conditional needs a kernel with expectations: ekernels.RBF or ekernels.Sum")
    prog = kern._psi_program(Xnew_mu)
    return be.get_handle().uncertain_conditional(prog, feat.Z, Xnew_mu, Xnew_var, q_mu, q_sqrt, settings.numerics.jitter_level,
                                                 white=white, full_cov_output=full_cov_output)


def base_conditional(Kmn, Kmm, Knn, f, *, full_cov=False, q_sqrt=None, white=False):
    """conditionals.py:80-121"""
    return be.get_handle().base_conditional(Kmn, Kmm, Knn, f, q_sqrt=q_sqrt, white=white, full_cov=full_cov)
