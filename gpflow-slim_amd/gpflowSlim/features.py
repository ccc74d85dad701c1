"""Inducing features: InducingPoints, Multiscale and the conditional dispatch.

Mirrors gpflowSlim/features.py:26-81 (InducingFeature / InducingPoints), :89-150 (Multiscale), :153-174 (dispatch),
:177-193 (inducingpoint_wrapper).
"""
from functools import singledispatch

import numpy as np

from . import _backend as be
from . import conditionals
from . import kernels
from . import transforms
from ._settings import settings
from .params import Parameter


class InducingFeature(object):
    def __len__(self):
        raise NotImplementedError()


class InducingPoints(InducingFeature):
    def __init__(self, Z):
        self._Z = Parameter(np.asarray(Z, dtype=settings.float_type))

    @property
    def Z(self):
        return self._Z.value

    def __len__(self):
        return self.Z.shape[0]

    def Kuu(self, kern, jitter=0.0):
        """features.py:74-77"""
        Kzz = kern.K(self.Z)
        Kzz += jitter * np.eye(len(self), dtype=settings.dtypes.float_type)
        return Kzz

    def Kuf(self, kern, Xnew):
        """features.py:79-81"""
        return kern.K(self.Z, Xnew)

    def eKfu(self, kern, mean, cov):
        """features.py:83-84: <K(x, Z)> under x_n ~ N(mean_n, diag cov_n), [N, M]"""
        return kern.eKxz(self.Z, mean, cov)

    def eKufKfu(self, kern, mean, cov):
        """features.py:86-87: <K(Z, x) K(x, Z)> point by point, [N, M, M] (small sizes: see ekernels.RBF.eKzxKxz_contract)"""
        return kern.eKzxKxz(self.Z, mean, cov)


class Multiscale(InducingPoints):
    """features.py:89-150: the inter-domain features of Lazaro-Gredilla & Figueiras-Vidal (2009).  Inducing variable m has its own
    width per dimension, L_md = lengthscale_d + scales_md, so a few wide features can cover the smooth parts of the input space.
    RBF kernels only.  Kuu and Kuf are built on the device (csrc/multiscale.hip); SVGP, SGPR, GPRFITC and features.conditional
    take the feature, and their gradients reach ``scales`` (a positive Parameter) like they reach Z."""

    def __init__(self, Z, scales):
        super().__init__(Z)
        scales = np.asarray(scales, dtype=settings.float_type)
        if self.Z.shape != scales.shape:
            raise ValueError("Input locations `Z` and `scales` must have the same shape.")
        self._scales = Parameter(scales, transform=transforms.positive, name='scales')

    @property
    def scales(self):
        return self._scales.value

    @staticmethod
    def _check_kern(kern):
        if not isinstance(kern, kernels.RBF):
            raise NotImplementedError("Multiscale features not implemented for `%s`." % str(type(kern)))

    def Kuu(self, kern, jitter=0.0):
        """features.py:137-147, [M, M] (exactly symmetric)"""
        self._check_kern(kern)
        return be.get_handle()._ms_kmat(kern._program(self.Z.shape[1]), self.Z, self.scales, jitter=jitter)

    def Kuf(self, kern, Xnew):
        """features.py:123-132, [M, N]"""
        self._check_kern(kern)
        Xnew = np.asarray(Xnew, dtype=settings.float_type)
        kern._check_inputs(self.Z, Xnew)
        return be.get_handle()._ms_kmat(kern._program(self.Z.shape[1]), self.Z, self.scales, X2=Xnew)

    def eKfu(self, kern, mean, cov):
        raise NotImplementedError("kernel expectations are not implemented for Multiscale features (nor are they in the reference)")

    def eKufKfu(self, kern, mean, cov):
        raise NotImplementedError("kernel expectations are not implemented for Multiscale features (nor are they in the reference)")


def feature_scales(feat, kern=None):
    """The widths [M, D] the backend needs next to feat.Z -- None for plain inducing points.  With ``kern`` the kernel is checked
    first, before anything touches the device."""
    if not isinstance(feat, Multiscale):
        return None
    if kern is not None:
        feat._check_kern(kern)
    return feat.scales


def refuse_multiscale(feat, who):
    """For the paths that take inducing points only."""
    if isinstance(feat, Multiscale):
        raise NotImplementedError("%s is not implemented for Multiscale features" % who)


@singledispatch
def conditional(feat, kern, Xnew, f, *, full_cov=False, q_sqrt=None, white=False):
    raise NotImplementedError("No implementation for {} found".format(type(feat).__name__))


@conditional.register(InducingPoints)
@conditional.register(Multiscale)
def default_feature_conditional(feat, kern, Xnew, f, *, full_cov=False, q_sqrt=None, white=False):
    """features.py:162-174"""
    return conditionals.feature_conditional(Xnew, feat, kern, f, full_cov=full_cov, q_sqrt=q_sqrt, white=white)


def inducingpoint_wrapper(feat, Z):
    """features.py:177-193"""
    if feat is not None and Z is not None:
        raise ValueError("Cannot pass both an InducingFeature instance and Z values")
    elif feat is None and Z is None:
        raise ValueError("You must pass either an InducingFeature instance or Z values")
    elif Z is not None:
        feat = InducingPoints(Z)
    elif isinstance(feat, np.ndarray):
        feat = InducingPoints(feat)
    else:
        assert isinstance(feat, InducingFeature)
    return feat
