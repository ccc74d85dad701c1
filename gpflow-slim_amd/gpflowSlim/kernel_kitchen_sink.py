"""Random-feature ("kitchen sink") kernels: k(x, x') = phi(x)^T phi(x') for an explicit feature map phi.

API mirror of gpflowSlim/kernel_kitchen_sink.py for Sampler :30-53, RBFSampler :56-118, LinearSampler :193-207,
ConstantSampler :304-318 and SamplerKernel :694-709.  A kernel with a callable ``features`` sends ``models.GPR`` down the
Woodbury branch (models/gpr.py:63-67, 86-117): cost N F^2 + F^3 / 3 instead of N^3 / 3.  The feature maps are evaluated on
the GPU (csrc/rff.hip); ``transform`` / ``features`` return host [N, F] arrays.

Differences from the reference, on purpose: ``rng`` (a ``np.random.Generator``) may be given to draw the random weights
from; by default they come from the ``np.random`` global state as in the reference.  ``sqrt(2 / n_components)`` is a double
(the reference takes the square root in single precision and widens it).  The other samplers and the sampler groups of the
reference module raise NotImplementedError.
"""
import numpy as np

from . import transforms
from . import _backend as be
from ._settings import settings
from .kernels import Kernel
from .params import Parameter

_AVAILABLE = "RBFSampler, LinearSampler and ConstantSampler"


class Sampler(object):
    """kernel_kitchen_sink.py:30-53"""
    _kind = None

    def __init__(self, input_dim, n_components):
        self.input_dim = int(input_dim)
        self.n_components = int(n_components)
        if self.input_dim < 1 or self.n_components < 1:
            raise ValueError("a sampler needs input_dim >= 1 and n_components >= 1")

    @property
    def parameters(self):
        return []

    def check_dim(self, X):
        if np.ndim(X) != 2 or np.shape(X)[1] != self.input_dim:
            raise ValueError("input dimension not compatible with the init value")

    def _descriptor(self):
        """(gps_rff_desc_t, arrays it points into) from the current parameter values."""
        raise NotImplementedError("only %s are implemented" % _AVAILABLE)

    def transform(self, X):
        """Apply the feature map to X [N, input_dim]: host [N, n_components]."""
        X = np.asarray(X, dtype=settings.float_type)
        self.check_dim(X)
        desc, keep = self._descriptor()
        return be.get_handle().rff_features(desc, X)


class RBFSampler(Sampler):
    """kernel_kitchen_sink.py:56-118: cos(X (omega / ls) + offset) sqrt(2 / F) sqrt(var).  omega [input_dim, F] ~ N(0, 1) and
    offset [F] ~ U(0, 2 pi) are drawn once, here; the weights omega / ls follow ``ls`` at every evaluation."""
    _kind = be.RFF_RBF

    def __init__(self, input_dim, ls=1., var=1., n_components=100, scope='RBFSampler', rng=None):
        Sampler.__init__(self, input_dim, n_components)
        self.scope = scope
        ls_arr = np.asarray(ls, dtype=settings.float_type)
        if ls_arr.size not in (1, self.input_dim):
            raise ValueError("ls must be a scalar or have one entry per input dimension")
        self._ls = Parameter(ls, transform=transforms.positive, name='ls')
        self._variance = Parameter(var, transform=transforms.positive, name='variance')
        if rng is None:
            self.omega = np.random.normal(size=(self.input_dim, self.n_components)).astype(settings.float_type)
            self.random_offset_ = np.random.uniform(0, 2 * np.pi, size=self.n_components).astype(settings.float_type)
        else:
            self.omega = rng.normal(size=(self.input_dim, self.n_components)).astype(settings.float_type)
            self.random_offset_ = rng.uniform(0, 2 * np.pi, size=self.n_components).astype(settings.float_type)

    @property
    def parameters(self):
        return [self._ls, self._variance]

    @property
    def ls(self):
        return self._ls.value

    @property
    def variance(self):
        return self._variance.value

    @property
    def random_weights_(self):
        return self.omega / np.reshape(self.ls, (-1, 1))

    def _descriptor(self):
        return be.make_rff(self._kind, self.input_dim, self.n_components, float(np.squeeze(self.variance)),
                           ls=np.atleast_1d(self.ls), omega=self.omega, offset=self.random_offset_)


class LinearSampler(Sampler):
    """kernel_kitchen_sink.py:193-207: tile(X)[:, :F] sqrt(var input_dim / F)"""
    _kind = be.RFF_LINEAR

    def __init__(self, input_dim, var=1., n_components=None, scope='LinearSampler', rng=None):
        Sampler.__init__(self, input_dim, n_components or input_dim)
        self.scope = scope
        self._variance = Parameter(var, transform=transforms.positive, name='variance')

    @property
    def parameters(self):
        return [self._variance]

    @property
    def variance(self):
        return self._variance.value

    def _descriptor(self):
        return be.make_rff(self._kind, self.input_dim, self.n_components, float(np.squeeze(self.variance)))


class ConstantSampler(LinearSampler):
    """kernel_kitchen_sink.py:304-318: ones [N, F] sqrt(var / F)"""
    _kind = be.RFF_CONSTANT

    def __init__(self, input_dim, var=1., n_components=1, scope='ConstantSampler', rng=None):
        Sampler.__init__(self, input_dim, n_components)
        self.scope = scope
        self._variance = Parameter(var, transform=transforms.positive, name='variance')


def _unsupported(name):
    class _Unsupported(object):
        def __init__(self, *args, **kwargs):
            raise NotImplementedError("kernel_kitchen_sink.%s is not implemented: only %s are" % (name, _AVAILABLE))
    _Unsupported.__name__ = name
    return _Unsupported


for _name in ("CosineRBFSampler", "CosineSampler", "CosineV2Sampler", "ArcCosineSampler", "EqApproxSumSampler",
              "NEqApproxSumSampler", "ApproxProdSampler", "RandomApproxProdSampler", "OrthogonalApproxProdSampler",
              "SubsetApproxProdSampler", "OneApproxProdSampler", "SketchApproxProdSampler", "OuterProductSampler", "RFFSampler",
              "RFFApproxSumSampler", "RFFApproxProdSampler", "TransformSampler", "SamplerGroup", "ListSamplerGroup",
              "FullyConnectedSamplerGroup", "ReduceProdSamplerGroup", "ConcatSamplerGroup", "SamplerGroupKernel"):
    globals()[_name] = _unsupported(_name)
del _name


class SamplerKernel(Kernel):
    """kernel_kitchen_sink.py:694-709"""

    def __init__(self, sampler):
        if not isinstance(sampler, Sampler) or sampler._kind is None:
            raise NotImplementedError("SamplerKernel takes one of %s" % _AVAILABLE)
        self.sampler = sampler
        Kernel.__init__(self, input_dim=sampler.input_dim)
        self._parameters = list(sampler.parameters)

    def _on_combine(self):
        """Called by kernels.Combination for every kernel it is given: Sum / Product refuse a SamplerKernel at construction."""
        self._combine()

    def _combine(self, *args):
        raise NotImplementedError("a SamplerKernel cannot be combined with other kernels (Sum / Product / neural kernel "
                                  "network): only %s on their own are implemented" % _AVAILABLE)

    __add__ = __radd__ = __mul__ = __rmul__ = _combine

    def _nodes(self, presliced, d_all):
        self._combine()

    def _grad_layout(self, d_all):
        self._combine()

    def K(self, X, X2=None, presliced=False):
        X = np.asarray(X, dtype=settings.float_type)
        self.sampler.check_dim(X)
        if X2 is not None:
            X2 = np.asarray(X2, dtype=settings.float_type)
            self.sampler.check_dim(X2)
        desc, keep = self.sampler._descriptor()
        return be.get_handle().rff_gram(desc, X, X2)[0]

    def Kdiag(self, X, presliced=False):
        X = np.asarray(X, dtype=settings.float_type)
        self.sampler.check_dim(X)
        desc, keep = self.sampler._descriptor()
        return be.get_handle().rff_gram(desc, X, None, want_K=False, want_diag=True)[1]

    def features(self, X):
        return self.sampler.transform(X)
