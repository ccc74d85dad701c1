"""Covariance functions of the exact-GP path, evaluated on the GPU.

API mirror of gpflowSlim/kernels.py for the kernels on the hot path: Kernel (active-dims
slicing :217-253, ``+`` / ``*`` :277-281), Static/White/Constant/Bias :308-357, Stationary
:360-429, RBF :432-439, RatQuad :447-471, Linear :474-515, Polynomial :518-554, Exponential :557-565,
Matern12/32/52 :569-610, Cosine :617-646, ArcCosine :649-766, Periodic :769-819, Coregion :822-881,
Combination/Sum/Product :1000-1084.

Differences from the reference, on purpose: values are eager numpy fp64 arrays (there is no
TensorFlow graph); ``K`` compiles the kernel *tree* into one reverse-Polish program and
evaluates it in a single fused HIP pass (csrc/kmat.hip) instead of one TF op per arithmetic
step; ``name=None`` is accepted for Static kernels (the reference crashes on it).
"""
from functools import reduce

import numpy as np

from . import transforms
from . import _backend as be
from ._settings import settings
from .params import Parameter


class Kernel(object):
    """kernels.py:33-76"""

    def __init__(self, input_dim, active_dims=None, name=None):
        self._name = name
        self.input_dim = int(input_dim)
        if active_dims is None:
            self.active_dims = slice(input_dim)
        elif isinstance(active_dims, slice):
            self.active_dims = active_dims
            if active_dims.start is not None and active_dims.stop is not None and active_dims.step is not None:
                assert len(range(active_dims.start, active_dims.stop, active_dims.step)) == input_dim
        else:
            self.active_dims = np.array(active_dims, dtype=np.int32)
            assert len(active_dims) == input_dim
        self._parameters = []

    @property
    def name(self):
        return self._name

    @property
    def parameters(self):
        return self._parameters

    # ---- program construction -------------------------------------------------------------
    def _dims(self, presliced, d_all):
        """Column indices this kernel reads (Kernel._slice, kernels.py:238-245)."""
        if presliced:
            return list(range(self.input_dim))
        if isinstance(self.active_dims, slice):
            return list(range(*self.active_dims.indices(d_all)))
        return [int(d) for d in self.active_dims]

    def _nodes(self, presliced, d_all):
        raise NotImplementedError

    def _program(self, d_all, presliced=False):
        return be.make_program(self._nodes(presliced, d_all))

    def _grad_layout(self, d_all):
        """One entry per gradient slot of gps_gpr_lml_grad, in slot order: (Parameter or None, index
        into the parameter's flattened value or None = add to every element)."""
        raise NotImplementedError

    def _check_inputs(self, *Xs):
        """Raise ValueError for inputs this kernel cannot take, before anything reaches the device (None entries are
        skipped).  Only kernels that read a column as something other than a real number have anything to check."""

    # ---- reference API -------------------------------------------------------------------
    def K(self, X, X2=None, presliced=False):
        X = np.asarray(X, dtype=settings.float_type)
        prog = self._program(X.shape[1], presliced)
        if not presliced:
            self._check_inputs(X, X2)
        return be.get_handle().kmat(prog, X, None if X2 is None else np.asarray(X2, dtype=settings.float_type))

    def Kdiag(self, X, presliced=False):
        raise NotImplementedError

    # eager helpers of the reference (kernels.py:68-75): there they build the tensor and evaluate it; here K / Kdiag are eager
    def compute_K(self, X, Z):
        return self.K(X, Z)

    def compute_K_symm(self, X):
        return self.K(X)

    def compute_Kdiag(self, X):
        return self.Kdiag(X)

    def _slice(self, X, X2):
        """kernels.py:217-253: the columns this kernel reads (host-side view; the device kernels gather the active dims
        themselves from the un-sliced X)."""
        X = np.asarray(X, dtype=settings.float_type)
        dims = self._dims(False, X.shape[1])
        Xs = X[:, dims]
        X2s = None if X2 is None else np.asarray(X2, dtype=settings.float_type)[:, dims]
        if Xs.shape[1] != self.input_dim:
            raise ValueError("Input 1st dimension does not match kernel dimension.")
        return Xs, X2s

    def Kdim(self, dim, X, X2=None):
        """kernels.py:287-306: the covariance along one input dimension -- X [n, 1] is placed in column `dim` of an otherwise
        zero [n, input_dim] input."""
        def pad(a):
            a = np.asarray(a, dtype=settings.float_type)
            out = np.zeros((a.shape[0], self.input_dim), dtype=settings.float_type)
            out[:, dim] = a[:, 0]
            return out
        return self.K(pad(X), None if X2 is None else pad(X2), presliced=True)

    def __add__(self, other):
        return Sum([self, other])

    def __mul__(self, other):
        return Product([self, other])


class Static(Kernel):
    """kernels.py:308-325"""

    def __init__(self, input_dim, variance=1.0, active_dims=None, name=None):
        super().__init__(input_dim, active_dims, name=name)
        self._variance = Parameter(variance, transform=transforms.positive, name='variance')
        self._parameters = self._parameters + [self._variance]

    @property
    def variance(self):
        return self._variance.value

    def Kdiag(self, X, presliced=False):
        return np.ones(np.shape(X)[0], dtype=settings.float_type) * self.variance


class White(Static):
    """kernels.py:328-338"""

    def _grad_layout(self, d_all):
        return [(self._variance, None)]

    def _nodes(self, presliced, d_all):
        return [be.primitive_node(be.K_WHITE, np.squeeze(self.variance))]


class Constant(Static):
    """kernels.py:341-350"""

    def _grad_layout(self, d_all):
        return [(self._variance, None)]

    def _nodes(self, presliced, d_all):
        return [be.primitive_node(be.K_CONSTANT, np.squeeze(self.variance))]


class Bias(Constant):
    """kernels.py:353-357"""
    pass


class Stationary(Kernel):
    """kernels.py:360-429"""
    _op = None

    def __init__(self, input_dim, variance=1.0, lengthscales=None,
                 active_dims=None, ARD=False, min_ls=1e-6, name='kernel'):
        super().__init__(input_dim, active_dims, name=name)
        self._variance = Parameter(variance, transform=transforms.positive, name='variance',
                                   dtype=settings.float_type)
        if ARD:
            if lengthscales is None:
                lengthscales = np.ones(input_dim, dtype=settings.float_type)
            else:
                lengthscales = lengthscales * np.ones(input_dim, dtype=settings.float_type)
        else:
            lengthscales = 1.0 if lengthscales is None else lengthscales
        self.ARD = ARD
        self._ls = Parameter(lengthscales, transform=transforms.Log1pe(min_ls), name='ls')
        self._parameters = self._parameters + [self._variance, self._ls]

    @property
    def variance(self):
        return self._variance.value

    @property
    def lengthscales(self):
        return self._ls.value

    def _nodes(self, presliced, d_all):
        dims = self._dims(presliced, d_all)
        ls = np.atleast_1d(self.lengthscales)
        if ls.size not in (1, len(dims)):
            raise ValueError("lengthscales do not match the active dims")
        return [be.primitive_node(self._op, np.squeeze(self.variance), dims, ls)]

    def Kdiag(self, X, presliced=False):
        """kernels.py:428-429"""
        return np.ones(np.shape(X)[0], dtype=settings.float_type) * self.variance

    def _grad_layout(self, d_all):
        nd = len(self._dims(False, d_all))
        ard = np.atleast_1d(self.lengthscales).size > 1
        return [(self._variance, None)] + [(self._ls, d if ard else None) for d in range(nd)]

    def _dist(self, op, X, X2):
        # the reference calls these on already-sliced inputs (K slices first, kernels.py:436-438): columns 0 .. input_dim - 1
        X = np.asarray(X, dtype=settings.float_type)
        ls = np.atleast_1d(self.lengthscales)
        node = be.primitive_node(op, 1.0, list(range(X.shape[1])), ls)
        return be.get_handle().kmat(be.make_program([node]), X, None if X2 is None else np.asarray(X2, dtype=settings.float_type))

    def square_dist(self, X, X2):
        """kernels.py:408-421: max(0, |a|^2 + |b|^2 - 2 a.b) with a = X / lengthscales -- evaluated by the same device tile pass
        (program op GPS_K_SQDIST) every stationary K is built on."""
        return self._dist(be.K_SQDIST, X, X2)

    def euclid_dist(self, X, X2):
        """kernels.py:424-426: sqrt(square_dist + 1e-12)"""
        return self._dist(be.K_EUCLID, X, X2)

    def dimwise(self, dim):
        """kernels.py:441-444, 579-582, ...: the one-dimensional factor of this kernel along `dim` (variance^(1 / input_dim))."""
        ls = np.atleast_1d(self.lengthscales)
        return type(self)(input_dim=1, variance=float(np.squeeze(self.variance)) ** (1.0 / self.input_dim),
                          lengthscales=float(ls[dim] if self.ARD else ls[0]), name='%s_dimwise_%d' % (type(self).__name__, dim))


class RBF(Stationary):
    """kernels.py:432-439"""
    _op = be.K_RBF


class RatQuad(Stationary):
    """kernels.py:447-471: variance * (1 + r2 / (2 alpha))^(-alpha)"""
    _op = be.K_RATQUAD

    def __init__(self, input_dim, alpha=1., variance=1.0, lengthscales=None,
                 active_dims=None, ARD=False, min_ls=1e-6, name='kernel'):
        super().__init__(input_dim=input_dim, variance=variance, lengthscales=lengthscales, active_dims=active_dims,
                         ARD=ARD, min_ls=min_ls, name=name)
        self._alpha = Parameter(alpha, transform=transforms.positive, name='alpha')
        self._parameters = self._parameters + [self._alpha]

    @property
    def alpha(self):
        return self._alpha.value

    def _nodes(self, presliced, d_all):
        node, = super()._nodes(presliced, d_all)
        node.period = float(np.squeeze(self.alpha))         # (the field Periodic keeps its period in)
        return [node]

    def _grad_layout(self, d_all):
        return super()._grad_layout(d_all) + [(self._alpha, None)]

    def dimwise(self, dim):
        k = super().dimwise(dim)
        k._alpha.assign(self.alpha)
        return k


class Linear(Kernel):
    """kernels.py:474-515: sum_d v_d x_d x'_d.  Kdiag depends on the point, so the device paths that assume a constant
    Kdiag (SVGP, SGPR, FITC, the distributed ones) refuse this kernel; GPR and conditional take it."""
    _op = be.K_LINEAR

    def __init__(self, input_dim, variance=1.0, active_dims=None, ARD=False, name='kernel'):
        super().__init__(input_dim, active_dims, name=name)
        self.ARD = ARD
        variance = np.ones(self.input_dim, dtype=settings.float_type) * variance if ARD else variance
        self._variance = Parameter(variance, transform=transforms.positive, name='variance')
        self._parameters = self._parameters + [self._variance]

    @property
    def variance(self):
        return self._variance.value

    def _dim_variances(self, presliced, d_all):
        dims = self._dims(presliced, d_all)
        v = np.atleast_1d(self.variance)
        if v.size not in (1, len(dims)):
            raise ValueError("variances do not match the active dims")
        return dims, v

    def _nodes(self, presliced, d_all):
        dims, v = self._dim_variances(presliced, d_all)
        return [be.primitive_node(be.K_LINEAR, 1.0, dims, v)]

    def _lin_diag(self, X, presliced):
        X = np.asarray(X, dtype=settings.float_type)
        dims, v = self._dim_variances(presliced, X.shape[1])
        return np.sum(np.square(X[:, dims]) * v, 1)

    def Kdiag(self, X, presliced=False):
        """kernels.py:507-510"""
        return self._lin_diag(X, presliced)

    def _grad_layout(self, d_all):
        nd = len(self._dims(False, d_all))
        ard = np.atleast_1d(self.variance).size > 1
        return [(self._variance, d if ard else None) for d in range(nd)]

    def dimwise(self, dim):
        """kernels.py:512-515"""
        v = np.atleast_1d(self.variance)
        return Linear(input_dim=1, variance=float(v[dim]) if self.ARD else float(v[0]) ** (1.0 / self.input_dim),
                      name='Linear_dimwise_%d' % dim)


class Polynomial(Linear):
    """kernels.py:518-554: (Linear + offset)^degree; the degree is fixed (not a Parameter) and, on the device, an integer in
    1 .. 64.  Unlike the reference, which appends ``_variance`` to ``parameters`` a second time (kernels.py:544) and so
    would count its gradient twice, every Parameter is listed once."""
    _op = be.K_POLYNOMIAL

    def __init__(self, input_dim, degree=3.0, variance=1.0, offset=1.0, active_dims=None, ARD=False, name='kernel'):
        super().__init__(input_dim, variance, active_dims, ARD, name=name)
        self.degree = degree
        self._offset = Parameter(offset, transform=transforms.positive, name='offset')
        self._parameters = self._parameters + [self._offset]

    @property
    def offset(self):
        return self._offset.value

    def _nodes(self, presliced, d_all):
        dims, v = self._dim_variances(presliced, d_all)
        return [be.primitive_node(be.K_POLYNOMIAL, np.squeeze(self.offset), dims, v, degree=self.degree)]

    def Kdiag(self, X, presliced=False):
        """kernels.py:553-554"""
        return (self._lin_diag(X, presliced) + self.offset) ** self.degree

    def _grad_layout(self, d_all):
        return super()._grad_layout(d_all) + [(self._offset, None)]

    def dimwise(self, dim):
        raise NotImplementedError("Polynomial has no one-dimensional factors")


class Exponential(Stationary):
    """kernels.py:557-565"""
    _op = be.K_EXPONENTIAL


class Matern12(Stationary):
    """kernels.py:569-577"""
    _op = be.K_MATERN12


class Matern32(Stationary):
    """kernels.py:585-594"""
    _op = be.K_MATERN32


class Matern52(Stationary):
    """kernels.py:601-610"""
    _op = be.K_MATERN52


class Cosine(Stationary):
    """kernels.py:617-646: variance * cos(a - a'), a = sum_d x_d w_d / l_d; parameters [variance, lengthscales, weights].

    ``weights`` is an untransformed [input_dim, 1] parameter drawn from ``np.random.normal`` as in the reference; the
    ``weights=`` argument (not in the reference) fixes it.  Unlike the reference, which divides X by the lengthscales before
    it slices (kernels.py:634-636: wrong or failing with ``active_dims`` on a subset), the active columns are sliced first.
    The device op keeps lengthscales and weights in one 32-entry field: at most 16 active dims."""
    _op = be.K_COSINE

    def __init__(self, input_dim, variance=1.0, lengthscales=None, active_dims=None, ARD=False, min_ls=1e-6, name='kernel',
                 weights=None):
        super().__init__(input_dim, variance=variance, lengthscales=lengthscales, active_dims=active_dims, ARD=ARD,
                         min_ls=min_ls, name=name)
        if self.input_dim > be.GPS_MAX_DIMS // 2:
            raise ValueError("Cosine supports at most %d active dims" % (be.GPS_MAX_DIMS // 2))
        if weights is None:
            weights = np.random.normal(size=[self.input_dim, 1])
        weights = np.asarray(weights, dtype=settings.float_type).reshape(self.input_dim, 1)
        self._weights = Parameter(weights, name='weights')
        self._parameters = self._parameters + [self._weights]

    @property
    def weights(self):
        return self._weights.value

    def _nodes(self, presliced, d_all):
        dims = self._dims(presliced, d_all)
        ls = np.atleast_1d(self.lengthscales)
        w = np.asarray(self.weights, dtype=settings.float_type).ravel()
        if ls.size not in (1, len(dims)) or w.size != len(dims):
            raise ValueError("lengthscales / weights do not match the active dims")
        if len(dims) > be.GPS_MAX_DIMS // 2:
            raise ValueError("Cosine supports at most %d active dims" % (be.GPS_MAX_DIMS // 2))
        ls = ls * np.ones(len(dims), dtype=settings.float_type)
        return [be.primitive_node(be.K_COSINE, np.squeeze(self.variance), dims, np.concatenate([ls, w]))]

    def _grad_layout(self, d_all):
        nd = len(self._dims(False, d_all))
        return super()._grad_layout(d_all) + [(self._weights, d) for d in range(nd)]

    def dimwise(self, dim):
        raise NotImplementedError("Cosine has no one-dimensional factors")


class ArcCosine(Kernel):
    """kernels.py:649-766 (Cho & Saul 2009): with P(x, x') = sum_d w_d x_d x'_d + b, n = P(x, x),
    theta = acos(1e-15 + (1 - 2e-15) P / (sqrt(n) sqrt(n'))):  variance / pi * J_order(theta) * (n n')^(order / 2).
    Parameters [variance, bias_variance, weight_variances].  Kdiag depends on the point, so the device paths that assume a
    constant Kdiag refuse this kernel exactly where they refuse Linear.  The device op keeps the weight variances and the
    bias variance in one 32-entry field: at most 31 active dims."""
    implemented_orders = {0, 1, 2}

    def __init__(self, input_dim, order=0, variance=1.0, weight_variances=1., bias_variance=1.0, active_dims=None, ARD=False,
                 name='kernel'):
        super().__init__(input_dim, active_dims, name=name)
        if order not in self.implemented_orders:
            raise ValueError('Requested kernel order is not implemented.')
        if self.input_dim > be.GPS_MAX_DIMS - 1:
            raise ValueError("ArcCosine supports at most %d active dims" % (be.GPS_MAX_DIMS - 1))
        self.order = order
        self._variance = Parameter(variance, transform=transforms.positive, name='variance')
        self._bias_variance = Parameter(bias_variance, transform=transforms.positive, name='bias_variance')
        if ARD:
            weight_variances = (1.0 if weight_variances is None else weight_variances) * np.ones(self.input_dim, dtype=settings.float_type)
        elif weight_variances is None:
            weight_variances = 1.0
        self.ARD = ARD
        self._weight_variances = Parameter(weight_variances, transform=transforms.positive, name='weight_variances')
        self._parameters = self._parameters + [self._variance, self._bias_variance, self._weight_variances]

    @property
    def variance(self):
        return self._variance.value

    @property
    def bias_variance(self):
        return self._bias_variance.value

    @property
    def weight_variances(self):
        return self._weight_variances.value

    def _dim_weights(self, presliced, d_all):
        dims = self._dims(presliced, d_all)
        w = np.atleast_1d(self.weight_variances)
        if w.size not in (1, len(dims)):
            raise ValueError("weight variances do not match the active dims")
        if len(dims) > be.GPS_MAX_DIMS - 1:
            raise ValueError("ArcCosine supports at most %d active dims" % (be.GPS_MAX_DIMS - 1))
        return dims, w * np.ones(len(dims), dtype=settings.float_type)

    def _nodes(self, presliced, d_all):
        dims, w = self._dim_weights(presliced, d_all)
        b = float(np.squeeze(self.bias_variance))
        return [be.primitive_node(be.K_ARCCOSINE, np.squeeze(self.variance), dims, np.concatenate([w, [b]]), period=float(self.order))]

    def _J0(self):
        return (np.pi, np.pi, 3.0 * np.pi)[self.order]

    def Kdiag(self, X, presliced=False):
        """kernels.py:760-766"""
        X = np.asarray(X, dtype=settings.float_type)
        dims, w = self._dim_weights(presliced, X.shape[1])
        n = np.sum(np.square(X[:, dims]) * w, 1) + self.bias_variance
        return self.variance * (1. / np.pi) * self._J0() * n ** self.order

    def _grad_layout(self, d_all):
        nd = len(self._dims(False, d_all))
        ard = np.atleast_1d(self.weight_variances).size > 1
        return [(self._variance, None), (self._bias_variance, None)] + [(self._weight_variances, d if ard else None) for d in range(nd)]


class Coregion(Kernel):
    """kernels.py:822-881: K(x, y) = B[x, y] with B = W W^T + diag(kappa), indexed by the integer in one column of X (cast from
    float by truncation toward zero, as tf.cast does).  ``RBF(active_dims=inputs) * Coregion(1, P, R, active_dims=[label])`` is
    the intrinsic coregionalisation model: P correlated outputs, observed at inputs of their own, stacked into one exact GP.

    W starts at zero as in the reference, where there is a symmetry between its elements and so a stationary point: start an
    optimisation from a random W.  Kdiag depends on the point, so the device paths that assume a constant Kdiag refuse this
    kernel exactly where they refuse Linear.  The device op keeps W and kappa in one 32-entry field:
    output_dim * (rank + 1) <= 32.  Unlike the reference, whose tf.gather fails on the CPU for such input, a label that is
    not finite or whose truncated value lies outside [0, output_dim) raises ValueError before anything reaches the device."""

    def __init__(self, input_dim, output_dim, rank, active_dims=None, name='kernel'):
        assert input_dim == 1, "Coregion kernel in 1D only"
        super().__init__(input_dim, active_dims, name=name)
        self.output_dim, self.rank = int(output_dim), int(rank)
        if self.output_dim < 1 or self.rank < 0:
            raise ValueError("Coregion needs output_dim >= 1 and rank >= 0")
        self._W = Parameter(np.zeros((self.output_dim, self.rank), dtype=settings.float_type), name='W')
        self._kappa = Parameter(np.ones(self.output_dim, dtype=settings.float_type), transform=transforms.positive, name='kappa')
        self._parameters = self._parameters + [self._W, self._kappa]

    @property
    def W(self):
        return self._W.value

    @property
    def kappa(self):
        return self._kappa.value

    def _column(self, presliced, d_all):
        dims = self._dims(presliced, d_all)
        if len(dims) != 1:
            raise ValueError("Input 1st dimension does not match kernel dimension.")
        return dims[0]

    def _labels(self, X, presliced=False):
        """The integer labels of X's index column; ValueError for one that is not finite or outside [0, output_dim)."""
        X = np.asarray(X, dtype=settings.float_type)
        x = X[:, self._column(presliced, X.shape[1])]
        if not np.all(np.isfinite(x)):
            raise ValueError("Coregion: the index column holds a value that is not finite")
        a = np.trunc(x)
        if np.any(a < 0) or np.any(a >= self.output_dim):
            raise ValueError("Coregion: the index column holds a label outside [0, %d)" % self.output_dim)
        return a.astype(np.int64)

    def _check_inputs(self, *Xs):
        for X in Xs:
            if X is not None:
                self._labels(X)

    def _nodes(self, presliced, d_all):
        return [be.coregion_node(self._column(presliced, d_all), np.reshape(self.W, (self.output_dim, self.rank)), self.kappa)]

    def K(self, X, X2=None, presliced=False):
        if presliced:
            self._labels(X, True)
            if X2 is not None:
                self._labels(X2, True)
        return super().K(X, X2, presliced)

    def Kdiag(self, X, presliced=False):
        """kernels.py:877-881"""
        a = self._labels(X, presliced)
        return (np.sum(np.square(np.reshape(self.W, (self.output_dim, self.rank))), 1) + self.kappa)[a]

    def _grad_layout(self, d_all):
        return [(self._W, q) for q in range(self.output_dim * self.rank)] + [(self._kappa, p) for p in range(self.output_dim)]


class Periodic(Kernel):
    """kernels.py:769-819 (no ARD for lengthscale or period, as in the reference)"""

    def __init__(self, input_dim, period=1.0, variance=1.0, lengthscales=1.0, active_dims=None, name='kernel'):
        super().__init__(input_dim, active_dims, name=name)
        self._variance = Parameter(variance, transform=transforms.positive, name='variance')
        self._ls = Parameter(lengthscales, transform=transforms.positive, name='ls')
        self._period = Parameter(period, transform=transforms.positive, name='period')
        self._parameters = self._parameters + [self._variance, self._ls, self._period]

    @property
    def variance(self):
        return self._variance.value

    @property
    def lengthscales(self):
        return self._ls.value

    @property
    def period(self):
        return self._period.value

    def _nodes(self, presliced, d_all):
        dims = self._dims(presliced, d_all)
        return [be.primitive_node(be.K_PERIODIC, np.squeeze(self.variance), dims,
                                  float(np.squeeze(self.lengthscales)), period=float(np.squeeze(self.period)))]

    def Kdiag(self, X, presliced=False):
        """kernels.py:803-804"""
        return np.full(np.shape(X)[0], np.squeeze(self.variance), dtype=settings.float_type)

    def _grad_layout(self, d_all):
        return [(self._variance, None), (self._ls, None), (self._period, None)]


_SCALARS = (int, float, np.floating, np.integer)


class Combination(Kernel):
    """kernels.py:1000-1057"""
    _fold_op = None

    def __init__(self, kern_list, name='kernel'):
        extra_dims = np.asarray([], dtype=int)
        active_dims = reduce(np.union1d, (np.r_[x.active_dims] for x in kern_list if isinstance(x, Kernel)),
                             extra_dims)
        input_dim = active_dims.size
        super().__init__(input_dim=input_dim, name=name, active_dims=active_dims)
        # flatten instances of the same class (kernels.py:1019-1029)
        self.kern_list = []
        self.const_list = []
        for k in kern_list:
            if isinstance(k, self.__class__):
                self.kern_list.extend(k.kern_list)
                self.const_list.extend(k.const_list)
            elif isinstance(k, _SCALARS):
                self.const_list.append(float(k))
            elif isinstance(k, Kernel):
                if callable(getattr(k, "_on_combine", None)):
                    k._on_combine()                      # (kernels that cannot be part of a kernel program raise here)
                self.kern_list.append(k)
            else:
                raise TypeError("can only combine Kernel instances and scalars")
        for kern in kern_list:
            if isinstance(kern, Kernel):
                self._parameters = self._parameters + kern.parameters

    @property
    def on_separate_dimensions(self):
        """kernels.py:1039-1057"""
        if np.any([isinstance(k.active_dims, slice) for k in self.kern_list]):
            return False
        dimlist = [k.active_dims for k in self.kern_list]
        overlapping = False
        for i, dims_i in enumerate(dimlist):
            for dims_j in dimlist[i + 1:]:
                if np.any(dims_i.reshape(-1, 1) == dims_j.reshape(1, -1)):
                    overlapping = True
        return not overlapping

    def _nodes(self, presliced, d_all):
        # children slice from the *original* X (kernels.py:1073), left fold in list order and then
        # over const_list (reduce(op, [K1, K2, ...] + const_list))
        nodes = []
        first = True
        for k in self.kern_list:
            nodes.extend(k._nodes(False, d_all))
            if not first:
                nodes.append(be.op_node(self._fold_op))
            first = False
        for c in self.const_list:
            nodes.append(be.primitive_node(be.K_CONSTANT, c))
            if not first:
                nodes.append(be.op_node(self._fold_op))
            first = False
        return nodes

    def _fold(self, values):
        raise NotImplementedError

    def _grad_layout(self, d_all):
        out = []
        for k in self.kern_list:
            out.extend(k._grad_layout(d_all))
        out.extend([(None, None)] * len(self.const_list))     # scalar constants: slot exists, no parameter
        return out

    def _check_inputs(self, *Xs):
        for k in self.kern_list:
            k._check_inputs(*Xs)

    def Kdiag(self, X, presliced=False):
        return self._fold([k.Kdiag(X) for k in self.kern_list] + self.const_list)


class Sum(Combination):
    """kernels.py:1071-1076"""
    _fold_op = be.K_ADD

    def _fold(self, values):
        return reduce(np.add, values)


class Product(Combination):
    """kernels.py:1079-1084"""
    _fold_op = be.K_MUL

    def _fold(self, values):
        return reduce(np.multiply, values)


# the reference also registers these spellings
Add = Sum
Prod = Product
