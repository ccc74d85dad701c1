"""Likelihoods.

Mirrors gpflowSlim/likelihoods.py: the generic Gauss-Hermite routines of ``Likelihood`` (:45-152), Gaussian (:158-188),
Poisson (:191-224), Exponential (:226-243), StudentT (:246-266), probit / Bernoulli (:269-298), Gamma (:301-333), Beta
(:336-376), RobustMax / MultiClass (:379-487), Ordinal (:554-631).  Everything here is host numpy: it serves prediction (``predict_y`` / ``predict_density`` at modest N*) and is
the slow path of the SVGP bound for user-defined likelihoods and links.  The built-in classes additionally describe
themselves to the backend (``_device_spec``): for them the per-point term of the SVGP bound, its derivatives and the whole
backward pass run on the device (csrc/lik.hip, gps_svgp_elbo_lik / gps_svgp_elbo_lik_grad).
"""
import numpy as np
from scipy.special import erf, erfc, gammaln

from . import densities
from . import transforms
from ._settings import settings
from .params import Parameter

# kinds of include/gpflowslim_hip.h
LIK_GAUSSIAN, LIK_BERNOULLI, LIK_POISSON, LIK_EXPONENTIAL, LIK_STUDENT_T, LIK_MULTICLASS, LIK_GAMMA, LIK_BETA, LIK_ORDINAL = range(9)


def hermgauss(n):
    """quadrature.py: numpy's rule, as the reference takes it"""
    x, w = np.polynomial.hermite.hermgauss(n)
    return x.astype(settings.float_type), w.astype(settings.float_type)


class Likelihood(object):
    def __init__(self, name='likelihood'):
        self._name = name
        self.num_gauss_hermite_points = 20
        self._parameters = []

    @property
    def name(self):
        return self._name

    @property
    def parameters(self):
        return self._parameters

    def conditional_mean(self, F):
        raise NotImplementedError

    def conditional_variance(self, F):
        raise NotImplementedError

    def logp(self, F, Y):
        raise NotImplementedError

    def _device_spec(self):
        """(kind, [up to four scalar parameters], trainable Parameter behind parameter 0 or None[, Ordinal's bin edges]) when
        the device kernels implement this likelihood, else None (host path)."""
        return None

    def predict_mean_and_var(self, Fmu, Fvar):
        """likelihoods.py:45-86"""
        gh_x, gh_w = hermgauss(self.num_gauss_hermite_points)
        gh_w = gh_w / np.sqrt(np.pi)
        gh_w = gh_w.reshape(-1, 1)
        shape = np.shape(Fmu)
        Fmu, Fvar = [np.reshape(e, (-1, 1)) for e in (Fmu, Fvar)]
        X = gh_x[None, :] * np.sqrt(2.0 * Fvar) + Fmu
        E_y = np.reshape(np.matmul(self.conditional_mean(X), gh_w), shape)
        integrand = self.conditional_variance(X) + np.square(self.conditional_mean(X))
        V_y = np.reshape(np.matmul(integrand, gh_w), shape) - np.square(E_y)
        return E_y, V_y

    def predict_density(self, Fmu, Fvar, Y):
        """likelihoods.py:88-119"""
        gh_x, gh_w = hermgauss(self.num_gauss_hermite_points)
        gh_w = gh_w.reshape(-1, 1) / np.sqrt(np.pi)
        shape = np.shape(Fmu)
        Fmu, Fvar, Y = [np.reshape(e, (-1, 1)) for e in (Fmu, Fvar, Y)]
        X = gh_x[None, :] * np.sqrt(2.0 * Fvar) + Fmu
        Y = np.tile(Y, [1, self.num_gauss_hermite_points])
        logp = self.logp(X, Y)
        return np.reshape(np.log(np.matmul(np.exp(logp), gh_w)), shape)

    def variational_expectations(self, Fmu, Fvar, Y):
        """likelihoods.py:121-152"""
        gh_x, gh_w = hermgauss(self.num_gauss_hermite_points)
        gh_x = gh_x.reshape(1, -1)
        gh_w = gh_w.reshape(-1, 1) / np.sqrt(np.pi)
        shape = np.shape(Fmu)
        Fmu, Fvar, Y = [np.reshape(e, (-1, 1)) for e in (Fmu, Fvar, Y)]
        X = gh_x * np.sqrt(2.0 * Fvar) + Fmu
        Y = np.tile(Y, [1, self.num_gauss_hermite_points])
        logp = self.logp(X, Y)
        return np.reshape(np.matmul(logp, gh_w), shape)


class Gaussian(Likelihood):
    def __init__(self, var=1.0, min_var=None):
        super().__init__()
        trans = transforms.positive if min_var is None else transforms.Log1pe(min_var)   # :162
        self._variance = Parameter(var, transform=trans, dtype=settings.float_type, name='variance')
        self._parameters = self._parameters + [self._variance]

    @property
    def variance(self):
        return self._variance.value

    def logp(self, F, Y):
        return densities.gaussian(F, Y, self.variance)

    def conditional_mean(self, F):
        return np.array(F, copy=True)

    def conditional_variance(self, F):
        return np.full(np.shape(F), np.squeeze(self.variance))

    def predict_mean_and_var(self, Fmu, Fvar):
        """likelihoods.py:180-181"""
        return np.array(Fmu, copy=True), Fvar + self.variance

    def predict_density(self, Fmu, Fvar, Y):
        """likelihoods.py:183-184"""
        return densities.gaussian(Fmu, Y, Fvar + self.variance)

    def variational_expectations(self, Fmu, Fvar, Y):
        """likelihoods.py:186-188"""
        return -0.5 * np.log(2 * np.pi) - 0.5 * np.log(self.variance) \
               - 0.5 * (np.square(Y - Fmu) + Fvar) / self.variance


class Poisson(Likelihood):
    """likelihoods.py:191-224: p(y | f) = Poisson(y | invlink(f) * binsize)"""

    def __init__(self, invlink=np.exp, binsize=1.):
        Likelihood.__init__(self)
        self.invlink = invlink
        self.binsize = np.double(binsize)

    def logp(self, F, Y):
        return densities.poisson(self.invlink(F) * self.binsize, Y)

    def conditional_variance(self, F):
        return self.invlink(F) * self.binsize

    def conditional_mean(self, F):
        return self.invlink(F) * self.binsize

    def variational_expectations(self, Fmu, Fvar, Y):
        if self.invlink is np.exp:
            return Y * Fmu - np.exp(Fmu + Fvar / 2) * self.binsize \
                   - gammaln(Y + 1) + Y * np.log(self.binsize)
        return super(Poisson, self).variational_expectations(Fmu, Fvar, Y)

    def _device_spec(self):
        return (LIK_POISSON, [float(self.binsize)], None) if self.invlink is np.exp else None


class Exponential(Likelihood):
    """likelihoods.py:226-243"""

    def __init__(self, invlink=np.exp):
        super().__init__()
        self.invlink = invlink

    def logp(self, F, Y):
        return densities.exponential(self.invlink(F), Y)

    def conditional_mean(self, F):
        return self.invlink(F)

    def conditional_variance(self, F):
        return np.square(self.invlink(F))

    def variational_expectations(self, Fmu, Fvar, Y):
        if self.invlink is np.exp:
            return - np.exp(-Fmu + Fvar / 2) * Y - Fmu
        return super().variational_expectations(Fmu, Fvar, Y)

    def _device_spec(self):
        return (LIK_EXPONENTIAL, [], None) if self.invlink is np.exp else None


class StudentT(Likelihood):
    """likelihoods.py:246-266"""

    def __init__(self, deg_free=3.0):
        Likelihood.__init__(self)
        self.deg_free = deg_free
        self._scale = Parameter(1.0, transform=transforms.positive, dtype=settings.float_type, name='scale')
        self._parameters = self._parameters + [self._scale]

    @property
    def scale(self):
        return self._scale.value

    def logp(self, F, Y):
        return densities.student_t(Y, F, self.scale, self.deg_free)

    def conditional_mean(self, F):
        return np.array(F, copy=True)

    def conditional_variance(self, F):
        return F * 0.0 + (self.deg_free / (self.deg_free - 2.0))

    def _device_spec(self):
        return (LIK_STUDENT_T, [float(np.squeeze(self.scale)), float(self.deg_free)], self._scale)


def probit(x):
    """likelihoods.py:269-270"""
    return 0.5 * (1.0 + erf(x / np.sqrt(2.0))) * (1 - 2e-3) + 1e-3


def probit_difference(zl, zr):
    """probit(zl) - probit(zr) for zl >= zr, = (1 - 2e-3) (Phi(zl) - Phi(zr)): the number :605-606 subtract, taken on the side
    where both Phi are small, as a difference of two erfc.  As written there, two numbers near 1 (or 1e-3) are subtracted where
    both arguments lie in the same far tail, and what is left next to the 1e-6 floor of Ordinal.logp is their rounding: 1e-10
    relative in log p, measured 1.35e-11 of max(1, |log p|).  This form is within a few eps of its own value everywhere, and
    it is what the device kernels compute (csrc/lik.hip), term by term."""
    zl, zr = np.broadcast_arrays(np.asarray(zl, dtype=settings.float_type), np.asarray(zr, dtype=settings.float_type))
    up = (zl + zr) > 0.0                    # (zl = +inf: up, its erfc is 0; zr = -inf: down, likewise; never both)
    ea = erfc(np.where(up, zr, -zl) / np.sqrt(2.0))
    eb = erfc(np.where(up, zl, -zr) / np.sqrt(2.0))
    return (1 - 2e-3) * (0.5 * (ea - eb))


class Bernoulli(Likelihood):
    """likelihoods.py:273-298"""

    def __init__(self, invlink=probit):
        Likelihood.__init__(self)
        self.invlink = invlink

    def logp(self, F, Y):
        return densities.bernoulli(self.invlink(F), Y)

    def predict_mean_and_var(self, Fmu, Fvar):
        if self.invlink is probit:
            p = probit(Fmu / np.sqrt(1 + Fvar))
            return p, p - np.square(p)
        return Likelihood.predict_mean_and_var(self, Fmu, Fvar)

    def predict_density(self, Fmu, Fvar, Y):
        p = self.predict_mean_and_var(Fmu, Fvar)[0]
        return densities.bernoulli(p, Y)

    def conditional_mean(self, F):
        return self.invlink(F)

    def conditional_variance(self, F):
        p = self.invlink(F)
        return p - np.square(p)

    def _device_spec(self):
        return (LIK_BERNOULLI, [], None) if self.invlink is probit else None


class Gamma(Likelihood):
    """likelihoods.py:301-333: the transformed GP gives the *scale* (inverse rate) of the Gamma"""

    def __init__(self, invlink=np.exp):
        Likelihood.__init__(self)
        self.invlink = invlink
        self._shape = Parameter(1.0, transform=transforms.positive, dtype=settings.float_type, name='shape')
        self._parameters = self._parameters + [self._shape]

    @property
    def shape(self):
        return self._shape.value

    def logp(self, F, Y):
        return densities.gamma(self.shape, self.invlink(F), Y)

    def conditional_mean(self, F):
        return self.shape * self.invlink(F)

    def conditional_variance(self, F):
        scale = self.invlink(F)
        return self.shape * np.square(scale)

    def variational_expectations(self, Fmu, Fvar, Y):
        if self.invlink is np.exp:
            return -self.shape * Fmu - gammaln(self.shape) \
                + (self.shape - 1.) * np.log(Y) - Y * np.exp(-Fmu + Fvar / 2.)
        return Likelihood.variational_expectations(self, Fmu, Fvar, Y)

    def _device_spec(self):
        return (LIK_GAMMA, [float(np.squeeze(self.shape))], self._shape) if self.invlink is np.exp else None


class Beta(Likelihood):
    """likelihoods.py:336-376: the mean of the Beta density is the transformed process, m = invlink(f), with a scale
    parameter: alpha = scale * m, beta = scale * (1 - m)."""

    def __init__(self, invlink=probit, scale=1.0):
        Likelihood.__init__(self)
        self._scale = Parameter(scale, transform=transforms.positive, dtype=settings.float_type, name='scale')
        self.invlink = invlink
        self._parameters = self._parameters + [self._scale]

    @property
    def scale(self):
        return self._scale.value

    def logp(self, F, Y):
        mean = self.invlink(F)
        alpha = mean * self.scale
        beta = self.scale - alpha
        return densities.beta(alpha, beta, Y)

    def conditional_mean(self, F):
        return self.invlink(F)

    def conditional_variance(self, F):
        mean = self.invlink(F)
        return (mean - np.square(mean)) / (self.scale + 1.)

    def _device_spec(self):
        return (LIK_BETA, [float(np.squeeze(self.scale))], self._scale) if self.invlink is probit else None


class Ordinal(Likelihood):
    """likelihoods.py:554-631: ordinal regression (Chu and Ghahramani 2005).  The data are the integers 0 .. K and the K bin
    edges a_0 < ... < a_{K-1} say where the label switches:
        p(Y = 0 | F) = phi((a_0 - F) / sigma),  p(Y = j | F) = phi((a_j - F) / sigma) - phi((a_{j-1} - F) / sigma),
        p(Y = K | F) = 1 - phi((a_{K-1} - F) / sigma)
    with phi the (squashed) probit and sigma a parameter to be learned."""

    def __init__(self, bin_edges):
        Likelihood.__init__(self)
        self.bin_edges = np.asarray(bin_edges, dtype=settings.float_type).ravel()
        self.num_bins = self.bin_edges.size + 1
        self._sigma = Parameter(1.0, transform=transforms.positive, dtype=settings.float_type, name='sigma')
        self._parameters = self._parameters + [self._sigma]

    @property
    def sigma(self):
        return self._sigma.value

    def _labels(self, Y):
        """tf.cast(Y, tf.int64) + tf.gather (:599-603), which refuses an index outside the table"""
        Y = np.asarray(Y)
        if not (np.all(np.isfinite(Y)) and np.all(Y == np.floor(Y)) and Y.min() >= 0 and Y.max() <= self.bin_edges.size):
            raise ValueError("Ordinal labels must be integers in [0, %d] (the number of bin edges)" % self.bin_edges.size)
        return Y.astype(np.int64)

    def logp(self, F, Y):
        Y = self._labels(Y)
        scaled_bins_left = np.concatenate([self.bin_edges / self.sigma, np.array([np.inf])], 0)
        scaled_bins_right = np.concatenate([np.array([-np.inf]), self.bin_edges / self.sigma], 0)
        selected_bins_left = scaled_bins_left[Y]
        selected_bins_right = scaled_bins_right[Y]
        return np.log(probit_difference(selected_bins_left - F / self.sigma,
                                        selected_bins_right - F / self.sigma) + 1e-6)

    def _make_phi(self, F):
        """:608-619: one row per entry of F (flattened), one column per label: the probability of that label"""
        scaled_bins_left = np.concatenate([self.bin_edges / self.sigma, np.array([np.inf])], 0)
        scaled_bins_right = np.concatenate([np.array([-np.inf]), self.bin_edges / self.sigma], 0)
        return probit(scaled_bins_left - np.reshape(F, (-1, 1)) / self.sigma) \
            - probit(scaled_bins_right - np.reshape(F, (-1, 1)) / self.sigma)

    def conditional_mean(self, F):
        phi = self._make_phi(F)
        Ys = np.reshape(np.arange(self.num_bins, dtype=np.float64), (-1, 1))
        return np.reshape(np.matmul(phi, Ys), np.shape(F))

    def conditional_variance(self, F):
        phi = self._make_phi(F)
        Ys = np.reshape(np.arange(self.num_bins, dtype=np.float64), (-1, 1))
        E_y = np.matmul(phi, Ys)
        E_y2 = np.matmul(phi, np.square(Ys))
        return np.reshape(E_y2 - np.square(E_y), np.shape(F))

    def _device_spec(self):
        """a fourth element: the table of bin edges (at most 32 on the device; _backend.make_lik raises beyond)"""
        return (LIK_ORDINAL, [float(np.squeeze(self.sigma))], self._sigma, self.bin_edges)


class RobustMax(object):
    """likelihoods.py:379-425: y_i = 1 - eps for i = argmax(f), eps / (k - 1) otherwise."""

    def __init__(self, num_classes, epsilon=1e-3):
        self.epsilon = epsilon
        self.num_classes = num_classes
        self._eps_K1 = self.epsilon / (self.num_classes - 1.)

    def __call__(self, F):
        i = np.argmax(F, 1)
        out = np.full((np.shape(F)[0], self.num_classes), self._eps_K1, dtype=settings.float_type)
        out[np.arange(out.shape[0]), i] = 1. - self.epsilon
        return out

    def prob_is_largest(self, Y, mu, var, gh_x, gh_w):
        """likelihoods.py:404-425"""
        Y = np.asarray(Y).astype(np.int64).reshape(-1)
        oh_on = np.zeros((Y.shape[0], self.num_classes), dtype=settings.float_type)
        oh_on[np.arange(Y.shape[0]), Y] = 1.
        mu_selected = np.sum(oh_on * mu, 1)
        var_selected = np.sum(oh_on * var, 1)
        X = np.reshape(mu_selected, (-1, 1)) + gh_x * np.reshape(
            np.sqrt(np.clip(2. * var_selected, 1e-10, np.inf)), (-1, 1))
        dist = (np.expand_dims(X, 1) - np.expand_dims(mu, 2)) / np.expand_dims(
            np.sqrt(np.clip(var, 1e-10, np.inf)), 2)
        cdfs = 0.5 * (1.0 + erf(dist / np.sqrt(2.0)))
        cdfs = cdfs * (1 - 2e-4) + 1e-4
        oh_off = 1. - oh_on
        cdfs = cdfs * np.expand_dims(oh_off, 2) + np.expand_dims(oh_on, 2)
        return np.matmul(np.prod(cdfs, axis=1), np.reshape(gh_w / np.sqrt(np.pi), (-1, 1)))


class MultiClass(Likelihood):
    """likelihoods.py:428-487; the only inverse link is a RobustMax."""

    def __init__(self, num_classes, invlink=None):
        Likelihood.__init__(self)
        self.num_classes = num_classes
        if invlink is None:
            invlink = RobustMax(self.num_classes)
        elif not isinstance(invlink, RobustMax):
            raise NotImplementedError
        self.invlink = invlink

    def logp(self, F, Y):
        hits = np.equal(np.expand_dims(np.argmax(F, 1), 1), np.asarray(Y).astype(np.int64))
        yes = np.ones(np.shape(Y), dtype=settings.float_type) - self.invlink.epsilon
        no = np.zeros(np.shape(Y), dtype=settings.float_type) + self.invlink._eps_K1
        return np.log(np.where(hits, yes, no))

    def variational_expectations(self, Fmu, Fvar, Y):
        gh_x, gh_w = hermgauss(self.num_gauss_hermite_points)
        p = self.invlink.prob_is_largest(Y, Fmu, Fvar, gh_x, gh_w)
        return p * np.log(1 - self.invlink.epsilon) + (1. - p) * np.log(self.invlink._eps_K1)

    def predict_mean_and_var(self, Fmu, Fvar):
        n = np.shape(Fmu)[0]
        ps = [self._predict_non_logged_density(Fmu, Fvar, np.full((n, 1), i, dtype=np.int64))
              for i in range(self.num_classes)]
        ps = np.transpose(np.stack([np.reshape(p, (-1,)) for p in ps]))
        return ps, ps - np.square(ps)

    def predict_density(self, Fmu, Fvar, Y):
        return np.log(self._predict_non_logged_density(Fmu, Fvar, Y))

    def _predict_non_logged_density(self, Fmu, Fvar, Y):
        gh_x, gh_w = hermgauss(self.num_gauss_hermite_points)
        p = self.invlink.prob_is_largest(Y, Fmu, Fvar, gh_x, gh_w)
        return p * (1 - self.invlink.epsilon) + (1. - p) * (self.invlink._eps_K1)

    def conditional_mean(self, F):
        return self.invlink(F)

    def conditional_variance(self, F):
        p = self.conditional_mean(F)
        return p - np.square(p)

    def _device_spec(self):
        return (LIK_MULTICLASS, [float(self.invlink.epsilon)], None)
