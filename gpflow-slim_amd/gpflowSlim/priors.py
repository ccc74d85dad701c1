"""Priors on parameters: log-densities of the constrained value, on the host.

Mirrors gpflowSlim/priors.py:31-125 (constructors, ``logp`` summed over the elements, ``sample``, ``__str__``).  Every class
also has ``dlogp(x)``, the derivative of its log-density element by element: with the transforms' ``log_jacobian_grad`` it
gives Model._prior_and_grad the gradient of a log-prior in closed form (an N(0, 1) prior on the [N, R] whitened variables
of GPMC / SGPMC costs one pass then, not one evaluation of the whole prior per entry).
"""
import numpy as np

from . import densities
from ._settings import settings


class Prior(object):
    def logp(self, x):
        raise NotImplementedError

    def dlogp(self, x):
        """d log p(x_i) / d x_i, shaped like x"""
        raise NotImplementedError

    def sample(self, shape=(1,)):
        raise NotImplementedError


def _vec(v):
    return np.atleast_1d(np.array(v, settings.float_type))


class Gaussian(Prior):
    def __init__(self, mu, var):
        self.mu, self.var = _vec(mu), _vec(var)

    def logp(self, x):
        return np.sum(densities.gaussian(np.asarray(x, dtype=settings.float_type), self.mu, self.var))

    def dlogp(self, x):
        return (self.mu - np.asarray(x, dtype=settings.float_type)) / self.var

    def sample(self, shape=(1,)):
        return self.mu + np.sqrt(self.var) * np.random.randn(*shape)

    def __str__(self):
        return "N(" + str(self.mu) + "," + str(self.var) + ")"


class LogNormal(Prior):
    def __init__(self, mu, var):
        self.mu, self.var = _vec(mu), _vec(var)

    def logp(self, x):
        return np.sum(densities.lognormal(np.asarray(x, dtype=settings.float_type), self.mu, self.var))

    def dlogp(self, x):
        x = np.asarray(x, dtype=settings.float_type)
        return ((self.mu - np.log(x)) / self.var - 1.0) / x

    def sample(self, shape=(1,)):
        return np.exp(self.mu + np.sqrt(self.var) * np.random.randn(*shape))

    def __str__(self):
        return "logN(" + str(self.mu) + "," + str(self.var) + ")"


class Gamma(Prior):
    def __init__(self, shape, scale):
        self.shape, self.scale = _vec(shape), _vec(scale)

    def logp(self, x):
        return np.sum(densities.gamma(self.shape, self.scale, np.asarray(x, dtype=settings.float_type)))

    def dlogp(self, x):
        return (self.shape - 1.0) / np.asarray(x, dtype=settings.float_type) - 1.0 / self.scale

    def sample(self, shape=(1,)):
        return np.random.gamma(self.shape, self.scale, size=shape)

    def __str__(self):
        return "Ga(" + str(self.shape) + "," + str(self.scale) + ")"


class Laplace(Prior):
    def __init__(self, mu, sigma):
        self.mu, self.sigma = _vec(mu), _vec(sigma)

    def logp(self, x):
        return np.sum(densities.laplace(self.mu, self.sigma, np.asarray(x, dtype=settings.float_type)))

    def dlogp(self, x):
        return np.sign(self.mu - np.asarray(x, dtype=settings.float_type)) / self.sigma

    def sample(self, shape=(1,)):
        return np.random.laplace(self.mu, self.sigma, size=shape)

    def __str__(self):
        return "Lap.(" + str(self.mu) + "," + str(self.sigma) + ")"


class Beta(Prior):
    def __init__(self, a, b):
        self.a, self.b = _vec(a), _vec(b)

    def logp(self, x):
        return np.sum(densities.beta(self.a, self.b, np.asarray(x, dtype=settings.float_type)))

    def dlogp(self, x):
        x = np.asarray(x, dtype=settings.float_type)
        inside = (x > 1e-6) & (x < 1 - 1e-6)                       # (the density clips its argument: flat outside)
        xc = np.clip(x, 1e-6, 1 - 1e-6)
        return np.where(inside, (self.a - 1.0) / xc - (self.b - 1.0) / (1.0 - xc), 0.0)

    def sample(self, shape=(1,)):
        return np.random.beta(self.a, self.b, size=shape)

    def __str__(self):
        return "Beta(" + str(self.a) + "," + str(self.b) + ")"


class Uniform(Prior):
    def __init__(self, lower=0., upper=1.):
        self.log_height = -np.log(upper - lower)
        self.lower, self.upper = lower, upper

    def logp(self, x):
        return self.log_height * float(np.size(x))

    def dlogp(self, x):
        return np.zeros(np.shape(x), dtype=settings.float_type)

    def sample(self, shape=(1,)):
        return self.lower + (self.upper - self.lower) * np.random.rand(*shape)

    def __str__(self):
        return "U(" + str(self.lower) + "," + str(self.upper) + ")"
