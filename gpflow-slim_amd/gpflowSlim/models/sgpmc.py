"""Sparse GP with a non-Gaussian likelihood and whitened inducing values, for MCMC / MAP (Hensman et al. 2015, "MCMC for
variationally sparse Gaussian processes").

Mirrors gpflowSlim/models/sgpmc.py:58-104:  v ~ N(0, I),  u = Lm v,  Lm Lm^T = Kuu + jitter I, and the model's likelihood is the
sum of the variational expectations at the exact marginals of p(f | u = Lm v) -- the N(0, 1) prior on V enters through
``Parameter.prior`` like every other prior.  It is GPMC's sampler-facing model at M inducing points instead of N data points.

With one of the built-in likelihoods (Gaussian, Bernoulli, Poisson, Exponential, StudentT, MultiClass, Gamma, Beta, Ordinal
with their default links) the likelihood is one device call that streams the data in row chunks (gps_sgpmc_lik: device memory O(M^2 + M chunk), no
[M, N] array), and so is its gradient in every kernel parameter, the likelihood's parameter, V, the mean and, with
``train_inducing``, Z (gps_sgpmc_lik_grad: the same single pass).  MultiClass is fine here, unlike in GPMC: the variational
expectation at fvar > 0 is smooth.  Any other likelihood object with a ``variational_expectations`` gets the marginals from
``features.conditional`` and is summed on the host (value only: there is no autodiff to differentiate it).

The reference has no sampler of its own either; examples/sgpmc.py runs HMC on ``_objective_and_grad``.
"""
import numpy as np

from .. import _backend as be
from .. import features
from .. import priors
from .._settings import settings
from ..params import Parameter
from . import gpmc as _gpmc
from .model import GPModel


def device_likelihood(likelihood):
    """gpmc.device_likelihood with MultiClass allowed: the variational expectation at fvar > 0 is smooth in the moments"""
    return _gpmc.device_likelihood(likelihood, allow_multiclass=True)


class SGPMC(GPModel):
    def __init__(self, X, Y, kern, likelihood, feat=None, mean_function=None, num_latent=None, Z=None, train_inducing=False,
                 **kwargs):
        """X [N, D], Y [N, R] ([N, 1] class labels for MultiClass), Z [M, D] or feat; kern, likelihood, mean_function as
        everywhere (models/sgpmc.py:58-77).  train_inducing puts Z into ``parameters`` as SVGP's does."""
        X = np.ascontiguousarray(X, dtype=settings.float_type)
        Y = np.ascontiguousarray(Y, dtype=settings.float_type)
        GPModel.__init__(self, X, Y, kern, likelihood, mean_function, **kwargs)
        self.num_data = X.shape[0]
        self.num_latent = num_latent or Y.shape[1]
        self.feature = features.inducingpoint_wrapper(feat, Z)
        features.refuse_multiscale(self.feature, "SGPMC")
        self._V = Parameter(np.zeros((len(self.feature), self.num_latent), dtype=settings.float_type), name='V')
        self._V.prior = priors.Gaussian(0., 1.)
        self._parameters = self._parameters + [self._V]
        self.train_inducing = bool(train_inducing)
        if self.train_inducing and getattr(self.feature, "_Z", None) is not None:
            self._parameters = self._parameters + [self.feature._Z]
        self.chunk_rows = 0                                        # rows of X per device chunk; 0: the library's choice

    @property
    def V(self):
        return self._V.value

    def _mean_on(self, X):
        mean = np.asarray(self.mean_function(X), dtype=settings.float_type)
        if not np.any(mean):
            return None
        return np.ascontiguousarray(np.broadcast_to(mean, (X.shape[0], self.num_latent)))

    def _build_likelihood(self):
        """models/sgpmc.py:83-89: the sum of the variational expectations at the marginals of p(f | u = Lm V)"""
        dl = device_likelihood(self.likelihood)
        self.kern._check_inputs(self.feature.Z, self.X)
        if dl is not None:
            return be.get_handle().sgpmc_lik(self.kern._program(self.X.shape[1]), self.feature.Z, self.X, self.Y, self.V,
                                             settings.numerics.jitter_level, dl[0], mean=self._mean_on(self.X),
                                             chunk_rows=self.chunk_rows)
        fmean, fvar = self._build_predict(self.X, full_cov=False)
        return float(np.sum(self.likelihood.variational_expectations(fmean, fvar, self.Y)))

    def compute_log_likelihood_and_gradients(self):
        """The likelihood and d likelihood / d(unconstrained parameter) for every parameter of the model, V included (and Z
        with train_inducing) -- what ``tf.gradients`` yields in the reference.  Returns (loglik, [(Parameter, gradient shaped
        like its unconstrained array), ...]) in the order of ``parameters``; the priors are Model._objective_and_grad's."""
        dl = device_likelihood(self.likelihood)
        if dl is None:
            raise NotImplementedError("analytic gradients of SGPMC need one of the built-in likelihoods (Gaussian, Bernoulli, "
                                      "Poisson, Exponential, StudentT, MultiClass, Gamma, Beta, Ordinal) with its default link")
        X = self.X
        self.kern._check_inputs(self.feature.Z, X)
        d_all = X.shape[1]
        layout = self.kern._grad_layout(d_all)
        zparam = getattr(self.feature, "_Z", None)
        want_z = zparam is not None and any(p is zparam for p in self.parameters)
        res = be.get_handle().sgpmc_lik_grad(self.kern._program(d_all), self.feature.Z, X, self.Y, self.V,
                                             settings.numerics.jitter_level, dl[0], mean=self._mean_on(X),
                                             chunk_rows=self.chunk_rows, want_grad_Z=want_z)
        ll, slots, glik, g_V, g_mean = res[:5]
        g_Z = res[5] if want_z else None
        if len(layout) != len(slots):
            raise RuntimeError("gradient slot layout mismatch: %d vs %d" % (len(layout), len(slots)))
        grads = {id(p): np.zeros_like(np.atleast_1d(p.vf_val), dtype=settings.float_type) for p in self.parameters}
        for (param, idx), g in zip(layout, slots):
            if param is None:
                continue
            if idx is None:
                grads[id(param)] += g
            else:
                grads[id(param)].reshape(-1)[idx] += g
        if dl[1] is not None:
            grads[id(dl[1])] += glik
        from ..mean_functions import Constant as _MConst, Linear as _MLin
        mf = self.mean_function

        def _fit(g, like):
            like = np.atleast_1d(like)
            return g.reshape(like.shape) if g.size == like.size else np.full(like.shape, np.sum(g))

        if isinstance(mf, _MConst):
            grads[id(mf.c)] = grads[id(mf.c)] + _fit(np.sum(g_mean, axis=0), mf.c.vf_val)
        elif isinstance(mf, _MLin):
            grads[id(mf.A)] = grads[id(mf.A)] + _fit(X.T @ g_mean, mf.A.vf_val)
            grads[id(mf.b)] = grads[id(mf.b)] + _fit(np.sum(g_mean, axis=0), mf.b.vf_val)
        grads[id(self._V)] = g_V
        if want_z:
            grads[id(zparam)] = g_Z
        out = []
        for p in self.parameters:
            g = grads[id(p)].reshape(np.atleast_1d(p.vf_val).shape) * np.atleast_1d(p.transform.forward_grad(p.vf_val))
            out.append((p, g.reshape(p.vf_val.shape)))
        return ll, out

    def _build_predict(self, Xnew, full_cov=False):
        """models/sgpmc.py:91-104: p(F* | U = Lm V) through the whitened conditional"""
        mu, var = features.conditional(self.feature, self.kern, Xnew, self.V, full_cov=full_cov, q_sqrt=None, white=True)
        return mu + self.mean_function(Xnew), var
