"""GP with a non-Gaussian likelihood and whitened latent values, for MCMC / MAP.

Mirrors gpflowSlim/models/gpmc.py:28-93:  v ~ N(0, I),  f = L v + m(x),  L L^T = K + jitter I, and the model's likelihood is
log p(Y | f) -- the N(0, 1) prior on V enters through ``Parameter.prior`` like every other prior.  With one of the built-in
likelihoods (Gaussian, Bernoulli, Poisson, Exponential, StudentT, Gamma, Beta, Ordinal with their default links) the likelihood is one device call
(gps_gpmc_lik: K, its factor, F = L V and the pointwise sum stay in HBM) and so is its gradient in every kernel parameter, the
likelihood's parameter, V and the mean (gps_gpmc_lik_grad); any other likelihood object with a ``logp`` gets F from the
device and is summed on the host (value only: there is no autodiff to differentiate it).  MultiClass is refused: its
``logp`` is piecewise constant in F, so neither a sampler nor an optimiser can use it.

The reference has no sampler of its own either; examples/gpmc.py runs HMC on ``_objective_and_grad``.
"""
import numpy as np

from .. import _backend as be
from .. import conditionals
from .. import likelihoods
from .. import priors
from .._settings import settings
from ..params import Parameter
from .model import GPModel


def device_likelihood(likelihood, allow_multiclass=False):
    """((descriptor, arrays it points into), Parameter behind its scalar or None) for a likelihood the device evaluates; None
    for everything else.  MultiClass raises unless allow_multiclass (SGPMC: its variational expectation is smooth; GPMC's
    pointwise log p is not)."""
    if isinstance(likelihood, likelihoods.MultiClass) and not allow_multiclass:
        raise NotImplementedError("GPMC / SGPMC with MultiClass: log p(y | f) of the RobustMax link is piecewise constant in f "
                                  "(its gradient is zero almost everywhere), so there is nothing to sample or optimise with")
    if type(likelihood) is likelihoods.Gaussian:
        spec = (likelihoods.LIK_GAUSSIAN, [float(np.squeeze(likelihood.variance))], likelihood._variance)
    else:
        spec = getattr(likelihood, "_device_spec", lambda: None)()
    if spec is None:
        return None
    kind, params, trainable = spec[:3]
    edges = spec[3] if len(spec) > 3 else None                   # (Ordinal's table of bin edges)
    return be.make_lik(kind, params, min(likelihood.num_gauss_hermite_points, be.LIK_MAX_GH), edges=edges), trainable


class GPMC(GPModel):
    def __init__(self, X, Y, kern, likelihood, mean_function=None, num_latent=None, **kwargs):
        """X [N, D], Y [N, R]; kern, likelihood, mean_function as everywhere (models/gpmc.py:29-58)."""
        X = np.ascontiguousarray(X, dtype=settings.float_type)
        Y = np.ascontiguousarray(Y, dtype=settings.float_type)
        if isinstance(likelihood, likelihoods.MultiClass):
            device_likelihood(likelihood)                           # (raises, with the reason)
        GPModel.__init__(self, X, Y, kern, likelihood, mean_function, **kwargs)
        self.num_data = X.shape[0]
        self.num_latent = num_latent or Y.shape[1]
        self._V = Parameter(np.zeros((self.num_data, self.num_latent), dtype=settings.float_type), name='V')
        self._V.prior = priors.Gaussian(0., 1.)
        self._parameters = self._parameters + [self._V]

    @property
    def V(self):
        return self._V.value

    def _mean_on(self, X):
        mean = np.asarray(self.mean_function(X), dtype=settings.float_type)
        if not np.any(mean):
            return None
        return np.ascontiguousarray(np.broadcast_to(mean, (X.shape[0], self.num_latent)))

    def _build_likelihood(self):
        """models/gpmc.py:64-77: log p(Y | F = L V + m(X))"""
        dl = device_likelihood(self.likelihood)
        self.kern._check_inputs(self.X)
        prog = self.kern._program(self.X.shape[1])
        h = be.get_handle()
        if dl is not None:
            return h.gpmc_lik(prog, self.X, self.V, self.Y, settings.numerics.jitter_level, dl[0], mean=self._mean_on(self.X))
        L = h.potrf(h.kmat(prog, self.X, diag_add=settings.numerics.jitter_level))
        F = h.tri_skinny(L, self.V) + self.mean_function(self.X)
        return float(np.sum(self.likelihood.logp(F, self.Y)))

    def compute_log_likelihood_and_gradients(self):
        """The likelihood and d likelihood / d(unconstrained parameter) for every parameter of the model, V included -- what
        ``tf.gradients`` yields in the reference.  Returns (loglik, [(Parameter, gradient shaped like its unconstrained
        array), ...]) in the order of ``parameters``; the priors are Model._objective_and_grad's."""
        dl = device_likelihood(self.likelihood)
        if dl is None:
            raise NotImplementedError("analytic gradients of GPMC need one of the built-in likelihoods (Gaussian, Bernoulli, "
                                      "Poisson, Exponential, StudentT, Gamma, Beta, Ordinal) with its default link")
        X = self.X
        self.kern._check_inputs(X)
        d_all = X.shape[1]
        layout = self.kern._grad_layout(d_all)
        ll, slots, glik, g_V, g_mean = be.get_handle().gpmc_lik_grad(
            self.kern._program(d_all), X, self.V, self.Y, settings.numerics.jitter_level, dl[0], mean=self._mean_on(X))
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
        out = []
        for p in self.parameters:
            g = grads[id(p)].reshape(np.atleast_1d(p.vf_val).shape) * np.atleast_1d(p.transform.forward_grad(p.vf_val))
            out.append((p, g.reshape(p.vf_val.shape)))
        return ll, out

    def _build_predict(self, Xnew, full_cov=False):
        """models/gpmc.py:79-93: p(F* | F = L V) through the whitened conditional"""
        mu, var = conditionals.conditional(Xnew, self.X, self.kern, self.V, full_cov=full_cov, q_sqrt=None, white=True)
        return mu + self.mean_function(Xnew), var
