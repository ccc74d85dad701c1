"""GPLVM, the point-estimate latent variable model, and the Bayesian GPLVM (Titsias & Lawrence 2010).

``GPLVM`` (gplvm.py:16-51) is a ``GPR`` whose inputs X [N, Q] are a trainable ``Parameter``: the likelihood is the exact-GP
log-marginal likelihood of Y given the latent positions, and its gradient with respect to them,
d LML / d X[i] = sum_j (A A^T - R K_y^-1)_ij d k(x_i, x_j) / d x_i, comes from the device with the rest of the gradient
(gps_gpr_lml_grad_x, csrc/grad_x.hip): inside the single synchronisation of the one-launch path at the sizes the model is
used at.  Any kernel with a likelihood gradient is accepted; at most 32 latent dimensions; no minibatching, no sharding over
ranks, no random-feature kernels.

Mirrors gpflowSlim/models/gplvm.py:54-220 (BayesianGPLVM, PCA_reduce).  The bound is the SGPR collapsed bound with
sum Kdiag, Kuf and Kuf Kuf^T replaced by the kernel expectations psi0, Psi1, Psi2 under q(x_n) = N(X_mean_n, diag X_var_n);
the expectations, both factorisations, the prediction and the whole gradient run in gps_bgplvm / gps_bgplvm_grad on the GPU.
The KL[q(x) || p(x)] term (gplvm.py:150-156) is elementwise over [N, Q] and is evaluated here with its gradient.

Scope: one ``ekernels.RBF`` over all Q latent dimensions, or an ``ekernels.Sum`` of RBF kernels on pairwise disjoint latent
dimensions (the kernel of the reference's examples/gplvm.py; gradients arrive per part in ``kern.kern_list[i]``), and diagonal
``X_var`` [N, Q]; no minibatching, no sharding over ranks.
"""
import numpy as np

from .. import ekernels
from .. import likelihoods
from .. import transforms
from .. import _backend as be
from ..params import Parameter
from ..mean_functions import Zero
from .._settings import settings
from .model import GPModel
from .gpr import GPR


class GPLVM(GPR):
    """gplvm.py:16-51: standard GPLVM, the likelihood is optimised with respect to the latent X as well."""
    MAX_LATENT = be.GPS_MAX_DIMS          # columns of X the device's input gradient takes

    def __init__(self, Y, latent_dim, X_mean=None, kern=None, mean_function=None, obs_var=0.1, **kwargs):
        """Y [N, D]; latent_dim Q; X_mean [N, Q] the initial latent positions (default: PCA_reduce(Y, Q)); kern (default: an
        ARD RBF on the Q latent dimensions); mean_function (default: Zero)."""
        from .. import kernels
        Y = np.ascontiguousarray(Y, dtype=settings.float_type)
        latent_dim = int(latent_dim)
        if latent_dim > self.MAX_LATENT:
            raise NotImplementedError("GPLVM takes at most %d latent dimensions (asked for %d)" % (self.MAX_LATENT, latent_dim))
        if mean_function is None:
            mean_function = Zero()
        if kern is None:
            kern = kernels.RBF(latent_dim, ARD=True)
        if X_mean is None:
            if Y.ndim == 2 and Y.shape[1] < latent_dim:
                raise ValueError('More latent dimensions than observed.')
            X_mean = PCA_reduce(Y, latent_dim)
        X_mean = np.ascontiguousarray(X_mean, dtype=settings.float_type)
        num_latent = X_mean.shape[1]
        if num_latent != latent_dim:
            raise ValueError('Passed in number of latent {0} does not match initial X {1}.'.format(latent_dim, num_latent))
        if Y.shape[1] < num_latent:
            raise ValueError('More latent dimensions than observed.')
        self._X = None
        GPR.__init__(self, X_mean, Y, kern, mean_function=mean_function, obs_var=obs_var, **kwargs)
        self._X = Parameter(X_mean, name='X')
        self._X_seen = None
        self._parameters = self._parameters + [self._X]

    @property
    def X(self):
        """The latent positions [N, Q].  GPR keys what is resident on the device on the IDENTITY of this array: the same
        object comes back for as long as the parameter's bytes are unchanged (an optimiser that writes equal values back
        causes no upload), a new one as soon as they differ."""
        v = np.ascontiguousarray(self._X.value, dtype=settings.float_type)
        if self._X_seen is None or self._X_seen.shape != v.shape or not np.array_equal(self._X_seen, v):
            self._X_seen = v.copy()
            self._X_seen.setflags(write=False)
        return self._X_seen

    @X.setter
    def X(self, value):
        if self._X is not None:
            self._X.assign(np.ascontiguousarray(value, dtype=settings.float_type))
        # (GPModel.__init__ stores the initial X before the Parameter exists: the Parameter made next holds it)

    def compute_log_likelihood_and_gradients(self, with_inputs=False):
        """(lml, [(Parameter, gradient), ...]): the list of GPR and, last, (the X parameter, d LML / d X) -- the device's input
        gradient plus the mean function's chain term (X has the identity transform).  with_inputs: d LML / d X once more as a
        third item, as GPR returns it."""
        if self._has_features():
            raise NotImplementedError("GPLVM needs d LML / d X, which the feature (random-feature) branch does not have")
        lml, grads, gX = GPR.compute_log_likelihood_and_gradients(self, with_inputs=True)
        last = grads[-1]
        assert last[0] is self._X
        grads[-1] = (self._X, gX * np.atleast_1d(self._X.transform.forward_grad(self._X.vf_val)))
        return (lml, grads, gX) if with_inputs else (lml, grads)


class BayesianGPLVM(GPModel):
    def __init__(self, X_mean, X_var, Y, kern, M, Z=None, X_prior_mean=None, X_prior_var=None, obs_var=0.1):
        """gplvm.py:55-112.  X_mean, X_var [N, Q]; Y [N, D]; M inducing points, Z [M, Q] (default: a random subset of X_mean)."""
        X_mean = np.ascontiguousarray(X_mean, dtype=settings.float_type)
        X_var = np.asarray(X_var, dtype=settings.float_type)
        Y = np.ascontiguousarray(Y, dtype=settings.float_type)
        if X_var.ndim == 3:
            raise NotImplementedError("full [N, Q, Q] covariances of q(x) are not implemented: pass the diagonals as [N, Q]")
        if not isinstance(kern, (ekernels.RBF, ekernels.Sum)):
            raise NotImplementedError("BayesianGPLVM is implemented for an ekernels.RBF kernel or an ekernels.Sum of such kernels "
                                      "on separate latent dimensions")
        if isinstance(kern, ekernels.Sum):
            kern._psi_program(X_mean)                                 # (overlapping parts, active_dims outside 0 .. Q-1)
        elif kern._dims(False, X_mean.shape[1]) != list(range(X_mean.shape[1])):
            raise NotImplementedError("the RBF kernel must act on all latent dimensions, in order (no active_dims subset)")
        GPModel.__init__(self, X_mean, Y, kern, likelihood=likelihoods.Gaussian(obs_var), mean_function=Zero())
        del self.X                      # in the GPLVM this is a parameter
        assert X_var.ndim == 2
        self._X_mean = Parameter(X_mean, name='X_mean')
        self._X_var = Parameter(np.ascontiguousarray(X_var), transform=transforms.positive, name='X_var')
        self.num_data = X_mean.shape[0]
        self.output_dim = Y.shape[1]
        assert np.all(X_mean.shape == X_var.shape)
        assert X_mean.shape[0] == Y.shape[0], 'X mean and Y must be same size.'
        assert X_var.shape[0] == Y.shape[0], 'X var and Y must be same size.'
        if Z is None:
            Z = np.random.permutation(X_mean.copy())[:M]
        else:
            Z = np.ascontiguousarray(Z, dtype=settings.float_type)
            assert Z.shape[0] == M
        self._Z = Parameter(Z, name='Z')
        self.num_latent = Z.shape[1]
        assert X_mean.shape[1] == self.num_latent
        if X_prior_mean is None:
            X_prior_mean = np.zeros((self.num_data, self.num_latent))
        if X_prior_var is None:
            X_prior_var = np.ones((self.num_data, self.num_latent))
        self.X_prior_mean = np.asarray(np.atleast_1d(X_prior_mean), dtype=settings.float_type)
        self.X_prior_var = np.asarray(np.atleast_1d(X_prior_var), dtype=settings.float_type)
        assert self.X_prior_mean.shape[0] == self.num_data
        assert self.X_prior_mean.shape[1] == self.num_latent
        assert self.X_prior_var.shape[0] == self.num_data
        assert self.X_prior_var.shape[1] == self.num_latent
        self._parameters = self._parameters + [self._X_mean, self._X_var, self._Z]

    @property
    def X_mean(self):
        return self._X_mean.value

    @property
    def X_var(self):
        return self._X_var.value

    @property
    def Z(self):
        return self._Z.value

    def _noise(self):
        return float(np.squeeze(self.likelihood.variance))

    def _kl(self):
        """KL[q(x) || p(x)] and its gradients with respect to X_mean and X_var  (gplvm.py:150-156)"""
        mu, S = self.X_mean, self.X_var
        diff = mu - self.X_prior_mean
        kl = (-0.5 * np.sum(np.log(S)) + 0.5 * np.sum(np.log(self.X_prior_var)) - 0.5 * mu.size
              + 0.5 * np.sum((np.square(diff) + S) / self.X_prior_var))
        return float(kl), diff / self.X_prior_var, -0.5 / S + 0.5 / self.X_prior_var

    def _build_likelihood(self):
        """gplvm.py:126-167"""
        prog = self.kern._psi_program(self.X_mean)
        F, _, _ = be.get_handle().bgplvm(prog, self.Z, self.X_mean, self.X_var, self.Y, settings.numerics.jitter_level, self._noise())
        return F - self._kl()[0]

    def compute_log_likelihood_and_gradients(self):
        """The bound and d bound / d(unconstrained parameter) for every parameter: (bound, [(Parameter, gradient), ...])."""
        q = self.num_latent
        prog = self.kern._psi_program(self.X_mean)
        layout = self.kern._grad_layout(q)
        F, slots, gnoise, g_Z, g_mu, g_S = be.get_handle().bgplvm_grad(
            prog, self.Z, self.X_mean, self.X_var, self.Y, settings.numerics.jitter_level, self._noise())
        if len(layout) != len(slots):
            raise RuntimeError("gradient slot layout mismatch: %d vs %d" % (len(layout), len(slots)))
        kl, kl_mu, kl_S = self._kl()
        grads = {id(p): np.zeros_like(np.atleast_1d(p.vf_val), dtype=settings.float_type) for p in self.parameters}
        for (param, idx), g in zip(layout, slots):
            if idx is None:
                grads[id(param)] += g
            else:
                grads[id(param)].reshape(-1)[idx] += g
        grads[id(self.likelihood._variance)] += gnoise
        grads[id(self._X_mean)] = g_mu - kl_mu
        grads[id(self._X_var)] = g_S - kl_S
        grads[id(self._Z)] = g_Z
        out = []
        for p in self.parameters:
            g = grads[id(p)].reshape(np.atleast_1d(p.vf_val).shape) * np.atleast_1d(p.transform.forward_grad(p.vf_val))
            out.append((p, g.reshape(np.shape(p.vf_val))))
        return F - kl, out

    def _build_predict(self, Xnew, full_cov=False):
        """gplvm.py:169-204"""
        Xnew = np.ascontiguousarray(Xnew, dtype=settings.float_type)
        prog = self.kern._psi_program(self.X_mean)
        _, mean, var = be.get_handle().bgplvm(prog, self.Z, self.X_mean, self.X_var, self.Y, settings.numerics.jitter_level,
                                              self._noise(), Xnew=Xnew, full_cov=full_cov, want_bound=False)
        R = self.Y.shape[1]
        if full_cov:
            var = np.tile(var[:, :, None], [1, 1, R])
        else:
            var = np.tile(var[:, None], [1, R])
        return mean + self.mean_function(Xnew), var


def PCA_reduce(X, Q):
    """gplvm.py:207-220: the centred data projected on the eigenvectors of np.cov(X.T), by descending eigenvalue; [N, Q]."""
    X = np.asarray(X, dtype=settings.float_type)
    assert Q <= X.shape[1], 'Cannot have more latent dimensions than observed'
    evals, evecs = np.linalg.eigh(np.cov(X.T))
    W = evecs[:, np.argsort(evals)[::-1]][:, :Q]
    return (X - X.mean(0)).dot(W)
