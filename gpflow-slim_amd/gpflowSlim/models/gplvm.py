"""Bayesian GPLVM (Titsias & Lawrence 2010).

Mirrors gpflowSlim/models/gplvm.py:54-220 (BayesianGPLVM, PCA_reduce).  The bound is the SGPR collapsed bound with
sum Kdiag, Kuf and Kuf Kuf^T replaced by the kernel expectations psi0, Psi1, Psi2 under q(x_n) = N(X_mean_n, diag X_var_n);
the expectations, both factorisations, the prediction and the whole gradient run in gps_bgplvm / gps_bgplvm_grad on the GPU.
The KL[q(x) || p(x)] term (gplvm.py:150-156) is elementwise over [N, Q] and is evaluated here with its gradient.

Scope: one ``ekernels.RBF`` over all Q latent dimensions, or an ``ekernels.Sum`` of RBF kernels on pairwise disjoint latent
dimensions (the kernel of the reference's examples/gplvm.py; gradients arrive per part in ``kern.kern_list[i]``), and diagonal
``X_var`` [N, Q]; no minibatching, no sharding over ranks.  The point-estimate ``GPLVM`` is not implemented.
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
