"""Exact Gaussian-process regression on one MI355X.

Mirrors gpflowSlim/models/gpr.py:28-132 (exact branch :69-72, :119-131).  X is uploaded once
and stays in HBM; every ``likelihood_tensor`` / ``objective`` read rebuilds K, re-factors and
re-solves on the device, as the reference's ``sess.run(objective)`` does; ``predict_f``
re-factors too (models/gpr.py:119-121) unless ``reuse_factor`` is switched on.
"""
import numpy as np

from .. import likelihoods
from .. import _backend as be
from .._settings import settings
from .model import GPModel


class _FactorKey(object):
    """What the resident factor was computed from: the hyper-parameter bytes and the X / Y array OBJECTS (held, so
    that their addresses cannot be recycled while the key is alive)."""

    def __init__(self, params, X, Y):
        self.params, self.X, self.Y = params, X, Y

    def __eq__(self, other):
        return isinstance(other, _FactorKey) and self.params == other.params and self.X is other.X and self.Y is other.Y

    def __ne__(self, other):
        return not self.__eq__(other)


class GPR(GPModel):
    def __init__(self, X, Y, kern, mean_function=None, obs_var=0.1, num_latent=None, min_var=None, **kwargs):
        """X [N, D], Y [N, R]; kern, mean_function as in the reference (models/gpr.py:41-53)."""
        X = np.ascontiguousarray(X, dtype=settings.float_type)
        Y = np.ascontiguousarray(Y, dtype=settings.float_type)
        if X.ndim != 2 or Y.ndim != 2 or X.shape[0] != Y.shape[0]:
            raise ValueError("GPR needs X [N, D] and Y [N, R]")
        likelihood = likelihoods.Gaussian(var=obs_var, min_var=min_var)
        GPModel.__init__(self, X, Y, kern, likelihood, mean_function, **kwargs)
        self.num_latent = Y.shape[1] if num_latent is None else num_latent
        # not in the reference: opt-in reuse of the resident factor by predict_f
        self.reuse_factor = False
        # feature branch: rows of X per device chunk (0: the library chooses, about 1 GiB per chunk buffer)
        self.rff_chunk_rows = 0

    # ---- device plumbing -------------------------------------------------------------------
    @property
    def _factor_key(self):
        """What the factor resident on the device was computed from (kept on the HANDLE: several models may share
        one handle, and even one X array; the factor belongs to whoever evaluated last)."""
        return be.get_handle().factor_key

    @_factor_key.setter
    def _factor_key(self, key):
        be.get_handle().factor_key = key

    def _handle(self):
        h = be.get_handle()
        # The handle keeps a reference to the array it uploaded, so "is" cannot be fooled by a new array that the
        # allocator placed at a freed model's address (ids and data pointers are reused; object identity of a live
        # object is not).  X is treated as immutable, like the reference's tensor; assign a new array to change it.
        if h.resident_token is not self.X:
            h.gpr_set_data(self.X, self.X)
            self._factor_key = None
        return h

    def _state_key(self):
        parts = [p.vf_val.tobytes() for p in self.parameters]
        return _FactorKey(b"|".join(parts), self.X, self.Y)

    def _resid(self):
        return np.ascontiguousarray(self.Y - self.mean_function(self.X))

    # ---- feature branch (models/gpr.py:63-67, 86-117): kernels with a callable ``features`` ---------------------------
    def _has_features(self):
        return callable(getattr(self.kern, 'features', None))

    def _rff(self, Xnew=None):
        """(descriptor, arrays it points into, X, Xnew) for the device entries: the sampler's own descriptor where the
        kernel has one (the feature map then runs on the device), else the kernel's features as explicit host matrices."""
        sampler = getattr(self.kern, 'sampler', None)
        if callable(getattr(sampler, '_descriptor', None)):
            desc, keep = sampler._descriptor()
            return desc, keep, self.X, Xnew
        feat = np.ascontiguousarray(self.kern.features(self.X), dtype=settings.float_type)
        desc, keep = be.make_rff(be.RFF_EXPLICIT, feat.shape[1], feat.shape[1])
        fnew = None if Xnew is None else np.ascontiguousarray(self.kern.features(Xnew), dtype=settings.float_type)
        return desc, keep, feat, fnew

    def _rff_likelihood(self):
        h = be.get_handle()
        desc, keep, X, _ = self._rff()
        with h.factor_claim(self._state_key()):
            lml = h.rff_lml(desc, X, float(np.squeeze(self.likelihood.variance)), self._resid(), self.rff_chunk_rows)
        return lml

    def _rff_likelihood_and_gradients(self):
        h = be.get_handle()
        desc, keep, X, _ = self._rff()
        if desc.kind == be.RFF_EXPLICIT:
            raise NotImplementedError("gradients of the feature branch need a kernel_kitchen_sink sampler")
        sampler = self.kern.sampler
        with h.factor_claim(self._state_key()):
            lml, gvar, gls, gnoise, kinv_resid = h.rff_lml_grad(desc, X, float(np.squeeze(self.likelihood.variance)),
                                                                self._resid(), self.rff_chunk_rows)
        layout, slots = [(sampler._variance, None)], [gvar]
        if desc.kind == be.RFF_RBF:
            layout += [(sampler._ls, None)] if gls.size == 1 else [(sampler._ls, i) for i in range(gls.size)]
            slots += list(gls)
        return lml, self._gradients_from_slots(layout, slots, gnoise, kinv_resid)

    def _rff_predict(self, Xnew, full_cov):
        h = be.get_handle()
        desc, keep, X, Xn = self._rff(Xnew)
        key = self._state_key()
        warm = bool(self.reuse_factor) and self._factor_key is not None and self._factor_key == key
        with h.factor_claim(key):
            mean, var = h.rff_predict(desc, X, float(np.squeeze(self.likelihood.variance)), self._resid(), Xn,
                                      full_cov=full_cov, refactor=not warm, chunk_rows=self.rff_chunk_rows)
        return mean, var

    # ---- reference API ---------------------------------------------------------------------
    def _build_likelihood(self):
        """models/gpr.py:63-72 + densities.py:73-124, fused on the device."""
        if self._has_features():
            return self._rff_likelihood()
        self.kern._check_inputs(self.X)
        h = self._handle()
        prog = self.kern._program(self.X.shape[1])
        with h.factor_claim(self._state_key()):
            lml = h.gpr_lml(prog, float(np.squeeze(self.likelihood.variance)), self._resid())
        return lml

    def compute_log_likelihood_and_gradients(self, with_inputs=False):
        """LML and d LML / d(unconstrained parameter) for every parameter of the model -- what
        `tf.gradients(objective, variables)` yields in the reference (examples/gpr.py:53-54) up to the
        sign of `objective = -LML`.  Returns (lml, [(Parameter, gradient array shaped like
        Parameter.unconstrained_tensor), ...]) in `self.parameters` order.  Priors are not included.

        with_inputs: (lml, grads, dLML_dX) with d LML / d X [N, D], the derivative of the evidence with respect to the input
        locations: the kernel's part from the device (gps_gpr_lml_grad_x) plus the mean function's chain term."""
        if self._has_features():
            if with_inputs:
                raise NotImplementedError("d LML / d X is not available on the feature (random-feature) branch")
            return self._rff_likelihood_and_gradients()
        if with_inputs:
            self._input_chain(None)               # (refuse a mean function without a known chain before any device work)
        self.kern._check_inputs(self.X)
        h = self._handle()
        d_all = self.X.shape[1]
        prog = self.kern._program(d_all)
        layout = self.kern._grad_layout(d_all)
        resid = self._resid()
        noise = float(np.squeeze(self.likelihood.variance))
        with h.factor_claim(self._state_key()):
            if with_inputs:
                lml, slots, gnoise, kinv_resid, grad_X = h.gpr_lml_grad(prog, noise, resid, want_grad_X=True)
            else:
                lml, slots, gnoise, kinv_resid = h.gpr_lml_grad(prog, noise, resid)
        grads = self._gradients_from_slots(layout, slots, gnoise, kinv_resid)
        if with_inputs:
            return lml, grads, grad_X + self._input_chain(kinv_resid)
        return lml, grads

    def _input_chain(self, kinv_resid):
        """What the mean function adds to d LML / d X: d LML / d m(X) = K_y^-1 (Y - m) chained through d m / d X -- A^T rows for
        Linear (m = X A + b), nothing for Zero and Constant.  kinv_resid None: only the check that the chain is known."""
        from ..mean_functions import Zero as _MZero, Constant as _MConst, Linear as _MLin
        mf = self.mean_function
        if isinstance(mf, _MLin):
            if kinv_resid is None:
                return 0.0
            A = np.atleast_2d(mf.A.value)                       # [D, R], or [D, 1] broadcast over the outputs
            g = kinv_resid if A.shape[1] == kinv_resid.shape[1] else np.sum(kinv_resid, axis=1, keepdims=True)
            return g @ A.T
        if isinstance(mf, (_MZero, _MConst)):
            return 0.0
        raise NotImplementedError("d LML / d X through a %s mean function is not implemented" % type(mf).__name__)

    def _gradients_from_slots(self, layout, slots, gnoise, kinv_resid):
        """Map the kernel's gradient slots, d LML / d(noise variance) and K_y^-1 (Y - m) onto
        [(Parameter, d LML / d(unconstrained parameter)), ...] in `self.parameters` order: the slot layout of
        the kernel program, the mean-function chain rule through K_y^-1 (Y - m) and the transforms.  Shared
        by compute_log_likelihood_and_gradients and gpflowSlim.distributed.gpr_lml_grad_distributed."""
        if len(layout) != len(slots):
            raise RuntimeError("gradient slot layout mismatch: %d vs %d" % (len(layout), len(slots)))
        grads = {id(p): np.zeros_like(np.atleast_1d(p.vf_val), dtype=settings.float_type) for p in self.parameters}
        for (param, idx), g in zip(layout, slots):
            if param is None:
                continue
            if idx is None:
                grads[id(param)] += g
            else:
                grads[id(param)].reshape(-1)[idx] += g          # index into the flattened parameter
        grads[id(self.likelihood._variance)] += gnoise
        # mean function: d LML / d m(X) = K_y^-1 (Y - m) ; Zero has no parameters
        from ..mean_functions import Constant as _MConst, Linear as _MLin
        mf = self.mean_function

        def _fit(g, like):           # sum a per-output gradient into a parameter that broadcasts over outputs
            like = np.atleast_1d(like)
            return g.reshape(like.shape) if g.size == like.size else np.full(like.shape, np.sum(g))

        if isinstance(mf, _MConst):
            grads[id(mf.c)] = grads[id(mf.c)] + _fit(np.sum(kinv_resid, axis=0), mf.c.vf_val)
        elif isinstance(mf, _MLin):
            grads[id(mf.A)] = grads[id(mf.A)] + _fit(self.X.T @ kinv_resid, mf.A.vf_val)
            grads[id(mf.b)] = grads[id(mf.b)] + _fit(np.sum(kinv_resid, axis=0), mf.b.vf_val)
        out = []
        for p in self.parameters:
            g = grads[id(p)].reshape(np.atleast_1d(p.vf_val).shape) * np.atleast_1d(p.transform.forward_grad(p.vf_val))
            out.append((p, g.reshape(p.vf_val.shape)))
        return out

    def _build_predict(self, Xnew, full_cov=False):
        """models/gpr.py:86-131"""
        Xnew = np.ascontiguousarray(Xnew, dtype=settings.float_type)
        if self._has_features():
            mean, var = self._rff_predict(Xnew, full_cov)
        else:
            self.kern._check_inputs(self.X, Xnew)
            h = self._handle()
            prog = self.kern._program(self.X.shape[1])
            key = self._state_key()
            warm = bool(self.reuse_factor) and self._factor_key is not None and self._factor_key == key
            with h.factor_claim(key):
                mean, var = h.gpr_predict(prog, float(np.squeeze(self.likelihood.variance)), self._resid(), Xnew,
                                          full_cov=full_cov, refactor=not warm)
        fmean = mean + self.mean_function(Xnew)
        R = self.Y.shape[1]
        if full_cov:
            fvar = np.tile(var[:, :, None], [1, 1, R])             # models/gpr.py:127-128
        else:
            fvar = np.tile(np.reshape(var, (-1, 1)), [1, R])       # models/gpr.py:131
        return fmean, fvar
