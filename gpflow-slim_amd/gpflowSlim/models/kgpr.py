"""Kronecker GP regression on one MI355X (mirrors gpflowSlim/models/kgpr.py:28-117).

Observations Y [m, n] on the grid X1 x X2 with covariance K1 (x) K2; missing cells are marked by ``mask`` and get 1e6 added to
their noise.  (K + D)^-1 y comes from conjugate gradients whose matrix-vector product is two small GEMMs, K1 P K2, so no
N x N matrix (N = m n) is ever formed; the log-determinant is the reference's spectral one: the M = N - sum(mask) largest
products of the eigenvalues of K1 and K2, scaled by M / N.  The solver loop, the spectrum sums and the gradient products run on
the device (gps_kgpr_lml / _lml_grad / _predict); the two eigendecompositions run on the host (numpy).
"""
import numpy as np

from .. import likelihoods
from .. import _backend as be
from ..mean_functions import Zero
from .._settings import settings
from .model import Model


def _float_key(x):
    """A Python int that orders like the double x (-0.0 and 0.0 share a key)."""
    b = int(np.array(x, dtype=np.float64).view(np.int64))
    return b if b >= 0 else -(b & 0x7fffffffffffffff)


def _key_float(k):
    b = k if k >= 0 else ((-k) | (1 << 63))
    return float(np.array(b, dtype=np.uint64).view(np.float64))


def _row_counts(e1, e2, t, strict):
    """Per row i, how many of the products e1_i * e2_j are >= t (strict: > t).  e2 is sorted descending, so with e1_i >= 0 the
    products fall along j and with e1_i < 0 they rise: either way they are counted by one bisection per row, all rows at once,
    on the products as the device forms them (a floating-point product with a fixed factor is monotone in the other)."""
    m, n = e1.size, e2.size
    neg = e1 < 0
    lo = np.zeros(m, dtype=np.int64)
    hi = np.full(m, n, dtype=np.int64)
    while True:
        act = lo < hi
        if not act.any():
            return lo
        mid = (lo + hi) // 2
        idx = np.minimum(np.where(neg, n - 1 - mid, mid), n - 1)
        p = e1 * e2[np.maximum(idx, 0)]
        ok = (p > t) if strict else (p >= t)
        lo = np.where(act & ok, mid + 1, lo)
        hi = np.where(act & ~ok, mid, hi)


def _select(e1, e2, M):
    """The M largest of the products e1_i * e2_j (kgpr.py:72, tf.nn.top_k) as one range of the sorted e2 per row of the sorted e1.

    Returns (e1 sorted descending, e2 sorted descending, ranges int32 [m, 2]): row i takes e2[lo_i:hi_i] -- a prefix where
    e1_i >= 0, a suffix where e1_i < 0.  The M-th largest product is found by counting over the two sorted spectra
    (O(m log n) per step, at most 64 steps over the doubles between the smallest and the largest product); the N products are
    never formed or sorted.  Ties at the threshold go to the lower row index first."""
    e1 = np.sort(np.asarray(e1, dtype=np.float64).ravel())[::-1].copy()
    e2 = np.sort(np.asarray(e2, dtype=np.float64).ravel())[::-1].copy()
    m, n = e1.size, e2.size
    N, M = m * n, int(M)
    if not 0 <= M <= N:
        raise ValueError("cannot select %d of %d products" % (M, N))
    rng = np.zeros((m, 2), dtype=np.int32)
    if M == 0 or N == 0:
        return e1, e2, rng
    if M == N:
        count = np.full(m, n, dtype=np.int64)
    else:
        corners = [e1[0] * e2[0], e1[0] * e2[-1], e1[-1] * e2[0], e1[-1] * e2[-1]]
        klo, khi = _float_key(min(corners)), _float_key(max(corners))       # count(>= lo) = N >= M
        while klo < khi:                                                    # the largest t with count(>= t) >= M
            kmid = (klo + khi + 1) // 2
            if int(_row_counts(e1, e2, _key_float(kmid), False).sum()) >= M:
                klo = kmid
            else:
                khi = kmid - 1
        t = _key_float(klo)
        above = _row_counts(e1, e2, t, True)
        ties = _row_counts(e1, e2, t, False) - above
        need = M - int(above.sum())
        before = np.cumsum(ties) - ties
        count = above + np.clip(need - before, 0, ties)
    neg = e1 < 0
    rng[:, 0] = np.where(neg, n - count, 0)
    rng[:, 1] = np.where(neg, n, count)
    return e1, e2, rng


class KGPR(Model):
    def __init__(self, X1, X2, Y, kern1, kern2, mask, mean_function=None, obs_var=0.1, cg_max_iter=100, cg_tol=1e-6, **kwargs):
        """X1 [m, d1], X2 [n, d2], Y [m, n], mask [m, n] (1 = missing); kern1, kern2 as in the reference (kgpr.py:29-55).
        cg_max_iter / cg_tol: the arguments of cgsolver, at the reference's defaults."""
        Model.__init__(self, **kwargs)
        if mean_function is not None and not isinstance(mean_function, Zero):
            # the reference accepts a mean function and never uses it (kgpr.py:76: y = vec(Y))
            raise NotImplementedError("KGPR takes no mean function other than Zero: the reference model ignores it")
        self.X1 = np.ascontiguousarray(X1, dtype=settings.float_type)
        self.X2 = np.ascontiguousarray(X2, dtype=settings.float_type)
        self.Y = np.ascontiguousarray(Y, dtype=settings.float_type)
        self.mask = np.ascontiguousarray(mask, dtype=settings.float_type)
        if self.X1.ndim != 2 or self.X2.ndim != 2 or self.Y.shape != (self.X1.shape[0], self.X2.shape[0]) \
                or self.mask.shape != self.Y.shape:
            raise ValueError("KGPR needs X1 [m, d1], X2 [n, d2] and Y, mask [m, n]")
        self.likelihood = likelihoods.Gaussian(var=obs_var)
        self.kern1, self.kern2 = kern1, kern2
        self.mean_function = mean_function or Zero()
        self.N = int(np.prod(self.Y.shape))
        self.M = int(round(self.N - np.sum(self.mask)))
        self.cg_max_iter, self.cg_tol = int(cg_max_iter), float(cg_tol)
        self.last_solve = None       # dict(lml, quadratic, logdet, iters, rr, delta) of the last evaluation
        self._parameters = self.mean_function.parameters + self.kern1.parameters + self.kern2.parameters \
            + self.likelihood.parameters

    # ---- device plumbing -------------------------------------------------------------------
    def _programs(self):
        return self.kern1._program(self.X1.shape[1]), self.kern2._program(self.X2.shape[1])

    def _state_key(self):
        return ("kgpr", id(self), b"|".join(p.vf_val.tobytes() for p in self.parameters), self.cg_max_iter, self.cg_tol)

    def _spectra(self, prog1, prog2, vectors):
        """Eigenvalues (and eigenvectors) of K1 and K2 on the host, sorted descending, with the selected ranges."""
        h = be.get_handle()
        K1, K2 = h.kmat(prog1, self.X1), h.kmat(prog2, self.X2)
        if not vectors:
            e1, e2, sel = _select(np.linalg.eigvalsh(K1), np.linalg.eigvalsh(K2), self.M)
            return e1, e2, sel, None, None
        (w1, V1), (w2, V2) = np.linalg.eigh(K1), np.linalg.eigh(K2)
        o1, o2 = np.argsort(-w1, kind='stable'), np.argsort(-w2, kind='stable')
        e1, e2, sel = _select(w1[o1], w2[o2], self.M)
        return e1, e2, sel, np.ascontiguousarray(V1[:, o1]), np.ascontiguousarray(V2[:, o2])

    # ---- reference API ---------------------------------------------------------------------
    def _build_likelihood(self):
        """kgpr.py:57-83"""
        h = be.get_handle()
        prog1, prog2 = self._programs()
        e1, e2, sel, _, _ = self._spectra(prog1, prog2, False)
        with h.factor_claim(self._state_key()):
            res = h.kgpr_lml(prog1, self.X1, prog2, self.X2, self.Y, self.mask, float(np.squeeze(self.likelihood.variance)),
                             e1, e2, sel, max_iter=self.cg_max_iter, tol=self.cg_tol)
        self.last_solve = res
        return res["lml"]

    def compute_log_likelihood_and_gradients(self):
        """LML and d LML / d(unconstrained parameter) for every parameter, analytic at the CG solution (exact once CG has
        converged).  Returns (lml, [(Parameter, gradient), ...]) in `self.parameters` order."""
        h = be.get_handle()
        prog1, prog2 = self._programs()
        layout = self.kern1._grad_layout(self.X1.shape[1]) + self.kern2._grad_layout(self.X2.shape[1])
        e1, e2, sel, V1, V2 = self._spectra(prog1, prog2, True)
        with h.factor_claim(self._state_key()):
            res, s1, s2, gnoise = h.kgpr_lml_grad(prog1, self.X1, prog2, self.X2, self.Y, self.mask,
                                                  float(np.squeeze(self.likelihood.variance)), e1, e2, sel, V1, V2,
                                                  max_iter=self.cg_max_iter, tol=self.cg_tol)
        self.last_solve = res
        slots = list(s1) + list(s2)
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
        grads[id(self.likelihood._variance)] += gnoise
        out = []
        for p in self.parameters:
            g = grads[id(p)].reshape(np.atleast_1d(p.vf_val).shape) * np.atleast_1d(p.transform.forward_grad(p.vf_val))
            out.append((p, g.reshape(p.vf_val.shape)))
        return res["lml"], out

    def _build_predict(self, Xnew1, Xnew2):
        """kgpr.py:86-110: K1u^T alpha K2u [m*, n*], the mean only.  The reference solves again for every prediction; here
        the alpha of the last likelihood evaluation is reused while the parameters have not changed."""
        Xnew1 = np.ascontiguousarray(Xnew1, dtype=settings.float_type)
        Xnew2 = np.ascontiguousarray(Xnew2, dtype=settings.float_type)
        h = be.get_handle()
        if h.factor_key != self._state_key():
            self._build_likelihood()
        prog1, prog2 = self._programs()
        return h.kgpr_predict(prog1, self.X1, Xnew1, prog2, self.X2, Xnew2)

    def predict_f(self, Xnew1, Xnew2):
        """kgpr.py:112-117"""
        return self._build_predict(Xnew1, Xnew2)
