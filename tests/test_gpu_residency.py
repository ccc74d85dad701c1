"""GPU test of the residency table in the docstring of gpflowSlim._backend.Handle: which wrappers leave the resident GPR data
set and factor alone ("keeps") and which drop them.

A GPR model with reuse_factor = True evaluates its likelihood; one Handle wrapper then runs on unrelated tiny inputs (5 inducing
points, 70 rows, 2 latent functions, a 3 x 4 grid for the Kronecker entries); predict_f follows.  Whatever the wrapper did to the
handle's buffers, the prediction must be bit-equal to that of a fresh model that re-factorises (reuse_factor = False): a wrapper
that drops the factor on the device and does not say so on the Python side fails here with "no resident factor" or with
different bits.  For the wrappers marked "keeps", the claim on the factor must also survive the call, so that the prediction
is the warm one.  Two GPR sizes: N = 200 pads to 256 and takes the one-launch small-N path; N = 2200 pads to 2304, above
small_n_max = 2048, and takes the blocked path."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _entry_catalogue as cat  # noqa: E402

pytestmark = pytest.mark.gpu

D = 2
SIZES = [200, 2200]


def _gpf():
    import gpflowSlim as gpf
    return gpf


def inputs():
    """The intruding calls' inputs: the small set of the catalogue (seeded, made once)."""
    return cat.inputs("small")


# name -> (keeps the resident data and factor, the call): every call form of tests/_entry_catalogue.py, and so every wrapper that the
# table in Handle's docstring names (tests/test_entry_catalogue_cpu.py checks that against the docstring)
WRAPPERS = {name: (e.keeps, e.call) for name, e in cat.ENTRIES.items()}


def _model(n, reuse):
    """A new GPR model (its own arrays and kernel) on the seeded data set of n points."""
    gpf = _gpf()
    g = np.random.default_rng(n)
    X = g.standard_normal((n, D))
    Y = np.sin(X[:, :1]) + 0.1 * g.standard_normal((n, 1))
    m = gpf.models.GPR(X, Y, gpf.kernels.RBF(D, variance=1.2, lengthscales=[0.9, 1.4], ARD=True), obs_var=0.1)
    m.reuse_factor = reuse
    return m, g.standard_normal((9, D))


_COLD = {}


def _cold(n):
    """predict_f of a fresh model that re-factorises: computed once per size, never written to."""
    if n not in _COLD:
        m, Xs = _model(n, False)
        m.compute_log_likelihood()
        _COLD[n] = m.predict_f(Xs)
    return _COLD[n]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", sorted(WRAPPERS))
def test_predict_after_an_intruding_call(handle, name, n):
    keeps, call = WRAPPERS[name]
    mu0, var0 = _cold(n)
    m, Xs = _model(n, True)
    m.compute_log_likelihood()
    key = handle.factor_key
    assert key is not None and key == m._state_key()
    call(handle, inputs())
    if keeps:
        assert handle.factor_key is key, "%s is listed as keeping the resident factor but dropped the claim on it" % name
    mu, var = m.predict_f(Xs)
    assert np.array_equal(mu, mu0) and np.array_equal(var, var0), \
        "%s: max |d mean| %.3g, max |d var| %.3g" % (name, np.abs(mu - mu0).max(), np.abs(var - var0).max())
