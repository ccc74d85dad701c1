"""Models shared by tests/test_gpu_dist_grad*.py and their worker processes (no tests here)."""
import numpy as np

import gpflowSlim as gpf

XS = np.random.default_rng(3).standard_normal((20, 3))


def flat(grads):
    return np.concatenate([np.atleast_1d(g).ravel() for _, g in grads])


def linear_mean_model():
    """N = 1500, r = 2, RBF-ARD with a Linear mean function (its gradient needs K_y^-1 resid)"""
    rng = np.random.default_rng(13)
    X = rng.standard_normal((1500, 3))
    Y = np.sin(X @ rng.standard_normal((3, 2))) + 0.1 * rng.standard_normal((1500, 2))
    mf = gpf.mean_functions.Linear(rng.standard_normal((3, 2)) * 0.1, np.array([0.05, -0.02]))
    return gpf.models.GPR(X, Y, gpf.kernels.RBF(3, variance=1.1, lengthscales=np.array([0.9, 1.4, 2.0]), ARD=True),
                          mean_function=mf, obs_var=0.1)


def npd_model():
    """Points far apart against the length-scale (K close to the identity) except a duplicate in the last panel, and a noise
    variance of -5e-10 (the transform's floor set below it): the last pivot is negative.  Assigning a noise variance of 0.1
    afterwards makes it an ordinary, well-conditioned model."""
    rng = np.random.default_rng(0)
    X = rng.standard_normal((1024, 6))
    X[-1] = X[-2]
    Y = rng.standard_normal((1024, 1))
    return gpf.models.GPR(X, Y, gpf.kernels.RBF(6, variance=1.0, lengthscales=0.3), obs_var=-5e-10, min_var=-1e-9)
