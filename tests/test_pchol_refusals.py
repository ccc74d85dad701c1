"""The refusals of the preconditioned matrix-free path happen on the host, before any device work: no GPU needed."""
import numpy as np
import pytest


@pytest.mark.parametrize("rank,noise,kernel,exc,match", [
    (129, 0.5, "RBF", ValueError, "0 .. 128"),
    (-1, 0.5, "RBF", ValueError, "0 .. 128"),
    (16, 0.0, "RBF", ValueError, "noise variance > 0"),
    (16, 0.5, "Periodic", NotImplementedError, "one stationary kernel"),
])
def test_refusals(rank, noise, kernel, exc, match):
    import gpflowSlim as gpf
    cg = gpf.conjugate_gradient
    X, B = np.zeros((5, 2)), np.ones((5, 1))
    kern = getattr(gpf.kernels, kernel)(2)
    m = gpf.models.GPR(X, B, kern, obs_var=0.5)
    calls = [lambda: cg.kernel_cgsolver(kern, X, B, noise, precond_rank=rank),
             lambda: cg.kernel_logdet(kern, X, noise, precond_rank=rank),
             lambda: cg.kernel_precond_solve(kern, X, B, noise, rank)]
    if noise > 0:
        calls += [lambda: cg.kernel_pivoted_cholesky(kern, X, rank),
                  lambda: m.predict_f_iterative(X, precond_rank=rank),
                  lambda: m.compute_log_likelihood_and_gradients_iterative(precond_rank=rank)]
    for call in calls:
        with pytest.raises(exc, match=match):
            call()
