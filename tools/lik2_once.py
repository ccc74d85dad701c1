"""The likelihood launch on its own at N = 10^6, K = 1, 20 nodes, with derivatives, a few times per kind (for rocprofv3
--kernel-trace --stats, in a run of its own: the kernels are lik_elem_kernel<kind, 1>):
    python tools/lik2_once.py [bernoulli beta gamma ordinal ...]
The wall time printed per call is dominated by the copies of the [N, 1] arrays in and out (gps_lik_varexp takes host arrays)."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gpflow-slim_amd"), ROOT]
import gpflowSlim as gpf
from gpflowSlim import _backend as be
kinds = sys.argv[1:] or ["bernoulli", "beta", "gamma", "ordinal"]
h = gpf.get_handle()
N = 1000000
rng = np.random.default_rng(1)
mu = rng.standard_normal((N, 1)) * 1.5
var = np.exp(rng.uniform(np.log(1e-6), np.log(10.0), (N, 1)))
edges = np.linspace(-2.0, 2.0, 5)
for kind in kinds:
    if kind == "bernoulli":
        lik, Y = be.make_lik(1, [], 20), (rng.random((N, 1)) < 0.5).astype(float)
    elif kind == "beta":                                          # alpha = m s from 3e-3 to 3: digamma's shift and lgamma's small arguments
        lik, Y = be.make_lik(7, [3.0], 20), rng.beta(2.0, 3.0, (N, 1))
    elif kind == "gamma":
        lik, Y = be.make_lik(6, [1.7], 20), rng.gamma(2.0, 1.0, (N, 1)) + 1e-3
    else:
        lik, Y = be.make_lik(8, [0.7], 20, edges=edges), rng.integers(0, 6, (N, 1)).astype(float)
    for i in range(4):
        t0 = time.perf_counter(); ve, dmu, dvar, dpar = h.lik_varexp(lik, mu, var, Y, want_grad=True); t1 = time.perf_counter()
        print("%s call %d: %.1f ms sum %.6f dparam %.6f" % (kind, i, 1e3 * (t1 - t0), ve, dpar), flush=True)
