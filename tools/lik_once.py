"""The non-Gaussian SVGP bound at config 5's size, a few times (for rocprofv3 --kernel-trace --stats, in a run of its own):
    python tools/lik_once.py bernoulli | multiclass | gaussian | host
bernoulli: M = 4096, N = 10^6, K = 1;  multiclass: M = 512, N = 10^6, K = 10;  gaussian: the Gaussian bound on the bernoulli
problem (the baseline the likelihood launch is added to);  host: the bernoulli model through the host fallback."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gpflow-slim_amd"), ROOT]
import gpflowSlim as gpf
what = sys.argv[1] if len(sys.argv) > 1 else "bernoulli"
h = gpf.get_handle()
N, d = 1000000, 8
M, K = (512, 10) if what == "multiclass" else (4096, 1)
rng = np.random.default_rng(1)
X = rng.standard_normal((N, d)); Z = X[:M].copy()
F = np.sin(X @ (rng.standard_normal((d, K)) / np.sqrt(d)))
kern = gpf.kernels.RBF(d, variance=1.0, lengthscales=np.sqrt(d) * np.ones(d), ARD=True)
if what == "multiclass":
    Y, like = np.argmax(F + 0.1 * rng.standard_normal((N, K)), 1).astype(float)[:, None], gpf.likelihoods.MultiClass(K)
elif what == "gaussian":
    Y, like = F + 0.1 * rng.standard_normal((N, K)), gpf.likelihoods.Gaussian(0.1)
else:
    Y, like = (F + 0.1 * rng.standard_normal((N, K)) > 0).astype(float), gpf.likelihoods.Bernoulli()
    if what == "host":
        like._device_spec = lambda: None
q_mu = rng.standard_normal((M, K)) * 0.3
q_sqrt = np.stack([np.tril(rng.standard_normal((M, M))) * (0.5 / M) + 0.5 * np.eye(M) for _ in range(K)], 2)
sv = gpf.models.SVGP(X, Y, kern, like, Z=Z, whiten=True, num_latent=K)
sv._q_mu.assign(q_mu); sv._q_sqrt.assign(q_sqrt)
for i in range(2 if what == "host" else 4):
    t0 = time.perf_counter(); v = sv.compute_log_likelihood(); t1 = time.perf_counter()
    print("%s call %d: %.1f ms elbo %.6f" % (what, i, 1e3 * (t1 - t0), v), flush=True)
if "grad" in sys.argv and what != "host":
    for i in range(2):
        t0 = time.perf_counter(); v, g = sv.compute_log_likelihood_and_gradients(); t1 = time.perf_counter()
        print("%s bound + gradient call %d: %.1f ms" % (what, i, 1e3 * (t1 - t0)), flush=True)
