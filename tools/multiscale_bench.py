"""Kuf build, SVGP Gaussian bound and bound + gradient with features.Multiscale beside plain inducing points in the same process
(the comparison point: the InducingPoints number of the same run), at M = 4096, D = 8 and N = 10^6 by default.  The build is
timed through the library's own per-class kernel timers (profile class "kmat": Kuu, the prep passes and the Kuf tile pass,
device time), the bound and bound + gradient as wall time of the backend calls, which end in a device synchronisation.  One
warm-up evaluation per shape, then `reps` repetitions: median, minimum and maximum are reported.  Prints one JSON line.

    python tools/multiscale_bench.py [N] [reps] [M]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gpflow-slim_amd"), ROOT]
import gpflowSlim as gpf  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10 ** 6
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
m = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
d = 8
rng = np.random.default_rng(0)
X = rng.standard_normal((n, d))
Y = np.sin(X[:, :1]) + 0.1 * rng.standard_normal((n, 1))
Z = X[rng.choice(n, m, replace=False)].copy()
S = rng.uniform(0.05, 0.8, (m, d))
q_mu = 0.1 * rng.standard_normal((m, 1))
q_sqrt = np.full((m, 1), 0.5)
kern = gpf.kernels.RBF(d, variance=1.0, lengthscales=np.sqrt(d) * np.ones(d), ARD=True)
prog = kern._program(d)
h = gpf.get_handle()
pad = lambda v: 128 * -(-v // 128)  # noqa: E731
kuf_bytes = 8.0 * pad(n) * pad(m)


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


out = {"n": n, "m": m, "d": d, "reps": reps, "kuf_gbytes": kuf_bytes / 1e9, "device": str(h.device_info())}
for name, scales in (("inducing_points", None), ("multiscale", S)):
    args = (prog, Z, X, Y, q_mu, q_sqrt, 1e-6, 0.1)
    h.svgp_elbo(*args, white=True, scales=scales)                      # warm-up: buffers, code objects
    h.svgp_elbo_grad(*args, white=True, want_grad_Z=True, scales=scales)
    build, bound, grad = [], [], []
    for _ in range(reps):
        # (profiling synchronises around every launch: the build's device time from one evaluation, the wall times from others)
        h.profile_reset(); h.profile_enable(True)
        h.svgp_elbo(*args, white=True, scales=scales)
        h.profile_enable(False)
        build.append(h.profile_get("kmat")["ms"])
        t0 = time.perf_counter(); v = h.svgp_elbo(*args, white=True, scales=scales)[0]; t1 = time.perf_counter()
        bound.append(1e3 * (t1 - t0))
        t0 = time.perf_counter(); h.svgp_elbo_grad(*args, white=True, want_grad_Z=True, scales=scales); t1 = time.perf_counter()
        grad.append(1e3 * (t1 - t0))
    out[name] = {"kmat_build_ms": stats(build), "kuf_store_gb_per_s": kuf_bytes / 1e6 / float(np.median(build)),
                 "bound_ms": stats(bound), "bound_grad_ms": stats(grad), "elbo": v}
    print(name, out[name], flush=True)
for key in ("kmat_build_ms", "bound_ms", "bound_grad_ms"):
    out["ratio_" + key] = out["multiscale"][key]["median"] / out["inducing_points"][key]["median"]
print(json.dumps(out))
