"""Kernel-matrix build and LML + gradient of RBF(ARD, D = 8) * Coregion(P = 4, R = 2) at N = 32768, with plain RBF(ARD, D = 8)
beside it in the same process (the comparison point: the plain-RBF number of the same run).  The build is timed through the
library's own per-class kernel timers (profile class "kmat": prep + tile pass, device time), the LML + gradient as wall time
of compute_log_likelihood_and_gradients.  Prints one JSON line.

    python tools/coregion_bench.py [N] [reps]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gpflow-slim_amd"), ROOT]
import gpflowSlim as gpf  # noqa: E402
import oracle.gp_oracle as orc  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
d, P, R = 8, 4, 2
X0, Y, _ = orc.synthetic_gpr_data(n, d, 0)
rng = np.random.default_rng(0)
X = np.concatenate([X0, rng.integers(0, P, n).astype(float)[:, None]], 1)
k = gpf.kernels


def rbf():
    return k.RBF(d, variance=1.0, lengthscales=np.sqrt(d) * np.ones(d), ARD=True, active_dims=list(range(d)))


def icm():
    c = k.Coregion(1, P, R, active_dims=[d])
    c._W.assign(0.5 * rng.standard_normal((P, R)))
    return rbf() * c


h = gpf.get_handle()
out = {"n": n, "d": d, "P": P, "R": R, "reps": reps, "device": str(h.device_info())}
for name, make in (("rbf", rbf), ("rbf_x_coregion", icm)):
    kern = make()
    m = gpf.models.GPR(X, Y, kern, obs_var=0.1)
    m.compute_log_likelihood()                                   # warm-up: buffers, code objects
    build, lml_ms, grad_ms = [], [], []
    for _ in range(reps):
        # (profiling synchronises around every launch: the build's device time from one evaluation, the wall time from another)
        h.profile_reset(); h.profile_enable(True)
        m.compute_log_likelihood()
        h.profile_enable(False)
        build.append(h.profile_get("kmat")["ms"])
        t0 = time.perf_counter(); v = m.compute_log_likelihood(); t1 = time.perf_counter()
        lml_ms.append(1e3 * (t1 - t0))
        t0 = time.perf_counter(); v2, g = m.compute_log_likelihood_and_gradients(); t1 = time.perf_counter()
        grad_ms.append(1e3 * (t1 - t0))
    out[name] = {"kmat_build_ms": build, "lml_ms": lml_ms, "lml_grad_ms": grad_ms, "lml": v}
    print(name, out[name], flush=True)
for key in ("kmat_build_ms", "lml_ms", "lml_grad_ms"):
    out["ratio_" + key] = min(out["rbf_x_coregion"][key]) / min(out["rbf"][key])
print(json.dumps(out))
