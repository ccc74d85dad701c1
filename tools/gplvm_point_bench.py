"""LML + gradient with and without d LML / d X (Handle.gpr_lml_grad(want_grad_X=...)) in one process, at the sizes of the
point-estimate GPLVM and above:

    N = 512 and N = 2048, Q = 5 latent dimensions, R = 12 outputs, RBF-ARD   (the one-launch small path)
    N = 8192 and N = 32768, D = 8, R = 1, RBF-ARD                            (launch by launch)

Wall time of the two calls (minimum and median over the repetitions), their ratio, and -- from one profiled call each, through the
library's per-launch list (GPS_PROF_DUMP) -- the device time of the two launches the input gradient adds (the walk over the
mirrored square, grad_x_kernel, and the reduction of its slices) with the walk's achieved bytes/s against the 8 N_pad^2 bytes it
reads.  Prints one JSON line.

    python tools/gplvm_point_bench.py [reps] [largest N]
"""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gpflow-slim_amd"), ROOT]
DUMP = os.path.join(tempfile.mkdtemp(prefix="gplvm_point_bench_"), "launches.txt")
os.environ["GPS_PROF_DUMP"] = DUMP                 # (read once, when the library first collects a profile)
import gpflowSlim as gpf  # noqa: E402
import oracle.gp_oracle as orc  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
n_max = int(sys.argv[2]) if len(sys.argv) > 2 else 32768
CASES = [(512, 5, 12), (2048, 5, 12), (8192, 8, 1), (32768, 8, 1)]
h = gpf.get_handle()
out = {"reps": reps, "device": str(h.device_info()), "cases": []}


def timed(call, count):
    ts = []
    for _ in range(count):
        t0 = time.perf_counter()
        call()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.min(ts)), float(np.median(ts))


def profiled(call):
    """device microseconds of every launch of class "reduce" of one call, in launch order"""
    open(DUMP, "w").close()
    h.profile_reset(); h.profile_enable(True)
    call()
    h.profile_enable(False)
    h.profile_get("reduce")                        # (collects: writes the per-launch list)
    us = []
    for line in open(DUMP):
        w = line.split()
        if w and w[0] == "reduce":
            us.append(float(w[-1]))
    return us


for n, d, r in CASES:
    if n > n_max:
        continue
    X, Y, _ = orc.synthetic_gpr_data(n, d, 0)
    if r > 1:
        rng = np.random.default_rng(1)
        Y = np.sin(X @ rng.standard_normal((d, r))) + 0.1 * rng.standard_normal((n, r))
    kern = gpf.kernels.RBF(d, variance=1.0, lengthscales=np.sqrt(d) * np.linspace(0.8, 1.2, d), ARD=True)
    prog = kern._program(d)
    h.gpr_set_data(X, X)
    plain = lambda: h.gpr_lml_grad(prog, 0.1, Y)
    withx = lambda: h.gpr_lml_grad(prog, 0.1, Y, want_grad_X=True)
    count = reps if n <= 2048 else max(2, reps // 8)
    plain(); withx()                               # warm-up: buffers, code objects
    p_min, p_med = timed(plain, count)
    x_min, x_med = timed(withx, count)
    p_min2, p_med2 = timed(plain, count)           # (once more after: drift of the process shows as a difference between the two)
    us = profiled(withx)
    walk_us, reduce_us = us[-2], us[-1]
    npad = 128 * -(-n // 128)
    case = {"n": n, "d": d, "r": r, "count": count, "slicing": list(gpf._backend.grad_x_slicing(n)),
            "lml_grad_ms": {"min": p_min, "median": p_med, "min_after": p_min2, "median_after": p_med2},
            "lml_grad_x_ms": {"min": x_min, "median": x_med},
            "ratio_min": x_min / min(p_min, p_min2), "ratio_median": x_med / (0.5 * (p_med + p_med2)),
            "walk_us": walk_us, "reduce_us": reduce_us, "walk_bytes": 8.0 * npad * npad,
            "walk_GBps": 8.0 * npad * npad / (walk_us * 1e-6) / 1e9}
    out["cases"].append(case)
    print(case, flush=True)
print(json.dumps(out))
