"""Times of Kronecker GP regression (csrc/kron.hip, csrc/gps_kgpr.hip) on m x n grids of 512^2, 2048^2 and 4096 x 1024 with
tol = 0 and max_iter = 100 (every iteration runs), after a warm-up, each timed call ending in a stream synchronise:

  ms per CG iteration          host clock: (a 100-iteration solve - a 0-iteration solve) / 100, uploads cancel
  its GEMM and vector shares   per-class launch brackets of a profiled run ("gemm_f64" / "other"), same difference
  the two GEMMs alone          gps_diag_gemm_timeline on device-resident operands of the two shapes
  the spectrum launches        per-launch list of the profiled run (GPS_PROF_DUMP), rows pass and columns pass
  host eigvalsh / eigh         numpy on K1 and K2
  one LML, one LML + gradient  host clock around the model's calls, eigendecompositions included

Prints one JSON line.

    python tools/kgpr_bench.py [--sizes 512x512,2048x2048,4096x1024] [--reps 3]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gpflow-slim_amd"), ROOT]
DUMP = os.path.join(tempfile.mkdtemp(prefix="kgpr_bench_"), "launches.txt")
os.environ["GPS_PROF_DUMP"] = DUMP            # (read once, when the first profiled launch is collected)
import numpy as np  # noqa: E402
import gpflowSlim as gpf  # noqa: E402


def best(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * min(t)


def class_ms(h, fn):
    h.profile_reset()
    fn()
    return {k: h.profile_get(k)["ms"] for k in ("gemm_f64", "other")}


def spectrum_ms(m, n):
    """microseconds of the last rows pass and columns pass in the per-launch list"""
    rows = cols = None
    if os.path.exists(DUMP):
        for line in open(DUMP):
            f = line.split()
            if f[0] == "other" and int(f[1]) == m and int(f[2]) == n and f[3] in ("1", "2"):
                if f[3] == "1":
                    rows = float(f[5]) * 1e-3
                else:
                    cols = float(f[5]) * 1e-3
    return rows, cols


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512x512,2048x2048,4096x1024")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    h = gpf.get_handle()
    out = {"device": h.device_info()["name"], "max_iter": 100, "tol": 0.0, "cases": []}
    for size in a.sizes.split(","):
        m, n = (int(v) for v in size.split("x"))
        rng = np.random.default_rng(0)
        X1, X2 = rng.uniform(0, 0.05 * m, (m, 2)), rng.uniform(0, 0.5 * n, (n, 1))
        Y = np.sin(X1[:, :1]) * np.cos(X2[:, 0])[None, :] + 0.1 * rng.standard_normal((m, n))
        mask = (rng.uniform(size=(m, n)) < 0.2).astype(float)
        model = gpf.models.KGPR(X1, X2, Y, gpf.kernels.RBF(2, lengthscales=0.7, variance=1.3),
                                gpf.kernels.RBF(1, lengthscales=0.5, variance=0.8), mask, obs_var=0.1, cg_max_iter=100, cg_tol=0.0)
        p1, p2 = model._programs()
        K1, K2 = h.kmat(p1, X1), h.kmat(p2, X2)
        C = (0.1 + 1e6 * mask) ** -0.5
        b = C * Y
        h.profile_enable(False)
        t100 = best(lambda: h.kron_cg(K1, K2, b, C, 100, 0.0), a.reps)
        t0 = best(lambda: h.kron_cg(K1, K2, b, C, 0, 0.0), a.reps)
        iters = h.kron_cg(K1, K2, b, C, 100, 0.0)[1]
        h.profile_enable(True)
        c100 = class_ms(h, lambda: h.kron_cg(K1, K2, b, C, 100, 0.0))
        c0 = class_ms(h, lambda: h.kron_cg(K1, K2, b, C, 0, 0.0))
        h.profile_enable(False)
        mp, np_ = -(-m // 128) * 128, -(-n // 128) * 128
        g1, _ = h.diag_gemm_timeline(1, 0, np_, mp, np_, reps=5)
        g2, _ = h.diag_gemm_timeline(1, 0, mp, np_, mp, reps=5)
        te = time.perf_counter()
        np.linalg.eigvalsh(K1), np.linalg.eigvalsh(K2)
        t_eigvalsh = 1e3 * (time.perf_counter() - te)
        te = time.perf_counter()
        np.linalg.eigh(K1), np.linalg.eigh(K2)
        t_eigh = 1e3 * (time.perf_counter() - te)
        t_lml = best(model.compute_log_likelihood, 1)
        t_grad = best(model.compute_log_likelihood_and_gradients, 1)
        h.profile_enable(True)
        h.profile_reset()
        model.compute_log_likelihood_and_gradients()
        h.profile_reset()
        h.profile_enable(False)
        rows_ms, cols_ms = spectrum_ms(m, n)
        per_iter = (t100 - t0) / 100
        gemm_it, vec_it = (c100["gemm_f64"] - c0["gemm_f64"]) / 100, (c100["other"] - c0["other"]) / 100
        out["cases"].append({
            "m": m, "n": n, "iterations_run": iters, "ms_per_iteration": per_iter, "gemm_class_ms_per_iteration": gemm_it,
            "vector_class_ms_per_iteration": vec_it, "vector_share": vec_it / (gemm_it + vec_it),
            "gemm_alone_ms": [g1, g2], "gemm_alone_share_of_iteration": (g1 + g2) / per_iter,
            "vector_GBps": 15 * 8.0 * mp * np_ / (vec_it * 1e-3) / 1e9,
            "spectrum_rows_ms": rows_ms, "spectrum_cols_ms": cols_ms, "host_eigvalsh_ms": t_eigvalsh, "host_eigh_ms": t_eigh,
            "lml_ms": t_lml, "lml_grad_ms": t_grad, "eig_share_of_lml": t_eigvalsh / t_lml, "eig_share_of_lml_grad": t_eigh / t_grad})
        h.release_buffers()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
