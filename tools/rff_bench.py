"""Stage times of the random-feature GPR branch (csrc/gps_rff.hip) at N = 2^20, D = 8, F in {512, 2048}: per likelihood and
per likelihood + gradient, from the handle's hipEvent stage marks and per-class launch brackets -- feature build (with the GB/s
of Phit written), Gram (with the fraction of the 78.6 TFLOP/s fp64 peak on N F^2), factor + solves, contraction -- and, in the
same run, gps_launch_gemm_nt alone on device-resident random operands of the shape of one chunk's Gram launch: the Gram stage
can be no faster than that, the gap between the two is what the chunking costs.  In the gradient run the first pass's share of
the feature class is taken as one third of it (bytes written: Phit, then Phit and St).  Prints one JSON line.

    python tools/rff_bench.py [--n 1048576] [--d 8] [--f 512,2048] [--reps 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gpflow-slim_amd"), ROOT]
import numpy as np  # noqa: E402
import gpflowSlim as gpf  # noqa: E402
from gpflowSlim import _backend as be  # noqa: E402

PEAK = 78.6e12
CLASSES = ("rff_features", "gemm_f64", "rff_contract", "potrf_base", "trsv", "reduce", "other")


def measure(h, fn, reps):
    """min over reps of (stage marks, per-class ms) of one call of fn, after one warm-up call."""
    fn()
    best = None
    for _ in range(reps):
        h.profile_reset()
        fn()
        st = h.last_stage_ms()
        cls = {k: h.profile_get(k)["ms"] for k in CLASSES}
        tot = st["kmat"] + st["potrf"] + st["trsv"] + st["predict"]
        if best is None or tot < best[0]:
            best = (tot, st, cls)
    return best[1], best[2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--f", default="512,2048")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    X = rng.standard_normal((a.n, a.d))
    Y = np.sin(X[:, :1]) + 0.1 * rng.standard_normal((a.n, 1))
    h = gpf.get_handle()
    h.profile_enable(True)
    out = {"n": a.n, "d": a.d, "device": h.device_info()["name"], "cases": []}
    for F in [int(v) for v in a.f.split(",")]:
        s = gpf.kernel_kitchen_sink.RBFSampler(a.d, ls=np.sqrt(a.d) * np.ones(a.d), n_components=F, rng=rng)
        desc, keep = s._descriptor()
        Fp = -(-F // 128) * 128
        nc = min(max(128, ((1 << 30) // (Fp * 8)) // 128 * 128), -(-a.n // 128) * 128)
        chunks = -(-a.n // nc)
        st, cls = measure(h, lambda: h.rff_lml(desc, X, 0.1, Y), a.reps)
        stg, clsg = measure(h, lambda: h.rff_lml_grad(desc, X, 0.1, Y), a.reps)
        # the parent commit's GEMM alone, on device-resident random operands of the shape of one chunk's Gram launch: the
        # (Fp + 128) x Fp lower trapezoid with K = chunk rows
        raw_ms, _ = h.diag_gemm_timeline(2, 1, Fp + 128, Fp, nc, reps=3)

        def first_pass(stage, klass, feat_share):
            g = stage["kmat"] - klass["rff_features"] * feat_share      # the first pass without its feature launches
            return g, a.n * F * F / (g * 1e-3) / PEAK

        gram, gram_frac = first_pass(st, cls, 1.0)
        gram_g, gram_g_frac = first_pass(stg, clsg, 1.0 / 3.0)   # the feature class holds Phit (first pass), Phit + St (second)
        c = {"F": F, "chunk_rows": nc, "chunks": chunks,
             "lml": {"feature_ms": cls["rff_features"], "feature_GBps": 8.0 * Fp * nc * chunks / cls["rff_features"] / 1e6,
                     "gram_ms": gram, "gram_frac_peak": gram_frac,
                     "factor_solves_ms": st["potrf"], "gemm_class_ms": cls["gemm_f64"], "total_ms": st["kmat"] + st["potrf"]},
             "lml_grad": {"feature_ms": clsg["rff_features"],
                          "feature_GBps": 8.0 * Fp * nc * chunks * 3 / clsg["rff_features"] / 1e6,     # Phit, then Phit and St
                          "gram_ms": gram_g, "gram_frac_peak": gram_g_frac, "factor_solves_ms": stg["potrf"],
                          "inverse_ms": stg["trsv"], "second_pass_ms": stg["predict"], "contraction_ms": clsg["rff_contract"],
                          "gemm_class_ms": clsg["gemm_f64"], "other_class_ms": clsg["other"],
                          "total_ms": stg["kmat"] + stg["potrf"] + stg["trsv"] + stg["predict"]},
             "raw_gemm_ms_per_chunk": raw_ms, "raw_gemm_ms_all_chunks": raw_ms * chunks,
             "raw_gemm_frac_peak": a.n * F * F / (raw_ms * chunks * 1e-3) / PEAK}
        out["cases"].append(c)
        h.release_buffers()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
