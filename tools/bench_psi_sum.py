"""Times the Bayesian GPLVM bound + gradient with the reference example's kernel -- an ekernels.Sum of two RBF parts on separate
latent dimensions (csrc/psi_sum.hip, csrc/gps_gplvm.hip) -- next to the single ARD RBF at the same N, M, Q on the same build.
Sibling of tools/bench_psi.py (whose "bound_and_gradient_wall" is the single-RBF figure to compare across commits); not part of
bench.py.

    python tools/bench_psi_sum.py [--reps 7] [--out FILE.json]

Sizes: the example's (N = 1000, M = 20, Q = 5 split 3 + 2) and N = 10^5, M = 512, Q = 8 split 4 + 4; R = 12 outputs.
Bound + gradient: host clock around gps_bgplvm_grad (it ends in a stream synchronise); median and min / max over the reps.
Device time by kernel class comes from the handle's profile (events around the launches, uploads excluded):
  cross_term_gemm   the "gemm_f64" class of one gps_psi_stats(Psi2) call of the Sum: nothing else in that call is a GEMM
  psi2_sum_forward  "kmat" + "reduce" + "other" of the same call: the parts' Psi2 kernels, the chunks' Psi1 blocks, the glue
  grad_classes      every class of one gps_bgplvm_grad call, for the Sum and for the single RBF; dense_vjp_extra is the Sum's
                    "kmat" + "gemm_f64" + "other" time beyond the single RBF's, minus the forward difference measured the same way
                    on gps_bgplvm: what the second Psi2 VJP, the recomputed Psi1 blocks, the cotangent GEMM and the dense passes add.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpflow-slim_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

CLASSES = ("gemm_f64", "kmat", "reduce", "other", "potrf_base", "trsv")


def stats(x):
    return {"median_ms": float(np.median(x)), "min_ms": float(np.min(x)), "max_ms": float(np.max(x))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import gpflowSlim as gpf
    from gpflowSlim import _backend as be
    import _psi_ref as pr
    h = gpf.get_handle()
    E = gpf.ekernels
    results = []
    for (N, M, Q, split, R) in ((1000, 20, 5, 3, 12), (100000, 512, 8, 4, 12)):
        d = pr.inputs(N, M, Q, R=R, seed=1)
        single = E.RBF(Q, variance=d["var"], lengthscales=d["ls"], ARD=True)
        summed = E.Sum([E.RBF(split, variance=1.7, lengthscales=d["ls"][:split], active_dims=slice(0, split), ARD=True),
                        E.RBF(Q - split, variance=1.1, lengthscales=d["ls"][split:], active_dims=slice(split, Q), ARD=True)])
        progs = {"single": single._psi_program(d["mu"]), "sum": summed._psi_program(d["mu"])}

        def classes(fn):
            h.profile_reset(); h.profile_enable(True)
            fn()
            h.profile_enable(False)
            return {c: h.profile_get(c)["ms"] for c in CLASSES}

        res = {"N": N, "M": M, "Q": Q, "split": [split, Q - split], "R": R, "cross_term_chunking": list(be.psi_sum_chunking(N, M))}
        per = {}
        for name, prog in progs.items():
            grad = lambda: h.bgplvm_grad(prog, d["Z"], d["mu"], d["S"], d["Y"], 1e-6, 0.1)
            fwd = lambda: h.bgplvm(prog, d["Z"], d["mu"], d["S"], d["Y"], 1e-6, 0.1)
            grad(); fwd()                                             # warm-up
            wall = []
            for _ in range(args.reps):
                t0 = time.perf_counter(); grad(); wall.append(1e3 * (time.perf_counter() - t0))
            per[name] = {"bound_and_gradient_wall": stats(wall), "grad_classes": classes(grad), "bound_classes": classes(fwd)}
        res.update(per)
        psi2 = classes(lambda: h.psi_stats(progs["sum"], d["Z"], d["mu"], d["S"], want_psi2=True))
        res["cross_term_gemm_ms"] = psi2["gemm_f64"]
        res["psi2_sum_forward_ms"] = psi2["kmat"] + psi2["reduce"] + psi2["other"]
        part = lambda r: r["kmat"] + r["gemm_f64"] + r["other"]
        res["dense_vjp_extra_ms"] = ((part(per["sum"]["grad_classes"]) - part(per["single"]["grad_classes"]))
                                     - (part(per["sum"]["bound_classes"]) - part(per["single"]["bound_classes"])))
        res["sum_over_single_wall"] = (per["sum"]["bound_and_gradient_wall"]["median_ms"]
                                       / per["single"]["bound_and_gradient_wall"]["median_ms"])
        print(json.dumps(res), flush=True)
        results.append(res)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
