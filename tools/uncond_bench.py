"""Times the stages of the conditional at Gaussian inputs (csrc/gps_uncond.hip) at N = 4096, M = 256, Q = 4, D = 4, where the
reference's eKufKfu [N, M, M] is 2.1 GB, next to the materialising route on the API that existed before it:
psi_stats(want_psi2n=True) plus a host einsum with the same weights.  Not part of bench.py; nothing here is gated.

    python tools/uncond_bench.py [--reps 5] [--out FILE.json]

Device times come from the handle's kernel-class profile (events on the handle's stream around the launches; uploads excluded):
  contraction   "kmat" + "reduce" of one gps_psi2_contract call with D weights (psi2_contract_kernel and its fold; the
                pre-weighting psi_pkw_kernel is in "other")
  psi1          "kmat" + "reduce" of one gps_uncertain_conditional call minus the contraction: the chunked Psi1 blocks and their
                row-dot with L^-T a
  weights       every other class of that call: the Kuu build and factorisation, the triangular solves and products that form W_d
  psi2_forward  "kmat" + "reduce" of gps_psi_stats(Psi2) on the same inputs: the rate of psi2_kernel to compare against
Rates are exponentials per second, N M (M + 1) / 2 per pass over the pairs.  Every figure: median and min / max over the reps.
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

CLASSES = ("gemm_f64", "potrf_base", "kmat", "trsv", "reduce", "other")


def stats(x):
    return {"median_ms": float(np.median(x)), "min_ms": float(np.min(x)), "max_ms": float(np.max(x))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--m", type=int, default=256)
    args = ap.parse_args()
    import gpflowSlim as gpf
    import _uncond_ref as ur
    N, M, Q, D = args.n, args.m, 4, 4
    x = ur.inputs(N, M, Q, D, seed=1, lsf=0.35)
    q_mu, q_sqrt = ur.posterior(x, True)
    p = x["parts"][0]
    k = gpf.ekernels.RBF(Q, variance=p["var"], lengthscales=p["ls"], ARD=True)
    prog = k._psi_program(x["mu"])
    h = gpf.get_handle()
    rng = np.random.default_rng(0)
    W = rng.standard_normal((D, M, M))
    nexp = N * M * (M + 1) / 2

    def classes(fn):
        h.profile_reset(); h.profile_enable(True)
        fn()
        h.profile_enable(False)
        return {c: h.profile_get(c)["ms"] for c in CLASSES}

    uc = lambda: h.uncertain_conditional(prog, x["Z"], x["mu"], x["S"], q_mu, q_sqrt, 1e-6, white=True)
    con = lambda: h.psi2_contract(prog, x["Z"], x["mu"], x["S"], W)
    fwd = lambda: h.psi_stats(prog, x["Z"], x["mu"], x["S"], want_psi2=True)

    def materialise():
        p2n = h.psi_stats(prog, x["Z"], x["mu"], x["S"], want_psi2n=True)[2]
        return np.tensordot(p2n, 0.5 * (W + W.transpose(0, 2, 1)), axes=([1, 2], [1, 2]))

    got = con(); uc(); fwd()                                          # warm-up
    ref = materialise()
    diff = float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
    t = {kk: [] for kk in ("contraction", "psi1", "weights", "psi2_forward", "uc_wall", "contract_wall", "materialise_wall")}
    for _ in range(args.reps):
        c = classes(con)
        t["contraction"].append(c["kmat"] + c["reduce"])
        u = classes(uc)
        t["psi1"].append(u["kmat"] + u["reduce"] - (c["kmat"] + c["reduce"]))
        t["weights"].append(sum(u[kk] for kk in CLASSES if kk not in ("kmat", "reduce")))
        f = classes(fwd)
        t["psi2_forward"].append(f["kmat"] + f["reduce"])
        for name, fn in (("uc_wall", uc), ("contract_wall", con), ("materialise_wall", materialise)):
            t0 = time.perf_counter(); fn(); t[name].append(1e3 * (time.perf_counter() - t0))
    res = {"N": N, "M": M, "Q": Q, "D": D, "psi2n_bytes": 8.0 * N * M * M}
    res.update({kk: stats(v) for kk, v in t.items()})
    res["contraction_Gexp_per_s"] = nexp / res["contraction"]["median_ms"] / 1e6
    res["psi2_forward_Gexp_per_s"] = nexp / res["psi2_forward"]["median_ms"] / 1e6
    res["materialise_over_contract_wall"] = res["materialise_wall"]["median_ms"] / res["contract_wall"]["median_ms"]
    res["max_rel_diff_contract_vs_materialise"] = diff
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
