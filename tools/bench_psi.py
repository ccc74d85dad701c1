"""Times the Psi2 kernel, its vector-Jacobian product and the full Bayesian GPLVM bound + gradient (csrc/psi.hip,
csrc/gps_gplvm.hip) against a chunked torch fp64 broadcast implementation of the same Psi2 on the same GPU.  torch is the
comparator only; it is never on the product path.  Not part of bench.py.

    python tools/bench_psi.py [--reps 7] [--out FILE.json]

Psi2 forward: device time from the handle's kernel-class profile ("kmat" + "reduce" launches of one gps_psi_stats call, i.e.
events on the handle's stream around the launches; uploads excluded).  VJP: the same for the two recomputing passes of one
gps_bgplvm_grad call minus one forward.  Bound + gradient: host clock around the call (it ends in a stream synchronise).
Rates are exponentials per second with N M (M + 1) / 2 exponentials per Psi2.  Every figure: median and min / max over the reps.
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


def torch_psi2(torch, var, ls, Z, mu, S, block):
    """the same Psi2, broadcast over [block, M, M, Q] chunks in fp64"""
    M = Z.shape[0]
    zbar = 0.5 * (Z[:, None, :] + Z[None, :, :])
    kz = var ** 2 * torch.exp(-((Z[:, None, :] - Z[None, :, :]) ** 2 / (4 * ls ** 2)).sum(-1))
    out = torch.zeros((M, M), dtype=torch.float64, device=Z.device)
    for i in range(0, mu.shape[0], block):
        m_, s_ = mu[i:i + block], S[i:i + block]
        a = 1.0 / (ls ** 2 + 2 * s_)
        c = -0.5 * torch.log1p(2 * s_ / ls ** 2).sum(-1)
        e = (((m_[:, None, None, :] - zbar[None]) ** 2) * a[:, None, None, :]).sum(-1)
        out += torch.exp(c[:, None, None] - e).sum(0)
    return out * kz


def stats(x):
    return {"median_ms": float(np.median(x)), "min_ms": float(np.min(x)), "max_ms": float(np.max(x))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import gpflowSlim as gpf
    import _psi_ref as pr
    h = gpf.get_handle()
    dev = torch.device("cuda:%d" % h.device)
    results = []
    for (N, M, Q, R) in ((1000, 20, 5, 12), (100000, 512, 8, 12)):
        d = pr.inputs(N, M, Q, R=R, seed=1)
        k = gpf.ekernels.RBF(Q, variance=d["var"], lengthscales=d["ls"], ARD=True)
        prog = k._psi_program(d["mu"])
        nexp = N * M * (M + 1) / 2

        def dev_ms(fn):
            h.profile_reset(); h.profile_enable(True)
            fn()
            h.profile_enable(False)
            return h.profile_get("kmat")["ms"] + h.profile_get("reduce")["ms"]

        fwd = lambda: h.psi_stats(prog, d["Z"], d["mu"], d["S"], want_psi2=True)[1]
        grad = lambda: h.bgplvm_grad(prog, d["Z"], d["mu"], d["S"], d["Y"], 1e-6, 0.1)
        p2 = fwd(); grad()                                            # warm-up
        t_fwd, t_all_dev, t_wall = [], [], []
        for _ in range(args.reps):
            t_fwd.append(dev_ms(fwd))
            t0 = time.perf_counter(); grad(); t_wall.append(1e3 * (time.perf_counter() - t0))
            t_all_dev.append(dev_ms(grad))
        tz = {kk: torch.tensor(np.asarray(d[kk]), dtype=torch.float64, device=dev) for kk in ("Z", "mu", "S", "ls")}
        block = max(1, int(2 ** 27 // (M * M * Q)))                   # 1 GiB of fp64 per [block, M, M, Q] temporary
        ref = lambda: torch_psi2(torch, d["var"], tz["ls"], tz["Z"], tz["mu"], tz["S"], block)
        p2t = ref(); torch.cuda.synchronize()
        err = float(np.max(np.abs(p2t.cpu().numpy() - p2) / np.abs(p2)))
        t_torch = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); ref(); e1.record(); torch.cuda.synchronize()
            t_torch.append(e0.elapsed_time(e1))
        f, t = stats(t_fwd), stats(t_torch)
        vjp = stats(np.asarray(t_all_dev) - np.asarray(t_fwd))
        res = {"N": N, "M": M, "Q": Q, "R": R, "psi2_forward": f, "psi2_forward_Gexp_per_s": nexp / f["median_ms"] / 1e6,
               "torch_psi2": t, "torch_block": block, "torch_over_hip": t["median_ms"] / f["median_ms"],
               "max_rel_diff_torch_vs_hip": err, "psi_vjps_device": vjp, "vjp_Gexp_per_s": 3 * nexp / vjp["median_ms"] / 1e6,
               "bound_and_gradient_wall": stats(t_wall)}
        print(json.dumps(res), flush=True)
        results.append(res)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)
    slow = [r for r in results if r["torch_over_hip"] < 1.0]
    if slow:
        print("FAIL: the HIP Psi2 kernel is slower than the torch comparator at", [(r["N"], r["M"]) for r in slow])
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
