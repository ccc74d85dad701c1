"""One-shot timer: LML + gradient of a GPR (RBF-ARD, d = 3, r = 1) through gpflowSlim.distributed.gpr_lml_grad_distributed on
P virtual ranks (host threads, one handle each, on ONE GPU; panels exchanged by device copies) against the fused single-GPU
GPR.compute_log_likelihood_and_gradients.  Warm: one untimed call of each first.  Virtual ranks share one GPU, so P > 1 times
are the sum of all ranks' work plus the exchanges, not a multi-GPU figure.

    python tools/dist_grad_once.py --n 16384 --P 1 --nb 512
    python tools/dist_grad_once.py --n 32768 --P 8 --nb 512
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpflow-slim_amd"))


class _Done(object):
    def wait(self):
        return True


class ThreadComm(object):
    """P host threads as P ranks: broadcast by device copy, row gather through a shared dict (barrier-ordered)."""
    bytes_sent = 0
    exchanges = 0

    def __init__(self, rank, world, shared):
        self.rank, self.world, self.shared = rank, world, shared

    def exchange(self, tensor, src):
        import torch
        sh = self.shared
        torch.cuda.synchronize()
        if self.rank == src:
            sh["slot"] = tensor
        sh["barrier"].wait()
        if self.rank != src:
            tensor.copy_(sh["slot"])
            torch.cuda.synchronize()
        sh["barrier"].wait()
        return _Done()

    def all_gather_rows(self, local, counts):
        sh = self.shared
        sh["barrier"].wait()
        sh.setdefault("rows", {})[self.rank] = np.array(local, copy=True)
        sh["barrier"].wait()
        out = np.concatenate([sh["rows"][r] for r in range(self.world)], axis=0)
        sh["barrier"].wait()
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--P", type=int, default=1)
    ap.add_argument("--nb", type=int, default=512)
    a = ap.parse_args()
    import torch
    import gpflowSlim as gpf
    from gpflowSlim import _backend as be
    from gpflowSlim.distributed import SingleComm, gpr_lml_grad_distributed
    rng = np.random.default_rng(0)
    X = rng.standard_normal((a.n, 3))
    Y = np.sin(X @ rng.standard_normal((3, 1))) + 0.1 * rng.standard_normal((a.n, 1))
    mk = lambda: gpf.models.GPR(X, Y, gpf.kernels.RBF(3, variance=1.1, lengthscales=np.array([0.9, 1.5, 2.2]), ARD=True), obs_var=0.1)
    ref = mk()
    ref.compute_log_likelihood_and_gradients()
    t0 = time.perf_counter()
    ref.compute_log_likelihood_and_gradients()
    fused = time.perf_counter() - t0
    res = {"n": a.n, "P": a.P, "nb": a.nb, "fused_s": fused}
    if a.P == 1:
        m = mk()
        gpr_lml_grad_distributed(m, SingleComm(), nb=a.nb)
        t0 = time.perf_counter()
        gpr_lml_grad_distributed(m, SingleComm(), nb=a.nb)
        res["dist_s"] = time.perf_counter() - t0
    else:
        del ref
        shared = {"barrier": threading.Barrier(a.P), "slot": None}
        times = [None] * a.P

        def run(rank):
            torch.cuda.set_device(0)
            h = be.Handle(0)
            m = mk()

            def _handle():
                if h.resident_token is not m.X:
                    h.gpr_set_data(m.X, m.X)
                    m._factor_key = None
                return h
            m._handle = _handle
            comm = ThreadComm(rank, a.P, shared)
            try:
                gpr_lml_grad_distributed(m, comm, nb=a.nb)
                shared["barrier"].wait()
                t0 = time.perf_counter()
                gpr_lml_grad_distributed(m, comm, nb=a.nb)
                times[rank] = time.perf_counter() - t0
            finally:
                h.close()

        th = [threading.Thread(target=run, args=(r,)) for r in range(a.P)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        res["dist_virtual_s"] = max(times)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
