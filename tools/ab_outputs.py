"""Bit-for-bit A/B of two builds of the library on the host paths of the inducing-point, MCMC, BGPLVM and likelihood entries.

    python tools/ab_outputs.py [--libs lib_parent,lib] [--cases gpmc,sgpmc,...] [--out DIR] [--timeout 300]

For each case one fresh child process per library (GPFLOWSLIM_HIP_LIB, as tools/ab_lib.py; libdirs relative to
gpflow-slim_amd/), one GPU process at a time, each under its own time limit; the first non-zero exit ends the run.  A child runs
the case's entries through Handle on seeded inputs with the kernel-class profile on and saves every output array and scalar,
and the launch count of every kernel class after each entry, to DIR/<case>.<libdir>.npz.  The parent compares the two files of a
case key by key with np.array_equal, NaN positions included.  There is no tolerance: the builds are expected to run the same
arithmetic in the same order.  Prints one JSON line; exit status 1 on any difference.

The shapes are the smallest that reach both sides of every branch of those host paths: 129 inducing points (two diagonal blocks),
1 / 5 / 17 latents (the 1-, 16- and 16 + 1-plane kernels), three data chunks with a partial last one, a single RBF and a Sum of
two RBF parts with at least two chunks of the streamed cross terms.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("gemm_f64", "potrf_base", "kmat", "trsv", "reduce", "other")
sys.path.insert(0, os.path.join(ROOT, "tests"))
# (the likelihood table and the input helpers are shared with the call-order tests)
from _entry_catalogue import LIK_KINDS, _psi_kernels, lik_table as _lik, psi_inputs as _psi_inputs, tril_stack as _tril_stack  # noqa: E402


class Recorder(object):
    """Runs entries on the handle and keeps what they return, flattened, next to the launch counts they made."""

    def __init__(self, h):
        self.h, self.out = h, {}

    def run(self, name, fn):
        h = self.h
        h.profile_reset()
        h.profile_enable(True)
        try:
            res = fn()
        except RuntimeError as e:                                     # (a refusal is an output too: its text)
            res = ("raised: %s" % e,)
        h.profile_enable(False)
        if not isinstance(res, tuple):
            res = (res,)
        for i, v in enumerate(res):
            if v is None:
                continue
            self.out["%s/%d" % (name, i)] = np.array(v) if isinstance(v, str) else np.asarray(v, dtype=np.float64)
        self.out["%s/launches" % name] = np.array([h.profile_get(c)["launches"] for c in CLASSES], dtype=np.int64)


def _kernels(gpf, d):
    ls = np.linspace(0.8, 1.3, d)
    # "linear": Kdiag depends on the point (a Linear part alone would leave Kuu with rank d)
    return {"rbf": gpf.kernels.RBF(d, variance=1.3, lengthscales=ls, ARD=True),
            "linear": gpf.kernels.Matern52(d, variance=0.9, lengthscales=ls, ARD=True)
                      + gpf.kernels.Linear(d, variance=np.linspace(0.2, 0.4, d), ARD=True)}


def case_gpmc(gpf, be, rec):
    n, d = 129, 3
    prog = _kernels(gpf, d)["rbf"]._program(d)
    for r in (1, 5, 17):
        rng = np.random.default_rng(100 + r)
        X, V = rng.standard_normal((n, d)), 0.5 * rng.standard_normal((n, r))
        lik, ys = _lik(be, "bernoulli", r)
        Y = ys(rng, (n, r))
        mean = 0.3 * rng.standard_normal((n, r))
        for mname, mval in (("nomean", None), ("mean", mean)):
            rec.run("gpmc_lik_grad/r%d/%s" % (r, mname), lambda: rec.h.gpmc_lik_grad(prog, X, V, Y, 1e-6, lik, mean=mval))


def case_sgpmc(gpf, be, rec):
    m, n, d = 129, 300, 3
    for kname, kern in _kernels(gpf, d).items():
        prog = kern._program(d)
        for r in (1, 5, 17):
            rng = np.random.default_rng(200 + r)
            Z, X, V = rng.standard_normal((m, d)), rng.standard_normal((n, d)), 0.5 * rng.standard_normal((m, r))
            lik, ys = _lik(be, "bernoulli", r)
            Y = ys(rng, (n, r))
            mean = 0.3 * rng.standard_normal((n, r))
            rec.run("sgpmc_lik_grad/%s/r%d" % (kname, r),
                    lambda: rec.h.sgpmc_lik_grad(prog, Z, X, Y, V, 1e-6, lik, mean=mean, chunk_rows=128, want_grad_Z=True))


def case_bgplvm(gpf, be, rec):
    m, n, q, r = 129, 70, 3, 2
    rng = np.random.default_rng(300)
    Z, mu, S = _psi_inputs(rng, n, m, q)
    Y, Xnew = rng.standard_normal((n, r)), rng.standard_normal((9, q))
    rec.h.psi_sum_set_chunk(32)                                       # 70 points: three chunks of the streamed cross terms
    for kname, kern in _psi_kernels(gpf, q).items():
        prog = kern._psi_program(mu)
        rec.run("bgplvm/%s" % kname, lambda: rec.h.bgplvm(prog, Z, mu, S, Y, 1e-6, 0.1, Xnew=Xnew))
        rec.run("bgplvm_full_cov/%s" % kname, lambda: rec.h.bgplvm(prog, Z, mu, S, Y, 1e-6, 0.1, Xnew=Xnew, full_cov=True))
        rec.run("bgplvm_grad/%s" % kname, lambda: rec.h.bgplvm_grad(prog, Z, mu, S, Y, 1e-6, 0.1))
    rec.h.psi_sum_set_chunk(0)


def case_psi(gpf, be, rec):
    m, n, q = 5, 7, 3
    rng = np.random.default_rng(400)
    Z, mu, S = _psi_inputs(rng, n, m, q)
    for kname, kern in _psi_kernels(gpf, q).items():
        prog = kern._psi_program(mu)
        rec.run("psi_stats/%s" % kname, lambda: rec.h.psi_stats(prog, Z, mu, S, want_psi1=True, want_psi2=True, want_psi2n=True))


def case_uncond(gpf, be, rec):
    m, n, q, k = 129, 70, 3, 3
    rng = np.random.default_rng(500)
    Z, mu, S = _psi_inputs(rng, n, m, q)
    q_mu = rng.standard_normal((m, k))
    q_sqrts = {"diag": 0.5 + rng.random((m, k)), "full": _tril_stack(rng, m, k)}
    W = rng.standard_normal((k, m, m))
    rec.h.psi_sum_set_chunk(32)
    for kname, kern in _psi_kernels(gpf, q).items():
        prog = kern._psi_program(mu)
        for white in (True, False):
            for full in (False, True):
                for qname, q_sqrt in q_sqrts.items():
                    rec.run("uncertain_conditional/%s/white%d/full%d/%s" % (kname, white, full, qname),
                            lambda: rec.h.uncertain_conditional(prog, Z, mu, S, q_mu, q_sqrt, 1e-6, white=white, full_cov_output=full))
        rec.run("psi2_contract/%s" % kname, lambda: rec.h.psi2_contract(prog, Z, mu, S, W))
    rec.h.psi_sum_set_chunk(0)


def case_svgp(gpf, be, rec):
    m, n, d, k = 129, 130, 3, 3
    rng = np.random.default_rng(600)
    prog = _kernels(gpf, d)["rbf"]._program(d)
    Z, X = rng.standard_normal((m, d)), rng.standard_normal((n, d))
    yres, q_mu = rng.standard_normal((n, k)), 0.5 * rng.standard_normal((m, k))
    q_sqrts = {"diag": 0.5 + rng.random((m, k)), "full": _tril_stack(rng, m, k)}
    for qname, q_sqrt in q_sqrts.items():
        rec.run("svgp_elbo_grad/unwhitened/%s" % qname,
                lambda: rec.h.svgp_elbo_grad(prog, Z, X, yres, q_mu, q_sqrt, 1e-6, 0.2, white=False, scale=1.5, want_grad_Z=True))
    lik, ys = _lik(be, "bernoulli", k)
    Y = ys(rng, (n, k))
    for white in (True, False):
        rec.run("svgp_elbo_lik_grad/bernoulli/white%d" % white,
                lambda: rec.h.svgp_elbo_lik_grad(prog, Z, X, Y, q_mu, q_sqrts["full"], 1e-6, lik, white=white, want_grad_Z=True))


def case_sparse(gpf, be, rec):
    m, n, d, r = 129, 130, 3, 2
    rng = np.random.default_rng(700)
    prog = _kernels(gpf, d)["rbf"]._program(d)
    Z, X, Xnew = rng.standard_normal((m, d)), rng.standard_normal((n, d)), rng.standard_normal((9, d))
    resid = rng.standard_normal((n, r))
    rec.run("sgpr_grad", lambda: rec.h.sgpr_grad(prog, Z, X, resid, 1e-6, 0.2))
    rec.run("fitc_grad", lambda: rec.h.sgpr_grad(prog, Z, X, resid, 1e-6, 0.2, fitc=True))
    rec.run("fitc_predict", lambda: rec.h.sgpr(prog, Z, X, resid, 1e-6, 0.2, Xnew=Xnew, fitc=True))
    rec.run("sgpr_predict_full_cov", lambda: rec.h.sgpr(prog, Z, X, resid, 1e-6, 0.2, Xnew=Xnew, full_cov=True))


def case_conditional(gpf, be, rec):
    m, n, d, k = 129, 70, 3, 3
    rng = np.random.default_rng(800)
    prog = _kernels(gpf, d)["rbf"]._program(d)
    Z, Xnew, f = rng.standard_normal((m, d)), rng.standard_normal((n, d)), rng.standard_normal((m, k))
    q_sqrt = _tril_stack(rng, m, k)
    for white in (True, False):
        for full in (False, True):
            rec.run("conditional/white%d/full%d" % (white, full),
                    lambda: rec.h.conditional(prog, Z, Xnew, f, 1e-6, q_sqrt=q_sqrt, white=white, full_cov=full))


def case_lik(gpf, be, rec):
    n, k = 65, 3
    for kind in LIK_KINDS:
        rng = np.random.default_rng(900 + LIK_KINDS[kind])
        lik, ys = _lik(be, kind, k)
        Y = ys(rng, (n, k))
        F, Fvar = rng.standard_normal((n, k)), np.exp(rng.uniform(np.log(1e-3), np.log(2.0), (n, k)))
        rec.run("lik_varexp/%s" % kind, lambda: rec.h.lik_varexp(lik, F, Fvar, Y, want_grad=True))
        Yp = Y if kind != "multiclass" else np.zeros((n, k))         # (refused: only the message is compared)
        rec.run("lik_logp/%s" % kind, lambda: rec.h.lik_logp(lik, F, Yp, want_grad=True))


CASES = {"gpmc": case_gpmc, "sgpmc": case_sgpmc, "bgplvm": case_bgplvm, "psi": case_psi, "uncond": case_uncond, "svgp": case_svgp,
         "sparse": case_sparse, "conditional": case_conditional, "lik": case_lik}


def child(case, path):
    sys.path[:0] = [os.path.join(ROOT, "gpflow-slim_amd"), ROOT]
    import gpflowSlim as gpf
    from gpflowSlim import _backend as be
    rec = Recorder(gpf.get_handle())
    CASES[case](gpf, be, rec)
    np.savez(path, **rec.out)
    print("%s: %d arrays from %s" % (case, len(rec.out), os.environ.get("GPFLOWSLIM_HIP_LIB", "the default library")), flush=True)
    return 0


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = sorted(set(a.files) ^ set(b.files))
    for key in sorted(set(a.files) & set(b.files)):
        x, y = a[key], b[key]
        same = x.shape == y.shape and (np.array_equal(x, y) if x.dtype.kind in "US" else np.array_equal(x, y, equal_nan=True))
        if not same:
            bad.append(key)
    entries = len([k for k in a.files if k.endswith("/launches")])
    return len(a.files), entries, bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", default="lib_parent,lib")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "ab_outputs"))
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--child", nargs=2, metavar=("CASE", "FILE"), default=None)
    a = ap.parse_args()
    if a.child:
        return child(*a.child)
    libs = a.libs.split(",")
    if len(libs) != 2:
        ap.error("--libs takes two library directories")
    os.makedirs(a.out, exist_ok=True)
    report = {"libs": libs, "cases": {}, "arrays": 0, "entries": 0, "different": []}
    for case in a.cases.split(","):
        files = []
        for lib in libs:
            path = os.path.join(a.out, "%s.%s.npz" % (case, lib.replace(os.sep, "_")))
            env = dict(os.environ, GPFLOWSLIM_HIP_LIB=os.path.join(ROOT, "gpflow-slim_amd", lib, "libgpflowslim_hip.so"))
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", case, path]
            rc = subprocess.call(cmd, env=env)
            if rc != 0:                                               # (nothing more is started on the GPU after a failure)
                print(json.dumps(dict(report, failed={"case": case, "lib": lib, "exit": rc})), flush=True)
                return rc
            files.append(path)
        n, entries, bad = compare(*files)
        report["cases"][case] = {"arrays": n, "entries": entries, "different": bad}
        report["arrays"] += n
        report["entries"] += entries
        report["different"] += ["%s:%s" % (case, k) for k in bad]
        print("%s: %d arrays of %d entries, %d different" % (case, n, entries, len(bad)), flush=True)
    print(json.dumps(report), flush=True)
    return 1 if report["different"] else 0


if __name__ == "__main__":
    sys.exit(main())
