"""Every output of the kernel-matrix build (csrc/kmat.hip) on seeded inputs, one .npy per array.

    python tools/kmat_dump.py OUTDIR            dump (GPFLOWSLIM_HIP_LIB names another build of the library)
    python tools/kmat_dump.py --compare A B     every array of A must be np.array_equal to its namesake in B (NaN where B has NaN)

The cases are the smallest that reach each branch: Handle.kmat symmetric and rectangular on both sides of the 64-wide tile,
with and without diag_add, under every (kmat_fast, kmat_mfma) pair that changes the routing -- single primitives, left-deep
chains (the chain kernels), chains the chain kernels do not know and a program that is not left-deep (the interpreter), White
and Constant, Neural Kernel Networks; the feature table by pointer; a NaN input row; the lower-triangle builds that only the
models reach (GPR likelihood with the small-N path off); the per-point Kdiag behind predict_f; the sub-block build on two
virtual ranks (tests/test_gpu_dist.py).  Run twice at one build to see that the build repeats itself bit for bit, then once at
another to see that a refactor moved no bits."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gpflow-slim_amd"), ROOT, os.path.join(ROOT, "tests")]


def compare(a, b):
    """np.array_equal per array; where an array holds NaN (the NaN-input cases), the NaN masks and the other values"""
    names_a, names_b = sorted(os.listdir(a)), sorted(os.listdir(b))
    bad = sorted(set(names_a) ^ set(names_b))
    for name in sorted(set(names_a) & set(names_b)):
        x, y = np.load(os.path.join(a, name)), np.load(os.path.join(b, name))
        same = x.shape == y.shape and (np.array_equal(x, y) or (np.array_equal(np.isnan(x), np.isnan(y))
                                                                 and np.array_equal(x[~np.isnan(x)], y[~np.isnan(y)])))
        if not same:
            bad.append(name)
    print("%d arrays in %s, %d in %s, %d differ or are missing" % (len(names_a), a, len(names_b), b, len(bad)))
    for name in bad:
        print("  " + name)
    return 1 if bad else 0


OPTION_PAIRS = ((1, 1), (1, 0), (0, 1), (1, 2))          # (kmat_fast, kmat_mfma)


def _nkn_linear(gpf, d):
    """a network with a Linear primitive (the shape of tests/test_gpu_newkernels.py::_nkn)"""
    from gpflowSlim.neural_kernel_network import NKNWrapper, NeuralKernelNetwork
    k = gpf.kernels
    prims = [k.RBF(d, variance=1.1, lengthscales=1.3), k.Periodic(d, period=2.1, variance=0.9, lengthscales=1.2),
             k.Linear(d, variance=np.linspace(0.4, 0.8, d), ARD=True), k.RatQuad(d, alpha=1.5, variance=0.8, lengthscales=1.1)]
    np.random.seed(3)                     # (the wrapper draws its initial weights from numpy's global generator)
    hparams = [dict(name="Linear", params=dict(input_dim=4, output_dim=4, name="l1")),
               dict(name="Product", params=dict(input_dim=4, step=2, name="p1")),
               dict(name="Linear", params=dict(input_dim=2, output_dim=1, name="l2"))]
    return NeuralKernelNetwork(d, prims, NKNWrapper(hparams))


def _programs(gpf, d):
    from test_gpu_parity import _nkn_case          # (the suite's own network: a second copy here would drift from what it checks)
    k = gpf.kernels
    ls = np.linspace(0.8, 1.7, d)
    return {
        "rbf": k.RBF(d, variance=1.2, lengthscales=ls, ARD=True),
        "m12": k.Matern12(d, variance=0.7, lengthscales=2.0),
        "m32": k.Matern32(d, variance=1.1, lengthscales=ls * 1.3, ARD=True),
        "m52": k.Matern52(d, variance=0.9, lengthscales=1.4),
        "exp": k.Exponential(d, variance=0.6, lengthscales=1.5),
        "ratquad": k.RatQuad(d, alpha=0.5, variance=1.3, lengthscales=ls, ARD=True),
        "linear": k.Linear(d, variance=np.linspace(0.6, 1.9, d), ARD=True),
        "poly1": k.Polynomial(d, degree=1, variance=np.linspace(0.3, 0.5, d), offset=0.8, ARD=True),
        "poly3": k.Polynomial(d, degree=3, variance=0.4, offset=0.6),
        # the three chains of tests/test_gpu_kernels.py::test_kernel_matrix_chain_kernel_equals_interpreter (White and Constant
        # inside the second)
        "chain_m52_periodic": k.Matern52(d, variance=1.2, lengthscales=ls, ARD=True) + k.Periodic(d, variance=0.7, lengthscales=1.3, period=2.1),
        "chain_white_const": k.RBF(d, variance=0.9, lengthscales=1.1) * k.Periodic(d, variance=1.1, lengthscales=0.9, period=1.7)
        + k.White(d, variance=0.3) + k.Constant(d, variance=0.25),
        "chain_product3": k.Matern32(d, variance=1.0, lengthscales=0.7) * k.Matern12(d, variance=2.0, lengthscales=1.9)
        * k.Exponential(d, variance=0.5, lengthscales=1.2),
        "chain_ratquad": k.RatQuad(d, alpha=7.0, variance=0.6, lengthscales=0.9) + k.RBF(d, variance=1.1, lengthscales=1.6)
        + k.Linear(d, variance=0.5),
        "not_left_deep": (k.RBF(d, variance=1.2, lengthscales=1.6) + k.Matern12(d, variance=0.7, lengthscales=2.0))
        * (k.Periodic(d, period=2.0, variance=0.8, lengthscales=1.1) + k.Matern52(d, variance=0.9, lengthscales=1.3)),
        "nkn": _nkn_case(gpf, d, False)[0],
        "nkn_act": _nkn_case(gpf, d, True)[0],
        "nkn_linear": _nkn_linear(gpf, d),
    }


def dump(out):
    import gpflowSlim as gpf
    os.makedirs(out, exist_ok=True)
    count = [0]

    def save(case, **arrays):
        for key, val in arrays.items():
            np.save(os.path.join(out, "%s__%s.npy" % (case, key)), np.asarray(val, dtype=np.float64))
            count[0] += 1

    h = gpf.get_handle()
    d = 3
    progs = _programs(gpf, d)
    shapes = [(n, None) for n in (1, 63, 64, 65, 130, 257)] + [(40, 300), (257, 70)]
    try:
        for fast, mfma in OPTION_PAIRS:
            h.set_option("kmat_fast", fast); h.set_option("kmat_mfma", mfma)
            for n, m in shapes:
                rng = np.random.default_rng(1000 * n + (m or 0))
                X = rng.standard_normal((n, d))
                X2 = None if m is None else rng.standard_normal((m, d))
                for name, kern in progs.items():
                    prog = kern._program(d)
                    for diag_add in (0.0, 0.37):
                        save("kmat_f%dm%d_%s_n%d_m%s_diag%g" % (fast, mfma, name, n, m, diag_add), K=h.kmat(prog, X, X2, diag_add))
            # ---- prep by pointer: 26 feature rows
            rng = np.random.default_rng(26)
            X26 = rng.standard_normal((130, 26))
            kern = gpf.kernels.RBF(26, variance=1.2, lengthscales=np.linspace(3.0, 6.0, 26), ARD=True)
            save("kmat_f%dm%d_rbf_ard26" % (fast, mfma), K=h.kmat(kern._program(26), X26), K2=h.kmat(kern._program(26), X26, X26[:70]))
            # ---- a NaN coordinate poisons its row and column
            rng = np.random.default_rng(3)
            Xn = rng.standard_normal((300, d)); Xn[17, 1] = np.nan
            for name in ("rbf", "m52", "chain_m52_periodic", "chain_ratquad", "nkn"):
                save("nan_f%dm%d_%s" % (fast, mfma, name), K=h.kmat(progs[name]._program(d), Xn))
    finally:
        h.set_option("kmat_fast", 1); h.set_option("kmat_mfma", 1)

    # ---- lower-triangle builds (the models': K below the 128-block diagonal only) and the per-point Kdiag
    k = gpf.kernels
    lower = [("single", "rbf", 1, 1), ("single", "ratquad", 1, 1), ("chain_mfma", "chain_m52_periodic", 1, 1),
             ("chain_valu", "chain_m52_periodic", 1, 0), ("interp", "chain_ratquad", 1, 1), ("interp_off", "chain_white_const", 0, 1)]
    try:
        h.set_option("small_n", 0)
        for n in (130, 300):
            rng = np.random.default_rng(n)
            X = rng.standard_normal((n, d))
            Y = np.sin(X @ rng.standard_normal((d, 2))) + 0.1 * rng.standard_normal((n, 2))
            for tag, name, fast, mfma in lower:
                h.set_option("kmat_fast", fast); h.set_option("kmat_mfma", mfma)
                m = gpf.models.GPR(X, Y, progs[name], obs_var=0.15)
                save("lml_%s_%s_n%d" % (tag, name, n), lml=m.compute_log_likelihood())
        h.set_option("kmat_fast", 1); h.set_option("kmat_mfma", 1)
        rng = np.random.default_rng(12)
        X = rng.standard_normal((200, d)); Xs = 1.5 * rng.standard_normal((70, d))
        Y = X @ rng.standard_normal((d, 2)) + np.sin(X[:, :2]) + 0.1 * rng.standard_normal((200, 2))
        for name, kern in (("linear", progs["linear"]),
                           ("poly_plus_rbf", k.Polynomial(d, degree=2, variance=0.3, offset=0.7) + k.RBF(d, variance=1.2, lengthscales=1.1)),
                           ("nkn_linear", progs["nkn_linear"])):
            m = gpf.models.GPR(X, Y, kern, obs_var=0.15)
            mu, var = m.predict_f(Xs)
            save("predict_%s" % name, mu=mu, var=var, kdiag=kern.Kdiag(Xs))
    finally:
        h.set_option("small_n", 1); h.set_option("kmat_fast", 1); h.set_option("kmat_mfma", 1)

    # ---- gps_launch_kmat_block: one likelihood on two virtual ranks
    from test_gpu_dist import _run_virtual_ranks
    rng = np.random.default_rng(2)
    X = rng.standard_normal((1024, d))
    Y = np.sin(X @ rng.standard_normal((d, 1))) + 0.1 * rng.standard_normal((1024, 1))
    for name in ("rbf", "chain_m52_periodic"):
        outs, errs = _run_virtual_ranks(2, X, Y, progs[name]._program(d), 0.1, 128)
        assert all(e is None for e in errs), errs
        for rank, res in enumerate(outs):
            save("block_%s_rank%d" % (name, rank), lml=np.asarray(res, dtype=np.float64).ravel())
    print("kmat_dump: %d arrays in %s" % (count[0], out), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    dump(sys.argv[1])
