"""Every output array of the gradient kernels (csrc/grad.hip, csrc/grad_general.hip) on seeded inputs, one .npy per array.

    python tools/grad_dump.py OUTDIR            dump (GPFLOWSLIM_HIP_LIB names another build of the library)
    python tools/grad_dump.py --compare A B     every array of A must be np.array_equal to its namesake in B

The cases are the smallest that reach each branch: the four-primitive kernel over kernel kinds, sizes on both sides of the
one-launch path and of the 2048-workgroup grid, one and several outputs, with and without K_y^-1 resid, both feature-prep
kernels; the general kernel (six primitives, Neural Kernel Networks); the kernel-matrix VJPs; one SVGP and one SGPR
gradient; the block-cyclic column mode on virtual ranks (tests/test_gpu_dist_grad.py).  Run twice at one build to see that
the build repeats itself bit for bit, then once at another to see that a refactor moved no bits."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gpflow-slim_amd"), ROOT, os.path.join(ROOT, "tests")]


def compare(a, b):
    names_a, names_b = sorted(os.listdir(a)), sorted(os.listdir(b))
    bad = sorted(set(names_a) ^ set(names_b))
    for name in sorted(set(names_a) & set(names_b)):
        x, y = np.load(os.path.join(a, name)), np.load(os.path.join(b, name))
        if x.shape != y.shape or not np.array_equal(x, y):
            bad.append(name)
    print("%d arrays in %s, %d in %s, %d differ or are missing" % (len(names_a), a, len(names_b), b, len(bad)))
    for name in bad:
        print("  " + name)
    return 1 if bad else 0


def _data(n, d, r, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    Y = np.sin(X @ rng.standard_normal((d, r))) + 0.1 * rng.standard_normal((n, r))
    return X, Y


def _kernels(gpf, d):
    k = gpf.kernels
    ls = np.linspace(0.8, 1.7, d)
    return {
        "m52_plus_periodic": lambda: k.Matern52(d, variance=1.1, lengthscales=ls * 1.5, ARD=True)
        + k.Periodic(d, period=2.0, variance=0.9, lengthscales=1.2),
        "rbf_times_periodic_plus_white": lambda: k.RBF(d, variance=1.2, lengthscales=1.6)
        * k.Periodic(d, period=3.0, variance=0.9, lengthscales=1.5) + k.White(d, variance=0.2),
        "m32_ard": lambda: k.Matern32(d, variance=1.1, lengthscales=ls * 1.3, ARD=True),
        "m12_plus_exp_plus_const": lambda: k.Matern12(d, variance=0.7, lengthscales=2.0)
        + k.Exponential(d, variance=0.6, lengthscales=1.5) + k.Constant(d, variance=0.3),
        "rbf_iso": lambda: k.RBF(d, variance=1.3, lengthscales=1.4),
    }


def _six(gpf, d):
    k = gpf.kernels
    ls = np.linspace(0.8, 1.7, d)
    return (k.RBF(d, variance=1.3, lengthscales=ls, ARD=True) * k.Periodic(d, period=2.5, variance=0.8, lengthscales=1.2)
            + k.Matern52(d, variance=0.9, lengthscales=1.4) * k.Matern12(1, variance=0.7, lengthscales=2.0, active_dims=[1])
            + k.Matern32(d, variance=1.1, lengthscales=1.3) + k.White(d, variance=0.2))


def _lml_grad(h, prog, noise, resid, want_kinv_resid):
    """Handle.gpr_lml_grad, with the K_y^-1 resid output optional as in the C entry point"""
    from gpflowSlim import _backend as be
    if want_kinv_resid:
        return h.gpr_lml_grad(prog, noise, resid)
    resid = np.ascontiguousarray(resid, dtype=np.float64)
    lml, gnoise = ctypes.c_double(0), ctypes.c_double(0)
    info, ns = ctypes.c_int(0), ctypes.c_int(0)
    slots = np.zeros(160)
    h._check(h._lib.gps_gpr_lml_grad(h._h, prog, len(prog), float(noise), be._ptr(resid), resid.shape[1], ctypes.byref(lml),
                                     be._ptr(slots), 160, ctypes.byref(ns), ctypes.byref(gnoise), None, ctypes.byref(info)),
             "gps_gpr_lml_grad")
    assert info.value == 0
    return lml.value, slots[:ns.value].copy(), gnoise.value, np.zeros(0)


def dump(out):
    import gpflowSlim as gpf
    from gpflowSlim import _backend as be
    # (the tests' own NKN program and, below, their virtual-rank harness, on purpose: a second copy here would drift from what the
    # suite checks.  These are test internals -- when they change, this tool follows them)
    from test_gpu_parity import _nkn_case
    os.makedirs(out, exist_ok=True)
    count = [0]

    def save(case, **arrays):
        for key, val in arrays.items():
            np.save(os.path.join(out, "%s__%s.npy" % (case, key)), np.asarray(val, dtype=np.float64))
            count[0] += 1

    def gpr(case, h, kern, X, Y, want_kinv_resid=True):
        h.gpr_set_data(X, X)
        lml, slots, gnoise, kr = _lml_grad(h, kern._program(X.shape[1]), 0.15, Y, want_kinv_resid)
        save(case, lml=lml, slots=slots, gnoise=gnoise, kinv_resid=kr)

    h = be.Handle(0)
    d = 3
    # ---- the four-primitive kernel
    for name, make in _kernels(gpf, d).items():
        for n in (1, 60, 129, 515, 2100):
            for r in (1, 3):
                X, Y = _data(n, d, r, seed=n + r)
                gpr("gpr_%s_n%d_r%d" % (name, n, r), h, make(), X, Y)
    for name in ("m52_plus_periodic", "rbf_iso"):
        for n in (60, 515):
            X, Y = _data(n, d, 1, seed=n)
            gpr("gpr_nokr_%s_n%d" % (name, n), h, _kernels(gpf, d)[name](), X, Y, want_kinv_resid=False)
    X, Y = _data(129, 26, 1, seed=26)              # 26 feature rows: the feature table goes by pointer
    gpr("gpr_rbf_ard26_n129", h, gpf.kernels.RBF(26, variance=1.2, lengthscales=np.linspace(3.0, 6.0, 26), ARD=True), X, Y)
    # ---- the general kernel
    for n in (60, 515, 1500):
        X, Y = _data(n, d, 1, seed=8 + n)
        gpr("gpr_six_n%d" % n, h, _six(gpf, d), X, Y)
    for act in (False, True):
        for n in (60, 515):
            X, Y = _data(n, d, 1, seed=31 + n)
            gpr("gpr_nkn_act%d_n%d" % (act, n), h, _nkn_case(gpf, d, act)[0], X, Y)
    # ---- kernel-matrix VJPs
    progs = {"four": _kernels(gpf, d)["rbf_times_periodic_plus_white"](), "six": _six(gpf, d), "nkn": _nkn_case(gpf, d, True)[0]}
    for n, m in ((40, 300), (130, None), (257, 70)):
        rng = np.random.default_rng(n)
        X = rng.standard_normal((n, d))
        X2 = None if m is None else rng.standard_normal((m, d))
        W = rng.standard_normal((n, n if m is None else m))
        for name, kern in progs.items():
            prog = kern._program(d)
            save("vjp_%s_n%d_m%s" % (name, n, m), slots=h.kmat_vjp(prog, X, W, X2), grad_X=h.kmat_input_vjp(prog, X, W, X2))
    # ---- inducing-point gradients
    rng = np.random.default_rng(5)
    n, m, k = 200, 130, 2
    X, Y = _data(n, d, k, seed=5)
    Z = X[:m] + 0.05 * rng.standard_normal((m, d))
    kern = _kernels(gpf, d)["m52_plus_periodic"]()
    q_mu = rng.standard_normal((m, k))
    q_sqrt = np.stack([np.tril(0.1 * rng.standard_normal((m, m))) + np.eye(m) for _ in range(k)], axis=2)
    res = h.svgp_elbo_grad(kern._program(d), Z, X, Y, q_mu, q_sqrt, 1e-6, 0.1, white=True, scale=1.0, want_grad_Z=True)
    save("svgp", **{"out%d" % i: v for i, v in enumerate(res)})
    res = h.sgpr_grad(kern._program(d), Z, X, Y[:, :1], 1e-6, 0.1, want_grad_Z=True)
    save("sgpr", **{"out%d" % i: v for i, v in enumerate(res)})
    h.close()

    # ---- block-cyclic column mode: P virtual ranks, every rank's raw sums and the folded gradient
    from gpflowSlim.distributed import gpr_lml_grad_distributed
    from test_gpu_dist_grad import _flat, _kernel, _virtual

    for world, n, nb, kname, r in ((2, 1024, 128, "rbf_ard", 1), (3, 1400, 256, "m52_plus_periodic", 2), (2, 1024, 128, "six", 1)):
        X, Y = _data(n, d, r, seed=world)

        def body(rank, model, comm, hr):
            rows = []
            gather = comm.all_gather_rows
            comm.all_gather_rows = lambda local, counts: rows.append(gather(local, counts)) or rows[-1]
            lml, g = gpr_lml_grad_distributed(model, comm, nb=nb)
            return lml, _flat(g), rows[-1]

        outs, errs = _virtual(world, lambda: gpf.models.GPR(X, Y, _kernel(gpf, kname, d), obs_var=0.1), body)
        assert all(e is None for e in errs), errs
        for rank, (lml, g, rows) in enumerate(outs):
            save("cyclic_%s_P%d_rank%d" % (kname, world, rank), lml=lml, grad=g, rank_sums_and_kinv_resid=rows)
    print("grad_dump: %d arrays in %s" % (count[0], out), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    dump(sys.argv[1])
