"""One catalogue of the Handle wrappers that run device work, with seeded inputs: what tests/test_gpu_call_order.py (through
tests/_entry_worker.py) calls in every order, what tests/test_gpu_residency.py intrudes with, and what tools/ab_outputs.py takes
its likelihood table and input helpers from.  Host only: numpy, and gpflowSlim for the kernel programs and descriptors (ctypes
structures; nothing here touches the device or loads the library).

An ``Entry`` is one call form of one or more wrappers: name, family, the wrappers it runs (keys of ``WRAPPER_CLASS``), its
residency class (the strongest of its wrappers': "keeps" < "drops_factor" < "drops_all", the three lines of the table in
the docstring of gpflowSlim._backend.Handle) and ``call(h, c)`` on a dictionary of inputs ``c = inputs(set)``.

Input sets (``EXTENTS``):
  small  every extent under one 128 tile: M = 5, N = 70, K = 2, N* = 7, D = 2 (the residency test's sizes)
  edge   the smallest shapes across each padding or grouping edge: M = 129 (two diagonal blocks), N = 257 (three row tiles, partial
         last), K = R = 17 (16 + 1 planes), N* = 130 with full_cov where the entry has it, D = Q = 3, chunk_rows = 128 for SGPMC and
         RFF (three chunks, partial last), 129 random features, psi_sum_set_chunk(64) for the Sum kernel (five chunks), a 17 x 9
         Kronecker grid; psi2n [N, M, M] is asked for on the first 33 points only (4.4 MB instead of 34 MB per output)
  twin   the edge extents with another seed
  big    GPR entries only: N = 2200, which pads to 2304 > small_n_max = 2048 and takes the blocked path

Every factorised matrix of a victim is K + jitter I with K positive semi-definite, jitter = 1e-6 and trace(K) <= 1.3 x 257, so
cond_2 <= 3.4e8 whatever the points (tests/test_entry_catalogue_cpu.py asserts cond_2 <= 1e9, the cap of tests/_many_outputs.py,
in numpy).  ``FAILING`` are calls that the library reports as handled errors: matrices with a negative eigenvalue and one
refused program.
"""
import functools

import numpy as np

SETS = ("small", "edge", "twin")
EXTENTS = {"small": dict(M=5, N=70, K=2, NS=7, D=2, F=6, G1=3, G2=4, P2N=70, chunk_rows=0, psi_chunk=0, full=False),
           "edge": dict(M=129, N=257, K=17, NS=130, D=3, F=129, G1=17, G2=9, P2N=33, chunk_rows=128, psi_chunk=64, full=True)}
EXTENTS["twin"] = EXTENTS["edge"]
EXTENTS["big"] = dict(N=2200, K=1, NS=9, D=2, full=False)
SEEDS = {"small": 20, "edge": 21, "twin": 22, "big": 23}
JITTER, NOISE = 1e-6, 0.1
COND_CAP = 1e9                                                        # tests/_many_outputs.py
KERN = dict(variance=1.3, ls_lo=0.7, ls_hi=0.9)
FAMILIES = ("gpr", "inducing", "sparse", "psi", "mcmc", "lik", "rff", "kron", "primitives")
LIK_KINDS = {"gaussian": 0, "bernoulli": 1, "poisson": 2, "exponential": 3, "student_t": 4, "multiclass": 5, "gamma": 6, "beta": 7,
             "ordinal": 8}
# svgp_elbo_lik_grad takes these whitened: their links are exponentials, and the unwhitened q(u) of the catalogue (a random q_mu and
# q_sqrt through Kuu^-1 at cond_2 ~ 1e8) gives means and variances of f in the thousands, where exp overflows on any device
WHITE_KINDS = ("gaussian", "poisson", "exponential", "gamma", "beta")
RANK = {"keeps": 0, "drops_factor": 1, "drops_all": 2}

# wrapper (with the qualifier the docstring table gives it) -> residency class
WRAPPER_CLASS = {}
for _n in ("gpr_set_data", "conditional", "base_conditional", "svgp_elbo", "svgp_elbo_grad", "svgp_elbo_lik", "svgp_elbo_lik_grad",
           "sgpr", "sgpr_grad", "psi_stats", "psi2_contract", "uncertain_conditional", "bgplvm", "bgplvm_grad", "rff_features",
           "rff_gram", "rff_lml", "rff_lml_grad", "rff_predict(refactor)", "kron_cg", "kgpr_lml", "kgpr_lml_grad", "gpmc_lik",
           "gpmc_lik_grad", "sgpmc_lik", "sgpmc_lik_grad"):
    WRAPPER_CLASS[_n] = "drops_all"
for _n in ("gpr_lml", "gpr_lml_grad", "gpr_predict(refactor)"):
    WRAPPER_CLASS[_n] = "drops_factor"
for _n in ("kmat", "potrf", "trsm_lower", "kmat_vjp", "kmat_input_vjp", "gauss_kl", "lik_varexp", "lik_logp", "tri_skinny", "chol_seed",
           "gpr_predict(refactor=False)", "rff_predict(refactor=False)", "kgpr_predict", "sparse_last_terms", "psi_sum_set_chunk"):
    WRAPPER_CLASS[_n] = "keeps"

_OWN_TESTS = "needs a communicator or a partitioned factor: tests/test_gpu_dist*.py"
_DIAG = "diagnostic probe on device data of its own, no result of the library: tests/test_gpu_kernels.py, tests/test_gpu_diag.py"
_COMM = "collective of the native communicator: tests/test_gpu_comm_native.py, tests/test_gpu_dist_grad_native.py"
EXCLUDED = {
    "close": "destroys the handle",
    "factor_claim": "host-side claim on the resident factor, no device work",
    "device_info": "query, no device work",
    "device_bytes": "query, no device work",
    "profile_enable": "profiling switch, no device work",
    "profile_reset": "profiling switch, no device work",
    "profile_get": "profiling query (the worker reads the three fall-back counters through it)",
    "last_stage_ms": "profiling query",
    "release_buffers": "frees every buffer: the call after it is the cold case, which every entry has",
    "set_option": "option; a changed option changes the arithmetic, so no call order with it is comparable with the cold bytes",
    "set_stream": "option: the caller's stream",
    "set_allreduce": "installs a host callback for the distributed sparse models: tests/test_gpu_dist_sparse.py",
    "allreduce_doubles": "size query, takes no handle",
}
EXCLUDED.update({n: _OWN_TESTS for n in (
    "dist_begin", "dist_msg_doubles", "dist_set_comm", "dist_set_comm_bufs", "dist_comm_bufs_needed", "dist_solve_begin",
    "dist_solve_pack", "dist_solve_apply", "dist_grad_begin", "dist_grad_fwd_apply", "dist_grad_bwd_apply", "dist_grad_local",
    "dist_grad_fold", "dist_lml_grad", "dist_solve_finish", "dist_lml", "dist_predict", "dist_panel_factor", "dist_unpack",
    "dist_update", "dist_set_bulk_stream", "dist_finish")})
EXCLUDED.update({n: _DIAG for n in (
    "diag_mfma_f64", "diag_gemm_nt", "diag_gemm_nt_batched", "diag_trsm_leaf", "diag_trsm512", "diag_trsm512_stamps",
    "diag_set_cu_mask", "diag_gemm_timeline", "diag_gpmc_front")})
EXCLUDED.update({n: _COMM for n in (
    "comm_init", "comm_destroy", "comm_abort", "comm_exchange", "comm_wait", "comm_allreduce", "comm_install_allreduce")})
# the words of the table's last line that are no method names
TABLE_WORDS = {"options": ("set_option", "set_stream", "psi_sum_set_chunk"),
               "profiling": ("profile_enable", "profile_reset", "profile_get", "last_stage_ms", "device_info", "device_bytes")}


def _gpf():
    import gpflowSlim as gpf
    return gpf


# ---- the comparator ------------------------------------------------------------------------------------------------------------------
def same_bytes(a, b):
    """the reference for "no leak" is exact: same shape, same type, same bytes (so -0.0 differs from +0.0 and a NaN only equals
    the same NaN at the same place)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def difference(a, b):
    """what a failure message says of two arrays that are not same_bytes: differing entries and the largest difference"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return "shape %s %s against %s %s" % (a.shape, a.dtype, b.shape, b.dtype)
    if a.dtype.kind in "US":
        return "%r against %r" % (str(a), str(b))
    ua, ub = np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (-1,)), np.ascontiguousarray(b).view(np.uint8).reshape(b.shape + (-1,))
    bad = np.any(ua != ub, axis=-1)
    with np.errstate(invalid="ignore"):
        d = np.abs(a.astype(np.float64) - b.astype(np.float64))[bad]
    finite = d[np.isfinite(d)]
    return "%d of %d entries differ, largest difference %.3g%s" % (
        int(bad.sum()), a.size, finite.max() if finite.size else 0.0,
        ", %d of them not finite on one side" % int((~np.isfinite(d)).sum()) if finite.size < d.size else "")


def flatten(res):
    """what an entry returned, as a list of arrays: tuples and dictionaries (sorted) opened, None left out, a text kept as text"""
    out = []
    if res is None:
        return out
    if isinstance(res, dict):
        for k in sorted(res):
            out += flatten(res[k])
    elif isinstance(res, (tuple, list)):
        for v in res:
            out += flatten(v)
    elif isinstance(res, str):
        out.append(np.array(res))
    else:
        out.append(np.array(res, dtype=np.float64))                  # (a copy, C order; a scalar stays 0-d)
    return out


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def rbf(var, ls, A, B=None):
    B = A if B is None else B
    d = (A[:, None, :] - B[None, :, :]) / ls
    return var * np.exp(-0.5 * (d * d).sum(-1))


def tril_stack(rng, m, k):
    """q_sqrt [M, M, K]: lower triangular with a positive diagonal"""
    L = 0.1 * np.tril(rng.standard_normal((k, m, m)))
    L[:, np.arange(m), np.arange(m)] = 0.5 + rng.random((k, m))
    return np.ascontiguousarray(np.transpose(L, (1, 2, 0)))


def psi_inputs(rng, n, m, q):
    return rng.standard_normal((m, q)), rng.standard_normal((n, q)), np.exp(rng.uniform(np.log(0.05), np.log(0.5), (n, q)))


def lik_table(be, kind, k):
    """(descriptor, targets sampler) of a likelihood kind with fixed parameters"""
    edges = np.linspace(-1.5, 1.5, 4)
    table = {
        "gaussian": (lambda: be.make_lik(0, [0.3]), lambda r, s: r.standard_normal(s)),
        "bernoulli": (lambda: be.make_lik(1, [], 20), lambda r, s: (r.random(s) < 0.5).astype(float)),
        "poisson": (lambda: be.make_lik(2, [1.0]), lambda r, s: r.poisson(2.0, s).astype(float)),
        "exponential": (lambda: be.make_lik(3, []), lambda r, s: r.exponential(1.0, s) + 1e-3),
        "student_t": (lambda: be.make_lik(4, [0.7, 4.0], 20), lambda r, s: r.standard_normal(s)),
        "multiclass": (lambda: be.make_lik(5, [1e-3], 20), lambda r, s: r.integers(0, k, (s[0], 1)).astype(float)),
        "gamma": (lambda: be.make_lik(6, [1.7]), lambda r, s: r.gamma(2.0, 1.0, s) + 1e-3),
        "beta": (lambda: be.make_lik(7, [3.0], 20), lambda r, s: r.beta(2.0, 3.0, s)),
        "ordinal": (lambda: be.make_lik(8, [0.7], 20, edges=edges), lambda r, s: r.integers(0, 5, s).astype(float)),
    }
    make, sampler = table[kind]
    return make(), sampler


def _psi_kernels(gpf, q):
    E = gpf.ekernels
    ls = np.linspace(0.7, 1.2, q)
    return {"single": E.RBF(q, variance=1.4, lengthscales=ls, ARD=True),
            "sum": E.Sum([E.RBF(1, variance=1.7, lengthscales=ls[:1], active_dims=[0], ARD=True),
                          E.RBF(q - 1, variance=1.1, lengthscales=ls[1:], active_dims=list(range(1, q)), ARD=True)])}


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The inputs of one set: seeded, made once, never written to."""
    gpf = _gpf()
    be = gpf._backend
    e = EXTENTS[name]
    g = np.random.default_rng(SEEDS[name])
    c = dict(e)
    c["set"] = name
    N, K, NS, D = e["N"], e["K"], e["NS"], e["D"]
    ls = np.linspace(KERN["ls_lo"], KERN["ls_hi"], D)
    c["ls"] = ls
    c["prog"] = gpf.kernels.RBF(D, variance=KERN["variance"], lengthscales=ls, ARD=True)._program(D)
    c["X"], c["Xs"], c["Y"] = g.standard_normal((N, D)), g.standard_normal((NS, D)), g.standard_normal((N, K))
    c["token"] = ("catalogue", name)
    # the Coregion program: RBF over the D inputs times Coregion(P = 3, rank 2) on a label column
    coreg = gpf.kernels.Coregion(1, 3, 2, active_dims=[D])
    coreg._W.assign(0.5 * g.standard_normal((3, 2)))
    coreg._kappa.assign(0.5 + g.random(3))
    kc = gpf.kernels.RBF(D, variance=1.1, lengthscales=0.8, active_dims=list(range(D))) * coreg
    c["progc"] = kc._program(D + 1)
    c["Xc"] = np.hstack([c["X"], g.integers(0, 3, (N, 1)).astype(float)])
    if name == "big":
        c["Y"] = np.sin(c["X"][:, :1]) + 0.1 * c["Y"]
        return c
    M = e["M"]
    c["Z"] = g.standard_normal((M, D))
    c["W"] = g.standard_normal((N, M))
    c["q_mu"] = g.standard_normal((M, K))
    c["q_sqrt"], c["q_diag"] = tril_stack(g, M, K), 0.5 + g.random((M, K))
    c["Kmm"] = rbf(KERN["variance"], ls, c["Z"]) + JITTER * np.eye(M)
    c["Kms"] = rbf(KERN["variance"], ls, c["Z"], c["Xs"])
    c["Kss"] = rbf(KERN["variance"], ls, c["Xs"])
    c["Kss_diag"] = np.full(NS, KERN["variance"])
    c["L"] = np.linalg.cholesky(c["Kmm"])
    c["Xvar"] = np.exp(g.uniform(np.log(0.05), np.log(0.5), (N, D)))
    c["F"], c["Fvar"] = g.standard_normal((N, K)), np.exp(g.uniform(np.log(1e-3), np.log(2.0), (N, K)))
    c["mean"] = 0.3 * g.standard_normal((N, K))
    c["Vm"], c["Vn"] = 0.5 * g.standard_normal((M, K)), 0.5 * g.standard_normal((N, K))
    c["U"] = g.standard_normal((M, K))
    c["Wc"] = g.standard_normal((K, M, M))
    c["lik"], c["Ylik"] = {}, {}
    for kind in LIK_KINDS:
        c["lik"][kind], sampler = lik_table(be, kind, K)
        c["Ylik"][kind] = sampler(g, (N, K))
    c["labels"] = c["Ylik"]["bernoulli"]
    # random features
    F = e["F"]
    c["rff"] = be.make_rff(be.RFF_RBF, D, F, variance=1.1, ls=np.array([0.8]), omega=g.standard_normal((D, F)),
                           offset=2 * np.pi * g.random(F))
    # the Kronecker grid, two cells missing at most
    G1, G2 = e["G1"], e["G2"]
    c["X1"], c["X2"] = np.linspace(0.0, 1.0, G1)[:, None], np.linspace(0.0, 2.0, G2)[:, None]
    c["Xn1"], c["Xn2"] = g.random((4, 1)), 2.0 * g.random((3, 1))
    c["prog1"] = gpf.kernels.RBF(1, variance=0.9, lengthscales=0.5)._program(1)
    c["prog2"] = gpf.kernels.RBF(1, variance=1.2, lengthscales=0.8)._program(1)
    c["K1"], c["K2"] = rbf(0.9, 0.5, c["X1"]), rbf(1.2, 0.8, c["X2"])
    c["Yg"] = g.standard_normal((G1, G2))
    c["mask"] = np.zeros((G1, G2))
    c["mask"][1, 2] = 1.0
    if G1 > 3:
        c["mask"][G1 - 1, 0] = 1.0
    c["C"] = 1.0 / np.sqrt(0.1 + 1e6 * c["mask"])
    w1, V1 = np.linalg.eigh(c["K1"])
    w2, V2 = np.linalg.eigh(c["K2"])
    o1, o2 = np.argsort(-w1, kind="stable"), np.argsort(-w2, kind="stable")
    c["e1"], c["e2"], c["sel"] = gpf.models.kgpr._select(w1[o1], w2[o2], G1 * G2 - int(c["mask"].sum()))
    c["V1"], c["V2"] = np.ascontiguousarray(V1[:, o1]), np.ascontiguousarray(V2[:, o2])
    # kernel expectations: one RBF, and a Sum of two RBF parts on separate latent dimensions
    for kname, kern in _psi_kernels(gpf, D).items():
        c["psi_" + kname] = kern._psi_program(c["X"])
    c["Xp"], c["Xpvar"] = c["X"][:e["P2N"]].copy(), c["Xvar"][:e["P2N"]].copy()
    return c


def pd_matrices(name):
    """{what: the matrix that a victim of this set factorises}, in numpy"""
    c = inputs(name)
    out = {"K(X) + noise I": rbf(KERN["variance"], c["ls"], c["X"]) + NOISE * np.eye(c["N"])}
    if name != "big":
        out["Kuu + jitter I"] = c["Kmm"]
        out["K(X) + jitter I"] = rbf(KERN["variance"], c["ls"], c["X"]) + JITTER * np.eye(c["N"])
    return out


# ---- entries -------------------------------------------------------------------------------------------------------------------------
class Entry(object):
    __slots__ = ("name", "family", "wrappers", "call", "sets")

    def __init__(self, name, family, wrappers, call, sets=SETS):
        assert family in FAMILIES and all(w in WRAPPER_CLASS for w in wrappers), (name, family, wrappers)
        self.name, self.family, self.wrappers, self.call, self.sets = name, family, tuple(wrappers), call, tuple(sets)

    @property
    def klass(self):
        return max((WRAPPER_CLASS[w] for w in self.wrappers), key=RANK.get)

    @property
    def keeps(self):
        return self.klass == "keeps"


ENTRIES = {}


def _add(name, family, wrappers, call, sets=SETS):
    assert name not in ENTRIES, name
    ENTRIES[name] = Entry(name, family, wrappers, call, sets)


def _with_chunk(call):
    """a Sum-kernel call under psi_sum_set_chunk(c["psi_chunk"]); the option goes back to automatic afterwards"""
    def run(h, c):
        h.psi_sum_set_chunk(c["psi_chunk"])
        try:
            return call(h, c)
        finally:
            h.psi_sum_set_chunk(0)
    return run


def _gpr(call, X="X"):
    def run(h, c):
        h.gpr_set_data(c[X], c["token"] + (X,))
        return call(h, c)
    return run


def _build():
    P, I, S, PS, MC, LK, R, KR, G = "primitives", "inducing", "sparse", "psi", "mcmc", "lik", "rff", "kron", "gpr"
    GSETS = SETS + ("big",)
    # ---- primitives
    _add("kmat", P, ["kmat"], lambda h, c: h.kmat(c["prog"], c["X"], c["Z"]))
    _add("kmat-self", P, ["kmat"], lambda h, c: h.kmat(c["prog"], c["X"], diag_add=NOISE))
    _add("kmat-coregion", P, ["kmat"], lambda h, c: h.kmat(c["progc"], c["Xc"]))
    _add("potrf", P, ["potrf"], lambda h, c: h.potrf(c["Kmm"]))
    _add("trsm_lower", P, ["trsm_lower"], lambda h, c: h.trsm_lower(c["L"], c["q_mu"]))
    _add("trsm_lower-trans", P, ["trsm_lower"], lambda h, c: h.trsm_lower(c["L"], c["q_mu"], trans=True))
    _add("kmat_vjp", P, ["kmat_vjp"], lambda h, c: h.kmat_vjp(c["prog"], c["X"], c["W"], c["Z"]))
    _add("kmat_input_vjp", P, ["kmat_input_vjp"], lambda h, c: h.kmat_input_vjp(c["prog"], c["X"], c["W"], c["Z"]))
    # ---- GPR (each call uploads its own X first: after an intruder nothing is resident)
    _add("gpr_lml", G, ["gpr_set_data", "gpr_lml"], _gpr(lambda h, c: h.gpr_lml(c["prog"], NOISE, c["Y"])), GSETS)
    _add("gpr_lml-r1", G, ["gpr_set_data", "gpr_lml"], _gpr(lambda h, c: h.gpr_lml(c["prog"], NOISE, c["Y"][:, :1])))
    _add("gpr_lml_grad", G, ["gpr_set_data", "gpr_lml_grad"], _gpr(lambda h, c: h.gpr_lml_grad(c["prog"], NOISE, c["Y"])), GSETS)
    _add("gpr_lml_grad-r1", G, ["gpr_set_data", "gpr_lml_grad"], _gpr(lambda h, c: h.gpr_lml_grad(c["prog"], NOISE, c["Y"][:, :1])))
    _add("gpr_lml_grad-coregion", G, ["gpr_set_data", "gpr_lml_grad"],
         _gpr(lambda h, c: h.gpr_lml_grad(c["progc"], NOISE, c["Y"]), "Xc"), GSETS)
    _add("gpr_predict", G, ["gpr_set_data", "gpr_predict(refactor)"],
         _gpr(lambda h, c: h.gpr_predict(c["prog"], NOISE, c["Y"], c["Xs"], full_cov=c["full"])), GSETS)
    _add("gpr_predict-resident", G, ["gpr_set_data", "gpr_lml", "gpr_predict(refactor=False)"],
         _gpr(lambda h, c: (h.gpr_lml(c["prog"], NOISE, c["Y"]),
                            h.gpr_predict(c["prog"], NOISE, c["Y"], c["Xs"], full_cov=c["full"], refactor=False))), GSETS)
    # ---- conditionals, gauss_kl, SVGP with the Gaussian likelihood
    _add("gauss_kl-K", I, ["gauss_kl"], lambda h, c: h.gauss_kl(c["q_mu"], c["q_sqrt"], c["Kmm"]))
    _add("gauss_kl-white", I, ["gauss_kl"], lambda h, c: h.gauss_kl(c["q_mu"], c["q_sqrt"]))
    _add("gauss_kl-K-diag", I, ["gauss_kl"], lambda h, c: h.gauss_kl(c["q_mu"], c["q_diag"], c["Kmm"]))
    for white in (False, True):
        for full in (False, True):
            name = "conditional" + ("-white" if white else "") + ("-full" if full else "")
            _add(name, I, ["conditional"], lambda h, c, white=white, full=full: h.conditional(
                c["prog"], c["Z"], c["Xs"], c["q_mu"], JITTER, q_sqrt=c["q_sqrt"], white=white, full_cov=full))
    _add("conditional-noq", I, ["conditional"], lambda h, c: h.conditional(c["prog"], c["Z"], c["Xs"], c["q_mu"], JITTER))
    _add("base_conditional", I, ["base_conditional"],
         lambda h, c: h.base_conditional(c["Kms"], c["Kmm"], c["Kss_diag"], c["q_mu"], q_sqrt=c["q_sqrt"]))
    _add("base_conditional-white-full", I, ["base_conditional"],
         lambda h, c: h.base_conditional(c["Kms"], c["Kmm"], c["Kss"], c["q_mu"], q_sqrt=c["q_diag"], white=True, full_cov=True))
    _add("svgp_elbo", I, ["svgp_elbo"],
         lambda h, c: h.svgp_elbo(c["prog"], c["Z"], c["X"], c["Y"], c["q_mu"], c["q_sqrt"], JITTER, NOISE))
    _add("svgp_elbo-unwhite-diag", I, ["svgp_elbo"],
         lambda h, c: h.svgp_elbo(c["prog"], c["Z"], c["X"], c["Y"], c["q_mu"], c["q_diag"], JITTER, NOISE, white=False, scale=1.5))
    _add("svgp_elbo_grad", I, ["svgp_elbo_grad"], lambda h, c: h.svgp_elbo_grad(
        c["prog"], c["Z"], c["X"], c["Y"], c["q_mu"], c["q_sqrt"], JITTER, NOISE, white=False, want_grad_Z=True))
    _add("svgp_elbo_grad-white-diag", I, ["svgp_elbo_grad"], lambda h, c: h.svgp_elbo_grad(
        c["prog"], c["Z"], c["X"], c["Y"], c["q_mu"], c["q_diag"], JITTER, NOISE, white=True, scale=1.5))
    # ---- SGPR, FITC
    for fitc in (False, True):
        sfx = "-fitc" if fitc else ""
        _add("sgpr" + sfx, S, ["sgpr"],
             lambda h, c, fitc=fitc: h.sgpr(c["prog"], c["Z"], c["X"], c["Y"], JITTER, NOISE, Xnew=c["Xs"], fitc=fitc))
        _add("sgpr-full" + sfx, S, ["sgpr"], lambda h, c, fitc=fitc: h.sgpr(
            c["prog"], c["Z"], c["X"], c["Y"], JITTER, NOISE, Xnew=c["Xs"], full_cov=True, fitc=fitc))
        _add("sgpr_grad" + sfx, S, ["sgpr_grad"],
             lambda h, c, fitc=fitc: h.sgpr_grad(c["prog"], c["Z"], c["X"], c["Y"], JITTER, NOISE, fitc=fitc))
    _add("sgpr_grad-noZ", S, ["sgpr_grad"],
         lambda h, c: h.sgpr_grad(c["prog"], c["Z"], c["X"], c["Y"], JITTER, NOISE, want_grad_Z=False))
    _add("sparse_last_terms", S, ["sgpr", "sparse_last_terms"],
         lambda h, c: (h.sgpr(c["prog"], c["Z"], c["X"], c["Y"], JITTER, NOISE), h.sparse_last_terms()))
    # ---- kernel expectations, the uncertain conditional, the Bayesian GPLVM: one RBF and a Sum of two parts
    for kname in ("single", "sum"):
        sfx, pk = ("" if kname == "single" else "-sum"), "psi_" + kname
        wrap = (lambda f: f) if kname == "single" else _with_chunk
        extra = [] if kname == "single" else ["psi_sum_set_chunk"]
        _add("psi_stats" + sfx, PS, ["psi_stats"] + extra,
             wrap(lambda h, c, pk=pk: h.psi_stats(c[pk], c["Z"], c["Xp"], c["Xpvar"], True, True, True)))
        _add("psi_stats-12" + sfx, PS, ["psi_stats"] + extra,
             wrap(lambda h, c, pk=pk: h.psi_stats(c[pk], c["Z"], c["X"], c["Xvar"], want_psi1=True, want_psi2=True)))
        _add("psi2_contract" + sfx, PS, ["psi2_contract"] + extra,
             wrap(lambda h, c, pk=pk: h.psi2_contract(c[pk], c["Z"], c["X"], c["Xvar"], c["Wc"])))
        _add("uncertain_conditional" + sfx, PS, ["uncertain_conditional"] + extra, wrap(
            lambda h, c, pk=pk: h.uncertain_conditional(c[pk], c["Z"], c["X"], c["Xvar"], c["q_mu"], c["q_sqrt"], JITTER)))
        _add("uncertain_conditional-white-diag" + sfx, PS, ["uncertain_conditional"] + extra, wrap(
            lambda h, c, pk=pk: h.uncertain_conditional(c[pk], c["Z"], c["X"], c["Xvar"], c["q_mu"], c["q_diag"], JITTER, white=True)))
        # (full_cov_output takes at most 16 outputs: the first 16 of the 17 columns)
        _add("uncertain_conditional-fullout" + sfx, PS, ["uncertain_conditional"] + extra, wrap(
            lambda h, c, pk=pk: h.uncertain_conditional(c[pk], c["Z"], c["X"], c["Xvar"], np.ascontiguousarray(c["q_mu"][:, :16]),
                                                        np.ascontiguousarray(c["q_sqrt"][:, :, :16]), JITTER, full_cov_output=True)))
        _add("bgplvm" + sfx, PS, ["bgplvm"] + extra, wrap(
            lambda h, c, pk=pk: h.bgplvm(c[pk], c["Z"], c["X"], c["Xvar"], c["Y"], JITTER, NOISE, Xnew=c["Xs"])))
        _add("bgplvm-full" + sfx, PS, ["bgplvm"] + extra, wrap(
            lambda h, c, pk=pk: h.bgplvm(c[pk], c["Z"], c["X"], c["Xvar"], c["Y"], JITTER, NOISE, Xnew=c["Xs"], full_cov=True)))
        _add("bgplvm_grad" + sfx, PS, ["bgplvm_grad"] + extra,
             wrap(lambda h, c, pk=pk: h.bgplvm_grad(c[pk], c["Z"], c["X"], c["Xvar"], c["Y"], JITTER, NOISE)))
    # ---- the MCMC models and their kernels on their own
    bern = lambda c: (c["lik"]["bernoulli"], c["Ylik"]["bernoulli"])                                               # noqa: E731
    _add("gpmc_lik", MC, ["gpmc_lik"], lambda h, c: h.gpmc_lik(c["prog"], c["X"], c["Vn"], bern(c)[1], JITTER, bern(c)[0]))
    _add("gpmc_lik-mean", MC, ["gpmc_lik"],
         lambda h, c: h.gpmc_lik(c["prog"], c["X"], c["Vn"], bern(c)[1], JITTER, bern(c)[0], mean=c["mean"]))
    _add("gpmc_lik_grad", MC, ["gpmc_lik_grad"],
         lambda h, c: h.gpmc_lik_grad(c["prog"], c["X"], c["Vn"], bern(c)[1], JITTER, bern(c)[0]))
    _add("gpmc_lik_grad-mean", MC, ["gpmc_lik_grad"],
         lambda h, c: h.gpmc_lik_grad(c["prog"], c["X"], c["Vn"], bern(c)[1], JITTER, bern(c)[0], mean=c["mean"]))
    _add("sgpmc_lik", MC, ["sgpmc_lik"], lambda h, c: h.sgpmc_lik(
        c["prog"], c["Z"], c["X"], bern(c)[1], c["Vm"], JITTER, bern(c)[0], mean=c["mean"], chunk_rows=c["chunk_rows"]))
    _add("sgpmc_lik_grad", MC, ["sgpmc_lik_grad"], lambda h, c: h.sgpmc_lik_grad(
        c["prog"], c["Z"], c["X"], bern(c)[1], c["Vm"], JITTER, bern(c)[0], mean=c["mean"], chunk_rows=c["chunk_rows"],
        want_grad_Z=True))
    _add("sgpmc_lik_grad-nomean", MC, ["sgpmc_lik_grad"], lambda h, c: h.sgpmc_lik_grad(
        c["prog"], c["Z"], c["X"], bern(c)[1], c["Vm"], JITTER, bern(c)[0], chunk_rows=c["chunk_rows"], want_grad_mean=False))
    _add("tri_skinny", MC, ["tri_skinny"], lambda h, c: h.tri_skinny(c["L"], c["q_mu"]))
    _add("tri_skinny-trans", MC, ["tri_skinny"], lambda h, c: h.tri_skinny(c["L"], c["q_mu"], trans=True))
    _add("chol_seed", MC, ["chol_seed"], lambda h, c: h.chol_seed(c["U"], c["Vm"]))
    # ---- likelihoods: one case per kind
    for kind in LIK_KINDS:
        sfx = "" if kind == "bernoulli" else "-" + kind
        _add("lik_varexp" + sfx, LK, ["lik_varexp"],
             lambda h, c, kind=kind: h.lik_varexp(c["lik"][kind], c["F"], c["Fvar"], c["Ylik"][kind], want_grad=True))
        if kind != "multiclass":                                      # (no pointwise form: refused on the host)
            _add("lik_logp" + sfx, LK, ["lik_logp"],
                 lambda h, c, kind=kind: h.lik_logp(c["lik"][kind], c["F"], c["Ylik"][kind], want_grad=True))
        _add("svgp_elbo_lik_grad" + sfx, LK, ["svgp_elbo_lik_grad"], lambda h, c, kind=kind: h.svgp_elbo_lik_grad(
            c["prog"], c["Z"], c["X"], c["Ylik"][kind], c["q_mu"], c["q_sqrt"], JITTER, c["lik"][kind], mean=c["mean"],
            white=kind in WHITE_KINDS, want_grad_Z=True))
    _add("svgp_elbo_lik", LK, ["svgp_elbo_lik"], lambda h, c: h.svgp_elbo_lik(
        c["prog"], c["Z"], c["X"], c["labels"], c["q_mu"], c["q_sqrt"], JITTER, c["lik"]["bernoulli"]))
    _add("svgp_elbo_lik-unwhite", LK, ["svgp_elbo_lik"], lambda h, c: h.svgp_elbo_lik(
        c["prog"], c["Z"], c["X"], c["labels"], c["q_mu"], c["q_diag"], JITTER, c["lik"]["bernoulli"], mean=c["mean"], white=False))
    # ---- random features
    _add("rff_features", R, ["rff_features"], lambda h, c: h.rff_features(c["rff"][0], c["X"]))
    _add("rff_gram", R, ["rff_gram"], lambda h, c: h.rff_gram(c["rff"][0], c["X"], want_diag=True))
    _add("rff_gram-x2", R, ["rff_gram"], lambda h, c: h.rff_gram(c["rff"][0], c["X"], X2=c["Xs"]))
    _add("rff_lml", R, ["rff_lml"], lambda h, c: h.rff_lml(c["rff"][0], c["X"], NOISE, c["Y"], chunk_rows=c["chunk_rows"]))
    _add("rff_lml_grad", R, ["rff_lml_grad"],
         lambda h, c: h.rff_lml_grad(c["rff"][0], c["X"], NOISE, c["Y"], chunk_rows=c["chunk_rows"]))
    _add("rff_predict", R, ["rff_predict(refactor)"], lambda h, c: h.rff_predict(
        c["rff"][0], c["X"], NOISE, c["Y"], c["Xs"], full_cov=c["full"], chunk_rows=c["chunk_rows"]))
    _add("rff_predict-resident", R, ["rff_lml", "rff_predict(refactor=False)"], lambda h, c: (
        h.rff_lml(c["rff"][0], c["X"], NOISE, c["Y"], chunk_rows=c["chunk_rows"]),
        h.rff_predict(c["rff"][0], c["X"], NOISE, c["Y"], c["Xs"], full_cov=c["full"], refactor=False, chunk_rows=c["chunk_rows"])))
    # ---- Kronecker
    kg = lambda c: (c["prog1"], c["X1"], c["prog2"], c["X2"], c["Yg"], c["mask"], NOISE, c["e1"], c["e2"], c["sel"])    # noqa: E731
    _add("kron_cg", KR, ["kron_cg"], lambda h, c: h.kron_cg(c["K1"], c["K2"], c["Yg"], c["C"]))
    _add("kgpr_lml", KR, ["kgpr_lml"], lambda h, c: h.kgpr_lml(*kg(c)))
    _add("kgpr_lml_grad", KR, ["kgpr_lml_grad"], lambda h, c: h.kgpr_lml_grad(*(kg(c) + (c["V1"], c["V2"]))))
    _add("kgpr_predict", KR, ["kgpr_lml", "kgpr_predict"], lambda h, c: (
        h.kgpr_lml(*kg(c)), h.kgpr_predict(c["prog1"], c["X1"], c["Xn1"], c["prog2"], c["X2"], c["Xn2"])))


_build()

# entries that read what an earlier call left resident run as their documented pair; GPS_POISON_ALLOC=2 is invalid for them
# (csrc/gps_common.hpp, DevBuf::ensure) and they take GPS_POISON_ALLOC=1
RESIDENT_READERS = ("gpr_predict-resident", "rff_predict-resident", "kgpr_predict", "sparse_last_terms")
# one fixed edge-shape call per family, the same list for every child
INTRUDERS = ("gpr_lml_grad", "svgp_elbo_grad", "sgpr_grad", "bgplvm_grad-sum", "sgpmc_lik_grad", "svgp_elbo_lik_grad", "rff_lml_grad",
             "kgpr_lml_grad", "potrf")
assert sorted(ENTRIES[n].family for n in INTRUDERS) == sorted(FAMILIES)
assert all(n in ENTRIES for n in RESIDENT_READERS)


def of_family(family):
    return [e for e in ENTRIES.values() if e.family == family]


# ---- calls that fail: handled errors, never a fault --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def failing_inputs():
    gpf = _gpf()
    be = gpf._backend
    g = np.random.default_rng(99)
    m = 129
    G = g.standard_normal((m, m))
    A = G @ G.T + np.eye(m)
    A[100, 100] = -1.0                                                # tests/test_gpu_kernels.py::test_potrf_reports_not_positive_definite
    c = dict(A=A, f=g.standard_normal((m, 2)), q_diag=0.5 + g.random((m, 2)), Kmn=g.standard_normal((m, 7)), Knn=np.full(7, 200.0))
    c["prog1"] = be.make_program([be.primitive_node(be.K_RBF, 1.0, dims=(0, 1), lengthscales=(1.0, 1.0))])
    c["lik"] = be.make_lik(1, [], 20)
    # tests/test_gpu_parity.py::test_gpr_not_positive_definite_raises: every point the same and a "noise variance" of -1
    c["Xdup"], c["Ydup"] = np.zeros((40, 2)), np.ones((40, 1))
    c["Kdup"] = np.ones((40, 40)) - np.eye(40)
    # tests/test_gpu_sgpmc.py::test_sgpmc_not_positive_definite: every inducing point the same; a jitter of -1e-3 where that test has
    # 0, so that the second pivot is negative in exact arithmetic too
    c["Zdup"], c["Xs"], c["V"], c["Ys"] = np.zeros((m, 2)), np.ones((50, 2)), np.ones((m, 1)), np.ones((50, 1))
    c["Kuu_dup"] = np.ones((m, m)) - 1e-3 * np.eye(m)
    # a Coregion node with P (R + 1) = 11 x 3 = 33 > 32 values, made by hand (coregion_node refuses it on the host): the library
    # refuses the program (tests/test_gpu_coregion.py::test_bad_parameters_and_the_value_limit_are_loud)
    vals = np.zeros(32)
    vals[:] = np.concatenate([0.5 * np.ones(22), np.ones(11)])[:32]
    nd = be.primitive_node(be.K_COREGION, 1.0, [2], vals, period=11.0)
    nd.lengthscales[:32] = vals.tolist()
    nd.active_dims[1] = 2
    c["prog_refused"] = be.make_program([nd])
    c["Xlab"] = np.hstack([g.standard_normal((10, 2)), g.integers(0, 3, (10, 1)).astype(float)])
    return c


def _gpr_npd(h, c):
    h.gpr_set_data(c["Xdup"], ("catalogue", "npd"))
    return h.gpr_lml(c["prog1"], -1.0, c["Ydup"])


# name -> (call(h, c), key of the host matrix with a negative eigenvalue or None for a refused program)
FAILING = {
    "gpr_lml-npd": (_gpr_npd, "Kdup"),
    "sgpmc_lik_grad-npd": (lambda h, c: h.sgpmc_lik_grad(c["prog1"], c["Zdup"], c["Xs"], c["Ys"], c["V"], -1e-3, c["lik"]), "Kuu_dup"),
    "potrf-indefinite": (lambda h, c: h.potrf(c["A"]), "A"),
    "base_conditional-indefinite": (lambda h, c: h.base_conditional(c["Kmn"], c["A"], c["Knn"], c["f"]), "A"),
    "gauss_kl-indefinite": (lambda h, c: h.gauss_kl(c["f"], c["q_diag"], c["A"]), "A"),
    "kmat-refused": (lambda h, c: h.kmat(c["prog_refused"], c["Xlab"]), None),
}


# ---- a resident GPR factor that a "keeps" entry must leave alone -----------------------------------------------------------------
RESIDENT = ("resident-gpr", "n200")                                   # (label, set) of its record


@functools.lru_cache(maxsize=None)
def resident_inputs():
    """N = 200 pads to 256 and takes the one-launch small-N path (tests/test_gpu_residency.py)"""
    g = np.random.default_rng(200)
    X = g.standard_normal((200, 2))
    Y = np.sin(X[:, :1]) + 0.1 * g.standard_normal((200, 1))
    prog = _gpf().kernels.RBF(2, variance=1.2, lengthscales=[0.9, 1.4], ARD=True)._program(2)
    return dict(X=X, Y=Y, Xs=g.standard_normal((9, 2)), prog=prog)


def resident_setup(h):
    c = resident_inputs()
    h.gpr_set_data(c["X"], ("catalogue", "resident"))
    return h.gpr_lml(c["prog"], NOISE, c["Y"])


def resident_read(h):
    c = resident_inputs()
    return h.gpr_predict(c["prog"], NOISE, c["Y"], c["Xs"], refactor=False)


# ---- the residency table of Handle's docstring ------------------------------------------------------------------------------------
def residency_table(doc):
    """{class: [names]} of the three lines of the table in the docstring of Handle; a name keeps its (refactor) qualifier and its
    trailing *"""
    import re
    labels = [("drops_all", "drops X and factor"), ("drops_factor", "drops the factor"), ("keeps", "keeps both")]
    pos = [doc.index(text) for _, text in labels] + [len(doc)]
    out = {}
    for i, (klass, text) in enumerate(labels):
        body = doc[pos[i] + len(text):pos[i + 1]]
        body = re.sub(r"\((?!refactor)[^)]*\)", " ", body)             # what a wrapper uses as scratch
        body = re.sub(r"(\w+)\s*/\s*(\w+)\((refactor=False)\)", r"\1(\3), \2(\3)", body)
        names = []
        for tok in body.split(","):
            words = tok.split()
            if words:
                names.append(words[-1])                               # ("the per-panel dist_*" -> "dist_*")
        out[klass] = names
    return out


def resolve(name, methods):
    """the WRAPPER_CLASS keys, EXCLUDED names or Handle methods that a name of the table stands for"""
    import fnmatch
    if name in TABLE_WORDS:
        return list(TABLE_WORDS[name])
    if "(" in name:
        return [name]
    pool = sorted(set(methods) | {k for k in WRAPPER_CLASS if "(" not in k})
    return fnmatch.filter(pool, name) if name.endswith("*") else [name]
