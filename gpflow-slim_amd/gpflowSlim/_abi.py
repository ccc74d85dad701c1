"""Python mirror of the C ABI of libgpflowslim_hip.so (include/gpflowslim_hip.h): constants, structs and their makers, the
argument types of every exported function, and the loader.  Nothing here touches a device; gpflowSlim._backend.Handle does.
"""
import ctypes
import importlib.util
import os
import threading

import numpy as np

GPS_MAX_DIMS = 32
GPS_MAX_NODES = 64
GPS_MAX_STACK = 4

# enum gps_kern_op
K_RBF, K_MATERN12, K_MATERN32, K_MATERN52, K_PERIODIC, K_WHITE, K_CONSTANT, K_EXPONENTIAL = 1, 2, 3, 4, 5, 6, 7, 8
K_SQDIST, K_EUCLID = 9, 10
K_RATQUAD, K_LINEAR, K_POLYNOMIAL = 11, 12, 13      # (below K_ADD: network programs find their primitives with op < K_ADD)
K_COSINE, K_ARCCOSINE = 14, 15
K_ADD, K_MUL = 16, 17
K_COREGION = 18                                     # (above K_ADD: not a network primitive)
K_NKN_LINROW, K_NKN_PRODUCT, K_NKN_ACT = 32, 33, 34

_c_double_p = ctypes.POINTER(ctypes.c_double)
_c_int_p = ctypes.POINTER(ctypes.c_int)
_i64 = ctypes.c_int64


class KernNode(ctypes.Structure):
    """gps_kern_node_t"""
    _fields_ = [("op", ctypes.c_int32),
                ("n_dims", ctypes.c_int32),
                ("active_dims", ctypes.c_int32 * GPS_MAX_DIMS),
                ("variance", ctypes.c_double),
                ("period", ctypes.c_double),
                ("lengthscales", ctypes.c_double * GPS_MAX_DIMS)]


class LikDesc(ctypes.Structure):
    """gps_lik_t"""
    _fields_ = [("kind", ctypes.c_int),
                ("n_gh", ctypes.c_int),
                ("param", ctypes.c_double * 4),
                ("gh_x", ctypes.POINTER(ctypes.c_double)),
                ("gh_w", ctypes.POINTER(ctypes.c_double)),
                ("n_edges", ctypes.c_int),
                ("edges", ctypes.POINTER(ctypes.c_double))]


class RffDesc(ctypes.Structure):
    """gps_rff_desc_t"""
    _fields_ = [("kind", ctypes.c_int32),
                ("input_dim", ctypes.c_int32),
                ("n_components", ctypes.c_int32),
                ("variance", ctypes.c_double),
                ("ls", ctypes.POINTER(ctypes.c_double)),
                ("n_ls", ctypes.c_int32),
                ("omega", ctypes.POINTER(ctypes.c_double)),
                ("offset", ctypes.POINTER(ctypes.c_double))]


RFF_RBF, RFF_LINEAR, RFF_CONSTANT, RFF_EXPLICIT = 0, 1, 2, 3


def make_rff(kind, input_dim, n_components, variance=1.0, ls=None, omega=None, offset=None):
    """A gps_rff_desc_t and the arrays it points into (which the caller keeps alive)."""
    d = RffDesc()
    d.kind, d.input_dim, d.n_components, d.variance = int(kind), int(input_dim), int(n_components), float(variance)
    keep = []
    if kind == RFF_RBF:
        ls = np.ascontiguousarray(np.atleast_1d(ls), dtype=np.float64).ravel()
        omega = np.ascontiguousarray(omega, dtype=np.float64)
        offset = np.ascontiguousarray(offset, dtype=np.float64).ravel()
        if omega.shape != (d.input_dim, d.n_components) or offset.shape != (d.n_components,) or ls.size not in (1, d.input_dim):
            raise ValueError("RBF sampler: omega must be [input_dim, n_components], offset [n_components], ls scalar or [input_dim]")
        d.ls, d.n_ls = ls.ctypes.data_as(_c_double_p), int(ls.size)
        d.omega, d.offset = omega.ctypes.data_as(_c_double_p), offset.ctypes.data_as(_c_double_p)
        keep = [ls, omega, offset]
    return d, keep


LIK_MAX_GH = 64
LIK_MAX_EDGES = 32
LIK_MULTICLASS = 5
LIK_ORDINAL = 8


def make_lik(kind, params=(), n_gh=20, edges=None):
    """A gps_lik_t (and the arrays it points into, which the caller keeps alive): kind of include/gpflowslim_hip.h, up to four
    scalar parameters, the Gauss-Hermite rule computed here exactly as the reference does (numpy's hermgauss) and, for
    Ordinal, the table of bin edges (1..32 of them)."""
    params = [float(v) for v in params]
    if edges is not None:
        edges = np.ascontiguousarray(edges, dtype=np.float64).ravel()
        if not 1 <= edges.size <= LIK_MAX_EDGES:
            raise ValueError("the device Ordinal likelihood takes 1..%d bin edges, got %d" % (LIK_MAX_EDGES, edges.size))
    elif int(kind) == LIK_ORDINAL:
        raise ValueError("the Ordinal likelihood needs its bin edges")
    if len(params) > 4:
        raise ValueError("a likelihood has at most four scalar parameters")
    if not 1 <= int(n_gh) <= LIK_MAX_GH:
        raise ValueError("the device likelihoods take 1..%d Gauss-Hermite points, got %d" % (LIK_MAX_GH, n_gh))
    gx, gw = np.polynomial.hermite.hermgauss(int(n_gh))
    gx, gw = np.ascontiguousarray(gx, dtype=np.float64), np.ascontiguousarray(gw, dtype=np.float64)
    d = LikDesc()
    d.kind, d.n_gh = int(kind), int(n_gh)
    for i in range(4):
        d.param[i] = params[i] if i < len(params) else 0.0
    d.gh_x, d.gh_w = gx.ctypes.data_as(_c_double_p), gw.ctypes.data_as(_c_double_p)
    if edges is None:
        return d, (gx, gw)
    d.n_edges, d.edges = int(edges.size), edges.ctypes.data_as(_c_double_p)
    return d, (gx, gw, edges)


def make_program(nodes):
    if len(nodes) == 0 or len(nodes) > GPS_MAX_NODES:
        raise ValueError("kernel program must have 1..%d nodes, got %d" % (GPS_MAX_NODES, len(nodes)))
    arr = (KernNode * len(nodes))()
    for i, nd in enumerate(nodes):
        arr[i] = nd
    return arr


def primitive_node(op, variance, dims=(), lengthscales=(), period=0.0, alpha=None, degree=None):
    """One primitive of a kernel program.  The fields are shared (include/gpflowslim_hip.h): RatQuad keeps its ``alpha`` and
    Polynomial its ``degree`` where Periodic keeps the period; Linear / Polynomial pass their per-dim variances as
    ``lengthscales``, Polynomial its offset as ``variance`` and Linear 1.0."""
    nd = KernNode()
    nd.op = op
    nd.variance = float(variance)
    if alpha is not None:
        period = alpha
    if degree is not None:
        period = degree
    nd.period = float(period)
    k = len(dims)
    if k > GPS_MAX_DIMS:
        raise ValueError("a primitive kernel supports at most %d active dims" % GPS_MAX_DIMS)
    nd.n_dims = k
    if k:
        nd.active_dims[:k] = [int(d) for d in dims]      # (slice assignment: one call instead of one per element -- this runs every step)
    ls = np.asarray(lengthscales, dtype=np.float64).ravel()
    if ls.size == 1 and k > 1:
        nd.lengthscales[:k] = [float(ls[0])] * k
    elif ls.size:
        m = min(ls.size, GPS_MAX_DIMS)
        nd.lengthscales[:m] = ls[:m].tolist()
    return nd


def coregion_node(column, W, kappa):
    """The Coregion primitive (include/gpflowslim_hip.h): the index column in active_dims[0], the rank in active_dims[1], output_dim
    where Periodic keeps the period, W row-major and then kappa where the others keep their lengthscales."""
    W = np.asarray(W, dtype=np.float64)
    kappa = np.asarray(kappa, dtype=np.float64).ravel()
    P, R = W.shape
    if kappa.size != P:
        raise ValueError("Coregion: kappa must have output_dim entries")
    if P * (R + 1) > GPS_MAX_DIMS:
        raise ValueError("Coregion supports at most output_dim * (rank + 1) = %d values, got %d" % (GPS_MAX_DIMS, P * (R + 1)))
    nd = primitive_node(K_COREGION, 1.0, [column], np.concatenate([W.ravel(), kappa]), period=float(P))
    nd.active_dims[1] = int(R)
    return nd


def op_node(op):
    nd = KernNode()
    nd.op = op
    return nd


def psi2_chunking(n, m):
    """(tile edge, lower-triangle tiles, points per chunk, chunks) of the Psi2 kernel for n points and m inducing points
    (csrc/psi.hip: gps_psi2_chunking)."""
    tm = 64 if m > 48 else 32
    t = -(-m // tm)
    nt = t * (t + 1) // 2
    nc = min(max(-(-2048 // nt), 1), -(-n // 64))
    chunk = 64 * -(-n // (64 * nc))
    return tm, nt, chunk, -(-n // chunk)


def psi_sum_chunking(n, m, opt=0):
    """(points per chunk, chunks) of the streamed cross terms of a Sum of RBF parts for n points and m inducing points; opt is the
    value given to gps_psi_sum_set_chunk (0: automatic)  (csrc/psi_sum.hip: gps_psi_sum_chunking)."""
    if opt > 0:
        ch = min(int(opt), 32768)
    else:
        ch = min(max((1 << 22) // (128 * -(-m // 128)), 128), 8192)
    ch = 16 * -(-min(ch, n) // 16)
    return ch, -(-n // ch)


def ms_chunking(n, m):
    """(points per chunk, chunks) of the Multiscale VJP kernels for n points against m inducing features
    (csrc/multiscale.hip: gps_ms_chunking)."""
    mt = -(-m // 64)
    nc = max(min(-(-2048 // mt), -(-n // 64)), 1)
    chunk = 64 * -(-n // (64 * nc))
    return chunk, -(-n // chunk)


def grad_x_slicing(n):
    """(32-row blocks, slices of the column tiles, column tiles per slice) of the walk that d LML / d X makes over the padded
    square of n points: workgroup (block, slice) owns 32 rows and `per` 32-column tiles  (csrc/grad_x.hip: gps_grad_x_slicing;
    the kernels' `per`)."""
    tiles = 128 * -(-n // 128) // 32
    per = -(-tiles // max(1, min(2048 // tiles, tiles, 64)))
    return tiles, -(-tiles // per), per


# ---- argument types of every exported function, in the header's order of parameters (tests/test_host_api.py compares the two)
_int, _dbl, _vp, _str = ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_char_p
_dp, _ip, _i64p = _c_double_p, _c_int_p, ctypes.POINTER(_i64)
_i32p, _u32p, _llp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_longlong)
_prog, _lik, _rff = ctypes.POINTER(KernNode), ctypes.POINTER(LikDesc), ctypes.POINTER(RffDesc)
# (handle, program, nodes, Z, m, ...): the heads that the inducing-point entries share
_SVGP = [_vp, _prog, _int, _dp, _i64, _i64, _dbl, _dp, _i64]                   # h, prog, n, Z, m, d, jitter, X, n
_SPARSE = [_vp, _prog, _int, _dp, _i64, _dp, _i64, _i64, _dbl, _dbl, _dp, _i64]    # h, prog, n, Z, m, X, n, d, jitter, noise, resid, r
_GPLVM = [_vp, _prog, _int, _dp, _i64, _dp, _dp, _i64, _i64]                   # h, prog, n, Z, m, Xmu, Xvar, n, q
_KGPR = [_vp, _prog, _int, _dp, _i64, _i64, _prog, _int, _dp, _i64, _i64, _dp, _dp, _dbl, _dp, _dp, _i32p, _int, _dbl, _dp]
_GPMC = [_vp, _prog, _int, _dp, _i64, _i64, _dbl, _dp, _i64, _dp, _dp, _lik]    # h, prog, n, X, n, d, jitter, V, k, Y, mean, lik

_SIGNATURES = {
    "gps_create": [_int, ctypes.POINTER(_vp)],
    "gps_destroy": [_vp],
    "gps_release_buffers": [_vp],
    "gps_device_info": [_vp, _str, _int, _ip, _i64p, _str, _int],
    "gps_kmat": [_vp, _prog, _int, _dp, _i64, _dp, _i64, _i64, _dbl, _dp],
    "gps_potrf": [_vp, _dp, _i64, _dp, _ip],
    "gps_trsm_lower": [_vp, _dp, _i64, _dp, _i64, _int],
    "gps_gpr_set_data": [_vp, _dp, _i64, _i64],
    "gps_gpr_lml": [_vp, _prog, _int, _dbl, _dp, _i64, _dp, _ip],
    "gps_gpr_lml_grad": [_vp, _prog, _int, _dbl, _dp, _i64, _dp, _dp, _int, _ip, _dp, _dp, _ip],
    "gps_gpr_lml_grad_x": [_vp, _prog, _int, _dbl, _dp, _i64, _dp, _dp, _int, _ip, _dp, _dp, _dp, _ip],
    "gps_gpr_predict": [_vp, _prog, _int, _dbl, _dp, _i64, _dp, _i64, _int, _int, _dp, _dp, _ip],
    "gps_conditional": [_vp, _prog, _int, _dp, _i64, _i64, _dbl, _dp, _i64, _dp, _i64, _dp, _int, _int, _int, _dp, _dp, _ip],
    "gps_base_conditional": [_vp, _dp, _dp, _dp, _i64, _i64, _dp, _i64, _dp, _int, _int, _int, _dp, _dp, _ip],
    "gps_svgp_elbo": _SVGP + [_dp, _dp, _i64, _dp, _int, _int, _dbl, _dbl, _dp, _dp, _dp, _ip],
    "gps_svgp_elbo_grad": _SVGP + [_dp, _dp, _i64, _dp, _int, _int, _dbl, _dbl, _dp, _dp, _int, _ip, _dp, _dp, _dp, _dp, _dp, _ip],
    "gps_lik_varexp": [_vp, _lik, _dp, _dp, _dp, _i64, _i64, _dp, _dp, _dp, _dp],
    "gps_svgp_elbo_lik": _SVGP + [_dp, _dp, _dp, _i64, _dp, _int, _int, _lik, _dbl, _dp, _dp, _dp, _ip],
    "gps_svgp_elbo_lik_grad": _SVGP + [_dp, _dp, _dp, _i64, _dp, _int, _int, _lik, _dbl, _dp, _dp, _int, _ip, _dp, _dp, _dp, _dp,
                                       _dp, _ip],
    "gps_lik_logp": [_vp, _lik, _dp, _dp, _i64, _i64, _dp, _dp, _dp],
    "gps_tri_skinny": [_vp, _dp, _i64, _dp, _i64, _int, _dp],
    "gps_chol_seed": [_vp, _dp, _dp, _i64, _i64, _dp],
    "gps_gpmc_lik": _GPMC + [_dp, _ip],
    "gps_gpmc_lik_grad": _GPMC + [_dp, _dp, _int, _ip, _dp, _dp, _dp, _ip],
    "gps_sgpmc_lik": _SVGP + [_dp, _dp, _dp, _i64, _lik, _i64, _dp, _ip],
    "gps_sgpmc_lik_grad": _SVGP + [_dp, _dp, _dp, _i64, _lik, _i64, _dp, _dp, _int, _ip, _dp, _dp, _dp, _dp, _ip],
    "gps_kmat_vjp": [_vp, _prog, _int, _dp, _i64, _dp, _i64, _i64, _dp, _dp, _int, _ip],
    "gps_kmat_input_vjp": [_vp, _prog, _int, _dp, _i64, _dp, _i64, _i64, _dp, _dp],
    "gps_inducing_scales": [_vp, _dp, _i64, _i64],
    "gps_inducing_scales_grad": [_vp, _dp, _i64, _i64],
    "gps_gauss_kl": [_vp, _dp, _i64, _dp, _i64, _dp, _int, _dp, _ip],
    "gps_sgpr": _SPARSE + [_dp, _i64, _int, _dp, _dp, _dp, _ip],
    "gps_sgpr_grad": _SPARSE + [_dp, _dp, _int, _ip, _dp, _dp, _dp, _ip],
    "gps_fitc_grad": _SPARSE + [_dp, _dp, _int, _ip, _dp, _dp, _dp, _ip],
    "gps_fitc": _SPARSE + [_dp, _i64, _int, _dp, _dp, _dp, _ip],
    "gps_psi_stats": _GPLVM + [_dp, _dp, _dp],
    "gps_psi_sum_set_chunk": [_vp, _i64],
    "gps_bgplvm": _GPLVM + [_dbl, _dbl, _dp, _i64, _dp, _i64, _int, _dp, _dp, _dp, _ip],
    "gps_bgplvm_grad": _GPLVM + [_dbl, _dbl, _dp, _i64, _dp, _dp, _int, _ip, _dp, _dp, _dp, _dp, _ip],
    "gps_psi2_contract": _GPLVM + [_dp, _i64, _dp],
    "gps_uncertain_conditional": _GPLVM + [_dbl, _dp, _i64, _dp, _int, _int, _int, _dp, _dp, _ip],
    "gps_rff_features": [_vp, _rff, _dp, _i64, _dp],
    "gps_rff_gram": [_vp, _rff, _dp, _i64, _dp, _i64, _dp, _dp],
    "gps_rff_lml": [_vp, _rff, _dp, _i64, _dbl, _dp, _i64, _i64, _dp, _ip],
    "gps_rff_lml_grad": [_vp, _rff, _dp, _i64, _dbl, _dp, _i64, _i64, _dp, _dp, _dp, _dp, _dp, _ip],
    "gps_rff_predict": [_vp, _rff, _dp, _i64, _dbl, _dp, _i64, _i64, _dp, _i64, _int, _int, _dp, _dp, _ip],
    "gps_kron_cg": [_vp, _dp, _i64, _dp, _i64, _dp, _dp, _int, _dbl, _dp, _i64p, _dp, _dp],
    "gps_kgpr_lml": _KGPR,
    "gps_kgpr_lml_grad": _KGPR + [_dp, _dp, _dp, _int, _ip, _dp, _int, _ip, _dp],
    "gps_kgpr_predict": [_vp, _prog, _int, _dp, _i64, _i64, _dp, _i64, _prog, _int, _dp, _i64, _i64, _dp, _i64, _dp],
    "gps_sparse_last_terms": [_vp, _dp],
    "gps_profile_enable": [_vp, _int],
    "gps_profile_reset": [_vp],
    "gps_profile_get": [_vp, _str, _i64p, _dp, _dp, _dp],
    "gps_last_stage_ms": [_vp, _dp],
    "gps_set_option": [_vp, _str, _dbl],
    "gps_set_stream": [_vp, _vp, _int],
    "gps_dist_begin": [_vp, _prog, _int, _dbl, _dp, _i64, _int, _int, _i64, _i64p, _i64p],
    "gps_dist_msg_doubles": [_vp, _i64, _i64p],
    "gps_dist_set_comm": [_vp, _vp, _vp],
    "gps_dist_set_comm_bufs": [_vp, ctypes.POINTER(_vp), _int],
    "gps_dist_comm_bufs_needed": [_vp, _ip],
    "gps_device_bytes": [_vp, _i64p],
    "gps_dist_solve_begin": [_vp, _prog, _int, _dp, _i64],
    "gps_dist_solve_pack": [_vp, _i64, _int],
    "gps_dist_grad_begin": [_vp],
    "gps_dist_grad_fwd_apply": [_vp, _i64, _int],
    "gps_dist_grad_bwd_apply": [_vp, _i64, _int],
    "gps_dist_grad_local": [_vp, _prog, _int, _dp, _int, _ip, _dp],
    "gps_dist_grad_fold": [_vp, _prog, _int, _dp, _int, _i64, _dp, _int, _ip, _dp],
    "gps_dist_lml_grad": [_vp, _prog, _int, _dbl, _dp, _i64, _i64, _int, _int, _dp, _dp, _int, _ip, _dp, _dp, _ip],
    "gps_dist_solve_apply": [_vp, _i64, _int],
    "gps_dist_solve_finish": [_vp, _prog, _int, _dp, _dp],
    "gps_dist_lml": [_vp, _prog, _int, _dbl, _dp, _i64, _i64, _int, _int, _dp, _ip],
    "gps_dist_predict": [_vp, _prog, _int, _dp, _i64, _int, _dp, _dp],
    "gps_dist_panel_factor": [_vp, _i64, _int],
    "gps_dist_unpack": [_vp, _i64, _int],
    "gps_dist_update": [_vp, _i64, _i64, _i64, _int],
    "gps_dist_set_bulk_stream": [_vp, _vp],
    "gps_dist_finish": [_vp, _dp, _ip],
    "gps_comm_load": [_str],
    "gps_comm_version": [_ip],
    "gps_comm_unique_id": [_vp, _int],
    "gps_comm_init": [_vp, _int, _int, _vp, _int],
    "gps_comm_destroy": [_vp],
    "gps_comm_abort": [_vp],
    "gps_comm_exchange": [_vp, _vp, _i64, _int, _int, _int],
    "gps_comm_wait": [_vp, _int],
    "gps_comm_allreduce": [_vp, _vp, _i64],
    "gps_comm_install_allreduce": [_vp, _vp, _i64],
    "gps_set_allreduce": [_vp, _vp, _vp, _vp, _i64],
    "gps_allreduce_doubles": [_i64, _i64, _i64p],
    "gps_diag_potrf_base_stamps": [_vp, _int, _dp],
    "gps_diag_mfma_f64": [_vp, _int, _dp, _ip],
    "gps_diag_gemm_nt": [_vp, _int, _int, _i64, _i64, _i64, _dp, _dp, _dp],
    "gps_diag_gemm_nt_batched": [_vp, _int, _int, _i64, _i64, _i64, _i64, _dp, _dp, _dp],
    "gps_diag_trsm512": [_vp, _i64, _int, _int, _int, _dp, _dp],
    "gps_diag_trsm512_stamps": [_vp, _i64, _int, _int, _dp, _llp, _i64],
    "gps_diag_trsm_leaf": [_vp, _i64, _int, _int, _int, _dp, _dp],
    "gps_diag_gpmc_front": [_vp, _int, _dp],
    "gps_diag_set_cu_mask": [_vp, _u32p, _int],
    "gps_diag_gemm_timeline": [_vp, _int, _int, _i64, _i64, _i64, _int, _llp, _i64, _i64p, _dp],
}
EXPORTED_SYMBOLS = sorted(list(_SIGNATURES) + ["gps_last_error", "gps_comm_load_error"])
ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, _i64)      # gps_allreduce_fn


# ---- the loader
def lib_path():
    env = os.environ.get("GPFLOWSLIM_HIP_LIB")
    if env:
        return env
    here = os.path.dirname(os.path.abspath(__file__))
    return os.path.join(os.path.dirname(here), "lib", "libgpflowslim_hip.so")


_lib = None
_lib_lock = threading.Lock()


def _torch_bundled(name):
    """Path of `name` in the lib/ directory an installed PyTorch wheel bundles (found without importing torch), or None."""
    try:
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return None
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", name)
        return cand if os.path.exists(cand) else None
    except Exception:
        return None


def _share_hip_runtime_with_torch():
    """One HIP/HSA runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so (same
    SONAME as /opt/rocm's).  If this library pulled in /opt/rocm's copy first and torch then loaded its
    bundled one, the process would hold two HSA runtimes and the second would see no GPU.  So when a
    torch wheel with a bundled runtime is installed, load that copy first (without importing torch);
    our NEEDED libamdhip64.so.7 then resolves to it by SONAME, whichever of the two is imported first."""
    if os.environ.get("GPFLOWSLIM_NO_TORCH_RUNTIME"):
        return
    cand = _torch_bundled("libamdhip64.so")
    if cand:
        try:
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
        except Exception:
            pass


def load_library():
    """Load the C-ABI library (no GPU needed for this step).  Raises if it is missing."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        path = lib_path()
        if not os.path.exists(path):
            raise RuntimeError(
                "gpflowSlim (MI355X): HIP library not found at %s -- build it with "
                "`make -C gpflow-slim_amd/csrc` (or __graft_entry__.build()). There is no CPU fallback." % path)
        _share_hip_runtime_with_torch()
        lib = ctypes.CDLL(path)
        for name, argtypes in _SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                if os.environ.get("GPFLOWSLIM_HIP_LIB"):      # (an older build named for an A/B: entry points added since are simply absent)
                    continue
                raise
            fn.argtypes = argtypes
            fn.restype = ctypes.c_int
        lib.gps_last_error.argtypes = [ctypes.c_void_p]
        lib.gps_last_error.restype = ctypes.c_char_p
        lib.gps_comm_load_error.argtypes = []
        lib.gps_comm_load_error.restype = ctypes.c_char_p
        _lib = lib
        return lib


def comm_load(path=None):
    """Open librccl for the native collectives.  Default: $GPFLOWSLIM_RCCL_LIB if set, else the copy a PyTorch wheel bundles, if
    there is one (a process that also imports torch then holds ONE RCCL), else the system's."""
    lib = load_library()
    if path is None:
        path = os.environ.get("GPFLOWSLIM_RCCL_LIB") or _torch_bundled("librccl.so")
    rc = lib.gps_comm_load(path.encode() if path else None)
    if rc != 0:
        msg = lib.gps_comm_load_error()
        raise RuntimeError("librccl could not be loaded (%d): %s" % (rc, msg.decode() if msg else ""))


def comm_unique_id():
    """128 opaque bytes from ncclGetUniqueId: rank 0 draws them, every rank passes them to Handle.comm_init."""
    lib = load_library()
    comm_load()
    buf = ctypes.create_string_buffer(128)
    rc = lib.gps_comm_unique_id(buf, 128)
    if rc != 0:
        raise RuntimeError("gps_comm_unique_id failed (%d)" % rc)
    return buf.raw


def comm_version():
    lib = load_library()
    comm_load()
    v = ctypes.c_int(0)
    if lib.gps_comm_version(ctypes.byref(v)) != 0:
        raise RuntimeError("gps_comm_version failed")
    return v.value
