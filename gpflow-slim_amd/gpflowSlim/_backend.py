"""ctypes binding of libgpflowslim_hip.so (C ABI: include/gpflowslim_hip.h).

This is the only place where the Python mirror of the gpflowSlim API touches the device.
There is deliberately no CPU fallback: if the HIP library cannot be loaded, or no GPU is
visible, every compute entry point raises.  The mirror of the ABI itself (constants, structs,
argument types, the loader) is gpflowSlim._abi; its names are re-exported here.
"""
import ctypes
import os
import threading

import numpy as np

from ._abi import (GPS_MAX_DIMS, GPS_MAX_NODES, GPS_MAX_STACK,                                        # noqa: F401
                   K_RBF, K_MATERN12, K_MATERN32, K_MATERN52, K_PERIODIC, K_WHITE, K_CONSTANT, K_EXPONENTIAL,
                   K_SQDIST, K_EUCLID, K_RATQUAD, K_LINEAR, K_POLYNOMIAL, K_COSINE, K_ARCCOSINE, K_ADD, K_MUL, K_COREGION,
                   K_NKN_LINROW, K_NKN_PRODUCT, K_NKN_ACT, KernNode, LikDesc, RffDesc,
                   RFF_RBF, RFF_LINEAR, RFF_CONSTANT, RFF_EXPLICIT, LIK_MAX_GH, LIK_MAX_EDGES, LIK_MULTICLASS, LIK_ORDINAL,
                   make_rff, make_lik, make_program, primitive_node, coregion_node, op_node, psi2_chunking, psi_sum_chunking, ms_chunking, grad_x_slicing,
                   _SIGNATURES, EXPORTED_SYMBOLS, ALLREDUCE_FN, _c_double_p, _c_int_p, _i64,
                   lib_path, load_library, comm_load, comm_unique_id, comm_version)

# Capacity of every gradient-slot buffer handed to the library: its largest limit, GG_MAXSLOT = 640 (csrc/grad_general.hip;
# the specialised kernel's G_MAXSLOT = 160, csrc/grad.hip, is smaller), plus the noise slot that gps_dist_grad_local appends.
SLOT_CAP = 640 + 1

_byref = ctypes.byref
_i32_p = ctypes.POINTER(ctypes.c_int32)
_ll_p = ctypes.POINTER(ctypes.c_longlong)


class NotPositiveDefiniteError(ValueError):
    """Analogue of TensorFlow's InvalidArgumentError from tf.cholesky (models/gpr.py:70)."""


# the wordings of the not-positive-definite report, by family of entry points
_PD_CHOL = "Cholesky decomposition was not successful: leading minor of order %d is not positive definite"   # GPR, RFF, potrf, dist
_PD_ORDER = "Cholesky decomposition was not successful (order %d)"                                           # conditionals, sparse
_PD_KUU = "Kuu + jitter*I is not positive definite (leading minor of order %d)"                              # SVGP
_PD_K = "K is not positive definite (leading minor of order %d)"                                             # gauss_kl


def _raise_if_not_pd(info, wording):
    if info.value > 0:
        raise NotPositiveDefiniteError(wording % info.value)


def _need(cond, msg):
    """Shape errors surface as ValueError before any pointer reaches the library (the reference gets the
    equivalent InvalidArgumentError from the TF op that sees the mismatching shapes)."""
    if not cond:
        raise ValueError(msg)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _need_ordinal_labels(desc, Y):
    """Ordinal: the labels index the table of bin edges, so they are checked here, before any device call (the kernels clamp
    them, which keeps a bad label from reading outside the table but not from being wrong)."""
    if desc.kind == LIK_ORDINAL:
        _need(bool(np.all(np.isfinite(Y)) and np.all(Y == np.floor(Y)) and Y.min() >= 0 and Y.max() <= desc.n_edges),
              "Ordinal labels must be integers in [0, %d] (the number of bin edges)" % desc.n_edges)


def _ptr(a):
    return a.ctypes.data_as(_c_double_p)


def _opt(a):
    return None if a is None else _ptr(a)


class _FactorClaim(object):
    """Handle.factor_claim (a class, not a generator: it is entered once per training step)."""
    __slots__ = ("handle", "key")

    def __init__(self, handle, key):
        self.handle, self.key = handle, key

    def __enter__(self):
        self.handle.factor_key = None

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.handle.factor_key = self.key
        return False


class Handle(object):
    """One GPU, one stream, one set of resident buffers (gps_handle_t).

    Every wrapper reaches the library through ``_call``.  Residency: ``resident_token`` says whose X gps_gpr_set_data
    uploaded, ``factor_key`` what the resident factor / alpha were computed from (callers claim it with ``factor_claim``).
    A wrapper whose C entry goes through begin_inducing_call, drop_resident_factors or gps_gpr_set_data calls
    ``_drop_resident`` before the call; the others leave the claims alone (from the C sources, checked on the device by
    tests/test_gpu_residency.py):

      drops X and factor   release_buffers, gpr_set_data, conditional, base_conditional, svgp_elbo*, sgpr, sgpr_grad,
                           psi_stats, psi2_contract, uncertain_conditional, bgplvm*, rff_features, rff_gram, rff_lml*, rff_predict(refactor), kron_cg, kgpr_lml*,
                           gpmc_lik*, sgpmc_lik*
      drops the factor     gpr_lml, gpr_lml_grad, gpr_predict(refactor), dist_begin, dist_lml, dist_lml_grad
      keeps both           kmat, potrf, trsm_lower, kmat_vjp, kmat_input_vjp (scratch: dXnew, dTmp*), gauss_kl (dS2-dS4),
                           lik_varexp, lik_logp (dLik*), tri_skinny, chol_seed (dTmp*, dStage), gpr_predict /
                           rff_predict(refactor=False), kgpr_predict, sparse_last_terms,
                           the per-panel dist_*, comm_*, diag_*, options, profiling
    """

    def __init__(self, device=None):
        lib = load_library()
        if device is None:
            device = int(os.environ.get("GPFLOWSLIM_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        h = ctypes.c_void_p()
        rc = lib.gps_create(int(device), _byref(h))
        if rc != 0 or not h:
            raise RuntimeError("gpflowSlim (MI355X): gps_create(device=%d) failed with %d -- no usable GPU; "
                               "there is no CPU fallback" % (device, rc))
        self._lib = lib
        self._h = h
        self.device = int(device)
        self.resident_token = None     # identity of the data set held by gps_gpr_set_data
        self.resident_shape = None     # ... and its shape
        self.dist_state = None         # what a PARTITIONED factor on this handle was computed from (gpflowSlim.distributed)
        self.factor_key = None         # what the resident Cholesky factor / alpha were computed from (models/gpr.py)

    @property
    def factor_key(self):
        return self._factor_key

    @factor_key.setter
    def factor_key(self, key):
        # The claims "a factor is resident" live on the HANDLE, next to the factor: every evaluation that touches the
        # factor buffers passes through this setter (factor_claim, _drop_resident), and whatever partitioned factor a
        # distributed evaluation left behind is gone with it -- gpr_lml_distributed records its claim (dist_state) AFTER
        # resetting the key.
        self._factor_key = key
        self.dist_state = None

    def factor_claim(self, key):
        """``with h.factor_claim(key):`` around an evaluation that leaves a factor resident: no claim while it runs, ``key``
        after it came back clean (an exception leaves no claim)."""
        return _FactorClaim(self, key)

    def _drop_resident(self, data=True):
        """The entry about to run drops the resident factor and, unless data=False, the resident X."""
        if data:
            self.resident_token = None
        self.factor_key = None

    def close(self):
        if getattr(self, "_h", None):
            self._lib.gps_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            msg = self._lib.gps_last_error(self._h)
            raise RuntimeError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else ""))

    def _call(self, name, *args):
        """The library's function `name` on this handle; a non-zero return code raises with `name` and gps_last_error."""
        rc = getattr(self._lib, name)(self._h, *args)
        if rc != 0:
            self._check(rc, name)

    @staticmethod
    def _slot_buffer():
        """(gradient slots [SLOT_CAP], the count the library writes); pass SLOT_CAP as the capacity."""
        return np.zeros(SLOT_CAP), ctypes.c_int(0)

    @staticmethod
    def _predict_out(Xnew, r, full_cov):
        """Outputs of a prediction at Xnew [N*, D] (checked by the caller) with r columns: (mean [N*, r], var [N*] or, with
        full_cov, [N*, N*], N*, pointers to Xnew, mean, var).  N* = 0: the empty outputs, which the caller returns without
        a call.  Xnew None (no prediction asked for): None, None, 0 and NULL pointers."""
        if Xnew is None:
            return None, None, 0, None, None, None
        n_new = Xnew.shape[0]
        mean = np.empty((n_new, r))
        var = np.empty((n_new, n_new) if full_cov else (n_new,))
        return mean, var, n_new, _ptr(Xnew), _ptr(mean), _ptr(var)

    # ---- info / measurement
    def device_info(self):
        name = ctypes.create_string_buffer(256)
        arch = ctypes.create_string_buffer(256)
        ncu = ctypes.c_int(0)
        hbm = _i64(0)
        self._call("gps_device_info", name, 256, _byref(ncu), _byref(hbm), arch, 256)
        return {"name": name.value.decode(), "arch": arch.value.decode(), "n_cu": ncu.value, "hbm_bytes": hbm.value}

    def profile_enable(self, on):
        self._call("gps_profile_enable", 1 if on else 0)

    def profile_reset(self):
        self._call("gps_profile_reset")

    def profile_get(self, klass):
        n = _i64(0)
        ms, fl, by = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
        self._call("gps_profile_get", klass.encode(), _byref(n), _byref(ms), _byref(fl), _byref(by))
        return {"launches": n.value, "ms": ms.value, "flops": fl.value, "bytes": by.value}

    def last_stage_ms(self):
        out = np.zeros(5)
        self._call("gps_last_stage_ms", _ptr(out))
        return dict(zip(["kmat", "potrf", "trsv", "predict", "total"], out.tolist()))

    def release_buffers(self):
        """Give the device buffers back (the resident data set and factor are dropped with them)."""
        self._call("gps_release_buffers")
        self._drop_resident()
        self.resident_shape = None

    def set_option(self, key, value):
        self._call("gps_set_option", key.encode(), float(value))

    def set_stream(self, hip_stream, external=True):
        """Run the library's kernels on the caller's HIP stream (integer handle, 0 = legacy default
        stream); external=False restores the handle's own stream."""
        self._call("gps_set_stream", ctypes.c_void_p(hip_stream or 0), 1 if external else 0)

    def device_bytes(self):
        out = _i64(0)
        self._call("gps_device_bytes", _byref(out))
        return out.value

    # ---- block-column distributed factorisation (driven by gpflowSlim.distributed)
    def dist_begin(self, prog, noise_var, resid, nparts, part, nb):
        resid = _f64(resid)
        npan, mx = _i64(0), _i64(0)
        self._drop_resident(data=False)
        self._call("gps_dist_begin", prog, len(prog), float(noise_var), _ptr(resid), resid.shape[1], int(nparts), int(part),
                   int(nb), _byref(npan), _byref(mx))
        return npan.value, mx.value

    def dist_msg_doubles(self, j):
        out = _i64(0)
        self._call("gps_dist_msg_doubles", int(j), _byref(out))
        return out.value

    def dist_set_comm(self, ptr0, ptr1):
        self._call("gps_dist_set_comm", ctypes.c_void_p(ptr0), ctypes.c_void_p(ptr1))

    def dist_set_comm_bufs(self, ptrs):
        arr = (ctypes.c_void_p * len(ptrs))(*[ctypes.c_void_p(p) for p in ptrs])
        self._call("gps_dist_set_comm_bufs", arr, len(ptrs))

    def dist_comm_bufs_needed(self):
        out = ctypes.c_int(0)
        self._call("gps_dist_comm_bufs_needed", _byref(out))
        return out.value

    def dist_solve_begin(self, prog, Xnew):
        Xnew = _f64(Xnew)
        self._call("gps_dist_solve_begin", prog, len(prog), _ptr(Xnew), Xnew.shape[0])

    def dist_solve_pack(self, j, buf):
        self._call("gps_dist_solve_pack", int(j), int(buf))

    def dist_solve_apply(self, j, buf):
        self._call("gps_dist_solve_apply", int(j), int(buf))

    def dist_grad_begin(self):
        self._call("gps_dist_grad_begin")

    def dist_grad_fwd_apply(self, j, buf):
        self._call("gps_dist_grad_fwd_apply", int(j), int(buf))

    def dist_grad_bwd_apply(self, j, buf):
        self._call("gps_dist_grad_bwd_apply", int(j), int(buf))

    def dist_grad_local(self, prog, n, r):
        """gps_dist_grad_local: (raw sums [n_slots + 1] -- the noise-variance sum last --, K_y^-1 resid [n, r])."""
        sums, ns = self._slot_buffer()
        kinv_resid = np.empty((n, r))
        self._call("gps_dist_grad_local", prog, len(prog), _ptr(sums), SLOT_CAP, _byref(ns), _ptr(kinv_resid))
        return sums[:ns.value + 1].copy(), kinv_resid

    def dist_grad_fold(self, prog, rank_sums):
        """gps_dist_grad_fold over rank_sums [P, n_slots + 1]: (grad_slots, grad_noise)."""
        rank_sums = _f64(rank_sums)
        slots, ns = self._slot_buffer()
        gnoise = ctypes.c_double(0)
        self._call("gps_dist_grad_fold", prog, len(prog), _ptr(rank_sums), rank_sums.shape[0], rank_sums.shape[1],
                   _ptr(slots), SLOT_CAP, _byref(ns), _byref(gnoise))
        return slots[:ns.value].copy(), gnoise.value

    def dist_lml_grad(self, prog, noise_var, resid, nb, lookahead, exchange_mode):
        """gps_dist_lml_grad: (lml, grad_slots, grad_noise, K_y^-1 resid), the whole distributed LML + gradient inside the
        library (native communicator required)."""
        resid = _f64(resid)
        n, r = resid.shape
        lml, gnoise, info = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int(0)
        slots, ns = self._slot_buffer()
        kinv_resid = np.empty((n, r))
        self._drop_resident(data=False)
        self._call("gps_dist_lml_grad", prog, len(prog), float(noise_var), _ptr(resid), r, int(nb), int(lookahead),
                   int(exchange_mode), _byref(lml), _ptr(slots), SLOT_CAP, _byref(ns), _byref(gnoise), _ptr(kinv_resid),
                   _byref(info))
        _raise_if_not_pd(info, _PD_CHOL)
        return lml.value, slots[:ns.value].copy(), gnoise.value, kinv_resid

    def dist_solve_finish(self, prog, n_new, r):
        mean = np.empty((n_new, max(r, 1)))
        var = np.empty(n_new)
        self._call("gps_dist_solve_finish", prog, len(prog), _ptr(mean), _ptr(var))
        return mean[:, :r], var

    def dist_lml(self, prog, noise_var, resid, nb, lookahead, exchange_mode):
        """gps_dist_lml: the whole block-column factorisation driven inside the library (native communicator required)."""
        resid = _f64(resid)
        lml, info = ctypes.c_double(0), ctypes.c_int(0)
        self._drop_resident(data=False)
        self._call("gps_dist_lml", prog, len(prog), float(noise_var), _ptr(resid), resid.shape[1], int(nb), int(lookahead),
                   int(exchange_mode), _byref(lml), _byref(info))
        _raise_if_not_pd(info, _PD_CHOL)
        return lml.value

    def dist_predict(self, prog, Xnew, r, exchange_mode):
        Xnew = _f64(Xnew)
        n_new = Xnew.shape[0]
        mean = np.empty((n_new, max(r, 1)))
        var = np.empty(n_new)
        self._call("gps_dist_predict", prog, len(prog), _ptr(Xnew) if n_new else None, n_new, int(exchange_mode),
                   _ptr(mean) if n_new else None, _ptr(var) if n_new else None)
        return mean[:, :r], var

    def dist_panel_factor(self, j, buf):
        self._call("gps_dist_panel_factor", int(j), int(buf))

    def dist_unpack(self, j, buf):
        self._call("gps_dist_unpack", int(j), int(buf))

    def dist_update(self, j, c_lo, c_hi, lane=0):
        self._call("gps_dist_update", int(j), int(c_lo), int(c_hi), int(lane))

    def dist_set_bulk_stream(self, hip_stream):
        self._call("gps_dist_set_bulk_stream", ctypes.c_void_p(hip_stream) if hip_stream else None)

    def dist_finish(self):
        lml, info = ctypes.c_double(0), ctypes.c_int(0)
        self._call("gps_dist_finish", _byref(lml), _byref(info))
        _raise_if_not_pd(info, _PD_CHOL)
        return lml.value

    # ---- diagnostics
    def diag_mfma_f64(self, waves_per_simd=1):
        tf = ctypes.c_double(0)
        ok = ctypes.c_int(0)
        self._call("gps_diag_mfma_f64", waves_per_simd, _byref(tf), _byref(ok))
        return tf.value, bool(ok.value)

    def diag_gemm_nt(self, op, lower, A, B, C):
        A, B = _f64(A), _f64(B)
        C = np.array(C, dtype=np.float64, order="C", copy=True)
        m, k = A.shape
        n = B.shape[0]
        assert B.shape[1] == k and C.shape == (m, n)
        self._call("gps_diag_gemm_nt", op, int(lower), m, n, k, _ptr(A), _ptr(B), _ptr(C))
        return C

    def diag_gemm_nt_batched(self, op, tri, A, B, C):
        """A [batch, m, k], B [batch, n, k], C [batch, m, n]; tri: 0 none, 1 A upper, 2 A lower, 3 B lower triangular."""
        A, B = _f64(A), _f64(B)
        C = np.array(C, dtype=np.float64, order="C", copy=True)
        batch, m, k = A.shape
        n = B.shape[1]
        assert B.shape == (batch, n, k) and C.shape == (batch, m, n)
        self._call("gps_diag_gemm_nt_batched", op, int(tri), batch, m, n, k, _ptr(A), _ptr(B), _ptr(C))
        return C

    def diag_trsm_leaf(self, m, mode, upper=False, reps=50):
        """(microseconds per launch, scaled residual) of one 128-column solve leaf on m rows."""
        us, res = ctypes.c_double(0), ctypes.c_double(0)
        self._call("gps_diag_trsm_leaf", int(m), int(mode), int(bool(upper)), int(reps), _byref(us), _byref(res))
        return us.value, res.value

    def diag_trsm512(self, m, backward=False, panel=True, reps=20):
        """(microseconds per 512-column solve of m rows, max |one launch - launch by launch|)."""
        us, diff = ctypes.c_double(0), ctypes.c_double(0)
        self._call("gps_diag_trsm512", int(m), int(bool(backward)), int(bool(panel)), int(reps), _byref(us), _byref(diff))
        return us.value, diff.value

    def diag_trsm512_stamps(self, m, backward=False, reps=5):
        """(microseconds per solve, int64 array [m / 64, 32] of phase stamps) of the one-launch 512-column solve."""
        nb = int(m) // 32                # (64 or 32 rows per workgroup: the unused tail stays 0)
        buf = np.zeros((nb, 32), dtype=np.int64)
        us = ctypes.c_double(0)
        self._call("gps_diag_trsm512_stamps", int(m), int(bool(backward)), int(reps), _byref(us), buf.ctypes.data_as(_ll_p), nb)
        return us.value, buf

    def diag_set_cu_mask(self, words):
        arr = (ctypes.c_uint32 * len(words))(*[int(w) & 0xffffffff for w in words])
        self._call("gps_diag_set_cu_mask", arr, len(words))

    def diag_gemm_timeline(self, op, lower, m, n, k, reps=5, cap_blocks=1 << 17):
        """(ms per launch, stamps [nblocks, 6] = start, end (100 MHz ticks), HW_ID, XCC_ID, K-loop start, K-loop end) on random device data."""
        st = np.zeros((cap_blocks, 6), dtype=np.int64)
        nb, ms = ctypes.c_int64(), ctypes.c_double()
        self._call("gps_diag_gemm_timeline", op, int(lower), m, n, k, reps, st.ctypes.data_as(_ll_p), cap_blocks, _byref(nb),
                   _byref(ms))
        return ms.value, st[:nb.value]

    # ---- kernels.K and its vector-Jacobian products
    def kmat(self, prog, X, X2=None, diag_add=0.0):
        X = _f64(X)
        n, d = X.shape
        m = n
        if X2 is not None:
            X2 = _f64(X2)
            if X2.shape[1] != d:
                raise ValueError("X and X2 must have the same number of columns")
            m = X2.shape[0]
        out = np.empty((n, m))
        self._call("gps_kmat", prog, len(prog), _ptr(X), n, _opt(X2), 0 if X2 is None else m, d, float(diag_add), _ptr(out))
        return out

    @staticmethod
    def _kmat_vjp_args(X, W, X2):
        """X [N, D], the cotangent W [N, M] and X2 [M, D] or None (then M = N): (X, W, X2, n, m, d)."""
        X, W = _f64(X), _f64(W)
        n, d = X.shape
        m = n
        if X2 is not None:
            X2 = _f64(X2)
            _need(X2.ndim == 2 and X2.shape[1] == d, "X2 must be [M, %d]" % d)
            m = X2.shape[0]
        _need(W.shape == (n, m), "W must be [N, M]")
        return X, W, X2, n, m, d

    def kmat_input_vjp(self, prog, X, W, X2=None):
        """d/dX sum_ij W[i, j] k(X_i, X2_j)  [N, D]: reverse mode through kern.K(X, X2) with respect to the points X
        (X2 None: K(X, X), both arguments move)."""
        X, W, X2, n, m, d = self._kmat_vjp_args(X, W, X2)
        g = np.zeros((n, d))
        self._call("gps_kmat_input_vjp", prog, len(prog), _ptr(X), n, _opt(X2), m, d, _ptr(W), _ptr(g))
        return g

    def kmat_vjp(self, prog, X, W, X2=None):
        """sum_ij W[i, j] d k(X_i, X2_j) / d(kernel parameter slot): reverse mode through kern.K(X, X2)."""
        X, W, X2, n, m, d = self._kmat_vjp_args(X, W, X2)
        slots, ns = self._slot_buffer()
        self._call("gps_kmat_vjp", prog, len(prog), _ptr(X), n, _opt(X2), m, d, _ptr(W), _ptr(slots), SLOT_CAP, _byref(ns))
        return slots[:ns.value].copy()

    # ---- linear algebra on host matrices
    def potrf(self, A):
        A = _f64(A)
        n = A.shape[0]
        if A.shape != (n, n):
            raise ValueError("cholesky needs a square matrix")
        L = np.empty_like(A)
        info = ctypes.c_int(0)
        self._call("gps_potrf", _ptr(A), n, _ptr(L), _byref(info))
        _raise_if_not_pd(info, _PD_CHOL)
        return L

    def trsm_lower(self, L, B, trans=False):
        L = _f64(L)
        B = np.array(B, dtype=np.float64, order="C", copy=True)
        squeeze = B.ndim == 1
        if squeeze:
            B = B[:, None].copy()
        n = L.shape[0]
        if L.shape != (n, n) or B.shape[0] != n:
            raise ValueError("triangular solve: shape mismatch")
        self._call("gps_trsm_lower", _ptr(L), n, _ptr(B), B.shape[1], 1 if trans else 0)
        return B[:, 0] if squeeze else B

    # ---- GPR
    def gpr_set_data(self, X, token):
        X = _f64(X)
        _need(X.ndim == 2 and X.shape[0] > 0 and X.shape[1] > 0, "GPR needs a non-empty X [N, D]")
        self.resident_shape = X.shape
        self._drop_resident()
        self._call("gps_gpr_set_data", _ptr(X), X.shape[0], X.shape[1])
        self.resident_token = token

    def gpr_lml(self, prog, noise_var, resid):
        resid = _f64(resid)
        shape = self.resident_shape
        _need(shape is not None and resid.ndim == 2 and resid.shape[0] == shape[0], "Y must have one row per row of X")
        lml, info = ctypes.c_double(0), ctypes.c_int(0)
        self._drop_resident(data=False)
        self._call("gps_gpr_lml", prog, len(prog), float(noise_var), _ptr(resid), resid.shape[1], _byref(lml), _byref(info))
        _raise_if_not_pd(info, _PD_CHOL)
        return lml.value

    def gpr_lml_grad(self, prog, noise_var, resid, want_grad_X=False):
        """(lml, grad_slots, grad_noise, K_y^-1 resid)  -- see gps_gpr_lml_grad in the header.  want_grad_X: d LML / d X [N, D]
        as a fifth item (gps_gpr_lml_grad_x; the chain through a mean function is the caller's)."""
        resid = _f64(resid)
        shape = self.resident_shape
        _need(shape is not None and resid.ndim == 2 and resid.shape[0] == shape[0] and resid.shape[1] > 0,
              "Y must have one row per row of X")
        n, r = shape[0], resid.shape[1]          # the C side reads and writes n = rows of the resident X
        lml, gnoise, info = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int(0)
        slots, ns = self._slot_buffer()
        kinv_resid = np.empty((n, r))
        self._drop_resident(data=False)
        if want_grad_X:
            grad_X = np.empty((n, shape[1]))
            self._call("gps_gpr_lml_grad_x", prog, len(prog), float(noise_var), _ptr(resid), r, _byref(lml), _ptr(slots), SLOT_CAP,
                       _byref(ns), _byref(gnoise), _ptr(kinv_resid), _ptr(grad_X), _byref(info))
            _raise_if_not_pd(info, _PD_CHOL)
            return lml.value, slots[:ns.value].copy(), gnoise.value, kinv_resid, grad_X
        self._call("gps_gpr_lml_grad", prog, len(prog), float(noise_var), _ptr(resid), r, _byref(lml), _ptr(slots), SLOT_CAP,
                   _byref(ns), _byref(gnoise), _ptr(kinv_resid), _byref(info))
        _raise_if_not_pd(info, _PD_CHOL)
        return lml.value, slots[:ns.value].copy(), gnoise.value, kinv_resid

    def gpr_predict(self, prog, noise_var, resid, Xnew, full_cov=False, refactor=True):
        resid = _f64(resid)
        Xnew = _f64(Xnew)
        shape = self.resident_shape
        _need(Xnew.ndim == 2 and shape is not None and Xnew.shape[1] == shape[1],
              "Xnew must be [N*, %s]" % (shape[1] if shape else "D"))
        _need(resid.ndim == 2 and resid.shape[0] == shape[0], "Y must have one row per row of X")
        r = resid.shape[1]
        mean, var, n_new, xp, mp_, vp = self._predict_out(Xnew, r, full_cov)
        if n_new == 0:                       # nothing to predict: the reference returns empty tensors
            return mean, var
        info = ctypes.c_int(0)
        if refactor:
            self._drop_resident(data=False)
        self._call("gps_gpr_predict", prog, len(prog), float(noise_var), _ptr(resid), r, xp, n_new, 1 if full_cov else 0,
                   1 if refactor else 0, mp_, vp, _byref(info))
        _raise_if_not_pd(info, _PD_CHOL)
        return mean, var

    # ---- GPR on explicit features (kernel_kitchen_sink.py; models/gpr.py:63-67, 86-117)
    def _rff_x(self, desc, X):
        """X checked against the descriptor, for the entries that rebuild the feature factor (they drop what is resident)."""
        X = _f64(X)
        _need(X.ndim == 2 and X.shape[0] > 0 and X.shape[1] == desc.input_dim, "X must be [N, %d] with N > 0" % desc.input_dim)
        self._drop_resident()
        return X

    def rff_features(self, desc, X):
        """gps_rff_features: the feature map of the descriptor applied to X, host [N, F]."""
        if np.shape(X)[0] == 0:
            return np.empty((0, desc.n_components))
        X = self._rff_x(desc, X)
        out = np.empty((X.shape[0], desc.n_components))
        self._call("gps_rff_features", _byref(desc), _ptr(X), X.shape[0], _ptr(out))
        return out

    def rff_gram(self, desc, X, X2=None, want_K=True, want_diag=False):
        """gps_rff_gram: (Phi(X) Phi(X2)^T or None, row sums of squares of Phi(X) or None)."""
        X = self._rff_x(desc, X)
        n = X.shape[0]
        n2 = n
        if X2 is not None:
            X2 = _f64(X2)
            _need(X2.ndim == 2 and X2.shape[0] > 0 and X2.shape[1] == desc.input_dim, "X2 must be [N2, %d]" % desc.input_dim)
            n2 = X2.shape[0]
        K = np.empty((n, n2)) if want_K else None
        kd = np.empty(n) if want_diag else None
        self._call("gps_rff_gram", _byref(desc), _ptr(X), n, _opt(X2), n2, _opt(K), _opt(kd))
        return K, kd

    def rff_lml(self, desc, X, noise_var, resid, chunk_rows=0):
        X, resid = self._rff_x(desc, X), _f64(resid)
        _need(resid.ndim == 2 and resid.shape[0] == X.shape[0] and resid.shape[1] > 0, "Y must have one row per row of X")
        lml, info = ctypes.c_double(0), ctypes.c_int(0)
        self._call("gps_rff_lml", _byref(desc), _ptr(X), X.shape[0], float(noise_var), _ptr(resid), resid.shape[1],
                   int(chunk_rows), _byref(lml), _byref(info))
        _raise_if_not_pd(info, _PD_CHOL)
        return lml.value

    def rff_lml_grad(self, desc, X, noise_var, resid, chunk_rows=0):
        """(lml, d / d variance, d / d ls [n_ls], d / d noise_var, K_y^-1 resid [N, R]) -- gps_rff_lml_grad."""
        X, resid = self._rff_x(desc, X), _f64(resid)
        _need(resid.ndim == 2 and resid.shape[0] == X.shape[0] and resid.shape[1] > 0, "Y must have one row per row of X")
        lml, gvar, gnoise, info = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int(0)
        gls = np.zeros(max(int(desc.n_ls), 1))
        kinv_resid = np.empty(resid.shape)
        self._call("gps_rff_lml_grad", _byref(desc), _ptr(X), X.shape[0], float(noise_var), _ptr(resid), resid.shape[1],
                   int(chunk_rows), _byref(lml), _byref(gvar), _ptr(gls), _byref(gnoise), _ptr(kinv_resid), _byref(info))
        _raise_if_not_pd(info, _PD_CHOL)
        return lml.value, gvar.value, gls[:int(desc.n_ls)].copy(), gnoise.value, kinv_resid

    def rff_predict(self, desc, X, noise_var, resid, Xnew, full_cov=False, refactor=True, chunk_rows=0):
        resid, Xnew = _f64(resid), _f64(Xnew)
        _need(Xnew.ndim == 2 and Xnew.shape[1] == desc.input_dim, "Xnew must be [N*, %d]" % desc.input_dim)
        r = resid.shape[1]
        mean, var, n_new, xp, mp_, vp = self._predict_out(Xnew, r, full_cov)
        if n_new == 0:
            return mean, var
        X = self._rff_x(desc, X) if refactor else _f64(X)
        _need(resid.ndim == 2 and resid.shape[0] == X.shape[0] and r > 0, "Y must have one row per row of X")
        info = ctypes.c_int(0)
        self._call("gps_rff_predict", _byref(desc), _ptr(X), X.shape[0], float(noise_var), _ptr(resid), r, int(chunk_rows),
                   xp, n_new, 1 if full_cov else 0, 1 if refactor else 0, mp_, vp, _byref(info))
        _raise_if_not_pd(info, _PD_CHOL)
        return mean, var

    # ---- Kronecker GP regression (conjugate_gradient.py, models/kgpr.py)
    def kron_cg(self, K1, K2, B, C, max_iter=100, tol=1e-6):
        """gps_kron_cg: cgsolver on (I + C o (K1 (C o .) K2)) x = B with every vector the [m, n] matrix it came from:
        (x [m, n], iterations, the last r^T r, delta = tol * |B|)."""
        K1, K2, B, C = _f64(K1), _f64(K2), _f64(B), _f64(C)
        _need(K1.ndim == 2 and K1.shape[0] == K1.shape[1] and K2.ndim == 2 and K2.shape[0] == K2.shape[1],
              "K1 and K2 must be square")
        m, n = K1.shape[0], K2.shape[0]
        _need(B.shape == (m, n) and C.shape == (m, n), "b and C must be [%d, %d]" % (m, n))
        x = np.zeros((m, n))
        iters, rr, delta = _i64(0), ctypes.c_double(0), ctypes.c_double(0)
        self._drop_resident()
        self._call("gps_kron_cg", _ptr(K1), m, _ptr(K2), n, _ptr(B), _ptr(C), int(max_iter), float(tol), _ptr(x), _byref(iters),
                   _byref(rr), _byref(delta))
        return x, iters.value, rr.value, delta.value

    @staticmethod
    def _kgpr_args(X1, X2, Y, mask, e1, e2, sel):
        X1, X2, Y, mask, e1, e2 = _f64(X1), _f64(X2), _f64(Y), _f64(mask), _f64(e1), _f64(e2)
        sel = np.ascontiguousarray(sel, dtype=np.int32)
        _need(X1.ndim == 2 and X2.ndim == 2 and X1.shape[0] > 0 and X2.shape[0] > 0 and X1.shape[1] > 0 and X2.shape[1] > 0,
              "KGPR needs non-empty X1 [m, d1] and X2 [n, d2]")
        m, n = X1.shape[0], X2.shape[0]
        _need(Y.shape == (m, n) and mask.shape == (m, n), "Y and mask must be [%d, %d]" % (m, n))
        _need(e1.shape == (m,) and e2.shape == (n,) and sel.shape == (m, 2), "e1 [m], e2 [n] and the ranges [m, 2] do not fit the grid")
        return X1, X2, Y, mask, e1, e2, sel, m, n

    @staticmethod
    def _kgpr_out(out):
        return dict(lml=out[0], quadratic=out[1], logdet=out[2], iters=int(out[3]), rr=out[4], delta=out[5])

    def kgpr_lml(self, prog1, X1, prog2, X2, Y, mask, noise_var, e1, e2, sel, max_iter=100, tol=1e-6):
        """gps_kgpr_lml: dict(lml, quadratic, logdet, iters, rr, delta); alpha stays resident for kgpr_predict."""
        X1, X2, Y, mask, e1, e2, sel, m, n = self._kgpr_args(X1, X2, Y, mask, e1, e2, sel)
        out = np.zeros(6)
        self._drop_resident()
        self._call("gps_kgpr_lml", prog1, len(prog1), _ptr(X1), m, X1.shape[1], prog2, len(prog2), _ptr(X2), n, X2.shape[1],
                   _ptr(Y), _ptr(mask), float(noise_var), _ptr(e1), _ptr(e2), sel.ctypes.data_as(_i32_p), int(max_iter),
                   float(tol), _ptr(out))
        return self._kgpr_out(out)

    def kgpr_lml_grad(self, prog1, X1, prog2, X2, Y, mask, noise_var, e1, e2, sel, V1, V2, max_iter=100, tol=1e-6):
        """gps_kgpr_lml_grad: (the dict of kgpr_lml, slots of prog1, slots of prog2, d / d noise_var)."""
        X1, X2, Y, mask, e1, e2, sel, m, n = self._kgpr_args(X1, X2, Y, mask, e1, e2, sel)
        V1, V2 = _f64(V1), _f64(V2)
        _need(V1.shape == (m, m) and V2.shape == (n, n), "V1 must be [m, m] and V2 [n, n]")
        out = np.zeros(6)
        (s1, n1), (s2, n2) = self._slot_buffer(), self._slot_buffer()
        gnoise = ctypes.c_double(0)
        self._drop_resident()
        self._call("gps_kgpr_lml_grad", prog1, len(prog1), _ptr(X1), m, X1.shape[1], prog2, len(prog2), _ptr(X2), n, X2.shape[1],
                   _ptr(Y), _ptr(mask), float(noise_var), _ptr(e1), _ptr(e2), sel.ctypes.data_as(_i32_p), int(max_iter),
                   float(tol), _ptr(out), _ptr(V1), _ptr(V2), _ptr(s1), SLOT_CAP, _byref(n1), _ptr(s2), SLOT_CAP, _byref(n2),
                   _byref(gnoise))
        return self._kgpr_out(out), s1[:n1.value].copy(), s2[:n2.value].copy(), gnoise.value

    def kgpr_predict(self, prog1, X1, Xnew1, prog2, X2, Xnew2):
        """gps_kgpr_predict: K1u^T alpha K2u [m*, n*] from the alpha the last kgpr_lml / kgpr_lml_grad left resident."""
        X1, X2, Xnew1, Xnew2 = _f64(X1), _f64(X2), _f64(Xnew1), _f64(Xnew2)
        _need(X1.ndim == 2 and X2.ndim == 2 and X1.shape[0] > 0 and X2.shape[0] > 0, "KGPR needs non-empty X1 [m, d1] and X2 [n, d2]")
        _need(Xnew1.ndim == 2 and Xnew1.shape[1] == X1.shape[1], "Xnew1 must be [m*, %d]" % X1.shape[1])
        _need(Xnew2.ndim == 2 and Xnew2.shape[1] == X2.shape[1], "Xnew2 must be [n*, %d]" % X2.shape[1])
        mean = np.empty((Xnew1.shape[0], Xnew2.shape[0]))
        if mean.size == 0:
            return mean
        self._call("gps_kgpr_predict", prog1, len(prog1), _ptr(X1), X1.shape[0], X1.shape[1], _ptr(Xnew1), Xnew1.shape[0],
                   prog2, len(prog2), _ptr(X2), X2.shape[0], X2.shape[1], _ptr(Xnew2), Xnew2.shape[0], _ptr(mean))
        return mean

    # ---- SGPR
    def sgpr(self, prog, Z, X, resid, jitter, noise_var, Xnew=None, full_cov=False, want_bound=True, fitc=False, scales=None):
        """gps_sgpr (Titsias bound) or, with fitc=True, gps_fitc (Snelson & Ghahramani); scales [M, D]: Z are Multiscale
        features of these widths."""
        Z, X, resid = _f64(Z), _f64(X), _f64(resid)
        m, d = Z.shape
        n, r = resid.shape
        _need(X.ndim == 2 and X.shape == (n, d) and m > 0 and n > 0, "sparse GP regression needs Z [M, D], X [N, D], Y [N, R]")
        bound, info = ctypes.c_double(0), ctypes.c_int(0)
        if Xnew is not None:
            Xnew = _f64(Xnew)
            _need(Xnew.ndim == 2 and Xnew.shape[1] == d, "Xnew must be [N*, %d]" % d)
        mean, var, n_new, xp, mp_, vp = self._predict_out(Xnew, r, full_cov)
        if Xnew is not None and n_new == 0:
            return 0.0, mean, var
        self._drop_resident()
        self._arm_scales(scales, Z)
        self._call("gps_fitc" if fitc else "gps_sgpr", prog, len(prog), _ptr(Z), m, _ptr(X), n, d, float(jitter),
                   float(noise_var), _ptr(resid), r, xp, n_new, 1 if full_cov else 0, _byref(bound) if want_bound else None,
                   mp_, vp, _byref(info))
        _raise_if_not_pd(info, _PD_ORDER)
        return bound.value, mean, var

    def sgpr_grad(self, prog, Z, X, resid, jitter, noise_var, want_grad_Z=True, fitc=False, scales=None):
        """(bound, grad_slots, grad_noise, d/d mean(X) [N, R], grad_Z [M, D] or None) of the SGPR bound -- gps_sgpr_grad -- or,
        with fitc=True, of the FITC log-likelihood -- gps_fitc_grad; gradients with respect to the constrained values.  scales
        (Multiscale features): one more item at the end, grad_scales [M, D]."""
        Z, X, resid = _f64(Z), _f64(X), _f64(resid)
        m, d = Z.shape
        n, r = resid.shape
        _need(X.ndim == 2 and X.shape == (n, d) and m > 0 and n > 0, "sparse GP regression needs Z [M, D], X [N, D], Y [N, R]")
        bound, gnoise, info = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int(0)
        slots, ns = self._slot_buffer()
        g_mean = np.zeros((n, r))
        g_Z = np.zeros((m, d))
        self._drop_resident()
        armed = self._arm_scales(scales, Z)
        self._call("gps_fitc_grad" if fitc else "gps_sgpr_grad", prog, len(prog), _ptr(Z), m, _ptr(X), n, d, float(jitter),
                   float(noise_var), _ptr(resid), r, _byref(bound), _ptr(slots), SLOT_CAP, _byref(ns), _byref(gnoise),
                   _ptr(g_mean), _ptr(g_Z) if want_grad_Z else None, _byref(info))
        _raise_if_not_pd(info, _PD_ORDER)
        out = (bound.value, slots[:ns.value].copy(), gnoise.value, g_mean, (g_Z if want_grad_Z else None))
        return out + (self._scales_grad(m, d),) if armed else out

    def sparse_last_terms(self):
        """sum log diag LB, tr(A A^T), sum c^2, Kdiag constant, sum log nu of the last sgpr() call."""
        out = np.zeros(5)
        self._call("gps_sparse_last_terms", _ptr(out))
        return dict(sum_log_diag_LB=out[0], tr_AAT=out[1], sum_c2=out[2], kdiag=out[3], sum_log_nu=out[4])

    # ---- Bayesian GPLVM and the kernel expectations behind it (csrc/psi.hip, csrc/gps_gplvm.hip)
    @staticmethod
    def _psi_args(Z, Xmu, Xvar):
        Z, Xmu, Xvar = _f64(Z), _f64(Xmu), _f64(Xvar)
        _need(Z.ndim == 2 and Xmu.ndim == 2 and Z.shape[1] == Xmu.shape[1] and Z.shape[0] > 0 and Xmu.shape[0] > 0,
              "the kernel expectations need Z [M, Q] and Xmu [N, Q]")
        if Xvar.ndim == 3:
            raise NotImplementedError("full [N, Q, Q] covariances of q(x) are not implemented: pass the diagonals as [N, Q]")
        _need(Xvar.shape == Xmu.shape, "Xvar must be [N, Q] like Xmu")
        return Z, Xmu, Xvar

    def psi_sum_set_chunk(self, chunk):
        """gps_psi_sum_set_chunk: points per chunk of the streamed cross terms of a Sum of RBF parts (0: automatic; see
        psi_sum_chunking)."""
        self._call("gps_psi_sum_set_chunk", int(chunk))

    def psi_stats(self, prog, Z, Xmu, Xvar, want_psi1=False, want_psi2=False, want_psi2n=False):
        """gps_psi_stats: (Psi1 [N, M], Psi2 [M, M], psi2n [N, M, M]) of one RBF kernel, or of a Sum of RBF kernels on pairwise
        disjoint latent dimensions (cross terms included), under q(x_n) = N(Xmu_n, diag Xvar_n);
        None for what was not asked for."""
        Z, Xmu, Xvar = self._psi_args(Z, Xmu, Xvar)
        (m, q), n = Z.shape, Xmu.shape[0]
        p1 = np.empty((n, m)) if want_psi1 else None
        p2 = np.empty((m, m)) if want_psi2 else None
        p2n = np.empty((n, m, m)) if want_psi2n else None
        self._drop_resident()
        self._call("gps_psi_stats", prog, len(prog), _ptr(Z), m, _ptr(Xmu), _ptr(Xvar), n, q, _opt(p1), _opt(p2), _opt(p2n))
        return p1, p2, p2n

    def psi2_contract(self, prog, Z, Xmu, Xvar, W):
        """gps_psi2_contract: out [N, B], out[n, b] = sum_{m, m'} eKzxKxz[n, m, m'] W[b, m, m'] for W [B, M, M] (or one [M, M]
        matrix: out [N]); only the symmetric part of each W counts.  eKzxKxz [N, M, M] is never formed; prog as for psi_stats."""
        Z, Xmu, Xvar = self._psi_args(Z, Xmu, Xvar)
        W = _f64(W)
        (m, q), n = Z.shape, Xmu.shape[0]
        single = W.ndim == 2
        if single:
            W = W[None]
        _need(W.ndim == 3 and W.shape[0] > 0 and W.shape[1:] == (m, m), "W must be [B, M, M] or [M, M]")
        W = _f64(W)
        out = np.empty((n, W.shape[0]))
        self._drop_resident()
        self._call("gps_psi2_contract", prog, len(prog), _ptr(Z), m, _ptr(Xmu), _ptr(Xvar), n, q, _ptr(W), W.shape[0], _ptr(out))
        return out[:, 0].copy() if single else out

    def uncertain_conditional(self, prog, Z, Xmu, Xvar, q_mu, q_sqrt, jitter, white=False, full_cov_output=False):
        """gps_uncertain_conditional: (fmean [N, K], fvar [N, K] or, full_cov_output, [N, K, K]) of f(x_n), x_n ~ N(Xmu_n, diag
        Xvar_n), under q(u) = N(q_mu, q_sqrt q_sqrt^T) at Z; prog as for psi_stats, q_sqrt [M, K] or [M, M, K] as conditional."""
        Z, Xmu, Xvar = self._psi_args(Z, Xmu, Xvar)
        q_mu = _f64(q_mu)
        (m, q), n = Z.shape, Xmu.shape[0]
        _need(q_mu.ndim == 2 and q_mu.shape[0] == m and q_mu.shape[1] > 0, "q_mu must be [M, K]")
        k = q_mu.shape[1]
        qs, qnd = self._prep_q_sqrt(q_sqrt)
        if qs is None:
            raise ValueError("uncertain_conditional needs q_sqrt")
        self._check_q_sqrt(qs, qnd, m, k)
        fmean = np.empty((n, k))
        fvar = np.empty((n, k, k) if full_cov_output else (n, k))
        info = ctypes.c_int(0)
        self._drop_resident()
        self._call("gps_uncertain_conditional", prog, len(prog), _ptr(Z), m, _ptr(Xmu), _ptr(Xvar), n, q, float(jitter), _ptr(q_mu),
                   k, _ptr(qs), qnd, 1 if white else 0, 1 if full_cov_output else 0, _ptr(fmean), _ptr(fvar), _byref(info))
        _raise_if_not_pd(info, _PD_ORDER)
        return fmean, fvar

    def bgplvm(self, prog, Z, Xmu, Xvar, Y, jitter, noise_var, Xnew=None, full_cov=False, want_bound=True):
        """gps_bgplvm: (bound without the KL term, mean [N*, R], var [N*] or [N*, N*]); prog as for psi_stats."""
        Z, Xmu, Xvar = self._psi_args(Z, Xmu, Xvar)
        Y = _f64(Y)
        (m, q), n = Z.shape, Xmu.shape[0]
        _need(Y.ndim == 2 and Y.shape[0] == n, "Y must be [N, R]")
        r = Y.shape[1]
        bound, info = ctypes.c_double(0), ctypes.c_int(0)
        if Xnew is not None:
            Xnew = _f64(Xnew)
            _need(Xnew.ndim == 2 and Xnew.shape[1] == q, "Xnew must be [N*, %d]" % q)
        mean, var, n_new, xp, mp_, vp = self._predict_out(Xnew, r, full_cov)
        if Xnew is not None and n_new == 0:
            return 0.0, mean, var
        self._drop_resident()
        self._call("gps_bgplvm", prog, len(prog), _ptr(Z), m, _ptr(Xmu), _ptr(Xvar), n, q, float(jitter), float(noise_var),
                   _ptr(Y), r, xp, n_new, 1 if full_cov else 0, _byref(bound) if want_bound else None, mp_, vp, _byref(info))
        _raise_if_not_pd(info, _PD_ORDER)
        return bound.value, mean, var

    def bgplvm_grad(self, prog, Z, Xmu, Xvar, Y, jitter, noise_var):
        """gps_bgplvm_grad: (bound without the KL term, grad_slots, grad_noise, grad_Z [M, Q], grad_Xmu [N, Q], grad_Xvar [N, Q]),
        gradients with respect to the constrained values; the slots are (variance, lengthscales) part by part for a Sum."""
        Z, Xmu, Xvar = self._psi_args(Z, Xmu, Xvar)
        Y = _f64(Y)
        (m, q), n = Z.shape, Xmu.shape[0]
        _need(Y.ndim == 2 and Y.shape[0] == n, "Y must be [N, R]")
        bound, gnoise, info = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int(0)
        slots, ns = self._slot_buffer()
        g_Z, g_mu, g_var = np.zeros((m, q)), np.zeros((n, q)), np.zeros((n, q))
        self._drop_resident()
        self._call("gps_bgplvm_grad", prog, len(prog), _ptr(Z), m, _ptr(Xmu), _ptr(Xvar), n, q, float(jitter), float(noise_var),
                   _ptr(Y), Y.shape[1], _byref(bound), _ptr(slots), SLOT_CAP, _byref(ns), _byref(gnoise), _ptr(g_Z), _ptr(g_mu),
                   _ptr(g_var), _byref(info))
        _raise_if_not_pd(info, _PD_ORDER)
        return bound.value, slots[:ns.value].copy(), gnoise.value, g_Z, g_mu, g_var

    # ---- native collectives (csrc/comm_rccl.hip; driven by gpflowSlim.distributed.RcclComm)
    def comm_init(self, rank, world, unique_id):
        buf = ctypes.create_string_buffer(bytes(unique_id), len(unique_id))
        self._call("gps_comm_init", int(rank), int(world), buf, len(unique_id))

    def comm_destroy(self):
        self._call("gps_comm_destroy")

    def comm_abort(self):
        """ncclCommAbort: leave the communicator without waiting for the peers (a failing rank's way out)."""
        self._call("gps_comm_abort")

    def comm_exchange(self, dev_ptr, count, root, mode, slot):
        self._call("gps_comm_exchange", ctypes.c_void_p(dev_ptr), int(count), int(root), int(mode), int(slot))

    def comm_wait(self, slot):
        self._call("gps_comm_wait", int(slot))

    def comm_allreduce(self, dev_ptr, count):
        self._call("gps_comm_allreduce", ctypes.c_void_p(dev_ptr), int(count))

    def comm_install_allreduce(self, dev_ptr, capacity_doubles):
        self._call("gps_comm_install_allreduce", ctypes.c_void_p(dev_ptr), int(capacity_doubles))

    def set_allreduce(self, callback, dev_ptr, capacity_doubles):
        """gps_set_allreduce: `callback` an ALLREDUCE_FN instance (kept alive by the caller) or None to remove it."""
        cb = ctypes.cast(callback, ctypes.c_void_p) if callback is not None else None
        self._call("gps_set_allreduce", cb, None, ctypes.c_void_p(dev_ptr) if dev_ptr else None, int(capacity_doubles))

    def allreduce_doubles(self, m, r):
        out = _i64(0)
        self._check(self._lib.gps_allreduce_doubles(int(m), int(r), _byref(out)), "gps_allreduce_doubles")   # (takes no handle)
        return out.value

    # ---- Multiscale inducing features (features.Multiscale): the one-shot feature scales of the next inducing-point entry
    def _arm_scales(self, scales, Z):
        """gps_inducing_scales: the widths [M, D] of a Multiscale feature for the entry called next (the library clears them when
        that entry returns, whatever it returns).  scales None: nothing happens."""
        if scales is None:
            return False
        scales = _f64(scales)
        _need(scales.shape == Z.shape, "the scales of a Multiscale feature must have the shape of Z")
        self._call("gps_inducing_scales", _ptr(scales), Z.shape[0], Z.shape[1])
        return True

    def _scales_grad(self, m, d):
        """gps_inducing_scales_grad: d / d scales [M, D] of the gradient entry that just consumed the armed scales."""
        out = np.zeros((m, d))
        self._call("gps_inducing_scales_grad", _ptr(out), m, d)
        return out

    def _ms_kmat(self, prog, Z, scales, X2=None, jitter=0.0):
        """Kuu + jitter I [M, M] (X2 None) or Kuf [M, N] against the points X2 of a Multiscale feature (features.py:123-147)."""
        Z = _f64(Z)
        m, d = Z.shape
        if X2 is not None:
            X2 = _f64(X2)
            _need(X2.ndim == 2 and X2.shape[1] == d, "X2 must be [N, %d]" % d)
        out = np.empty((m, m if X2 is None else X2.shape[0]))
        if out.size == 0:
            return out
        self._arm_scales(scales, Z)
        self._call("gps_kmat", prog, len(prog), _ptr(Z), m, _opt(X2), 0 if X2 is None else X2.shape[0], d, float(jitter), _ptr(out))
        return out

    def _ms_kmat_vjp(self, prog, Z, scales, W, X2=None):
        """(grad_slots, grad_Z [M, D], grad_scales [M, D]) of sum_ij W_ij K_ij for K = Kuf (W [M, N], X2 the points) or
        K = Kuu (W [M, M] as given, X2 None) of a Multiscale feature."""
        Z, W = _f64(Z), _f64(W)
        m, d = Z.shape
        if X2 is not None:
            X2 = _f64(X2)
        nc = m if X2 is None else X2.shape[0]
        _need(W.shape == (m, nc), "W must be [M, N]")
        slots, ns = self._slot_buffer()
        g_Z = np.zeros((m, d))
        self._arm_scales(scales, Z)
        self._call("gps_kmat_vjp", prog, len(prog), _ptr(Z), m, _opt(X2), nc, d, _ptr(W), _ptr(slots), SLOT_CAP, _byref(ns))
        self._arm_scales(scales, Z)
        self._call("gps_kmat_input_vjp", prog, len(prog), _ptr(Z), m, _opt(X2), nc, d, _ptr(W), _ptr(g_Z))
        return slots[:ns.value].copy(), g_Z, self._scales_grad(m, d)

    # ---- conditionals, SVGP
    @staticmethod
    def _prep_q_sqrt(q_sqrt):
        if q_sqrt is None:
            return None, 0
        q_sqrt = np.asarray(q_sqrt, dtype=np.float64)
        if q_sqrt.ndim == 2:
            return _f64(q_sqrt), 2
        if q_sqrt.ndim == 3:
            return _f64(np.transpose(q_sqrt, (2, 0, 1))), 3       # [m,m,k] -> [k,m,m]
        raise ValueError("Bad dimension for q_sqrt: %s" % str(q_sqrt.ndim))

    @staticmethod
    def _check_q_sqrt(q, qnd, m, k):
        if q is None:
            return
        _need(q.shape == ((m, k) if qnd == 2 else (k, m, m)), "q_sqrt must be [M, K] or [M, M, K]")

    @staticmethod
    def _q_sqrt_grad(g_q, qnd):
        """The library's gradient with respect to q_sqrt, back in the caller's layout."""
        return np.ascontiguousarray(np.transpose(g_q, (1, 2, 0))) if qnd == 3 else g_q      # [k, m, m] -> [m, m, k]

    def _cond_outputs(self, n_new, k, full_cov):
        fmean = np.empty((n_new, k))
        fvar = np.empty((k, n_new, n_new) if full_cov else (n_new, k))
        return fmean, fvar

    def conditional(self, prog, Z, Xnew, f, jitter, q_sqrt=None, white=False, full_cov=False, scales=None):
        """gps_conditional; scales [M, D]: Z are Multiscale features of these widths (features.Multiscale)."""
        Z, Xnew, f = _f64(Z), _f64(Xnew), _f64(f)
        m, d = Z.shape
        _need(Xnew.ndim == 2 and Xnew.shape[1] == d, "Xnew must be [N*, %d]" % d)
        _need(f.ndim == 2 and f.shape[0] == m and m > 0, "f must be [M, K] with one row per row of X")
        n_new, k = Xnew.shape[0], f.shape[1]
        q, qnd = self._prep_q_sqrt(q_sqrt)
        self._check_q_sqrt(q, qnd, m, k)
        fmean, fvar = self._cond_outputs(n_new, k, full_cov)
        if n_new == 0:
            return fmean, (np.empty((0, 0, k)) if full_cov else fvar)
        info = ctypes.c_int(0)
        self._drop_resident()
        self._arm_scales(scales, Z)
        self._call("gps_conditional", prog, len(prog), _ptr(Z), m, d, float(jitter), _ptr(Xnew), n_new, _ptr(f), k, _opt(q), qnd,
                   1 if white else 0, 1 if full_cov else 0, _ptr(fmean), _ptr(fvar), _byref(info))
        _raise_if_not_pd(info, _PD_ORDER)
        if full_cov:
            fvar = np.ascontiguousarray(np.transpose(fvar, (1, 2, 0)))     # [n,n,k]  conditionals.py:119
        return fmean, fvar

    def base_conditional(self, Kmn, Kmm, Knn, f, q_sqrt=None, white=False, full_cov=False):
        Kmn, Kmm, Knn, f = _f64(Kmn), _f64(Kmm), _f64(Knn), _f64(f)
        _need(Kmn.ndim == 2 and f.ndim == 2, "Kmn must be [M, N] and f [M, K]")
        m, n_new = Kmn.shape
        k = f.shape[1]
        _need(Kmm.shape == (m, m) and f.shape[0] == m and m > 0, "Kmm must be [M, M] and f [M, K]")
        _need(Knn.shape == ((n_new, n_new) if full_cov else (n_new,)),
              "Knn must be [N, N] with full_cov and [N] without")
        q, qnd = self._prep_q_sqrt(q_sqrt)
        self._check_q_sqrt(q, qnd, m, k)
        fmean, fvar = self._cond_outputs(n_new, k, full_cov)
        if n_new == 0:
            return fmean, (np.empty((0, 0, k)) if full_cov else fvar)
        info = ctypes.c_int(0)
        self._drop_resident()
        self._call("gps_base_conditional", _ptr(Kmn), _ptr(Kmm), _ptr(Knn), m, n_new, _ptr(f), k, _opt(q), qnd,
                   1 if white else 0, 1 if full_cov else 0, _ptr(fmean), _ptr(fvar), _byref(info))
        _raise_if_not_pd(info, _PD_ORDER)
        if full_cov:
            fvar = np.ascontiguousarray(np.transpose(fvar, (1, 2, 0)))
        return fmean, fvar

    def _svgp_args(self, Z, X, q_mu, q_sqrt):
        """What every SVGP entry takes, checked: (Z [M, D], X [N, D], q_mu [M, K], q_sqrt in the library's layout and its
        ndim, M, D, N, K).  The targets are the caller's to check."""
        Z, X, q_mu = _f64(Z), _f64(X), _f64(q_mu)
        _need(Z.ndim == 2 and X.ndim == 2 and Z.shape[1] == X.shape[1], "Z [M, D] and X [N, D] must share D")
        m, d = Z.shape
        n = X.shape[0]
        _need(q_mu.ndim == 2 and q_mu.shape[0] == m, "q_mu must be [M, K]")
        k = q_mu.shape[1]
        _need(m > 0 and n > 0 and k > 0, "empty SVGP problem")
        q, qnd = self._prep_q_sqrt(q_sqrt)
        _need(q is not None, "SVGP needs q_sqrt")
        self._check_q_sqrt(q, qnd, m, k)
        return Z, X, q_mu, q, qnd, m, d, n, k

    def svgp_elbo(self, prog, Z, X, yres, q_mu, q_sqrt, jitter, noise_var, white=True, scale=1.0, scales=None):
        """(elbo, kl, sum of variational expectations) of models/svgp.py:108-125 for the Gaussian likelihood."""
        Z, X, q_mu, q, qnd, m, d, n, k = self._svgp_args(Z, X, q_mu, q_sqrt)
        yres = _f64(yres)
        _need(yres.shape == (n, k), "Y - mean must be [N, K] with K = number of latent functions")
        elbo, kl, ve, info = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int(0)
        self._drop_resident()
        self._arm_scales(scales, Z)
        self._call("gps_svgp_elbo", prog, len(prog), _ptr(Z), m, d, float(jitter), _ptr(X), n, _ptr(yres), _ptr(q_mu), k,
                   _ptr(q), qnd, 1 if white else 0, float(noise_var), float(scale), _byref(elbo), _byref(kl), _byref(ve),
                   _byref(info))
        _raise_if_not_pd(info, _PD_KUU)
        return elbo.value, kl.value, ve.value

    def svgp_elbo_grad(self, prog, Z, X, yres, q_mu, q_sqrt, jitter, noise_var, white=True, scale=1.0, want_grad_Z=False,
                       scales=None):
        """(elbo, grad_slots, grad_noise, grad_q_mu [M, K], grad_q_sqrt shaped like q_sqrt, d/d mean(X) [N, K]) -- gradients
        w.r.t. the constrained values, either parametrisation (gps_svgp_elbo_grad); want_grad_Z: a seventh item, the gradient
        with respect to the inducing inputs [M, D]; scales (Multiscale features): one more item at the end, grad_scales [M, D]."""
        Z, X, q_mu, q, qnd, m, d, n, k = self._svgp_args(Z, X, q_mu, q_sqrt)
        yres = _f64(yres)
        _need(yres.shape == (n, k), "Y - mean must be [N, K] with K = number of latent functions")
        elbo, gnoise, info = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int(0)
        slots, ns = self._slot_buffer()
        g_qmu, g_q, g_mean, g_Z = np.zeros((m, k)), np.zeros_like(q), np.zeros((n, k)), np.zeros((m, d))
        self._drop_resident()
        armed = self._arm_scales(scales, Z)
        self._call("gps_svgp_elbo_grad", prog, len(prog), _ptr(Z), m, d, float(jitter), _ptr(X), n, _ptr(yres), _ptr(q_mu), k,
                   _ptr(q), qnd, 1 if white else 0, float(noise_var), float(scale), _byref(elbo), _ptr(slots), SLOT_CAP,
                   _byref(ns), _byref(gnoise), _ptr(g_qmu), _ptr(g_q), _ptr(g_mean), _ptr(g_Z) if want_grad_Z else None,
                   _byref(info))
        _raise_if_not_pd(info, _PD_KUU)
        out = (elbo.value, slots[:ns.value].copy(), gnoise.value, g_qmu, self._q_sqrt_grad(g_q, qnd), g_mean)
        out = out + (g_Z,) if want_grad_Z else out
        return out + (self._scales_grad(m, d),) if armed else out

    def lik_varexp(self, lik, Fmu, Fvar, Y, want_grad=False):
        """Sum over points and latents of the variational expectations of a device likelihood (``lik`` from make_lik) for
        q(f) = N(Fmu, Fvar), both [N, K]; Y [N, K] ([N] or [N, 1] class labels for MultiClass).  want_grad: also
        (dmu [N, K], dvar [N, K], d sum / d parameter 0)."""
        desc, keep = lik
        Fmu, Fvar, Y = _f64(Fmu), _f64(Fvar), _f64(Y)
        _need(Fmu.ndim == 2 and Fvar.shape == Fmu.shape, "Fmu and Fvar must both be [N, K]")
        n, k = Fmu.shape
        _need(n > 0 and k > 0, "empty moments")
        _need(Y.size == (n if desc.kind == LIK_MULTICLASS else n * k), "Y must be [N, K] (one label per point for MultiClass)")
        _need_ordinal_labels(desc, Y)
        ve, dpar = ctypes.c_double(0), ctypes.c_double(0)
        dmu = np.zeros((n, k)) if want_grad else None
        dvar = np.zeros((n, k)) if want_grad else None
        self._call("gps_lik_varexp", _byref(desc), _ptr(Fmu), _ptr(Fvar), _ptr(Y), n, k, _byref(ve), _opt(dmu), _opt(dvar),
                   _byref(dpar) if want_grad else None)
        del keep
        if want_grad:
            return ve.value, dmu, dvar, dpar.value
        return ve.value

    def _svgp_lik_args(self, lik, Z, X, Y, mean, q_mu, q_sqrt):
        desc, _ = lik
        Z, X, q_mu, q, qnd, m, d, n, k = self._svgp_args(Z, X, q_mu, q_sqrt)
        Y = _f64(Y)
        if desc.kind == LIK_MULTICLASS:
            _need(Y.size == n, "MultiClass takes one class label per point")
            _need(np.all(Y == np.floor(Y)) and Y.min() >= 0 and Y.max() < k, "class labels must be integers in [0, K)")
        else:
            _need(Y.shape == (n, k), "Y must be [N, K] with K = number of latent functions")
            _need_ordinal_labels(desc, Y)
        if mean is not None:
            mean = _f64(np.broadcast_to(mean, (n, k)))
        return desc, Z, X, Y, mean, q_mu, q, qnd, m, d, n, k

    def svgp_elbo_lik(self, prog, Z, X, Y, q_mu, q_sqrt, jitter, lik, mean=None, white=True, scale=1.0, scales=None):
        """(elbo, kl, sum of variational expectations) of models/svgp.py:108-125 for a device likelihood (make_lik); mean:
        mean_function(X) [N, K] or None."""
        desc, Z, X, Y, mean, q_mu, q, qnd, m, d, n, k = self._svgp_lik_args(lik, Z, X, Y, mean, q_mu, q_sqrt)
        elbo, kl, ve, info = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int(0)
        self._drop_resident()
        self._arm_scales(scales, Z)
        self._call("gps_svgp_elbo_lik", prog, len(prog), _ptr(Z), m, d, float(jitter), _ptr(X), n, _ptr(Y), _opt(mean),
                   _ptr(q_mu), k, _ptr(q), qnd, 1 if white else 0, _byref(desc), float(scale), _byref(elbo), _byref(kl),
                   _byref(ve), _byref(info))
        _raise_if_not_pd(info, _PD_KUU)
        return elbo.value, kl.value, ve.value

    def svgp_elbo_lik_grad(self, prog, Z, X, Y, q_mu, q_sqrt, jitter, lik, mean=None, white=True, scale=1.0, want_grad_Z=False,
                           scales=None):
        """svgp_elbo_grad for a device likelihood: (elbo, grad_slots, d/d likelihood parameter 0, grad_q_mu, grad_q_sqrt,
        d/d mean(X) [N, K][, grad_Z][, grad_scales])."""
        desc, Z, X, Y, mean, q_mu, q, qnd, m, d, n, k = self._svgp_lik_args(lik, Z, X, Y, mean, q_mu, q_sqrt)
        elbo, glik, info = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int(0)
        slots, ns = self._slot_buffer()
        g_qmu, g_q, g_mean, g_Z = np.zeros((m, k)), np.zeros_like(q), np.zeros((n, k)), np.zeros((m, d))
        self._drop_resident()
        armed = self._arm_scales(scales, Z)
        self._call("gps_svgp_elbo_lik_grad", prog, len(prog), _ptr(Z), m, d, float(jitter), _ptr(X), n, _ptr(Y), _opt(mean),
                   _ptr(q_mu), k, _ptr(q), qnd, 1 if white else 0, _byref(desc), float(scale), _byref(elbo), _ptr(slots),
                   SLOT_CAP, _byref(ns), _byref(glik), _ptr(g_qmu), _ptr(g_q), _ptr(g_mean),
                   _ptr(g_Z) if want_grad_Z else None, _byref(info))
        _raise_if_not_pd(info, _PD_KUU)
        out = (elbo.value, slots[:ns.value].copy(), glik.value, g_qmu, self._q_sqrt_grad(g_q, qnd), g_mean)
        out = out + (g_Z,) if want_grad_Z else out
        return out + (self._scales_grad(m, d),) if armed else out

    # ---- GPMC: the whitened model for MCMC, and its kernels on their own
    def lik_logp(self, lik, F, Y, want_grad=False):
        """Sum over points and latents of log p(Y | F) of a device likelihood (``lik`` from make_lik; not MultiClass), F and
        Y [N, K].  want_grad: also (d log p / d F [N, K], d sum / d parameter 0)."""
        desc, keep = lik
        F, Y = _f64(F), _f64(Y)
        _need(F.ndim == 2 and Y.shape == F.shape and F.size > 0, "F and Y must both be [N, K]")
        if desc.kind == LIK_MULTICLASS:
            raise NotImplementedError("log p(y | f) of MultiClass is piecewise constant in f: no pointwise form with a gradient")
        _need_ordinal_labels(desc, Y)
        n, k = F.shape
        lp, dpar = ctypes.c_double(0), ctypes.c_double(0)
        G = np.zeros((n, k)) if want_grad else None
        self._call("gps_lik_logp", _byref(desc), _ptr(F), _ptr(Y), n, k, _byref(lp), _opt(G), _byref(dpar) if want_grad else None)
        del keep
        return (lp.value, G, dpar.value) if want_grad else lp.value

    def tri_skinny(self, L, B, trans=False):
        """tril(L) @ B, or tril(L).T @ B with trans, for L [N, N] and a skinny B [N, R]: whatever L holds above its diagonal
        is never read."""
        L, B = _f64(L), _f64(B)
        n = L.shape[0]
        _need(L.shape == (n, n) and B.ndim == 2 and B.shape[0] == n, "L must be [N, N] and B [N, R]")
        out = np.zeros_like(B)
        self._call("gps_tri_skinny", _ptr(L), n, _ptr(B), B.shape[1], 1 if trans else 0, _ptr(out))
        return out

    def chol_seed(self, U, V):
        """P [Np, Np], Np = N rounded up to a multiple of 128: P[i, j] = U[max(i, j)] . V[min(i, j)] for i, j < N, zero in
        the padding -- Phi(P) + Phi(P)^T of the Cholesky adjoint for the cotangent tril(G V^T), with U = L^T G."""
        U, V = _f64(U), _f64(V)
        _need(U.ndim == 2 and V.shape == U.shape and U.size > 0, "U and V must both be [N, R]")
        n, r = U.shape
        npad = -(-n // 128) * 128
        P = np.empty((npad, npad))
        self._call("gps_chol_seed", _ptr(U), _ptr(V), n, r, _ptr(P))
        return P

    def _gpmc_args(self, lik, X, V, Y, mean):
        desc, _ = lik
        X, V, Y = _f64(X), _f64(V), _f64(Y)
        _need(X.ndim == 2 and V.ndim == 2 and V.shape[0] == X.shape[0] and V.size > 0, "X must be [N, D] and V [N, K]")
        if desc.kind == LIK_MULTICLASS:
            raise NotImplementedError("log p(y | f) of MultiClass is piecewise constant in f: no pointwise form with a gradient")
        n, d = X.shape
        k = V.shape[1]
        _need(Y.shape == (n, k), "Y must be [N, K] with K = number of latent functions")
        _need_ordinal_labels(desc, Y)
        if mean is not None:
            mean = _f64(np.broadcast_to(mean, (n, k)))
        return desc, X, V, Y, mean, n, d, k

    def gpmc_lik(self, prog, X, V, Y, jitter, lik, mean=None):
        """sum log p(Y | L V + mean), L = chol(K(X) + jitter I)  (models/gpmc.py:72-77); mean: mean_function(X) or None."""
        desc, X, V, Y, mean, n, d, k = self._gpmc_args(lik, X, V, Y, mean)
        ll, info = ctypes.c_double(0), ctypes.c_int(0)
        self._drop_resident()
        self._call("gps_gpmc_lik", prog, len(prog), _ptr(X), n, d, float(jitter), _ptr(V), k, _ptr(Y), _opt(mean), _byref(desc),
                   _byref(ll), _byref(info))
        _raise_if_not_pd(info, _PD_CHOL)
        return ll.value

    def gpmc_lik_grad(self, prog, X, V, Y, jitter, lik, mean=None):
        """(loglik, grad_slots, d/d likelihood parameter 0, grad_V [N, K], d/d mean(X) [N, K]) -- gradients w.r.t. the
        constrained values (gps_gpmc_lik_grad)."""
        desc, X, V, Y, mean, n, d, k = self._gpmc_args(lik, X, V, Y, mean)
        ll, glik, info = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int(0)
        slots, ns = self._slot_buffer()
        g_V, g_mean = np.zeros((n, k)), np.zeros((n, k))
        self._drop_resident()
        self._call("gps_gpmc_lik_grad", prog, len(prog), _ptr(X), n, d, float(jitter), _ptr(V), k, _ptr(Y), _opt(mean),
                   _byref(desc), _byref(ll), _ptr(slots), SLOT_CAP, _byref(ns), _byref(glik), _ptr(g_V), _ptr(g_mean),
                   _byref(info))
        _raise_if_not_pd(info, _PD_CHOL)
        return ll.value, slots[:ns.value].copy(), glik.value, g_V, g_mean

    def diag_gpmc_front(self, reps=5):
        """Microseconds of (F = L V, U = L^T G, the rank-R seed, the seed by the generic adjoint's transpose + N^3 product +
        mirror) on what the last gpmc_lik_grad left on the device."""
        out = np.zeros(4)
        self._call("gps_diag_gpmc_front", int(reps), _ptr(out))
        return out

    # ---- SGPMC: the sparse model for MCMC, streamed over row chunks of the data
    def _sgpmc_args(self, lik, Z, X, Y, V, mean, chunk_rows):
        desc, _ = lik
        Z, X, Y, V = _f64(Z), _f64(X), _f64(Y), _f64(V)
        _need(Z.ndim == 2 and X.ndim == 2 and Z.shape[1] == X.shape[1] and Z.size > 0 and X.size > 0,
              "Z must be [M, D] and X [N, D]")
        _need(V.ndim == 2 and V.shape[0] == Z.shape[0] and V.size > 0, "V must be [M, K]")
        _need(int(chunk_rows) >= 0 and int(chunk_rows) % 128 == 0, "chunk_rows must be 0 or a multiple of 128")
        (m, d), n, k = Z.shape, X.shape[0], V.shape[1]
        if desc.kind == LIK_MULTICLASS:
            _need(Y.size == n, "MultiClass takes one class label per point")
            _need(np.all(Y == np.floor(Y)) and Y.min() >= 0 and Y.max() < k, "class labels must be integers in [0, K)")
        else:
            _need(Y.shape == (n, k), "Y must be [N, K] with K = number of latent functions")
            _need_ordinal_labels(desc, Y)
        if mean is not None:
            mean = _f64(np.broadcast_to(mean, (n, k)))
        return desc, Z, X, Y, V, mean, m, d, n, k

    def sgpmc_lik(self, prog, Z, X, Y, V, jitter, lik, mean=None, chunk_rows=0):
        """sum of the variational expectations at fmean = A^T V + mean, fvar = Kdiag - colsum(A^2), A = Lm^-1 Kuf
        (models/sgpmc.py:83-89), the data taken chunk_rows rows at a time (0: the library's choice)."""
        desc, Z, X, Y, V, mean, m, d, n, k = self._sgpmc_args(lik, Z, X, Y, V, mean, chunk_rows)
        ll, info = ctypes.c_double(0), ctypes.c_int(0)
        self._drop_resident()
        self._call("gps_sgpmc_lik", prog, len(prog), _ptr(Z), m, d, float(jitter), _ptr(X), n, _ptr(Y), _opt(mean), _ptr(V), k,
                   _byref(desc), int(chunk_rows), _byref(ll), _byref(info))
        _raise_if_not_pd(info, _PD_KUU)
        return ll.value

    def sgpmc_lik_grad(self, prog, Z, X, Y, V, jitter, lik, mean=None, chunk_rows=0, want_grad_Z=False, want_grad_mean=True):
        """(loglik, grad_slots, d/d likelihood parameter 0, grad_V [M, K], d/d mean(X) [N, K][, grad_Z]) -- gradients w.r.t.
        the constrained values, in the same single pass over the data (gps_sgpmc_lik_grad); want_grad_mean=False: the library is
        not asked for d/d mean(X) and None stands in its place."""
        desc, Z, X, Y, V, mean, m, d, n, k = self._sgpmc_args(lik, Z, X, Y, V, mean, chunk_rows)
        ll, glik, info = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int(0)
        slots, ns = self._slot_buffer()
        g_V, g_mean, g_Z = np.zeros((m, k)), (np.zeros((n, k)) if want_grad_mean else None), np.zeros((m, d))
        self._drop_resident()
        self._call("gps_sgpmc_lik_grad", prog, len(prog), _ptr(Z), m, d, float(jitter), _ptr(X), n, _ptr(Y), _opt(mean), _ptr(V),
                   k, _byref(desc), int(chunk_rows), _byref(ll), _ptr(slots), SLOT_CAP, _byref(ns), _byref(glik), _ptr(g_V),
                   _opt(g_mean), _ptr(g_Z) if want_grad_Z else None, _byref(info))
        _raise_if_not_pd(info, _PD_KUU)
        out = (ll.value, slots[:ns.value].copy(), glik.value, g_V, g_mean)
        return out + (g_Z,) if want_grad_Z else out

    def gauss_kl(self, q_mu, q_sqrt, K=None):
        """kullback_leiblers.py:26-105"""
        q_mu = _f64(q_mu)
        _need(q_mu.ndim == 2, "q_mu must be [M, K]")
        m, k = q_mu.shape
        q, qnd = self._prep_q_sqrt(q_sqrt)
        _need(q is not None, "gauss_kl needs q_sqrt")
        self._check_q_sqrt(q, qnd, m, k)
        if m == 0 or k == 0:
            return 0.0
        if K is not None:
            K = _f64(K)
            _need(K.shape == (m, m), "K must be [M, M]")
        out, info = ctypes.c_double(0), ctypes.c_int(0)
        self._call("gps_gauss_kl", _opt(K), m, _ptr(q_mu), k, _ptr(q), qnd, _byref(out), _byref(info))
        _raise_if_not_pd(info, _PD_K)
        return out.value


_default = None
_default_lock = threading.Lock()


def get_handle():
    """Process-wide default handle (device = $GPFLOWSLIM_DEVICE, else $LOCAL_RANK, else 0)."""
    global _default
    with _default_lock:
        if _default is None:
            _default = Handle()
        return _default


def set_handle(handle):
    global _default
    with _default_lock:
        _default = handle
