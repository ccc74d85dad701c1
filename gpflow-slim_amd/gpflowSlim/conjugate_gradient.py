"""Conjugate gradients on a Kronecker-structured system (mirrors gpflowSlim/conjugate_gradient.py:18-55).

``cgsolver`` solves (I + C o (K1 (C o .) K2)) x = b by plain CG from x = 0; the loop runs on the device
(gps_kron_cg: two fp64 GEMMs and three fused vector kernels per iteration, the loop's state in device memory).
Vectors are the reference's [N, 1] columns, ``vec`` column-major; the device keeps each as the [m, n] matrix it is.
"""
import numpy as np

from . import _backend as be
from ._settings import settings


def dot(a, b):
    """conjugate_gradient.py:18-20"""
    return np.sum(np.asarray(a) * np.asarray(b))


def vec(X):
    """conjugate_gradient.py:22-25: the columns of X stacked, [N, 1]."""
    return np.reshape(np.transpose(np.asarray(X)), [-1, 1])


def unvec(v, m, n):
    """The [m, n] matrix whose ``vec`` is v."""
    return np.ascontiguousarray(np.reshape(np.asarray(v), [n, m]).T)


def cgsolver(K1, K2, b, C, max_iter=100, tol=1e-6):
    """conjugate_gradient.py:28-55.  K1 [m, m], K2 [n, n]; b, C [N, 1] with N = m n.  Returns x [N, 1].  The stop rule
    compares tol * |b| with the SQUARED residual norm, as the reference does."""
    K1 = np.asarray(K1, dtype=settings.float_type)
    K2 = np.asarray(K2, dtype=settings.float_type)
    if K1.ndim != 2 or K2.ndim != 2:
        raise ValueError("K1 and K2 must be square")
    m, n = K1.shape[0], K2.shape[0]
    b = np.asarray(b, dtype=settings.float_type)
    C = np.broadcast_to(np.asarray(C, dtype=settings.float_type), b.shape) if np.ndim(C) else np.full(b.shape, float(C))
    if b.size != m * n:
        raise ValueError("b must have %d entries" % (m * n))
    x, _, _, _ = be.get_handle().kron_cg(K1, K2, unvec(b, m, n), unvec(C, m, n), max_iter=max_iter, tol=tol)
    return vec(x)


# ---- exact GPs without the N x N matrix (not in the reference) -------------------------------------------------------------------
# kernel_matmul is (K(X, X2) + c I) V with K generated tile by tile on the device and never stored; kernel_cgsolver solves
# (K(X, X) + s I) x = B on it, all columns of B at once (gps_kmvm, gps_kernel_cg: csrc/kmvm.hip).  kernel_logdet (stochastic Lanczos
# quadrature on the solve's own coefficients) and kernel_grad_form (sum_ij G_ij dK_ij / d theta for a low-rank G) are what training
# needs on top: GPR.compute_log_likelihood_and_gradients_iterative.
MATRIX_FREE_SCOPE = ("one stationary kernel: RBF, Matern12, Matern32, Matern52, Exponential or RatQuad; or, for products, solves "
                     "without a preconditioner and prediction, a Sum of Products of those, Periodic, Cosine, Constant and White "
                     "(at most 16 primitives and 64 feature rows)")
SOP_MAX_PRIMS, SOP_MAX_ROWS = 16, 64          # csrc/kmat_common.hpp: GPS_SOP_MAX_PRIMS, GPS_SOP_MAX_ROWS


def _sop_rows(k, d_all):
    """Feature rows of one primitive of a sum of products, rounded up to 4 (csrc/kmvm_sop.hip), or NotImplementedError"""
    from . import kernels
    if isinstance(k, (kernels.Constant, kernels.White)) or isinstance(k, kernels._SCALARS):
        return 0
    if isinstance(k, kernels.Cosine):
        nf = 2
    elif isinstance(k, kernels.Periodic):
        nf = 2 * len(k._dims(False, d_all))
    elif isinstance(k, (kernels.RBF, kernels.Matern12, kernels.Matern32, kernels.Matern52, kernels.Exponential, kernels.RatQuad)):
        nf = len(k._dims(False, d_all))
    elif isinstance(k, kernels.Sum):
        raise NotImplementedError("the matrix-free path takes a sum of products, not a Sum under a Product: expand (a + b) * c "
                                  "into a * c + b * c")
    else:
        raise NotImplementedError("the matrix-free path takes %s; got a %s factor" % (MATRIX_FREE_SCOPE, type(k).__name__))
    if len(k._dims(False, d_all)) > 32:
        raise ValueError("the matrix-free path takes at most 32 active dims per primitive")
    return -(-nf // 4) * 4


def _matrix_free_program(kern, d_all, composite=None):
    """The kernel's program if the matrix-free path takes it, else NotImplementedError -- before anything touches the device.  The
    one place where the scope is decided: a lone stationary primitive (one node: kmvm_kernel's route), or a Combination that is a
    Sum of Products of primitives (more nodes: kmvm_sop_kernel's, the postfix program whose term flags the library compiles).
    composite: None, or why the caller cannot take a Combination -- then the NotImplementedError names that limit."""
    from . import kernels
    if isinstance(kern, kernels.Combination):
        if composite is not None:
            raise NotImplementedError("%s takes %s; a %s kernel is %s" % (composite[0], MATRIX_FREE_SCOPE.split(";")[0],
                                                                          type(kern).__name__, composite[1]))
        terms = (kern.kern_list + kern.const_list) if isinstance(kern, kernels.Sum) else [kern]
        prims = []
        for t in terms:
            prims.extend(t.kern_list + t.const_list if isinstance(t, kernels.Product) else [t])
        if len(prims) == 1 and isinstance(prims[0], kernels.Kernel):      # (a Combination of one kernel is that kernel)
            return _matrix_free_program(prims[0], d_all)
        rows = sum(_sop_rows(k, d_all) for k in prims)
        if len(prims) > SOP_MAX_PRIMS or rows > SOP_MAX_ROWS:
            raise ValueError("the matrix-free path takes at most %d primitives and %d feature rows (active dims per primitive "
                             "rounded up to 4, twice the dims for Periodic); got %d and %d"
                             % (SOP_MAX_PRIMS, SOP_MAX_ROWS, len(prims), rows))
        return kern._program(d_all)
    if not isinstance(kern, (kernels.RBF, kernels.Matern12, kernels.Matern32, kernels.Matern52, kernels.Exponential,
                             kernels.RatQuad)):
        raise NotImplementedError("the matrix-free path takes %s; got %s" % (MATRIX_FREE_SCOPE, type(kern).__name__))
    return kern._program(d_all)


def _is_sop(prog):
    """more than one node: the sum-of-products entries (gps_*_sop)"""
    return len(prog) > 1


def _precision_program(who, kern, d_all, precision):
    """_matrix_free_program for a call that takes a precision: anything but 'fp64' knows one primitive (csrc/kmvm_f32.hip)"""
    composite = None if precision == "fp64" else ("%s(precision=%r)" % (who, precision), "served in fp64 only: the fp32 product "
                                                  "knows one primitive")
    return _matrix_free_program(kern, d_all, composite=composite)


def kernel_matmul(kern, X, V, X2=None, diag_add=0.0, precision="fp64"):
    """K(X, X2) V [n, T], or (K(X, X) + diag_add I) V without an X2; memory O(n (D + T)).  precision="fp32" (one stationary kernel
    only): dot products, the kernel's formula and the product with V on the fp32 pipes, the feature rows centred in fp64 first and
    every 64-column tile's share added in fp64 -- fp32-grade entries, about 1e-7 of sum_p |K_ip| |V_pt| whatever n; what the inner
    loop of kernel_cgsolver(precision="mixed") runs."""
    be._check_precision("kernel_matmul", precision, "kernel_matmul")
    X = np.ascontiguousarray(X, dtype=settings.float_type)
    prog = _precision_program("kernel_matmul", kern, X.shape[1], precision)
    kern._check_inputs(*([X] if X2 is None else [X, X2]))
    if precision == "fp32":
        return be.kmvm_f32(be.get_handle(), prog, X, V, X2=X2, diag_add=diag_add)
    return (be.kmvm_sop if _is_sop(prog) else be.kmvm)(be.get_handle(), prog, X, V, X2=X2, diag_add=diag_add)


def _precond_program(kern, X, rank, rel_tol, noise_var=None):
    """(X as the device takes it, the program) after the refusals of every call that takes a preconditioner's rank -- the kernel's
    scope, the rank in 0 .. 128, a noise above 0 with a rank --, all before anything touches the device."""
    X = np.ascontiguousarray(X, dtype=settings.float_type)
    prog = _matrix_free_program(kern, X.shape[1], composite=("the pivoted-Cholesky preconditioner (precond_rank > 0)",
                                                             "not preconditioned: its step kernel knows one primitive"))
    be._check_precond(rank, rel_tol, None if noise_var is None else float(noise_var))
    kern._check_inputs(X)
    return X, prog


def kernel_pivoted_cholesky(kern, X, rank, rel_tol=1e-10):
    """(L [n, k], pivots [k], residual trace): the pivoted partial Cholesky factor of K(X, X) -- no noise -- built on the device
    (csrc/pchol.hip), K ~ L L^T, with the largest residual diagonal entry as each step's pivot, ties to the lowest index.  k <= rank <= 128: the factor stops early once that entry is <= rel_tol * variance.  residual trace = tr(K - L L^T)."""
    X, prog = _precond_program(kern, X, rank, rel_tol)
    return be.kernel_pchol(be.get_handle(), prog, X, rank, rel_tol)


def kernel_lanczos(kern, X, noise_var, start, rank, breakdown_tol=1e-12):
    """(Q [n, k], alpha [k], beta [k - 1]): k <= rank <= min(128, n) steps of Lanczos with full reorthogonalisation on
    K_y = K(X, X) + noise_var I from q_0 = start / |start|, K never stored (csrc/lanczos.hip).  Q^T Q = I and
    Q^T K_y Q = tridiag(alpha, beta); the run stops early, with the columns it has, once beta_j <= breakdown_tol |K_y q_0| (the
    Krylov space of ``start`` is exhausted).  What GPR.predict_f_iterative(variance="lanczos") builds its variances on."""
    X = np.ascontiguousarray(X, dtype=settings.float_type)
    prog = _matrix_free_program(kern, X.shape[1])
    be._check_lanczos_rank(rank, X.shape[0])
    kern._check_inputs(X)
    return be.kernel_lanczos(be.get_handle(), prog, X, noise_var, start, rank, breakdown_tol)


def kernel_precond_solve(kern, X, V, noise_var, rank, rel_tol=1e-10, G1=None):
    """(M^-1 V [n, T], log det M) for the preconditioner M = L L^T + noise_var I of kernel_cgsolver(precond_rank=rank), by Woodbury
    on the device.  G1 [rank, T]: the sample L G1 + sqrt(noise_var) V of N(0, M) (G1, V standard normal) in place of M^-1 V."""
    X, prog = _precond_program(kern, X, rank, rel_tol, noise_var)
    out, logdet, _ = be.kernel_precond_solve(be.get_handle(), prog, X, V, noise_var, rank, rel_tol, G1=G1)
    return out, logdet


def _pcg(kern, X, B, noise_var, rank, rel_tol, max_iter, tol, n_probe=0, G1=None):
    """be.kernel_pcg as (x, info): kernel_cgsolver(lanczos=True)'s info and 'logdet_M', 'rank', 'Z', 'MinvZ', 'zMz'"""
    X, prog = _precond_program(kern, X, rank, rel_tol, noise_var)
    x, iters, rel, conv, al, bt, Z, MiZ, zmz, logdet, k = be.kernel_pcg(be.get_handle(), prog, X, B, noise_var, rank, rel_tol,
                                                                     max_iter=max_iter, tol=tol, n_probe=n_probe, G1=G1)
    rows = int(np.max(iters)) if iters.size else 0
    return x, {"iterations": iters, "relative_residual": rel, "converged": conv, "alpha": al[:rows], "beta": bt[:rows],
               "logdet_M": logdet, "rank": k, "Z": Z, "MinvZ": MiZ, "zMz": zmz}


def _probe_normals(seed, rank, n, num_probes):
    """(G1 [rank, T], G2 [n, T]) standard normal from default_rng(seed): Z = L G1 + sqrt(noise) G2 ~ N(0, M)"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((int(rank), int(num_probes))), rng.standard_normal((n, int(num_probes)))


def kernel_cgsolver(kern, X, B, noise_var, max_iter=1000, tol=1e-8, lanczos=False, precond_rank=0, precond_rel_tol=1e-10,
                    precision="fp64", inner_tol=1e-4, max_outer=20):
    """(K(X, X) + noise_var I) x = B by plain conjugate gradients from x = 0, the T columns of B at once.  A column stops when
    |r| <= tol |b| -- the unsquared norms; ``cgsolver`` above keeps the reference's rule, tol |b| against r^T r.  Returns
    (x [n, T], info) with info['iterations'] [T], info['relative_residual'] [T] (of the recurrence) and info['converged'] [T];
    a column that did not converge within max_iter is reported by a warning, not an error.  lanczos: info['alpha'] and
    info['beta'] [iterations, T] as well, the recurrence's coefficients per column (rows below the column's iteration count).
    precond_rank (0 .. 128; 0: the plain loop, byte for byte): the loop preconditioned by M = L L^T + noise_var I, L the pivoted
    partial Cholesky factor of that rank at most (kernel_pivoted_cholesky; rebuilt inside the call).  The stop rule stays on the
    unpreconditioned residual; the coefficients are then those of M^-1/2 (K + noise_var I) M^-1/2, and info gains 'logdet_M'
    and 'rank'.
    precision="mixed" (one stationary kernel, no lanczos, no preconditioner): iterative refinement -- an outer step solves
    A d = r by the same loop on the fp32 product (kernel_matmul(precision="fp32")) until |r_inner| <= inner_tol |r|, then x += d
    and r = b - A x with the fp64 product; a column stops by the same rule, on that fp64 residual.  If an outer step fails to halve
    a column's residual, or after max_outer steps, the fp64 loop finishes the columns that are left.  max_iter and
    info['iterations'] count inner iterations summed over the outer steps; info gains 'outer_iterations' [T], 'fp32_products',
    'fp64_products' and 'fell_back' [T]."""
    import warnings
    be._check_precision("kernel_cgsolver", precision, "solve", lanczos=lanczos, precond_rank=precond_rank)
    X = np.ascontiguousarray(X, dtype=settings.float_type)
    prog = _precision_program("kernel_cgsolver", kern, X.shape[1], precision)
    be._check_precond(precond_rank, precond_rel_tol, float(noise_var))
    kern._check_inputs(X)
    if precision == "mixed":
        x, iters, rel, conv, outer, p32, p64, fell = be.kernel_cg_mixed(be.get_handle(), prog, X, B, noise_var, max_iter=max_iter,
                                                                        tol=tol, inner_tol=inner_tol, max_outer=max_outer)
        info = {"iterations": iters, "relative_residual": rel, "converged": conv, "outer_iterations": outer, "fp32_products": p32,
                "fp64_products": p64, "fell_back": fell}
    elif _is_sop(prog):
        if precond_rank:
            _precond_program(kern, X, precond_rank, precond_rel_tol, noise_var)      # (raises: no preconditioner for a composite kernel)
        res = be.kernel_cg_sop(be.get_handle(), prog, X, B, noise_var, max_iter=max_iter, tol=tol, lanczos=lanczos)
        x, iters, rel, conv = res[:4]
        info = {"iterations": iters, "relative_residual": rel, "converged": conv}
        if lanczos:
            rows = int(np.max(iters)) if iters.size else 0
            info.update(alpha=res[4][:rows], beta=res[5][:rows])
    elif precond_rank:
        x, info = _pcg(kern, X, B, noise_var, precond_rank, precond_rel_tol, max_iter, tol)
        rel = info["relative_residual"]
        if not lanczos:
            info = {k: info[k] for k in ("iterations", "relative_residual", "converged", "logdet_M", "rank")}
    elif lanczos:
        x, iters, rel, conv, al, bt = be.kernel_cg_lanczos(be.get_handle(), prog, X, B, noise_var, max_iter=max_iter, tol=tol)
        rows = int(np.max(iters)) if iters.size else 0
        info = {"iterations": iters, "relative_residual": rel, "converged": conv, "alpha": al[:rows], "beta": bt[:rows]}
    else:
        x, iters, rel, conv = be.kernel_cg(be.get_handle(), prog, X, B, noise_var, max_iter=max_iter, tol=tol)
        info = {"iterations": iters, "relative_residual": rel, "converged": conv}
    if not np.all(info["converged"]):
        warnings.warn("kernel_cgsolver: %d of %d columns did not reach tol = %g in %d iterations (largest |r| / |b| = %.3g)"
                      % (int(np.sum(~info["converged"])), rel.size, tol, max_iter, float(np.max(rel))))
    return x, info


def kernel_grad_form(kern, X, P, Q):
    """(slots, trace): slots[s] = sum_ij (P Q^T)_ij dK(X, X)_ij / d theta_s for every gradient slot of the kernel, in the order
    of ``kern._grad_layout`` ([variance], one per active dimension's lengthscale, RatQuad: [alpha]), and trace = tr(P Q^T), the
    slot of a noise variance.  P, Q [n, C]; K, its derivative and the weight P Q^T are regenerated tile by tile on the device
    (csrc/kmvm.hip: kmvm_grad_kernel), memory O(n (D + C)).  ``Q is P`` runs the symmetric weight as it is."""
    X = np.ascontiguousarray(X, dtype=settings.float_type)
    prog = _matrix_free_program(kern, X.shape[1], composite=("kernel_grad_form", "products, solves and prediction only: the fused "
                                                             "gradient form knows one primitive"))
    kern._check_inputs(X)
    return be.kmvm_grad(be.get_handle(), prog, X, P, Q, len(kern._grad_layout(X.shape[1])))


def lanczos_quadrature(alpha, beta, iterations):
    """e_1^T log(T_t) e_1 per column from the CG coefficients alpha, beta [iterations, T]: the tridiagonal of column t has
    T_kk = 1 / alpha_k + beta_{k-1} / alpha_{k-1} and T_{k,k+1} = sqrt(beta_k) / alpha_k for k below iterations[t]; its
    eigen-decomposition on the host gives sum_i (first component of v_i)^2 log(lambda_i).  A column of 0 iterations gives 0."""
    out = np.zeros(len(iterations))
    for t, m in enumerate(np.asarray(iterations, dtype=int)):
        if m == 0:
            continue
        a, b = alpha[:m, t], beta[:m, t]
        diag = 1.0 / a
        diag[1:] += b[:-1] / a[:-1]
        off = np.sqrt(b[:-1]) / a[:-1]
        w, v = np.linalg.eigh(np.diag(diag) + np.diag(off, 1) + np.diag(off, -1))
        out[t] = np.sum(np.square(v[0]) * np.log(w))
    return out


def kernel_logdet(kern, X, noise_var, probes=None, num_probes=16, seed=0, max_iter=1000, tol=1e-8, precond_rank=0,
                  precond_rel_tol=1e-10):
    """log det (K(X, X) + noise_var I) by stochastic Lanczos quadrature (Gardner et al. 2018): one batched CG solve of the probes,
    whose coefficients are each probe's Lanczos tridiagonal.  probes [n, T]: Rademacher from ``np.random.default_rng(seed)``
    unless given.  Returns (estimate = mean of per_probe, per_probe [T] = |z_t|^2 e_1^T log(T_t) e_1 -- an estimate of
    z_t^T log(K_y) z_t --, info of the solve).  RuntimeError if a probe's solve did not converge: a cut-off recurrence is not an
    estimate of anything.
    precond_rank > 0 (Gardner et al. 2018, section 4): with M = L L^T + noise_var I the estimate is log det M + mean of per_probe,
    per_probe [T] = (z_t^T M^-1 z_t) e_1^T log(T_t) e_1 from the preconditioned solve of probes z_t ~ N(0, M): Z = L G1 +
    sqrt(noise_var) G2 formed on the device from standard normals of ``default_rng(seed)`` unless ``probes`` are given, which are
    used as Z as they are.  Only log det (M^-1 K_y) is estimated, so the spread falls with the rank."""
    X = np.ascontiguousarray(X, dtype=settings.float_type)
    if precond_rank:
        _precond_program(kern, X, precond_rank, precond_rel_tol, noise_var)
        if probes is None:
            G1, B = _probe_normals(seed, precond_rank, X.shape[0], num_probes)
        else:
            G1, B = None, np.ascontiguousarray(probes, dtype=settings.float_type)
        _, info = _pcg(kern, X, B, noise_var, precond_rank, precond_rel_tol, max_iter, tol, n_probe=B.shape[1], G1=G1)
        _raise_unconverged("kernel_logdet", info, tol, max_iter)
        per_probe = info["zMz"] * lanczos_quadrature(info["alpha"], info["beta"], info["iterations"])
        return float(info["logdet_M"] + np.mean(per_probe)), per_probe, info
    if probes is None:
        probes = np.random.default_rng(seed).integers(0, 2, size=(X.shape[0], int(num_probes))) * 2.0 - 1.0
    Z = np.ascontiguousarray(probes, dtype=settings.float_type)
    _, info = _solve_converged("kernel_logdet", kern, X, Z, noise_var, max_iter, tol)
    per_probe = np.sum(np.square(Z), 0) * lanczos_quadrature(info["alpha"], info["beta"], info["iterations"])
    return float(np.mean(per_probe)), per_probe, info


def _solve_converged(who, kern, X, B, noise_var, max_iter, tol):
    """kernel_cgsolver(lanczos=True) that raises where it would warn"""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        x, info = kernel_cgsolver(kern, X, B, noise_var, max_iter=max_iter, tol=tol, lanczos=True)
    _raise_unconverged(who, info, tol, max_iter)
    return x, info


def _raise_unconverged(who, info, tol, max_iter):
    if not np.all(info["converged"]):
        raise RuntimeError("%s: %d of %d columns did not reach tol = %g in %d iterations (largest |r| / |b| = %.3g); raise max_iter"
                           % (who, int(np.sum(~info["converged"])), info["converged"].size, tol, max_iter,
                              float(np.max(info["relative_residual"]))))
