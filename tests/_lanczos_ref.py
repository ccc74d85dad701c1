"""Plain reference of the Lanczos variance estimates (csrc/lanczos.hip) for tests/test_gpu_lanczos.py: Lanczos with full
reorthogonalisation (classical Gram-Schmidt, twice) on a dense K_y, and the estimate built on a given Q, all in numpy.longdouble.
Host only; the dense K_y comes from the caller (tests/test_gpu_kmvm_sop.py::dense)."""
import numpy as np

import _kmvm_ref as mr

LD = mr.LD


def lanczos(A, b, k, breakdown_tol=1e-12):
    """(Q [n, m], alpha [m], beta [m - 1]), m <= k: q_0 = b / |b|; w = A q_j; alpha_j = q_j^T w; w -= Q Q^T w twice; beta_j = |w|;
    stop at beta_j <= breakdown_tol |A q_0|"""
    A, b = np.asarray(A, dtype=LD), np.asarray(b, dtype=LD)
    Q, alpha, beta, scale = [b / np.sqrt(b @ b)], [], [], None
    for j in range(k):
        Qm = np.stack(Q, 1)
        w = A @ Q[j]
        scale = np.sqrt(w @ w) if scale is None else scale
        c1 = Qm.T @ w
        w = w - Qm @ c1
        c2 = Qm.T @ w
        w = w - Qm @ c2
        alpha.append(c1[j] + c2[j])
        bj = np.sqrt(w @ w)
        if j + 1 == k or not bj > breakdown_tol * scale:
            break
        beta.append(bj)
        Q.append(w / bj)
    return np.stack(Q, 1), np.array(alpha, dtype=LD), np.array(beta, dtype=LD)


def estimate(A, Q, Ks, kdiag):
    """Kdiag - a_j^T (Q^T A Q)^-1 a_j with a_j = Q^T k_j, k_j the columns of Ks [n, N*]: the Galerkin estimate on the span of Q"""
    Q = np.asarray(Q, dtype=LD)
    a = Q.T @ np.asarray(Ks, dtype=LD)
    return LD(kdiag) - np.sum(a * mr.solve(Q.T @ np.asarray(A, dtype=LD) @ Q, a), 0)


def exact(A, Ks, kdiag):
    return LD(kdiag) - np.sum(Ks * mr.solve(A, Ks), 0)
