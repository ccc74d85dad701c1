"""Matrix-free exact GP regression in mixed precision: the same solve and the same prediction as examples/gpr_matrix_free.py, with
the kernel products of the inner conjugate-gradient loop in fp32 (csrc/kmvm_f32.hip) under an fp64 residual -- iterative
refinement, so the answers stay fp64-grade.  Prints both routes side by side: what they agree to, and what each cost.

    python examples/gpr_matrix_free_mixed.py [N]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gpflow-slim_amd"), ROOT]
import gpflowSlim as gpf  # noqa: E402
from gpflowSlim import conjugate_gradient as cg  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
rng = np.random.default_rng(0)
X = rng.uniform(-3, 3, (n, 2))
f = lambda x: np.sin(2 * x[:, :1]) * np.cos(x[:, 1:2])  # noqa: E731
Y = f(X) + 0.3 * rng.standard_normal((n, 1))
Xs = rng.uniform(-3, 3, (32, 2))
kern = gpf.kernels.Matern52(2, lengthscales=np.array([0.9, 1.1]), ARD=True)
noise = 0.09

# 1. the product itself: fp32-grade entries, whatever n (each 64-column tile's share is added in fp64)
V = rng.standard_normal((n, 1))
p64, p32 = cg.kernel_matmul(kern, X, V, diag_add=noise), cg.kernel_matmul(kern, X, V, diag_add=noise, precision="fp32")
print("product: fp32 against fp64, largest difference %.2e of the largest entry" % (np.max(np.abs(p32 - p64)) / np.max(np.abs(p64))))

# 2. the solve: one stop rule, |r| <= tol |b| -- on the recurrence in fp64, on the fp64 residual b - A x in mixed precision
res = {}
for precision in ("fp64", "mixed"):
    t0 = time.perf_counter()
    x, info = cg.kernel_cgsolver(kern, X, Y, noise, max_iter=2000, tol=1e-8, precision=precision)
    res[precision] = x
    extra = "" if precision == "fp64" else " in %d outer steps, %d fp32 + %d fp64 products, fell back: %s" % (
        info["outer_iterations"][0], info["fp32_products"], info["fp64_products"], bool(info["fell_back"][0]))
    print("%-5s solve: %4d iterations%s, |r| / |b| %.1e, %.2f s" % (precision, info["iterations"][0], extra,
                                                                    info["relative_residual"][0], time.perf_counter() - t0))
print("solutions agree to %.1e of |x|" % (np.linalg.norm(res["mixed"] - res["fp64"]) / np.linalg.norm(res["fp64"])))

# 3. prediction, every solve through the mixed loop
m = gpf.models.GPR(X, Y, kern, obs_var=noise)
mean, var = m.predict_f_iterative(Xs, max_iter=2000, tol=1e-8, precision="mixed")
print("prediction from %d points: rmse against the noise-free function %.4f, mean predictive sd %.4f"
      % (n, float(np.sqrt(np.mean((mean - f(Xs)) ** 2))), float(np.mean(np.sqrt(var)))))
