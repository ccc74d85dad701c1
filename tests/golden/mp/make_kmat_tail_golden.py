"""50-digit references of kernel-matrix entries from 1 down through the denormals (tests/_kmat_tail.py has the inputs and says
why the arguments are exact; the formulas here are mpmath's alone).

Per stationary kind the scaled coordinates S = s 2^k, T = t 2^k are exact doubles and so is r2 = S^2 + T^2; the entry is the
correctly rounded double of the exact formula at that double r2, with the double constants of kmat_prim_value (1e-12,
1.7320508075688772, 2.23606797749979, the double 5.0 / 3.0) and a_d = fl(r2 + 1e-12) taken in fp64 first, as every
implementation of kernels.py:424-426 in fp64 does:
    rbf          exp(-r2 / 2)                                    kernels.py:436-439
    matern12     exp(-r),  r = sqrt(a_d)                         kernels.py:560-566
    exponential  exp(-r / 2)                                     kernels.py:573-579
    matern32     (1 + sq3 r) exp(-sq3 r)                         kernels.py:586-593
    matern52     (1 + sq5 r + (5/3) r^2) exp(-sq5 r)             kernels.py:600-610
    ratquad      (1 + r2 / (2 alpha))^-alpha, alpha = 64         kernels.py:467-471
    periodic     exp(-sum_d sin^2(pi (x_d - x'_d) / p) / (2 l^2)), p = 2, l = 1 and 2^-5, at the double inputs      kernels.py:806-819
General position (65 points in D = 3 and 32, rbf and matern52, the upper triangle of K(X) row by row): the difference form
r2 = sum_d ((x_d - x'_d) / l_d)^2  at 50 digits, then the same formulas with r = sqrt(r2 + 1e-12) (no fp64 step: here the
device's r2 is not exact).  Periodic at l = 1: the first 17 rows and columns of its grid.
All variances are 1.  The file is compressed: about half of the entries of the exact grids are exact zeros (arguments below
-745.2).
    python tests/golden/mp/make_kmat_tail_golden.py        # rewrites tests/golden/mp/kmat_tail.npz
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _kmat_tail as kt  # noqa: E402   (inputs only)

R_EPS, SQ3, SQ5, C53, ALPHA = 1e-12, 1.7320508075688772, 2.23606797749979, 5.0 / 3.0, 64.0


def mp_value(mp, kind, r2, exact_r2=True):
    """the entry at the squared distance r2 (a double when exact_r2, else an mpmath number)"""
    if kind == "rbf":
        return mp.exp(-mp.mpf(r2) / 2)
    if kind == "ratquad":
        return mp.exp(-mp.mpf(ALPHA) * mp.log1p(mp.mpf(r2) / (2 * mp.mpf(ALPHA))))
    r = mp.sqrt(mp.mpf(float(r2) + R_EPS)) if exact_r2 else mp.sqrt(r2 + mp.mpf(R_EPS))
    if kind == "matern12":
        return mp.exp(-r)
    if kind == "exponential":
        return mp.exp(-r / 2)
    if kind == "matern32":
        return (1 + mp.mpf(SQ3) * r) * mp.exp(-mp.mpf(SQ3) * r)
    assert kind == "matern52"
    return (1 + mp.mpf(SQ5) * r + mp.mpf(C53) * r * r) * mp.exp(-mp.mpf(SQ5) * r)


def build():
    """{name: array} of the fixture"""
    import mpmath as mp
    mp.mp.dps = 50
    out = {}
    for kind in kt.STATIONARY:
        s, t = kt.coordinates(kind)
        S, T = s * 2.0 ** kt.LOG2K[kind], t * 2.0 ** kt.LOG2K[kind]
        out[kind + "/s"], out[kind + "/t"] = s, t
        out[kind + "/K"] = np.array([[float(mp_value(mp, kind, float(mp.mpf(a) * a + mp.mpf(b) * b))) for b in T] for a in S])
    s, t = kt.periodic_coordinates()
    out["periodic/s"], out["periodic/t"] = s, t
    for q, ls in enumerate(kt.PERIODIC_LS):
        # the row point is (s, 0) and the column point (0, t): the differences are s and -t
        n = kt.PERIODIC_SUB if q == 0 else kt.N
        out["periodic/K_l%d" % q] = np.array([[float(mp.exp(-(mp.sin(mp.pi * mp.mpf(a) / kt.PERIOD) ** 2 + mp.sin(mp.pi * mp.mpf(-b) / kt.PERIOD) ** 2)
                                                            / (2 * mp.mpf(ls) ** 2))) for b in t[:n]] for a in s[:n]])
    iu = np.triu_indices(kt.N)
    for D in kt.GENERAL_DIMS:
        X = kt.general_points(D)
        out["general/X_d%d" % D] = X
        ls = [mp.mpf(2.0 ** ((c % 3) - 1)) for c in range(D)]
        r2 = [sum(((mp.mpf(X[i, c]) - mp.mpf(X[j, c])) / ls[c]) ** 2 for c in range(D)) for i, j in zip(*iu)]
        for kind in ("rbf", "matern52"):
            out["general/%s_d%d" % (kind, D)] = np.array([float(mp_value(mp, kind, v, exact_r2=False)) for v in r2])
    return out


def main():
    np.savez_compressed(os.path.join(HERE, "kmat_tail.npz"), **build())


if __name__ == "__main__":
    main()
