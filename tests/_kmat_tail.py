"""Inputs, fp64 restatements, units and gates of tests/test_kmat_tail_cpu.py and tests/test_gpu_kmat_tail.py: the entries of the
kernel-matrix build in RELATIVE error, from 1 down to the flush of the device exponential, and the tail below it.  Host only
(numpy and math); the 50-digit references are tests/golden/mp/kmat_tail.npz (make_kmat_tail_golden.py).

Inputs with exact arguments.  The row points are s_i e_p and the column points t_j e_q (p != q) with s, t multiples of 2^-10,
|s|, |t| <= 40, every lengthscale a power of two, 2^-k.  The features x / l are then exact, so are the squared norms, the dot
product is exactly 0 and  r2 = -2 dot + (ni + nj) = S_i^2 + T_j^2  (S = s 2^k, T = t 2^k) is exact in every kernel of
csrc/kmat.hip.  With common offsets w_c (multiples of 2^-3) on the other axes (``dim_case``) both norms and the dot product carry
the same exact W = sum (w_c / l_c)^2 and r2 is unchanged.  What is left between r2 and the stored entry is the device's own
arithmetic: (the fp64 sum r2 + 1e-12, which the reference reproduces,) gps_sqrt_pos, one product with a constant, the exponential,
and the value path.

Grid per kind (``grid``): 65 rows x 65 columns.
  row 0: S = 0;   rows 1 .. 64: a seeded spread, a quarter of it log-uniform in |a| over 2^-6 .. 2^5 (a: the argument of the
  exponential; there one ulp of the value is the whole unit), the rest half uniform in a over [-700, 0], half uniform in r2
  over the same range;
  column 0: T = 0;  columns 1 .. 32: the run, 32 equally spaced multiples of 2^-10 (consecutive ones for RBF) whose arguments on
  row 0 step by about 0.04 from -707.45 to -708.65, across a = -708 (the relative domain's edge) and a = -708.05 (where
  round(a log2 e) reaches -1022 and the device flushes);  columns 33 .. 36: on row 0 the single arguments -720, -744.5 (next to
  the last denormal), -746 (exp rounds to 0) and -800;  columns 37 .. 64: the spread again.
  k per kind (``LOG2K``) is the smallest at which the argument at |t| = 40 is below -800.

Periodic (period 2, two active dimensions, lengthscales 1 and 2^-5) has no exact argument: its grid (``periodic_grid``) has
points in [-2, 2], row 1 at s = 1 carries the run in multiples of 2^-14, and its unit has the term below.  At l = 1 every
argument lies in [-1, 0] and the first 17 rows and columns are taken (the fixture's size: the tiles are covered at l = 2^-5).

Domains.  Relative domain a >= -708: there round(a log2 e) >= -1021 and neither exponential may flush; every entry meets
|got - ref| <= LD_OWN_FACTOR x own x unit.  Tail a < -708: got >= 0, finite, |got - ref| <= pre 2^-1021 with pre = variance x
polynomial prefactor (the device may flush to 0 where the reference goes through the denormals).

Unit.  unit = eps (1 + |a|) |ref|: a relative perturbation delta of the argument moves e^a by |a| delta, and the 1 covers the
roundings of the value path.  RatQuad: a = -alpha log1p(r2 / (2 alpha)).  A Product of two factors has one more rounding,
eps (2 + |a|) |ref|.
Periodic adds the absolute error E of its exponent A = -(D - sum_d cos(a_d - b_d)) / (4 l^2), to first order, of the feature form:
    E = eps / (4 l^2) x ( U_ANG sum_d |sin(a_d - b_d)| (|a_d| + |b_d|)  +  2 D  +  D^2 )
  U_ANG = 0.5 + |fl(pi) - pi| / (pi eps) = 0.68: the angle a_d = fl(2 fl(pi) x_d) / p is rounded once and uses the double pi, and
  the cosine of the difference moves by |sin| times that; 2 D: the four factors of the D products cos cos + sin sin, each within
  one eps; D^2: the 2 D roundings of the accumulation, each eps / 2 of a partial sum <= D.  All of it is amplified by 1 / (4 l^2)
  because D - dot cancels.   unit = (eps (1 + |A|) + E) |ref|.
General position (``general_case``: the symmetric build of 65 points in 3 and in 32 dimensions, r2 from 0 to 1400; the fixture
keeps the upper triangle): the device's r2 = ni + nj - 2 dot cancels, which the reference's own formula
(kernels.py:409-421) carries too: unit = eps (1 + |a| + g (ni + nj + 2 |dot|)) |ref| with g = |da / dr2|.

Gate (the rule of tests/_many_outputs.py): LD_OWN_FACTOR x own(kind) x unit with LD_OWN_FACTOR = 10 ("another fp64 evaluation in
another operation order") and own(kind) the worst error, in these units and over the relative domain, of the plain fp64
restatement below (the device's operation order, glibc exp / log1p / cos / sin through ``math``, numpy's correctly rounded sqrt, no
fused operation) against the fixture -- and no less than the fixture's own error in the same units, half a spacing of the
stored double (``own_of`` says why: for RBF the restatement equals the fixture nearly everywhere).  No other floor.  For the
kinds with exact arguments own <= 3 is asserted
(tests/test_kmat_tail_cpu.py): at most two roundings of eps / 2 on the argument path, at most four on the value path.
"""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _many_outputs import LD_OWN_FACTOR  # noqa: E402

EPS = float(np.finfo(np.float64).eps)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mp", "kmat_tail.npz")
N = 65
A_EDGE = -708.0                                   # the relative domain: a >= A_EDGE
TAIL_ABS = 2.0 ** -1021                           # the tail: |got - ref| <= pre x TAIL_ABS
SQ3, SQ5, C53, R_EPS = 1.7320508075688772, 2.23606797749979, 5.0 / 3.0, 1e-12          # as kmat_prim_value has them
ALPHA = 64.0
STATIONARY = ("rbf", "matern12", "exponential", "matern32", "matern52", "ratquad")
LOG2K = {"rbf": 0, "matern12": 5, "exponential": 6, "matern32": 4, "matern52": 4, "ratquad": 8}
VARIANCES = (1.0, 4.0)
RUN_FROM, RUN_TO, RUN_LEN = -707.45, -708.65, 32
SINGLES = (-720.0, -744.5, -746.0, -800.0)
SPREAD_LO = -700.0
SMALL_LOG2 = (-6.0, 5.0)                          # a quarter of the spread: |a| log-uniform over 2^-6 .. 2^5
PERIOD, PERIODIC_LS = 2.0, (1.0, 2.0 ** -5)
PERIODIC_SUB = 17                                 # at l = 1 (arguments in [-1, 0]) the first 17 rows and columns of the Periodic grid
PI_ERR = 1.2246467991473532e-16 / math.pi / EPS   # |fl(pi) - pi| / (pi eps) = 0.176
U_ANG = 0.5 + PI_ERR                              # relative error of the device's angle, in eps (module docstring)
DIMS = (2, 3, 4, 5, 8, 9, 16, 17, 31, 32)
GENERAL_DIMS = (3, 32)
GENERAL_R2_MAX = 1400.0


# ---- the argument of the exponential and its inverse ----------------------------------------------------------------------------------
def radius(kind, a):
    """the scaled distance r at which the argument of kind's exponential is a (without the 1e-12 under the root)"""
    if kind == "rbf":
        return math.sqrt(-2.0 * a)
    if kind == "matern12":
        return -a
    if kind == "exponential":
        return -2.0 * a
    if kind == "matern32":
        return -a / SQ3
    if kind == "matern52":
        return -a / SQ5
    return math.sqrt(2.0 * ALPHA * math.expm1(-a / ALPHA))


def _quant(kind, r, unit=2.0 ** -10):
    """the multiple of `unit` whose scaled value is nearest r"""
    return round(r / 2.0 ** LOG2K[kind] / unit) * unit


def coordinates(kind):
    """(s, t): the 65 row and 65 column coordinates of kind's grid, multiples of 2^-10 with |.| <= 40 (module docstring)"""
    rng = np.random.default_rng(708 + STATIONARY.index(kind))

    def spread(n):
        u = rng.random(n)
        small = n // 4
        r = [radius(kind, -2.0 ** (SMALL_LOG2[0] + (SMALL_LOG2[1] - SMALL_LOG2[0]) * v)) for v in u[:small]]
        r += [radius(kind, SPREAD_LO * v) for v in u[small:(n + small) // 2]]
        r += [math.sqrt(v) * radius(kind, SPREAD_LO) for v in u[(n + small) // 2:]]
        sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
        return [sg * _quant(kind, x) for sg, x in zip(sign, r)]

    s = [0.0] + spread(N - 1)
    lo, hi = _quant(kind, radius(kind, RUN_FROM)), _quant(kind, radius(kind, RUN_TO))
    stride = max(1, int(round((hi - lo) * 1024 / (RUN_LEN - 1))))
    run = [lo + q * stride * 2.0 ** -10 for q in range(RUN_LEN)]
    t = [0.0] + run + [_quant(kind, radius(kind, a)) for a in SINGLES] + spread(N - 1 - RUN_LEN - len(SINGLES))
    s, t = np.array(s), np.array(t)
    assert s.shape == t.shape == (N,) and max(np.abs(s).max(), np.abs(t).max()) <= 40.0
    assert np.all(s * 1024 == np.round(s * 1024)) and np.all(t * 1024 == np.round(t * 1024))
    return s, t


def periodic_coordinates():
    """(s, t) of the Periodic grid: points in [-2, 2] (one period each way), multiples of 2^-10 but for the run and the singles of
    row 1 (s = 1), which are multiples of 2^-14: at l = 2^-5 the argument there is -512 (1 + sin^2(pi t / 2))"""
    rng = np.random.default_rng(715)
    s = np.concatenate([[0.0, 1.0], np.round(rng.uniform(-2, 2, N - 2) * 1024) / 1024])

    def t_of(a):
        return round(2.0 / math.pi * math.asin(math.sqrt((-a - 512.0) / 512.0)) * 2 ** 14) / 2 ** 14

    lo, hi = t_of(RUN_FROM), t_of(RUN_TO)
    stride = max(1, int(round((hi - lo) * 2 ** 14 / (RUN_LEN - 1))))
    run = [lo + q * stride * 2.0 ** -14 for q in range(RUN_LEN)]
    t = np.concatenate([[0.0], run, [t_of(a) for a in SINGLES], np.round(rng.uniform(-2, 2, N - 1 - RUN_LEN - len(SINGLES)) * 1024) / 1024])
    assert s.shape == t.shape == (N,)
    return s, t


# ---- plain fp64 restatements of the device's formulas (kmat_prim_value), no fused operation ---------------------------------------------
def _map(f, x):
    x = np.asarray(x, dtype=np.float64)
    return np.array([f(float(v)) for v in x.ravel()]).reshape(x.shape)


def _exp(x):
    return _map(math.exp, x)


def restate(kind, r2, variance=1.0):
    """(value, a, pre) from the squared distance: the entry in the device's operation order, the argument of its exponential and
    variance x polynomial prefactor"""
    r2 = np.asarray(r2, dtype=np.float64)
    one = np.ones_like(r2)
    if kind == "rbf":
        a, pre = -r2 / 2.0, variance * one
    elif kind == "ratquad":
        a, pre = -ALPHA * _map(math.log1p, 0.5 * r2 * (1.0 / ALPHA)), variance * one
    else:
        r = np.sqrt(r2 + R_EPS)
        if kind == "matern12":
            a, pre = -r, variance * one
        elif kind == "exponential":
            a, pre = -0.5 * r, variance * one
        elif kind == "matern32":
            a, pre = -SQ3 * r, variance * (1.0 + SQ3 * r)
        else:
            a, pre = -SQ5 * r, variance * (1.0 + SQ5 * r + C53 * (r * r))
    return pre * _exp(a), a, pre


def dadr2(kind, r2):
    """g = |da / dr2| of the general-position unit"""
    r2 = np.asarray(r2, dtype=np.float64)
    if kind == "rbf":
        return 0.5 * np.ones_like(r2)
    c = {"matern12": 1.0, "exponential": 0.5, "matern32": SQ3, "matern52": SQ5}[kind]
    return c / (2.0 * np.sqrt(r2 + R_EPS))


def gemm_r2(X, X2, ls):
    """(r2, ni, nj, dot) of kernels.py:409-421 as the VALU kernels take it: features x / l, sequential sums, clamp at 0"""
    F, G = X / ls, X2 / ls
    ni, nj, dot = np.zeros(len(F)), np.zeros(len(G)), np.zeros((len(F), len(G)))
    for c in range(F.shape[1]):
        ni = ni + F[:, c] * F[:, c]
        nj = nj + G[:, c] * G[:, c]
        dot = dot + F[:, c][:, None] * G[:, c][None, :]
    nsum = ni[:, None] + nj[None, :]
    r2 = -2.0 * dot + nsum
    return np.where(r2 < 0.0, 0.0, r2), ni, nj, dot


def restate_periodic(X, X2, ls, variance=1.0):
    """(value, A, E) of the Periodic primitive over all columns of X: the cos / sin feature form of kmat_prim_value, the exponent
    and the first-order absolute error bound of the exponent (module docstring)"""
    D = X.shape[1]
    ang = 2.0 * math.pi * X / PERIOD
    bng = 2.0 * math.pi * X2 / PERIOD
    ca, sa, cb, sb = _map(math.cos, ang), _map(math.sin, ang), _map(math.cos, bng), _map(math.sin, bng)
    dot = np.zeros((len(X), len(X2)))
    lin = np.zeros_like(dot)
    for d in range(D):
        dot = dot + ca[:, d][:, None] * cb[:, d][None, :]
        dot = dot + sa[:, d][:, None] * sb[:, d][None, :]
        sdiff = np.abs(sa[:, d][:, None] * cb[:, d][None, :] - ca[:, d][:, None] * sb[:, d][None, :])
        lin = lin + sdiff * (np.abs(ang[:, d])[:, None] + np.abs(bng[:, d])[None, :])
    rs = (0.5 * D - 0.5 * dot) / (ls * ls)
    A = -0.5 * rs
    E = EPS / (4.0 * ls * ls) * (U_ANG * lin + 2.0 * D + float(D) * D)
    return variance * _exp(A), A, E


# ---- the fixture and the grids ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def grid(kind):
    """the exact grid of one stationary kind: s, t (the fixture's), k, S, T, r2 [65, 65] (exact), a, pre (variance 1), ref"""
    fx = fixture()
    s, t = fx[kind + "/s"], fx[kind + "/t"]
    k = LOG2K[kind]
    S, T = s * 2.0 ** k, t * 2.0 ** k
    r2 = (S * S)[:, None] + (T * T)[None, :]
    val, a, pre = restate(kind, r2)
    return dict(kind=kind, s=s, t=t, k=k, S=S, T=T, r2=r2, a=a, pre=pre, val=val, ref=fx[kind + "/K"])


@functools.lru_cache(maxsize=None)
def periodic_grid(ls):
    """the Periodic grid at lengthscale ls in two dimensions: X, X2, A, E, val (fp64 restatement), ref"""
    fx = fixture()
    s, t = fx["periodic/s"], fx["periodic/t"]
    if ls == PERIODIC_LS[0]:
        s, t = s[:PERIODIC_SUB], t[:PERIODIC_SUB]
    X, X2 = np.stack([s, 0 * s], axis=1), np.stack([0 * t, t], axis=1)
    val, A, E = restate_periodic(X, X2, ls)
    return dict(kind="periodic", s=s, t=t, ls=ls, X=X, X2=X2, a=A, E=E, pre=np.ones_like(A), val=val,
                ref=fx["periodic/K_l%d" % PERIODIC_LS.index(ls)])


def points(s, t, D=2, p=0, q=1, scale_p=1.0, scale_q=1.0, offsets=None):
    """X = s scale_p e_p (+ offsets), X2 = t scale_q e_q (+ offsets): rows and columns on two different axes"""
    assert p != q
    X, X2 = np.zeros((len(s), D)), np.zeros((len(t), D))
    if offsets is not None:
        X[:] = offsets
        X2[:] = offsets
        X[:, q] = 0.0
        X2[:, p] = 0.0
    X[:, p] = s * scale_p
    X2[:, q] = t * scale_q
    return X, X2


def dim_case(kind, D, which):
    """(X, X2, ls, p, q) of the D-dimensional case `which` in 0, 1, 2 for one stationary kind or "periodic": ARD lengthscales
    2^((c mod 3) - 1) (Periodic: the one lengthscale 2^-5), (p, q) one of (0, D - 1), (D - 1, 0), (D // 2, D // 2 - 1), the same
    non-zero offset w_c (a multiple of 2^-3) on every other axis of every point, and the scaled coordinates of the kind's grid"""
    p, q = ((0, D - 1), (D - 1, 0), (D // 2, D // 2 - 1))[which]
    w = np.array([(1 + (3 * c) % 8) / 8.0 * (-1.0) ** c for c in range(D)])
    w[[p, q]] = 0.0
    if kind == "periodic":
        g = periodic_grid(PERIODIC_LS[1])
        X, X2 = points(g["s"], g["t"], D, p, q, offsets=w)
        return X, X2, PERIODIC_LS[1], p, q
    ls = np.array([2.0 ** ((c % 3) - 1) for c in range(D)])
    g = grid(kind)
    X, X2 = points(g["S"], g["T"], D, p, q, ls[p], ls[q], offsets=w)
    return X, X2, ls, p, q


@functools.lru_cache(maxsize=None)
def general_case(kind, D):
    """general position, the symmetric build K(X) of 65 points: X [65, D] (the fixture's), ARD lengthscales, the GEMM-form
    restatement, the unit's extra term and the reference (the fixture keeps its upper triangle, row by row)"""
    fx = fixture()
    X = fx["general/X_d%d" % D]
    ls = np.array([2.0 ** ((c % 3) - 1) for c in range(D)])
    r2, ni, nj, dot = gemm_r2(X, X, ls)
    val, a, pre = restate(kind, r2)
    extra = dadr2(kind, r2) * (ni[:, None] + nj[None, :] + 2.0 * np.abs(dot))
    ref = np.zeros((N, N))
    ref[np.triu_indices(N)] = fx["general/%s_d%d" % (kind, D)]
    ref = np.triu(ref) + np.triu(ref, 1).T
    return dict(kind=kind, X=X, ls=ls, r2=r2, a=a, pre=pre, val=val, extra=extra, ref=ref)


def general_points(D):
    """the seeded general-position inputs the generator stores: 65 standard-normal points, scaled so that the largest r2 is 1400"""
    X = np.random.default_rng(1400 + D).standard_normal((N, D))
    ls = np.array([2.0 ** ((c % 3) - 1) for c in range(D)])
    return X * math.sqrt(GENERAL_R2_MAX / gemm_r2(X, X, ls)[0].max())


# ---- units, own and the comparison -----------------------------------------------------------------------------------------------------
def unit(ref, a, roundings=1.0, extra=0.0):
    """eps (roundings + |a| + extra) |ref| ; `extra` is E / eps for Periodic and g (ni + nj + 2 |dot|) in general position"""
    return EPS * (roundings + np.abs(a) + extra) * np.abs(ref)


def errors(got, ref, a, pre, u):
    """(worst error / unit over the relative domain, worst |got - ref| / (pre 2^-1021) over the tail, entries of each domain)"""
    got = np.asarray(got, dtype=np.float64)
    rel = a >= A_EDGE
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(rel, np.where(err == 0.0, 0.0, err / u), 0.0)
    worst_rel = float(q.max()) if rel.any() else 0.0
    worst_tail = float((err / (pre * TAIL_ABS))[~rel].max()) if (~rel).any() else 0.0
    return worst_rel, worst_tail, int(rel.sum()), int((~rel).sum())


def own_raw(case, roundings=1.0, val=None):
    """the fp64 restatement's worst distance from the fixture over the relative domain, in units"""
    extra = case["E"] / EPS if "E" in case else case.get("extra", 0.0)
    return errors(case["val"] if val is None else val, case["ref"], case["a"], case["pre"], unit(case["ref"], case["a"], roundings, extra))[0]


def own_reference(case, roundings=1.0):
    """the fixture's own error in units: it holds the exact value rounded to fp64, up to half a spacing away from it"""
    extra = case["E"] / EPS if "E" in case else case.get("extra", 0.0)
    u = unit(case["ref"], case["a"], roundings, extra)
    rel = (case["a"] >= A_EDGE) & (case["ref"] > 0.0)
    return float((0.5 * np.spacing(case["ref"][rel]) / u[rel]).max())


def own_of(case, roundings=1.0, val=None):
    """own of the gate: the restatement's distance from the fixture, and no less than the fixture's own rounding.  The second
    term decides for RBF alone (and for Periodic at l = 1): its argument -r2 / 2 is exact and glibc's exp returns the correctly
    rounded double at all but a few of the sampled arguments, so the restatement EQUALS the fixture nearly everywhere (0.0015
    units, from one-ulp differences at |a| ~ 700) -- which says that the fixture cannot tell two neighbouring doubles apart, not
    that an fp64 evaluation is that near the exact value: the correctly rounded double itself is up to 0.5 units from it at a = 0."""
    return max(own_raw(case, roundings, val), own_reference(case, roundings))


@functools.lru_cache(maxsize=None)
def own_grid(kind, ls=None):
    """own of a stationary kind's grid, of the Periodic grid at lengthscale ls, or ("product") of the Product of two RBF factors,
    one per axis, against the RBF grid with one more rounding in the unit"""
    if kind == "periodic":
        return own_of(periodic_grid(ls))
    if kind == "product":
        g = grid("rbf")
        return own_of(g, 2.0, _exp(-(g["S"] * g["S"]) / 2.0)[:, None] * _exp(-(g["T"] * g["T"]) / 2.0)[None, :])
    return own_of(grid(kind))


def periodic_dim_case(D, which):
    """the D-dimensional Periodic case as a case dictionary (its restatement, unit term and own are those of D dimensions; the
    reference is the two-dimensional grid's: the offsets are common to both points)"""
    X, X2, ls, p, q = dim_case("periodic", D, which)
    val, A, E = restate_periodic(X, X2, ls)
    g = periodic_grid(ls)
    return dict(kind="periodic", X=X, X2=X2, ls=ls, a=A, E=E, pre=np.ones_like(A), val=val, ref=g["ref"])


def check(got, case, own, variance=1.0, roundings=1.0, what=""):
    """The comparison of one built matrix with its case: every entry of the relative domain within LD_OWN_FACTOR x own x unit, the
    tail non-negative, finite and within pre 2^-1021.  Returns (worst error / gate, worst tail error / bound)."""
    got = np.asarray(got, dtype=np.float64)
    ref, a, pre = variance * case["ref"], case["a"], variance * case["pre"]
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert own > 0.0
    extra = case["E"] / EPS if "E" in case else case.get("extra", 0.0)
    u = unit(ref, a, roundings, extra)
    assert np.all(np.isfinite(got)) and np.all(got >= 0.0), (what, "not finite or negative")
    worst_rel, worst_tail, n_rel, n_tail = errors(got, ref, a, pre, u)
    ratio = worst_rel / (LD_OWN_FACTOR * own)
    print("%s: relative domain %d entries, worst error %.3g units = %.3g of the gate (own %.3g); tail %d entries, worst %.3g of pre 2^-1021"
          % (what, n_rel, worst_rel, ratio, own, n_tail, worst_tail))
    if ratio > 1.0:
        rel = a >= A_EDGE
        with np.errstate(divide="ignore", invalid="ignore"):
            qq = np.where(rel, np.abs(got - ref) / u, 0.0)
        i, j = np.unravel_index(int(np.argmax(qq)), qq.shape)
        raise AssertionError("%s: entry (%d, %d) a = %.17g: got %.17g, reference %.17g, %.3g units > gate %.3g units"
                             % (what, i, j, a[i, j], got[i, j], ref[i, j], qq[i, j], LD_OWN_FACTOR * own))
    assert worst_tail <= 1.0, (what, "tail", worst_tail)
    return ratio, worst_tail
