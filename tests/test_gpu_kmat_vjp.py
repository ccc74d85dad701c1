"""The two kernel-matrix VJPs of csrc/grad_general.hip -- gg_kernel in rect mode (handle.kmat_vjp: the parameter slots) and
gg_input_kernel (handle.kmat_input_vjp: the gradient with respect to the points) -- for RBF, Matern12/32/52, Exponential,
Periodic, White and Constant, alone and in Sum / Product programs: EVERY slot and EVERY entry against the analytic reference
tests/_kern_ref.py (numpy; itself within 1e-13 of the same formulas at 50 digits, tests/test_kern_ref_cpu.py), at the tile and
pad edges, with several column tiles per slice, over permuted / partial / full dimension maps, on coincident and nearly
coincident points, with a short Periodic lengthscale, and where the kernel value underflows.

Bound: the suite's analytic-reference bound for these entry points (tests/test_gpu_newkernels.py::test_kernel_matrix_vjps),
|got - ref| <= 1e-10 max(1, scale) with scale = max |ref| over the output; for points 1e-5 apart, where single terms dwarf their
sum, scale is the reference's own sum_ij |W_ij| |d k_ij| of that slot / entry.  For K(X, X) both arguments move: the input
reference is input_vjp(W) + input_vjp(W.T).  Every test prints its worst error / max(1, scale); docs/LAB_NOTES.md keeps them."""
import numpy as np
import pytest

import _kern_ref as kr
from _kern_ref import spec_of

pytestmark = pytest.mark.gpu

TOL = 1e-10
STATIONARY = ("RBF", "Matern12", "Matern32", "Matern52", "Exponential")


def _alone(gpf, d=3):
    """each kernel alone over all d dims, and each stationary one over active_dims=[2, 0] of 3"""
    k = gpf.kernels
    ls = np.linspace(0.8, 1.7, d)
    out = {"rbf_iso": k.RBF(d, variance=1.2, lengthscales=1.6),
           "rbf_ard": k.RBF(d, variance=1.3, lengthscales=ls, ARD=True),
           "matern12": k.Matern12(d, variance=0.7, lengthscales=ls * 1.2, ARD=True),
           "matern32": k.Matern32(d, variance=1.1, lengthscales=ls * 1.3, ARD=True),
           "matern52": k.Matern52(d, variance=0.9, lengthscales=ls * 1.5, ARD=True),
           "exponential": k.Exponential(d, variance=1.2, lengthscales=ls * 0.9, ARD=True),
           "periodic": k.Periodic(d, period=2.5, variance=0.8, lengthscales=1.2),
           "white": k.White(d, variance=0.2),
           "constant": k.Constant(d, variance=0.4)}
    if d == 3:
        for name in STATIONARY:
            out[name.lower() + "_subset"] = getattr(k, name)(2, variance=1.1, lengthscales=[0.9, 1.4], ARD=True, active_dims=[2, 0])
    return out


def _programs(gpf):
    """the two programs of test_gpu_grad.py::_cases, and one of eight primitives (GG_MAXP) whose postfix form
    rbf per * m12 m32 const + * + exp m52 * + white +  reaches a stack depth of 4 (GPS_MAX_STACK)"""
    from test_gpu_grad import _cases
    k = gpf.kernels
    d = 3
    ls = np.linspace(0.8, 1.7, d)
    eight = k.Sum([k.Product([k.RBF(d, variance=1.2, lengthscales=ls, ARD=True), k.Periodic(d, period=3.0, variance=0.9, lengthscales=1.5)]),
                   k.Product([k.Matern12(2, variance=0.7, lengthscales=[2.0, 1.1], ARD=True, active_dims=[2, 0]),
                              k.Sum([k.Matern32(d, variance=1.1, lengthscales=1.9), k.Constant(d, variance=0.4)])]),
                   k.Product([k.Exponential(d, variance=1.2, lengthscales=ls * 0.9, ARD=True), k.Matern52(1, variance=0.9, lengthscales=1.4, active_dims=[1])]),
                   k.White(d, variance=0.2)])
    nodes = eight._nodes(False, d)
    assert sum(1 for nd in nodes if nd.op < 16) == 8
    return {"m52_plus_periodic": _cases(gpf, d)["m52_plus_periodic"]()[0],
            "rbf_times_periodic_plus_white": _cases(gpf, d)["rbf_times_periodic_plus_white"]()[0], "eight": eight}


def _check(handle, kern, X, W, X2=None, absolute=False):
    """every slot and every input-gradient entry within TOL max(1, scale); -> the two worst error / max(1, scale)"""
    d = X.shape[1]
    spec = spec_of(kern, d)
    prog = kern._program(d)
    got = handle.kmat_vjp(prog, X, W, X2)
    ref = kr.vjp_slots(spec, W, X, X2)
    assert got.shape == ref.shape
    assert np.isfinite(got).all() and np.isfinite(ref).all()
    scale = kr.vjp_slots(spec, W, X, X2, absolute=True) if absolute else np.abs(ref).max()
    worst_s = float(np.max(np.abs(got - ref) / np.maximum(1.0, scale)))
    gX = handle.kmat_input_vjp(prog, X, W, X2)
    rX = kr.input_vjp(spec, W, X, X2)
    sX = kr.input_vjp(spec, W, X, X2, absolute=True) if absolute else None
    if X2 is None:                                            # K(X, X): both arguments move
        rX = rX + kr.input_vjp(spec, W.T, X, X2)
        if absolute:
            sX = sX + kr.input_vjp(spec, W.T, X, X2, absolute=True)
    assert gX.shape == rX.shape == X.shape
    assert np.isfinite(gX).all() and np.isfinite(rX).all()
    if not absolute:
        sX = np.abs(rX).max()
    worst_x = float(np.max(np.abs(gX - rX) / np.maximum(1.0, sX)))
    # a column of X no primitive reads receives nothing at all
    touched = sorted({c for leaf in kr.leaves(spec) for c in leaf["dims"]})
    untouched = [c for c in range(d) if c not in touched]
    assert np.all(gX[:, untouched] == 0.0)
    assert worst_s <= TOL, ("slots", worst_s, got, ref)
    assert worst_x <= TOL, ("input", worst_x)
    return worst_s, worst_x


def _report(label, worst):
    print("%s: worst slot %.2e, worst input entry %.2e (of max(1, scale); bound %.0e)"
          % (label, max(w[0] for w in worst), max(w[1] for w in worst), TOL))


_RECT = [(1, 1), (31, 33), (32, 32), (33, 31), (127, 129), (128, 128), (129, 127)]
_SQUARE = [(1, None), (33, None), (128, None), (129, None)]


@pytest.mark.parametrize("weights", ["random", "ones"])
@pytest.mark.parametrize("nr,nc", _RECT + _SQUARE)
def test_tile_and_pad_edges(handle, nr, nc, weights):
    """32 x 32 tiles, a thread owns a 2 x 2 patch, the feature rows are padded to 128 with zeros -- a real point at the origin
    with a non-zero kernel value that only the i < nr && j < nc mask on W keeps out.  W = ones makes a masking error visible
    (a zero-mean W averages most of it away).  Every kernel alone at (33, 31) and n = 33; elsewhere RBF-ARD, Matern12, Periodic
    and the programs."""
    import gpflowSlim as gpf
    rng = np.random.default_rng(1000 * nr + (nc or 0))
    X = rng.standard_normal((nr, 3)); X2 = None if nc is None else rng.standard_normal((nc, 3))
    shape = (nr, nr if nc is None else nc)
    W = np.ones(shape) if weights == "ones" else rng.standard_normal(shape)
    kerns = dict(_programs(gpf))
    alone = _alone(gpf)
    kerns.update(alone if (nr, nc) in ((33, 31), (33, None)) else {q: alone[q] for q in ("rbf_ard", "matern12", "periodic")})
    worst = [_check(handle, kern, X, W, X2) for kern in kerns.values()]
    _report("edges %s %s" % (shape, weights), worst)


@pytest.mark.parametrize("nr,nc", [(40, 2100), (129, 2049), (40, 2150)])
def test_many_column_tiles_per_slice(handle, nr, nc):
    """gps_launch_kmat_input_vjp: slices = min(2048 / tiles, tiles_c, 64), per = ceil(tiles_c / slices) column tiles each.
    (40, 2100): rows pad to 128, tiles = 4; columns pad to 2176, tiles_c = 68; slices = 64, per = 2: slices 0..33 hold two
    tiles each, slices 34..63 start past the last tile and must add exactly zero.  (129, 2049): tiles = 8, tiles_c = 68, the same
    64 slices of 2; column 2048 is alone in tile 64, the first of slice 32.  In both, tiles 66 and 67 are padding only;
    (40, 2150) has data up to the last tile (67, the second of slice 33)."""
    import gpflowSlim as gpf
    rng = np.random.default_rng(nr + nc)
    X = rng.standard_normal((nr, 3)); X2 = rng.standard_normal((nc, 3))
    W = rng.standard_normal((nr, nc))
    kerns = {"rbf_ard": _alone(gpf)["rbf_ard"], "matern32": _alone(gpf)["matern32"], "m52_plus_periodic": _programs(gpf)["m52_plus_periodic"]}
    worst = [_check(handle, kern, X, W, X2) for kern in kerns.values()]
    _report("slices (%d, %d)" % (nr, nc), worst)
    worst = [_check(handle, kerns["rbf_ard"], X, np.ones((nr, nc)), X2)]
    _report("slices (%d, %d) ones" % (nr, nc), worst)


def _dimension_kernels(gpf, which):
    k = gpf.kernels
    if which == "d1":
        return 1, [k.RBF(1, variance=1.3, lengthscales=0.8), k.Matern12(1, variance=0.7, lengthscales=1.1),
                   k.Matern32(1, variance=1.1, lengthscales=1.2), k.Matern52(1, variance=0.9, lengthscales=1.4),
                   k.Exponential(1, variance=1.2, lengthscales=0.9), k.Periodic(1, period=2.5, variance=0.8, lengthscales=1.2)]
    if which == "rbf_ard_32_of_32":                           # fills rowacc[row][0..31] and the 32 feature rows
        return 32, [k.RBF(32, variance=1.3, lengthscales=np.linspace(4.0, 7.0, 32), ARD=True)]
    if which == "matern52_5_of_32":
        return 32, [k.Matern52(5, variance=0.9, lengthscales=np.linspace(1.5, 2.5, 5), ARD=True, active_dims=[17, 3, 31, 0, 9])]
    if which == "periodic_21_of_32":                          # 3 feature rows per dim: 63 of GRAD_MAXF = 64
        return 32, [k.Periodic(21, period=2.5, variance=0.8, lengthscales=3.0, active_dims=list(range(31, 10, -1)))]
    raise KeyError(which)


@pytest.mark.parametrize("which", ["d1", "rbf_ard_32_of_32", "matern52_5_of_32", "periodic_21_of_32"])
def test_dimension_mapping(handle, which):
    """rowacc[row][ft.dim] scatters by the ORIGINAL column of X: d_all = 1, all of GPS_MAX_DIMS = 32, a permuted 5-subset of 32,
    and Periodic at the 21 dims its three feature rows per dim allow; the columns nobody reads are exactly 0.0 (_check)."""
    import gpflowSlim as gpf
    d, kerns = _dimension_kernels(gpf, which)
    rng = np.random.default_rng(d)
    worst = []
    for nr, nc in ((33, 31), (33, None)):
        X = rng.standard_normal((nr, d)); X2 = None if nc is None else rng.standard_normal((nc, d))
        for W in (rng.standard_normal((nr, nc or nr)), np.ones((nr, nc or nr))):
            worst += [_check(handle, kern, X, W, X2) for kern in kerns]
    _report("dims " + which, worst)


def test_periodic_over_22_dims_is_refused(handle):
    import gpflowSlim as gpf
    rng = np.random.default_rng(22)
    X = rng.standard_normal((33, 32)); X2 = rng.standard_normal((31, 32)); W = rng.standard_normal((33, 31))
    kern = gpf.kernels.Periodic(22, period=2.5, variance=0.8, lengthscales=3.0, active_dims=list(range(22)))
    with pytest.raises(RuntimeError, match="too many active dims"):
        handle.kmat_vjp(kern._program(32), X, W, X2)
    with pytest.raises(RuntimeError, match="too many active dims"):
        handle.kmat_input_vjp(kern._program(32), X, W, X2)


def _coincident(rng, shift):
    """X [70, 3]; X2 [45, 3]: 20 rows of X bit for bit (moved by `shift` in one coordinate) and 25 fresh ones"""
    X = rng.standard_normal((70, 3))
    rows = rng.choice(70, 20, replace=False)
    X2 = np.vstack([X[rows], rng.standard_normal((25, 3))])
    X2[:20, 1] += shift
    X2 = X2[rng.permutation(45)].copy()
    return X, X2


@pytest.mark.parametrize("name", [s.lower() for s in STATIONARY] + [s.lower() + "_subset" for s in STATIONARY] + ["rbf_ard", "periodic"])
def test_coincident_points(handle, name):
    """Inducing points start as a subset of the data: K(Z, X) has entries at r = 0, where grad_dk_dq2 is -k / (2 sqrt(1e-12)) =
    -5e5 k for Matern12 (half of it for Exponential) times a difference that must be exactly 0 -- rectangular with 20 copied
    rows, and K(X, X), whose whole diagonal is r = 0.  Finite and within the bound."""
    import gpflowSlim as gpf
    kern = dict(_alone(gpf), rbf=_alone(gpf)["rbf_iso"])[name]
    rng = np.random.default_rng(70)
    X, X2 = _coincident(rng, 0.0)
    assert sum(1 for a in X2 for b in X if np.array_equal(a, b)) == 20
    worst = []
    for B in (X2, None):
        shape = (70, 70 if B is None else 45)
        for W in (rng.standard_normal(shape), np.ones(shape)):
            worst.append(_check(handle, kern, X, W, B))
    _report("coincident " + name, worst)


@pytest.mark.parametrize("name", ["matern12", "exponential", "matern32"])
def test_points_1e5_apart(handle, name):
    """20 columns 1e-5 from a row in one coordinate: d k / d r2 ~ 1 / rad is 5e4 k for Matern12 and the difference it multiplies
    is 1e-5, not 0.  scale: the reference's sum of absolute terms of each slot / entry."""
    import gpflowSlim as gpf
    kern = _alone(gpf)[name]
    rng = np.random.default_rng(71)
    X, X2 = _coincident(rng, 1e-5)
    worst = [_check(handle, kern, X, W, X2, absolute=True) for W in (rng.standard_normal((70, 45)), np.ones((70, 45)))]
    _report("1e-5 apart " + name, worst)


def test_periodic_short_lengthscale(handle):
    """lengthscales = 0.05, period = 2.5, half of X2 within 1e-4 of rows of X: grad_periodic_value forms
    S = (ndims - sum(cos cos + sin sin)) / 2, which has no relative accuracy left for such pairs, and divides it by l^2 = 0.0025.
    (Pairs further apart have k = exp(-200 S) ~ 0: only the near ones carry the sums.)"""
    import gpflowSlim as gpf
    rng = np.random.default_rng(72)
    X = rng.standard_normal((70, 3))
    X2 = rng.standard_normal((45, 3))
    near = rng.choice(45, 22, replace=False)
    X2[near] = X[rng.choice(70, 22, replace=False)] + 1e-4 * rng.uniform(-1.0, 1.0, (22, 3))
    kern = gpf.kernels.Periodic(3, period=2.5, variance=0.8, lengthscales=0.05)
    worst = [_check(handle, kern, X, W, X2) for W in (rng.standard_normal((70, 45)), np.ones((70, 45)))]
    _report("periodic l = 0.05", worst)


@pytest.mark.parametrize("name", ["rbf_ard", "matern12"])
def test_underflow_between_clusters(handle, name):
    """Two clusters 60 (of the largest) lengthscales apart: RBF's k = exp(-r2 / 2) underflows to 0 across them and the slots
    and input gradients must be finite, 0 k and not 0 * inf.  With a cotangent that only weighs cross-cluster pairs the RBF
    outputs are exactly zero, as the reference's; Matern12 (k ~ e^-60) is within the bound."""
    import gpflowSlim as gpf
    kern = _alone(gpf)[name]
    rng = np.random.default_rng(73)
    ls_max = float(np.max(kern.lengthscales))
    X = 0.5 * rng.standard_normal((70, 3)); X[40:, 0] += 60.0 * ls_max
    X2 = 0.5 * rng.standard_normal((45, 3)); X2[:15, 0] += 60.0 * ls_max
    cross = (np.arange(70)[:, None] >= 40) != (np.arange(45)[None, :] < 15)
    W = rng.standard_normal((70, 45))
    worst = [_check(handle, kern, X, W, X2), _check(handle, kern, X, np.ones((70, 45)), X2), _check(handle, kern, X, W * cross, X2)]
    crossX = (np.arange(70)[:, None] >= 40) != (np.arange(70)[None, :] >= 40)
    Ws = rng.standard_normal((70, 70))
    worst += [_check(handle, kern, X, Ws, None), _check(handle, kern, X, Ws * crossX, None)]
    if name == "rbf_ard":
        prog, spec = kern._program(3), spec_of(kern, 3)
        assert np.all(kr.K(spec, X, X2, diff=True)[cross] == 0.0)
        assert np.all(kr.vjp_slots(spec, W * cross, X, X2) == 0.0) and np.all(kr.input_vjp(spec, W * cross, X, X2) == 0.0)
        assert np.all(handle.kmat_vjp(prog, X, W * cross, X2) == 0.0) and np.all(handle.kmat_input_vjp(prog, X, W * cross, X2) == 0.0)
        assert np.all(handle.kmat_vjp(prog, X, Ws * crossX) == 0.0) and np.all(handle.kmat_input_vjp(prog, X, Ws * crossX) == 0.0)
    _report("underflow " + name, worst)


@pytest.mark.parametrize("nr,nc", [(129, 127), (40, 2100)])
def test_same_call_twice_is_bitwise_equal(handle, nr, nc):
    """fixed-order partial sums, no floating-point atomics: one rectangular and one many-slice shape"""
    import gpflowSlim as gpf
    rng = np.random.default_rng(nr)
    X = rng.standard_normal((nr, 3)); X2 = rng.standard_normal((nc, 3)); W = rng.standard_normal((nr, nc))
    for kern in (_programs(gpf)["m52_plus_periodic"], _programs(gpf)["eight"]):
        prog = kern._program(3)
        a, b = handle.kmat_vjp(prog, X, W, X2), handle.kmat_vjp(prog, X, W, X2)
        assert np.array_equal(a, b) and np.abs(a).max() > 0.0
        a, b = handle.kmat_input_vjp(prog, X, W, X2), handle.kmat_input_vjp(prog, X, W, X2)
        assert np.array_equal(a, b) and np.abs(a).max() > 0.0
