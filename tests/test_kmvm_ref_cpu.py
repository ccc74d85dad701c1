"""CPU proof of what tests/test_gpu_kmvm_large.py stands on (no GPU):

  * the row / column references of tests/_kmvm_ref.py (product_rows, K_rows, factor_columns, sample_rows) against the dense
    long-double ones of the small-n tests, at n = 130 and 200, to long-double rounding;
  * the launch-geometry thresholds that file's sizes are chosen against, read from the project's own sources (csrc/kmat_common.hpp,
    csrc/kmvm.hip, csrc/pchol.hip), and every size of that file restated against them.  A retune that moves a threshold above a
    size fails here and names the case that has gone blind.
"""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "gpflow-slim_amd"))
import _kern_ref as kr  # noqa: E402
import _kmvm_ref as mr  # noqa: E402
import test_gpu_kmvm_large as big  # noqa: E402
from test_gpu_pchol import _factor  # noqa: E402

CSRC = os.path.join(os.path.dirname(HERE), "gpflow-slim_amd", "csrc")
LD = mr.LD
EPS_LD = float(np.finfo(LD).eps)
EPS = np.finfo(np.float64).eps


def _case(kind, n, T, seed):
    rng = np.random.default_rng(seed)
    return mr.leaf(kind, range(3), seed), rng.normal(size=(n, 3)), rng.normal(size=(n, T))


# ---- the references ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rbf", "matern52"])
@pytest.mark.parametrize("n", [130, 200])
def test_product_rows_is_product(kind, n):
    """on every row, and on a shuffled subset: the dense product's entries to long-double rounding of their scale.  (Kernels flat
    at r = 0: the r2 = 0 of the rows' diagonal convention moves nothing there.)"""
    lf, X, V = _case(kind, n, 17, n)
    ref, scale, spread = mr.product(lf, X, V, None, 0.37)
    for rows in (np.arange(n), np.random.default_rng(1).permutation(n)[:37]):
        r, s, sp = mr.product_rows(lf, X, V, rows, 0.37)
        assert r.dtype == LD and r.shape == (len(rows), 17)
        assert np.all(np.abs(r - ref[rows]) <= 8 * EPS_LD * scale[rows])
        assert np.all(np.abs(s - scale[rows]) <= 8 * EPS_LD * scale[rows])
        assert sp <= spread + 4 * EPS and (len(rows) < n or sp >= spread - 4 * EPS)
    assert spread <= 1e-14


def test_product_rows_diagonal_convention():
    """Matern12 is not flat at r = 0: entry (i, rows[i]) is variance exp(-sqrt(1e-12)) exactly -- r2 = 0 --, every other entry K_ld's"""
    lf, X, _ = _case("matern12", 130, 1, 5)
    rows = np.array([129, 0, 64, 7])
    Kr, Kd = mr.K_rows(lf, X, rows), mr.K_ld(lf, X)
    exact = LD(lf["variance"]) * np.exp(-np.sqrt(LD(1e-12)))
    assert np.all(Kr[np.arange(4), rows] == exact)
    off = np.ones(Kr.shape, dtype=bool)
    off[np.arange(4), rows] = False
    assert np.array_equal(Kr[off], Kd[rows][off])


def _greedy_pivots(K, k):
    """the factor's own pivot rule on a dense fp64 K: the largest residual diagonal entry, ties to the lowest index"""
    d, L, piv = np.diag(K).copy(), np.zeros((K.shape[0], k)), []
    for m in range(k):
        p = int(np.argmax(d))
        piv.append(p)
        L[:, m] = (K[:, p] - L[:, :m] @ L[p, :m]) / np.sqrt(d[p])
        d = np.maximum(d - np.square(L[:, m]), 0)
        d[p] = 0
    return np.array(piv)


@pytest.mark.parametrize("kind,n,k", [("rbf", 130, 33), ("matern32", 200, 64)])
def test_factor_columns_is_factor(kind, n, k):
    """against _factor on the dense long-double K with the same pivots: L per column scale, d, d_p and dmax to long-double rounding
    (a step divides by sqrt(d_p) and the errors of the earlier columns travel: k steps' worth of a few eps)"""
    lf, X, _ = _case(kind, n, 1, 10 * n)
    piv = _greedy_pivots(kr.K(lf, X), k)
    assert piv[0] == 0 and len(set(piv.tolist())) == k
    L, d, dp, dmax = mr.factor_columns(lf, X, piv, LD)
    Lr, dr, dpr, dmaxr = _factor(mr.K_ld(lf, X), piv, LD)
    var = lf["variance"]
    col = np.sqrt(dpr) / var
    tol = 8 * k * EPS_LD / float(np.min(dpr) / var)             # (the residual's rounding relative to the smallest pivot)
    assert L.dtype == LD and L.shape == (n, k)
    assert float(np.max(np.abs(L - Lr) * col)) <= tol
    assert float(np.max(np.abs(d - dr))) <= tol * var and float(np.max(np.abs(dp - dpr))) <= tol * var
    assert float(np.max(np.abs(dmax - dmaxr))) <= tol * var
    L64 = mr.factor_columns(lf, X, piv, np.float64)[0]
    assert L64.dtype == np.float64 and float(np.max(np.abs(L64 - Lr) * col)) <= 1e-9


@pytest.mark.parametrize("n", [130, 200])
def test_rows_of_dense_system(n):
    """the residual the large CG test forms from K_rows is the dense one's rows"""
    lf, X, B = _case("rbf", n, 3, 3 * n)
    A, _ = mr.dense(lf, X, 0.5)
    x = np.asarray(mr.solve(A, B), dtype=np.float64) * (1 + 1e-6)
    rows = mr.sample_rows(n)
    xl = x.astype(LD)
    got = mr.K_rows(lf, X, rows) @ xl + LD(0.5) * xl[rows]
    assert np.all(np.abs(got - (A @ xl)[rows]) <= 8 * EPS_LD * (np.abs(A) @ np.abs(xl))[rows])


def test_sample_rows():
    assert np.array_equal(mr.sample_rows(1), [0]) and np.array_equal(mr.sample_rows(130), np.r_[0:64, 66:130])
    assert np.array_equal(mr.sample_rows(2112), np.r_[0:64, 2048:2112])
    assert np.array_equal(mr.sample_rows(4200), np.r_[0:64, 4096:4200])
    r = mr.sample_rows(8300)
    assert np.array_equal(r, np.r_[0:64, 4096:4160, 8160:8300]) and len(r) <= 300
    r = mr.sample_rows(65600)
    assert len(r) <= 364 and {8160, 8191, 8192, 65599} <= set(r.tolist()) and np.all(np.diff(r) > 0)


# ---- the thresholds, from the sources -----------------------------------------------------------------------------------------------
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _body(text, head):
    """the source from the line that starts the definition `head` to its closing brace at column 0"""
    at = text.index(head)
    return text[at:text.index("\n}", at)]


def _one(pattern, text, what):
    m = re.findall(pattern, text)
    assert len(m) == 1, "%s: expected one match of %r, found %d -- the geometry has been edited; revisit test_gpu_kmvm_large.py" % (
        what, pattern, len(m))
    return m[0]


@pytest.fixture(scope="module")
def geo():
    """the launch geometry as the sources state it"""
    g = {"max_blocks": int(_one(r"#define KCG_MAX_BLOCKS (\d+)", _src("kmat_common.hpp"), "KCG_MAX_BLOCKS"))}
    ws = _body(_src("pchol.hip"), "size_t gps_pchol_workspace(")
    g["gb"] = int(_one(r"pre->gb = \(int\)\(tiles < (\d+) \? tiles : \1\);", ws, "gb"))
    g["tg"] = int(_one(r"pre->tg = \(int\)\(tiles < (\d+) \? tiles : \1\);", ws, "tg"))
    _one(r"pre->lsg = \(int\)\(tiles < KCG_MAX_BLOCKS \? tiles : KCG_MAX_BLOCKS\);", ws, "lsg")
    _one(r"const int nblk = \(int\)\(\(np \+ 255\) / 256\);", ws, "pchol nblk")
    _one(r"const i64 tiles = np / 64;", ws, "pchol tiles")
    _one(re.escape("static i64 pchol_rows_per_block(i64 np, int blocks) { return ((np / 4 + blocks - 1) / blocks) * 4; }"),
         _src("pchol.hip"), "pchol_rows_per_block")
    kv = _src("kmvm.hip")
    ch = _body(kv, "int gps_kmvm_chunks(")
    g["chunk_wgs"] = int(_one(r"\((\d+) \+ row_tiles - 1\) / row_tiles", ch, "chunk rule"))
    g["chunk_cap"] = int(_one(r"if \(forced <= 0 && ch > (\d+)\) ch = \1;", ch, "chunk cap"))
    _one(r"const i64 b = \(npad \+ 15\) / 16;", _body(kv, "int gps_kcg_blocks("), "gps_kcg_blocks")
    _one(r"const i64 nrow = \(n \+ 255\) / 256;", _body(kv, "int gps_launch_kmvm_grad("), "grad nblk")
    return g


def test_thresholds_are_the_ones_the_large_tests_rely_on(geo):
    assert geo == {"max_blocks": 512, "gb": 64, "tg": 128, "chunk_wgs": 1024, "chunk_cap": 64}


def _pad64(n):
    return -(-n // 64) * 64


def _chunks(geo, n, n2):
    """gps_kmvm_chunks and kmvm_kernel's t0, t1 restated with the sources' constants"""
    rt, ct = _pad64(n) // 64, _pad64(n2) // 64
    ch = max(min(min(-(-geo["chunk_wgs"] // rt), geo["chunk_cap"]), ct), 1)
    return [(c * ct // ch, (c + 1) * ct // ch) for c in range(ch)]


def test_chunk_rule(geo):
    """_backend.kmvm_chunking is the sources' rule, and cuts unequal multi-tile chunks at the large product sizes"""
    from gpflowSlim import _abi
    for n, n2 in [(2112, 2112), (8300, 8300), (130, 2112), (130, 4200), (200, 200), (65, 130)]:
        assert _abi.kmvm_chunking(n, n2, 0) == _chunks(geo, n, n2)
    c = _abi.kmvm_chunking(2112, 2112, 0)
    assert len(c) == 32 and sorted({b - a for a, b in c}) == [1, 2] and c[-1] == (31, 33)
    c = _abi.kmvm_chunking(8300, 8300, 0)
    assert len(c) == 8 and sorted({b - a for a, b in c}) == [16, 17] and c[-1][1] == 130
    for n, T in big.PRODUCT_SYM:
        lengths = {b - a for a, b in _chunks(geo, n, n)}
        assert len(lengths) == 2 and max(lengths) >= 2, "product n = %d no longer gets unequal multi-tile chunks" % n
    assert any(T > 64 for _, T in big.PRODUCT_SYM), "no product case takes two passes (kmvm_fold_rows_kernel)"
    caps = [len(_chunks(geo, n, n2)) for _, n, n2, _ in big.PRODUCT_RECT]
    assert geo["chunk_cap"] in caps and any(-(-n2 // 64) > geo["chunk_cap"] for _, _, n2, _ in big.PRODUCT_RECT), \
        "no rectangular product is cut by the chunk cap"


def test_every_large_size_is_above_its_threshold(geo):
    mb = geo["max_blocks"]
    # gradient form: kmvm_grad_fold_kernel over more than one workgroup; auto chunks of more than one tile at the largest
    nblk = [-(-n // 256) for n, _ in big.FORM_SIZES]
    assert min(nblk) >= 2 and len(set(nblk)) == len(nblk) and max(nblk) <= mb
    n_top = max(n for n, _ in big.FORM_SIZES)
    assert max(b - a for a, b in _chunks(geo, n_top, n_top)) >= 2, "the largest form no longer walks a multi-tile chunk"
    # CG vector kernels: more rows than one pass of KCG_MAX_BLOCKS workgroups of 16, and rows sampled on both sides of the wrap
    assert -(-_pad64(big.N_CG) // 16) > mb and -(-big.N_CG // 16) > mb, "the CG case no longer strides its rows"
    rows = mr.sample_rows(big.N_CG)
    assert np.any(rows < 16 * mb) and np.any(rows >= 16 * mb)
    # pivot search: a fold across workgroups in every factor case, its second pass (blk += 256) in the largest
    pn = [-(-_pad64(n) // 256) for _, n, _, _, _ in big.FACTORS]
    assert min(pn) >= 2 and max(pn) > 256, "no factor case reaches the pivot fold's second pass"
    assert any(dup and n > 290 for _, n, _, _, dup in big.FACTORS)
    # preconditioner: gb (rows per workgroup no multiple of 64, trailing workgroups with no rows), tg, lsg
    tiles = {n: _pad64(n) // 64 for n, _, _ in big.PRECOND}
    over_gb = [n for n in tiles if tiles[n] > geo["gb"]]
    assert over_gb and any(tiles[n] > geo["tg"] for n in tiles) and any(tiles[n] > mb for n in tiles), tiles
    rpb = {n: -(-(_pad64(n) // 4) // geo["gb"]) * 4 for n in over_gb}
    assert any(rpb[n] % 64 and rpb[n] * (geo["gb"] - 1) >= _pad64(n) for n in over_gb), \
        "no preconditioner case leaves a Gram workgroup without rows at a ragged rows-per-workgroup: %s" % rpb
    # ... and the factor behind the 128-rank cap runs past gb as well
    assert any(cap == 128 and _pad64(n) // 64 > geo["gb"] for _, n, _, cap, _ in big.FACTORS)
