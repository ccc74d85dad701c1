"""The catalogue of tests/_entry_catalogue.py against gpflowSlim._backend.Handle, without a GPU: every public method is a catalogue
entry or excluded with a reason, the residency table of the docstring resolves to entries of that class, the input sets have the
shapes the call-order test states, and the byte comparator sees what it has to see."""
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _entry_catalogue as cat  # noqa: E402


def _methods():
    from gpflowSlim import _backend as be
    return sorted(n for n, _ in inspect.getmembers(be.Handle, inspect.isfunction) if not n.startswith("_"))


def _catalogued():
    return {w.split("(")[0] for e in cat.ENTRIES.values() for w in e.wrappers}


def uncovered(methods, catalogued, excluded):
    return sorted(m for m in methods if m not in catalogued and m not in excluded)


def test_every_public_method_is_catalogued_or_excluded():
    methods, done = _methods(), _catalogued()
    assert uncovered(methods, done, cat.EXCLUDED) == []
    assert sorted(set(cat.EXCLUDED) - set(methods)) == [], "EXCLUDED names that are no methods of Handle"
    assert sorted(done - set(methods)) == [], "catalogue wrappers that are no methods of Handle"
    assert sorted(done & set(cat.EXCLUDED)) == [], "both catalogued and excluded"
    assert all(isinstance(r, str) and len(r) > 10 for r in cat.EXCLUDED.values())
    # a method that is in neither is found: take one away from both
    victim = "tri_skinny"
    assert uncovered(methods, done - {victim}, cat.EXCLUDED) == [victim]
    assert uncovered(methods + ["a_new_entry"], done, cat.EXCLUDED) == ["a_new_entry"]


def test_the_docstring_table_resolves_to_entries_of_its_class():
    from gpflowSlim import _backend as be
    methods = _methods()
    table = cat.residency_table(be.Handle.__doc__)
    assert set(table) == {"drops_all", "drops_factor", "keeps"} and all(len(v) >= 6 for v in table.values())
    used = {w for e in cat.ENTRIES.values() for w in e.wrappers}
    seen = set()
    for klass, names in table.items():
        for name in names:
            keys = cat.resolve(name, methods)
            assert keys, "%s of the table stands for nothing" % name
            for key in keys:
                if key.split("(")[0] in cat.EXCLUDED:
                    continue
                assert cat.WRAPPER_CLASS.get(key) == klass, (name, key, klass, cat.WRAPPER_CLASS.get(key))
                assert key in used, "%s has no catalogue entry" % key
                seen.add(key)
    assert sorted(set(cat.WRAPPER_CLASS) - seen) == [], "wrappers with a class that the table does not name"
    # the thirteen that the residency test's table did not have
    for w in ("gpmc_lik", "gpmc_lik_grad", "sgpmc_lik", "sgpmc_lik_grad", "uncertain_conditional", "psi2_contract", "bgplvm_grad",
              "rff_lml_grad", "rff_predict(refactor)", "rff_predict(refactor=False)", "kgpr_lml_grad", "kgpr_predict", "lik_logp",
              "tri_skinny", "chol_seed", "svgp_elbo_lik_grad"):
        assert w in used
    # an entry's class is the strongest of its wrappers'
    assert cat.ENTRIES["kmat"].keeps and not cat.ENTRIES["gpr_predict-resident"].keeps
    assert cat.ENTRIES["gpr_lml"].klass == "drops_all" and cat.ENTRIES["sparse_last_terms"].klass == "drops_all"


def test_families_and_intruders():
    assert {e.family for e in cat.ENTRIES.values()} == set(cat.FAMILIES)
    assert len(cat.INTRUDERS) == len(cat.FAMILIES)
    kinds = set(cat.LIK_KINDS)
    assert {"gamma", "beta", "ordinal"} <= kinds
    for kind in kinds - {"bernoulli"}:
        assert "lik_varexp-" + kind in cat.ENTRIES and "svgp_elbo_lik_grad-" + kind in cat.ENTRIES
        assert ("lik_logp-" + kind in cat.ENTRIES) == (kind != "multiclass")
    for e in cat.ENTRIES.values():
        assert e.sets[:3] == cat.SETS and (e.sets[3:] in ((), ("big",)))
        assert (e.sets[3:] == ("big",)) <= (e.family == "gpr")


@pytest.mark.parametrize("name", ["small", "edge", "twin", "big"])
def test_input_sets_have_the_stated_shapes_and_are_finite(name):
    c = cat.inputs(name)
    want = {"small": (5, 70, 2, 7, 2), "edge": (129, 257, 17, 130, 3), "twin": (129, 257, 17, 130, 3), "big": (None, 2200, 1, 9, 2)}[name]
    M, N, K, NS, D = want
    assert c["X"].shape == (N, D) and c["Xs"].shape == (NS, D) and c["Y"].shape == (N, K) and c["Xc"].shape == (N, D + 1)
    assert set(np.unique(c["Xc"][:, D])) <= {0.0, 1.0, 2.0}
    if name != "big":
        assert c["Z"].shape == (M, D) and c["W"].shape == (N, M) and c["q_mu"].shape == (M, K) and c["q_sqrt"].shape == (M, M, K)
        assert c["q_diag"].shape == (M, K) and c["Kmm"].shape == (M, M) and c["Kms"].shape == (M, NS) and c["Kss"].shape == (NS, NS)
        assert c["Xvar"].shape == (N, D) and c["Fvar"].shape == (N, K) and c["mean"].shape == (N, K) and c["Wc"].shape == (K, M, M)
        assert c["Vm"].shape == (M, K) and c["Vn"].shape == (N, K) and c["U"].shape == (M, K)
        assert all(c["Ylik"][k].shape == ((N, 1) if k == "multiclass" else (N, K)) for k in cat.LIK_KINDS)
        assert np.all(np.tril(c["q_sqrt"][:, :, 0]) == c["q_sqrt"][:, :, 0]) and np.all(c["Xvar"] > 0) and np.all(c["Fvar"] > 0)
        small = name == "small"
        assert c["chunk_rows"] == (0 if small else 128) and c["psi_chunk"] == (0 if small else 64) and c["full"] == (not small)
        assert c["rff"][0].n_components == (6 if small else 129)
        assert c["Yg"].shape == ((3, 4) if small else (17, 9)) and c["mask"].sum() == (1 if small else 2)
        assert c["Xp"].shape == ((70, 2) if small else (33, 3))
        if not small:
            assert -(-N // c["chunk_rows"]) == 3 and N % c["chunk_rows"] != 0 and -(-N // c["psi_chunk"]) == 5
    for k, v in c.items():
        if isinstance(v, np.ndarray):
            assert np.all(np.isfinite(v)), k
    for what, A in cat.pd_matrices(name).items():
        w = np.linalg.eigvalsh(A)
        assert w[0] > 0 and w[-1] / w[0] <= cat.COND_CAP, (name, what, w[0], w[-1] / w[0])


def test_edge_and_twin_differ_in_values_only():
    a, b = cat.inputs("edge"), cat.inputs("twin")
    for k, v in a.items():
        if isinstance(v, np.ndarray) and k not in ("Kss_diag", "X1", "X2", "K1", "K2", "mask", "C", "e1", "e2", "sel", "V1", "V2", "ls"):
            assert v.shape == b[k].shape and not np.array_equal(v, b[k]), k


def test_failing_intruders_have_a_negative_eigenvalue():
    c = cat.failing_inputs()
    refused = 0
    for name, (call, key) in cat.FAILING.items():
        if key is None:
            refused += 1
            continue
        A = c[key]
        assert np.all(np.isfinite(A)) and np.array_equal(A, A.T) and np.linalg.eigvalsh(A)[0] < -1e-4, name
    assert refused == 1 and len(cat.FAILING) >= 6


def test_the_comparator_sees_what_a_leak_looks_like():
    a = np.array([[1.0, 2.0, 0.0], [np.nan, 5.0, 6.0]])
    assert cat.same_bytes(a, a.copy())
    one_ulp = a.copy()
    one_ulp[0, 1] = np.nextafter(2.0, 3.0)
    moved_nan = a.copy()
    moved_nan[1, 0], moved_nan[1, 1] = 5.0, np.nan
    minus_zero = a.copy()
    minus_zero[0, 2] = -0.0
    assert np.array_equal(minus_zero, a, equal_nan=True)             # (what array_equal lets through)
    for b in (one_ulp, moved_nan, minus_zero, a.reshape(3, 2), a[:, :2], a.ravel()):
        assert not cat.same_bytes(a, b) and not cat.same_bytes(b, a)
        assert isinstance(cat.difference(a, b), str)
    assert "1 of 6 entries differ, largest difference 4.44e-16" in cat.difference(a, one_ulp)
    assert "2 of 6 entries differ" in cat.difference(a, moved_nan) and "not finite" in cat.difference(a, moved_nan)
    assert "1 of 6 entries differ, largest difference 0" in cat.difference(a, minus_zero)
    assert "shape" in cat.difference(a, a.reshape(3, 2))
    assert not cat.same_bytes(np.array("raised: a"), np.array("raised: b")) and cat.same_bytes(np.array("x"), np.array("x"))
    assert not cat.same_bytes(np.array("x"), np.array(1.0))
    # flatten: tuples, dictionaries and None
    flat = cat.flatten((1.5, None, {"b": np.ones(2), "a": 2.0}, (np.zeros((2, 2)), "raised: x")))
    assert [f.shape for f in flat] == [(), (), (2,), (2, 2), ()] and float(flat[1]) == 2.0 and str(flat[4]) == "raised: x"
