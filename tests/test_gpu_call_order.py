"""Every device entry gives its cold-handle bytes in any call order.

One handle owns about sixty device buffers that about seventy entry points share, and DevBuf::ensure never clears one: correctness
between calls rests on unwritten contracts (identity- and zero-padded buffers, counters that every launch leaves at zero, who
holds what).  The library is bit-reproducible run to run (every atomic in csrc is an integer ticket or flag), so the reference
for "no leak" is exact: an entry of tests/_entry_catalogue.py must return the same BYTES on a cold handle, on a handle whose
buffers are filled with NaN patterns at every request (GPS_POISON_ALLOC=2; =1 for the entries that read a resident factor), and
after any other call -- a larger one, a smaller one, the same one on other values, one that failed (tests/_entry_worker.py
lists the sequences).  No tolerance.  Whether the cold bytes are right is what the other tests check against the oracles.

Each family's item starts its children one after another, each a fresh process under a 300 s limit (the per-child limit of
tools/ab_outputs.py).  A child that ends by a signal, an abort or the time limit fails the item and every later item, which then
start nothing more on the GPU.

The three fall-back counters must be zero in every child: an evaluation re-run without look-ahead is correct to 1e-8 but not
bit-identical (docs/LAB_NOTES.md, round 5), so a non-zero counter invalidates the comparison.  The shapes of at most 257 rows
stay below where the look-ahead engages: blocked.hpp::potrf_rl_groups hands over only with at least two diagonal blocks in the
group AND a remainder of at least HipOps::lookahead_min_rows() = 1024 rows (gps_ops.hpp), and the one-launch path of
gps_gpr.hip (p->small: padded size <= small_n_max = 2048, at most 16 columns) has no hand-over at all.  The GPR cases at
N = 2200 (padded 2304) do hand over; they are bit-reproducible as long as no hand-over is missed, which is what the counter
says -- tests/test_gpu_residency.py rests on the same.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _entry_catalogue as cat  # noqa: E402

pytestmark = pytest.mark.gpu

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_entry_worker.py")
CHILD_LIMIT_S = 300
MAX_MESSAGES = 12
_ENDED_BADLY = []                                                     # the module flag: what ended a child, if anything did


def _child(family, mode, tmp_path, poison):
    """one fresh process; (meta, arrays) of what it recorded"""
    if _ENDED_BADLY:
        pytest.fail("no child is started: %s" % _ENDED_BADLY[0])
    out = str(tmp_path / ("%s.%s.npz" % (family, mode)))
    env = {k: v for k, v in os.environ.items() if k != "GPS_POISON_ALLOC"}
    if poison:
        env["GPS_POISON_ALLOC"] = str(poison)                         # (reaches the child through env only)
    t0 = time.perf_counter()
    try:
        p = subprocess.run([sys.executable, WORKER, family, mode, out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           universal_newlines=True, timeout=CHILD_LIMIT_S)
    except subprocess.TimeoutExpired as e:
        _ENDED_BADLY.append("the %s child of %s ran into its %d s limit" % (mode, family, CHILD_LIMIT_S))
        pytest.fail("%s\n%s" % (_ENDED_BADLY[0], (e.stdout or "")[-2000:]))
    wall = time.perf_counter() - t0
    if p.returncode < 0 or p.returncode >= 128:                       # a signal, an abort, a segmentation fault
        _ENDED_BADLY.append("the %s child of %s ended with status %d" % (mode, family, p.returncode))
        pytest.fail("%s\n%s" % (_ENDED_BADLY[0], p.stdout[-2000:]))
    assert p.returncode == 0, "the %s child of %s failed (%d):\n%s" % (mode, family, p.returncode, p.stdout[-4000:])
    with np.load(out) as f:
        meta = json.loads(str(f["meta"]))
        arrays = {int(k[1:]): f[k] for k in f.files if k != "meta"}
    print("call-order child %-10s %-14s %6.1f s wall, %5.1f s of calls, %5d calls recorded, %5d distinct arrays" % (
        family, mode, wall, meta["seconds"], len(meta["occurrences"]), len(arrays)))
    assert meta["poison"] == (str(poison) if poison else "")
    assert meta["counters"] == dict.fromkeys(meta["counters"], 0) and len(meta["counters"]) == 3, \
        "%s %s: a fall-back ran, its result is not comparable bit for bit: %s" % (family, mode, meta["counters"])
    return meta, arrays


def _compare(meta, arrays, ref, ref_arrays, messages):
    """every occurrence against the cold outputs of its (entry, set); the number of arrays compared"""
    n, verdict = 0, {}
    for occ in meta["occurrences"]:
        key = (occ["entry"], occ["set"])
        assert key in ref, "no cold reference for %s[%s]" % key
        want = ref[key]
        if len(want) != len(occ["outputs"]):
            messages.append("%s[%s] %s after %s: %d outputs, cold %d" % (key + (occ["tag"], occ["prev"], len(occ["outputs"]), len(want))))
            continue
        for i, (a, b) in enumerate(zip(occ["outputs"], want)):
            n += 1
            if (a, b) not in verdict:
                verdict[(a, b)] = cat.same_bytes(arrays[a], ref_arrays[b])
            if not verdict[(a, b)] and len(messages) < MAX_MESSAGES:
                messages.append("%s[%s] (%s %s) after %s, output %d: %s" % (
                    key + (meta["mode"], occ["tag"], occ["prev"], i, cat.difference(arrays[a], ref_arrays[b]))))
            elif not verdict[(a, b)]:
                messages.append(None)
    return n


@pytest.mark.parametrize("family", cat.FAMILIES)
def test_cold_bytes_in_any_call_order(family, tmp_path):
    cold, cold_arrays = _child(family, "cold", tmp_path, None)
    ref, again = {}, {}
    for occ in cold["occurrences"]:
        (ref if occ["tag"] == "cold" else again)[(occ["entry"], occ["set"])] = occ["outputs"]
    # every cold output is finite, or the text of the error for the calls that fail
    for (entry, s), ids in ref.items():
        assert ids, "%s[%s] returned nothing" % (entry, s)
        for i in ids:
            a = cold_arrays[i]
            if entry.startswith("fail:"):
                assert a.dtype.kind == "U" and str(a).startswith("raised: "), (entry, a)
            else:
                assert a.dtype.kind == "f" and np.all(np.isfinite(a)), "%s[%s]: %s" % (entry, s, str(a)[:300])
    for name in cat.FAILING:
        assert ("fail:" + name, "-") in ref
    assert "NotPositiveDefiniteError" in str(cold_arrays[ref[("fail:potrf-indefinite", "-")][0]])
    assert "(-4)" in str(cold_arrays[ref[("fail:kmat-refused", "-")][0]])      # GPS_ERR_UNSUPPORTED, from the library
    wanted = {(e.name, s) for e in cat.of_family(family) for s in e.sets}
    assert wanted <= set(ref) and wanted <= set(again)
    # run to run on two cold handles: an entry that differs here is not bit-reproducible at all (a finding of its own)
    messages, counts = [], {}
    counts["cold-again"] = _compare(dict(cold, occurrences=[o for o in cold["occurrences"] if o["tag"] == "cold-again"]),
                                    cold_arrays, ref, cold_arrays, messages)
    assert not messages, "not bit-reproducible on two cold handles:\n" + "\n".join(m for m in messages if m)
    # (poison-readers in every family: the prediction from a resident GPR factor is one of them)
    for mode, poison in (("poison", 2), ("poison-readers", 1), ("warm", None)):
        meta, arrays = _child(family, mode, tmp_path, poison)
        counts[mode] = _compare(meta, arrays, ref, cold_arrays, messages)
        seen = {(o["entry"], o["set"]) for o in meta["occurrences"]}
        if mode == "warm":
            assert wanted <= seen and all(("fail:" + f, "-") in seen for f in cat.FAILING)
            assert (cat.RESIDENT in seen) == any(e.keeps for e in cat.of_family(family))
    print("call-order arrays compared, %s: %s" % (family, counts))
    assert not messages, "%d outputs differ from the cold handle's bytes:\n%s" % (len(messages), "\n".join(m for m in messages if m))
