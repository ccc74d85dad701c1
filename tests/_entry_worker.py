"""Worker of tests/test_gpu_call_order.py: the entries of one family of tests/_entry_catalogue.py on handles of its own, every
output kept.  argv: family mode out_file

modes
  cold            each (entry, input set) on a fresh Handle, closed afterwards; twice, on two handles ("cold", "cold-again": is the
                  entry bit-reproducible run to run at all?); each failing call on a fresh Handle; the resident GPR prediction
  poison          as cold, once; the parent starts this process with GPS_POISON_ALLOC=2, which is invalid for the entries that read a
                  factor an earlier call left resident (catalogue.RESIDENT_READERS, csrc/gps_common.hpp at DevBuf::ensure): left out
  poison-readers  those entries only, as their documented pair; the parent sets GPS_POISON_ALLOC=1
  warm            ONE handle for the whole process.  For every victim (entry x {small, edge}) of the family:
                    each intruder at edge, then the victim at small          (stale content beyond the new extent)
                    the victim at small, then at edge (and at big)           (growth and reallocation in the middle of a life)
                    the victim at edge, at twin, at edge again               (stale values at equal extents)
                    the victim at big, then at small                         (GPR only)
                    each failing call, then the victim at small and at edge  (an early error return)
                    for a "keeps" entry: a GPR factor at N = 200 made resident, the victim, the prediction from that factor
                  and then all those calls once more in one seeded shuffle (the seed is in the file; the resident-factor triples
                  stay together).

The file: an .npz with one array per DISTINCT output (outputs of one (entry, set, position) that are byte-equal within this
process are stored once) and "meta", a JSON text: the occurrences (entry, set, tag, the call before, the arrays it returned), the
three fall-back counters summed over the handles, the seconds.  A raised error is an output too: its text.
"""
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gpflow-slim_amd"), ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import _entry_catalogue as cat  # noqa: E402

COUNTERS = ("lookahead_retries", "trsv_wave_fallbacks", "small_n_fallbacks")
SHUFFLE_SEED = 20261021


class Recorder(object):
    def __init__(self):
        self.arrays, self.known, self.occurrences, self.prev = [], {}, [], "(a fresh handle)"
        self.counters = dict.fromkeys(COUNTERS, 0)

    def run(self, h, label, setname, call, tag, record=True):
        try:
            res = call(h)
        except Exception as e:                                        # (a refusal is an output too: its text)
            res = "raised: %s: %s" % (type(e).__name__, e)
        if record:
            ids = []
            for i, a in enumerate(cat.flatten(res)):
                known = self.known.setdefault((label, setname, i), [])
                for k in known:
                    if cat.same_bytes(self.arrays[k], a):
                        ids.append(k)
                        break
                else:
                    self.arrays.append(a)
                    known.append(len(self.arrays) - 1)
                    ids.append(len(self.arrays) - 1)
            self.occurrences.append(dict(entry=label, set=setname, tag=tag, prev=self.prev, outputs=ids))
        self.prev = "%s[%s]" % (label, setname)

    def count(self, h):
        for k in COUNTERS:
            self.counters[k] += int(h.profile_get(k)["launches"])

    def fresh(self, label, setname, call, tag):
        from gpflowSlim import _backend as be
        h = be.Handle()
        self.prev = "(a fresh handle)"
        try:
            self.run(h, label, setname, call, tag)
            self.count(h)
        finally:
            h.close()


def _entry_call(e, setname):
    c = cat.inputs(setname)
    return lambda h: e.call(h, c)


def _fail_call(name):
    call, _ = cat.FAILING[name]
    c = cat.failing_inputs()
    return lambda h: call(h, c)


def _resident_pair(h):
    cat.resident_setup(h)
    return cat.resident_read(h)


def run_cold(rec, family, mode):
    readers = set(cat.RESIDENT_READERS)
    tags = ("cold", "cold-again") if mode == "cold" else (mode,)
    for e in cat.of_family(family):
        if (mode == "poison" and e.name in readers) or (mode == "poison-readers" and e.name not in readers):
            continue
        for s in e.sets:
            for tag in tags:
                rec.fresh(e.name, s, _entry_call(e, s), tag)
    if mode == "cold":
        for name in cat.FAILING:
            rec.fresh("fail:" + name, "-", _fail_call(name), "cold")
    if mode != "poison":
        rec.fresh(cat.RESIDENT[0], cat.RESIDENT[1], _resident_pair, tags[0])


def warm_sequences(family):
    """the call sequences of the warm mode: lists of steps (kind, name, set)"""
    seqs = []
    for e in cat.of_family(family):
        V = lambda s: ("entry", e.name, s)                                                                     # noqa: E731
        for i in cat.INTRUDERS:
            seqs.append([("entry", i, "edge"), V("small")])
        for s in e.sets:
            if s not in ("small", "twin"):
                seqs.append([V("small"), V(s)])
        seqs.append([V("edge"), V("twin"), V("edge")])
        if "big" in e.sets:
            seqs.append([V("big"), V("small")])
        for f in cat.FAILING:
            for s in ("small", "edge"):
                seqs.append([("fail", f, "-"), V(s)])
        if e.keeps:
            for s in ("small", "edge"):
                seqs.append([("resident-setup", "", ""), V(s), ("resident-read", "", "")])
    return seqs


def run_warm(rec, family):
    from gpflowSlim import _backend as be
    h = be.Handle()

    def step(kind, name, s, tag):
        if kind == "entry":
            e = cat.ENTRIES[name]
            rec.run(h, name, s, _entry_call(e, s), tag, record=e.family == family)
        elif kind == "fail":
            rec.run(h, "fail:" + name, "-", _fail_call(name), tag)
        elif kind == "resident-setup":
            rec.run(h, "resident-setup", "n200", cat.resident_setup, tag, record=False)
        else:
            rec.run(h, cat.RESIDENT[0], cat.RESIDENT[1], cat.resident_read, tag)

    seqs = warm_sequences(family)
    for seq in seqs:
        for kind, name, s in seq:
            step(kind, name, s, "ordered")
    # one seeded shuffle of all the above: the calls one by one, the resident-factor triples as they are
    units = []
    for seq in seqs:
        units += [seq] if seq[0][0] == "resident-setup" else [[st] for st in seq]
    random.Random(SHUFFLE_SEED).shuffle(units)
    for unit in units:
        for kind, name, s in unit:
            step(kind, name, s, "shuffled")
    rec.count(h)
    h.close()


def main():
    family, mode, out = sys.argv[1], sys.argv[2], sys.argv[3]
    assert family in cat.FAMILIES and mode in ("cold", "poison", "poison-readers", "warm")
    t0 = time.perf_counter()
    rec = Recorder()
    if mode == "warm":
        run_warm(rec, family)
    else:
        run_cold(rec, family, mode)
    meta = dict(family=family, mode=mode, poison=os.environ.get("GPS_POISON_ALLOC", ""), shuffle_seed=SHUFFLE_SEED,
                occurrences=rec.occurrences, counters=rec.counters, seconds=round(time.perf_counter() - t0, 2))
    np.savez(out, meta=np.array(json.dumps(meta)), **{"a%d" % i: a for i, a in enumerate(rec.arrays)})
    print("%s %s: %d calls recorded, %d distinct arrays, counters %s, %.1f s" % (
        family, mode, len(rec.occurrences), len(rec.arrays), rec.counters, meta["seconds"]), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
