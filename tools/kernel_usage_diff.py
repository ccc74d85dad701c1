"""Compares the per-kernel resource figures of two builds: was any kernel body touched?

    make -C gpflow-slim_amd/csrc OUTDIR=../lib_parent CXXFLAGS="<the Makefile's> -Rpass-analysis=kernel-resource-usage" 2> parent.log   (at the parent commit)
    make -C gpflow-slim_amd/csrc                      CXXFLAGS="<the Makefile's> -Rpass-analysis=kernel-resource-usage" 2> branch.log
    python tools/kernel_usage_diff.py parent.log branch.log

The remark is a compile-time one (no GPU).  Kernels are matched by their mangled name, so one that moved to another file is still
compared; per kernel: VGPRs, AGPRs, SGPRs, spills, scratch, LDS, occupancy, dynamic stack.  Exit status 1 on any difference.
"""
import re
import sys


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            out.setdefault(cur, []).append({})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+(?:\[[^\]]*\])?): (\S+) \[-Rpass-analysis", line)
        if m and cur:
            out[cur][-1][m.group(1).strip()] = m.group(2)
    return out


def main():
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    bad = 0
    for k in sorted(set(a) | set(b)):
        if a.get(k) != b.get(k):
            bad += 1
            print("DIFF", k, a.get(k), b.get(k))
    print("kernels: %d in %s, %d in %s, %d differ" % (len(a), sys.argv[1], len(b), sys.argv[2], bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
