#!/usr/bin/env python3
"""Compare two `make isa` outputs kernel by kernel.

  tools/isa_diff.py OLD_DIR NEW_DIR [--per-block]

OLD_DIR and NEW_DIR are build/isa directories: every *.s and every
*resource_usage.txt in each is read, so a kernel that moved from one TU to
another still matches by symbol.  A symbol that two files of one directory
define is reported.  For every kernel in both: is the instruction stream the
same (labels renumbered, comments and directives dropped), and are the
register, LDS, scratch and occupancy figures the same?  Kernels that differ
are listed with the number of changed lines and whether every changed line is
a kernel-argument load (s_load_* from the kernarg pointer: what a grown
argument struct moves).  Symbols of one directory alone are listed with their
file.

--per-block: also list each per-block loss kernel (NEW_DIR/per_block*
resource_usage.txt) whose figures differ from its uniform twin's (loss
template argument L - 4) in occupancy, scratch or spills.
"""
import difflib
import glob
import os
import re
import sys


def bodies(path):
    out = {}
    text = open(path).read()
    for m in re.finditer(r"\n(_ZN3cse\w+):[^\n]*\n(.*?)\.Lfunc_end", text, re.S):
        lines = [l.strip() for l in m.group(2).split("\n")]
        out[m.group(1)] = [re.sub(r"\.LBB\d+_", ".LBB_", l) for l in lines
                           if l and not l.startswith((";", "."))]
    return out


def resources(path):
    out, cur = {}, None
    for l in open(path):
        m = re.search(r"Function Name: (\S+)", l)
        if m:
            cur = m.group(1)
            out[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\w+) \[-Rpass", l)
        if m and cur:
            out[cur][m.group(1).strip()] = m.group(2)
    return out


def short(r):
    return (f"VGPR {r.get('VGPRs')} SGPR {r.get('TotalSGPRs')} LDS {r.get('LDS Size [bytes/block]')} "
            f"scratch {r.get('ScratchSize [bytes/lane]')} spill {r.get('VGPRs Spill')} "
            f"occ {r.get('Occupancy [waves/SIMD]')}")


def read_dir(d):
    """Every symbol's body, file and resource figures over the directory's files."""
    body, where, res = {}, {}, {}
    for path in sorted(glob.glob(d + "/*.s")):
        for k, v in bodies(path).items():
            where.setdefault(k, []).append(os.path.basename(path))
            body[k] = v
    for path in sorted(glob.glob(d + "/*resource_usage.txt")):
        res.update(resources(path))
    for k, files in sorted(where.items()):
        if len(files) > 1:
            print(f"DUPLICATE {k} in {d}: {' '.join(files)}")
    return body, where, res


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    old, new = args[0].rstrip("/"), args[1].rstrip("/")
    (a, wa, ra), (b, wb, rb) = read_dir(old), read_dir(new)
    print(f"kernels: old {len(a)}, new {len(b)}; only old {len(set(a) - set(b))}, "
          f"only new {len(set(b) - set(a))}")
    for k in sorted(set(a) - set(b)):
        print(f"ONLY OLD {wa[k][0]} {k}")
    for k in sorted(set(b) - set(a)):
        print(f"ONLY NEW {wb[k][0]} {k}")
    moved = sorted(k for k in set(a) & set(b) if wa[k] != wb[k])
    print(f"in another file than before: {len(moved)}")
    for k in moved:
        print(f"MOVED {wa[k][0]} -> {wb[k][0]} {k}")
    same = 0
    for k in sorted(set(a) & set(b)):
        if a[k] == b[k] and ra.get(k) == rb.get(k):
            same += 1
            continue
        d = [l for l in difflib.unified_diff(a[k], b[k], lineterm="", n=0)
             if not l.startswith(("---", "+++", "@@"))]
        kernarg = all(re.match(r"[-+]s_load_dword\w* s\[\d+:\d+\], s\[0:1\]", l) for l in d)
        print(f"DIFF {k}\n     {len(a[k])} -> {len(b[k])} instructions, {len(d)} changed lines"
              f"{' (kernel-argument loads only)' if kernarg and d else ''}")
        if ra.get(k) != rb.get(k):
            print(f"     old {short(ra.get(k, {}))}\n     new {short(rb.get(k, {}))}")
    print(f"identical instruction stream and resource figures: {same} of {len(set(a) & set(b))}")
    if "--per-block" in sys.argv:
        rp = {}
        for path in glob.glob(new + "/per_block*resource_usage.txt"):
            rp.update(resources(path))
        twin = lambda k: re.sub(r"ELi([456])E", lambda m: "ELi%dE" % (int(m.group(1)) - 4), k, count=1)
        keys = ("Occupancy [waves/SIMD]", "ScratchSize [bytes/lane]", "VGPRs Spill")
        n = 0
        for k, v in rp.items():
            u = rb.get(twin(k))
            if u is None or twin(k) == k:
                continue
            n += 1
            if any(u.get(x) != v.get(x) for x in keys):
                print(f"PER-BLOCK {k}\n     uniform   {short(u)}\n     per-block {short(v)}")
        print(f"per-block kernels with a uniform twin: {n}")


if __name__ == "__main__":
    main()
