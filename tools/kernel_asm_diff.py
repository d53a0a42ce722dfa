#!/usr/bin/env python3
"""Which kernels of two device-only assembly listings (hipcc -S --cuda-device-only of kid_api.hip) have textually
identical bodies.  A body = the lines between a kernel's label and its .Lfunc_end; the function ordinal in local labels
(.LBB<n>_, and BB<n>_ in the comments behind them, whose column moves with the ordinal's width) is dropped, since it moves
with a kernel's place in the file.

  python3 tools/kernel_asm_diff.py parent.s branch.s"""
import hashlib
import re
import subprocess
import sys


def bodies(path):
    out, cur, buf = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and cur is None:
            cur, buf = m.group(1), []
        elif cur is not None:
            if line.startswith(".Lfunc_end"):
                out[cur] = re.sub(r"[ \t]+;", " ;", re.sub(r"BB\d+_", "BB_", "".join(buf)))
                cur = None
            else:
                buf.append(line)
    return out


def main():
    a, b = bodies(sys.argv[1]), bodies(sys.argv[2])
    assert sorted(a) == sorted(b), "the kernel sets differ: %s" % sorted(set(a) ^ set(b))
    names = subprocess.run(["c++filt"], input="\n".join(sorted(a)), capture_output=True, text=True).stdout.split("\n")
    same, diff = [], []
    for mangled, name in zip(sorted(a), names):
        name = re.sub(r"^void ", "", name)
        name = name[:name.index("(")] if "(" in name else name
        row = (name, a[mangled].count("\n"), b[mangled].count("\n"), hashlib.sha256(b[mangled].encode()).hexdigest()[:12])
        (same if a[mangled] == b[mangled] else diff).append(row)
    print("%d kernels, %d with textually identical bodies, %d that differ" % (len(a), len(same), len(diff)))
    print("identical (name, lines, sha256/12 of the body):")
    for r in same:
        print("  %-52s %6d  %s" % (r[0], r[1], r[3]))
    print("different (name, lines first -> second):")
    for r in diff:
        print("  %-52s %6d -> %d" % (r[0], r[1], r[2]))


if __name__ == "__main__":
    main()
