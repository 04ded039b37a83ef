#!/usr/bin/env python3
"""Sum the "blur-exact" lines that tests/test_blur_exact.py prints (python3 -m pytest tests/test_blur_exact.py -q -s) over shapes and sources:
one line per kernel and radius -- values compared, values within eps of a rounding tie (excused), values that are not rint(exact).
usage: python3 -m pytest tests/test_blur_exact.py -q -s | python3 tools/blur_exact_table.py > profiles/blur_exact.txt"""
import re
import sys

rows, ties, oracle = {}, {}, {}
for ln in sys.stdin:
    m = re.match(r"\s*blur-exact\s+(.*?)\s+r=([\d.]+)\s+(values|pixels)\s+(\d+)\s+(.*)$", ln)
    if not m:
        continue
    name, radius, n, rest = m.group(1), float(m.group(2)), int(m.group(4)), m.group(5)
    if rest.startswith("all equal"):
        ties[(name, radius)] = ties.get((name, radius), 0) + n
    elif rest.startswith("differing"):
        t = oracle.setdefault(radius, [0, 0])
        t[0] += n; t[1] += int(rest.split()[-1])
    else:
        k = re.match(r"excused\s+(\d+).*not rint\(exact\)\s+(\d+)", rest)
        t = rows.setdefault((name, radius), [0, 0, 0])
        t[0] += n; t[1] += int(k.group(1)); t[2] += int(k.group(2))
print("tests/test_blur_exact.py on an MI355X: every blur kernel against the float64 filter of tests/blur_ref.py, summed over shapes and sources")
print("(excused: the exact sum lies within eps of a rounding tie, the byte may be floor or ceil; every other byte IS rint(exact))\n")
print(f"{'kernel':44s} {'radius':>6s} {'values':>10s} {'excused':>8s} {'share':>8s} {'not rint(exact)':>16s}")
for (name, radius), (n, e, d) in sorted(rows.items()):
    print(f"{name:44s} {radius:6g} {n:10d} {e:8d} {e / max(n, 1):8.3%} {d:16d}")
print(f"\n{'tied bit for bit':44s} {'radius':>6s} {'values':>10s}")
for (name, radius), n in sorted(ties.items()):
    print(f"{name:44s} {radius:6g} {n:10d}")
print(f"\n{'final frames against the oracle (bar: 1 LSB)':44s} {'radius':>6s} {'pixels':>10s} {'1 LSB off':>10s}")
for radius, (n, d) in sorted(oracle.items()):
    print(f"{'':44s} {radius:6g} {n:10d} {d:10d}")
