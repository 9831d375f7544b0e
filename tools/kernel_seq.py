#!/usr/bin/env python3
"""The sequence of kernel names on every queue of a rocprofv3 --kernel-trace CSV (plain or .gz), runs of one launch folded into "x N".
usage: kernel_seq.py kernel_trace.csv > listing.txt
Two listings are equal exactly when every queue ran the same kernels with the same grids in the same order; the order ACROSS queues
is not recorded.  Queues are numbered by their first launch; template arguments are dropped except for the group (g1 / g2)."""
import csv
import gzip
import re
import sys


def short(n):
    m = re.search(r"\b(k_\w+)", n)
    if m:
        k = m.group(1)
    elif "rocprim" in n:
        k = "rocprim"
    else:
        k = re.split(r"[<(]", n.replace("void ", ""))[0].strip() or n[:40]
    if "Fq2" in n or "g2pair" in n or "G2Pair" in n:
        k += ".g2"
    elif "FqField" in n or "RedG1" in n:
        k += ".g1"
    return k


f = sys.argv[1]
rows = sorted(csv.DictReader(gzip.open(f, "rt") if f.endswith(".gz") else open(f)), key=lambda r: (int(r["Start_Timestamp"]), int(r["Dispatch_Id"])))
queues = {}
for r in rows:
    queues.setdefault(r["Queue_Id"], []).append("%s grid=%s" % (short(r["Kernel_Name"]), r["Grid_Size_X"]))
for i, seq in enumerate(queues.values()):
    print("== queue %d: %d launches" % (i, len(seq)))
    j = 0
    while j < len(seq):
        k = j
        while k < len(seq) and seq[k] == seq[j]:
            k += 1
        print(seq[j] + (" x %d" % (k - j) if k - j > 1 else ""))
        j = k
