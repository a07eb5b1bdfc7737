#!/usr/bin/env python3
"""The entropy stage of every decode in a rocprofv3 --kernel-trace results .db: per batch the span from the first start of
{zk_k_huf, zk_k_fse_predef_fed} to the last end of the two (or the one fused kernel, zk_k_entropy_frame), and each kernel's duration.
A batch whose two kernels do not overlap ran under per-kernel timing (serialised): those durations are the kernels ALONE.
   entropy_span.py <dir or .db> [skip first N batches = warm-up]"""
import glob
import sqlite3
import statistics
import sys

path = sys.argv[1]
skip = int(sys.argv[2]) if len(sys.argv) > 2 else 0
NAMES = ("zk_k_huf", "zk_k_fse_predef_fed", "zk_k_entropy_frame")


def stat(v):
    return f"n {len(v):3d}  min {min(v):6.3f}  median {statistics.median(v):6.3f}  max {max(v):6.3f}" if v else "n   0"


dbs = glob.glob(path + "/**/*_results.db", recursive=True) if not path.endswith(".db") else [path]
for dbp in dbs:
    cur = sqlite3.connect(dbp).cursor()
    cols = [r[1] for r in cur.execute("pragma table_info(kernels)")]
    end = "end" if "end" in cols else "start+duration"
    rows = [(r[0].split("(")[0].replace("void ", ""), r[1], r[2]) for r in cur.execute(f"select name,start,{end} from kernels order by start") if "zk_k_" in r[0]]
    # a decode's second walk (zk_k_scan between the two) is followed by its entropy stage; the batch runs to the next zk_k_exec of its queue.
    # Two batches in flight interleave in the trace, so the kernels are paired in start order per name: huf i with fse i.
    by = {n: [(s, e) for m, s, e in rows if m == n] for n in NAMES}
    huf, fse, fused = (by[n][skip:] for n in NAMES)
    print("==", dbp.split("/")[-1], f"({len(huf)} zk_k_huf, {len(fse)} zk_k_fse_predef_fed, {len(fused)} zk_k_entropy_frame after {skip} skipped)")
    span, h_side, f_side, h_alone, f_alone = [], [], [], [], []
    for (hs, he), (fs, fe) in zip(huf, fse):
        if min(he, fe) - max(hs, fs) <= 0:                 # serialised: per-kernel timing
            h_alone.append((he - hs) / 1e6); f_alone.append((fe - fs) / 1e6)
        else:
            span.append((max(he, fe) - min(hs, fs)) / 1e6); h_side.append((he - hs) / 1e6); f_side.append((fe - fs) / 1e6)
    print("side by side  span (ms)            ", stat(span))
    print("              zk_k_huf             ", stat(h_side))
    print("              zk_k_fse_predef_fed  ", stat(f_side))
    print("alone         zk_k_huf             ", stat(h_alone))
    print("              zk_k_fse_predef_fed  ", stat(f_alone))
    print("fused         zk_k_entropy_frame   ", stat([(e - s) / 1e6 for s, e in fused]))
    if span and h_alone:
        print(f"span - max(alone) = {statistics.median(span) - max(statistics.median(h_alone), statistics.median(f_alone)):.3f} ms (medians)")
