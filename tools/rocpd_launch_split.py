#!/usr/bin/env python3
"""Per kernel of a rocprofv3 (rocpd sqlite) kernel trace whose name matches a pattern: launches at or above / below a duration threshold, with
their total time - what shows a launch that became tiny (or went away) where the per-kernel sums of tools/rocpd_stats.py only move a little:
    python tools/rocpd_launch_split.py bench_results.db [--match 'k_attn|k_gemm'] [--ms 1.0] [--per N]      (--per: divide the counts by N passes)"""
import argparse
import re
import sqlite3

ap = argparse.ArgumentParser()
ap.add_argument("db")
ap.add_argument("--match", default="k_attn|k_gemm")
ap.add_argument("--ms", type=float, default=1.0)
ap.add_argument("--per", type=int, default=1)
a = ap.parse_args()
db = sqlite3.connect(a.db)
tabs = [r[0] for r in db.execute("select name from sqlite_master where type='table'")]
kd = next(t for t in tabs if t.startswith("rocpd_kernel_dispatch"))
ks = next(t for t in tabs if t.startswith("rocpd_info_kernel_symbol"))
scols = [r[1] for r in db.execute(f"pragma table_info({ks})")]
name_col = "display_name" if "display_name" in scols else ("kernel_name" if "kernel_name" in scols else scols[-1])
thr = int(a.ms * 1e6)
rows = db.execute(f"select s.{name_col}, sum(d.end - d.start >= {thr}), sum(case when d.end - d.start >= {thr} then d.end - d.start else 0 end), "
                  f"sum(d.end - d.start < {thr}), sum(case when d.end - d.start < {thr} then d.end - d.start else 0 end) "
                  f"from {kd} d join {ks} s on d.kernel_id = s.id group by s.{name_col} order by 3 desc").fetchall()
print(f"| kernel | launches >= {a.ms:g} ms (per pass) | their total ms | launches < {a.ms:g} ms (per pass) | their total ms |")
print("|---|---:|---:|---:|---:|")
for n, cl, tl, cs, ts in rows:
    n = re.sub(r"\(anonymous namespace\)::", "", n)
    if not re.search(a.match, n):
        continue
    n = n if len(n) < 90 else n[:87] + "..."
    print(f"| `{n}` | {cl} ({cl / a.per:g}) | {tl / 1e6:.3f} | {cs} ({cs / a.per:g}) | {ts / 1e6:.3f} |")
