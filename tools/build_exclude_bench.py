#!/usr/bin/env python3
"""nh_build_db_exclude at genome scale: what the exclusion pass and the filter of the inserting pass cost.

The host is build_db_bench.py's synthetic genome (iid ACGT in a few records, a few long N runs, from a seed).  The exclusion input
has the same size: iid ACGT of another seed, a tenth of it copied from the host in `--stretches` stretches, so a tenth of the host's
minimizers are found and flagged and the rest of the look-ups miss.  Both are written as FASTA wrapped at 60 columns.

In one process, after one warm-up build of either kind, `--runs` builds without the list and `--runs` with it; medians.  From the
library's trace lines (HIP events around every batch's launch) the kernels alone:
  (a) EXCLUDE in G k-mers/s of the exclusion text, beside COUNT in G k-mers/s of the host text -- texts of one size and one
      statistic, the same set (COUNT fills it, EXCLUDE probes it when it is full-grown);
  (b) INSERT with the filter (the build with the list) and without (the build without, FILTER = false: the code of the parent);
  (c) the whole call's seconds with and without the list;
  (d) the lowest free device memory seen while a build runs (polled every few ms from a thread), with and without the list.
--parent-lib PATH: a libnohuman_engine.so built from the parent commit; the builds without the list are repeated with it in a child
process on the same FASTA (NOHUMAN_ENGINE_LIB), for (b) and (c) "at the parent commit".

    python tools/build_exclude_bench.py --bases 512000000 --out profiles/build_exclude.txt
"""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from build_db_bench import make_genome, traced, write_fasta  # noqa: E402

TRACE = re.compile(r"kernels alone: count ([0-9.]+) s, insert ([0-9.]+) s")
TRACE_X = re.compile(r"kernels alone: exclude ([0-9.]+) s \(set of ([0-9]+) slots\)")


def make_exclusion(g, seed, share, stretches):
    """iid ACGT of g's size with `share` of it copied from g, in `stretches` stretches at the same offsets"""
    rng = np.random.default_rng(seed)
    x = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=g.size, dtype=np.uint8)]
    ln = int(g.size * share / stretches)
    for i in range(stretches):
        p = int(g.size // stretches * i + g.size // stretches // 3)
        x[p:p + ln] = g[p:p + ln]
    return x


def one_build(nohuman_amd, torch, host, d, threads, exclude, errf):
    """a build with the device's free memory polled beside it -> dict of its stats, kernel times, wall and peak memory in use"""
    low = [torch.cuda.mem_get_info()[0]]
    before = low[0]
    stop = threading.Event()

    def poll():
        while not stop.is_set():
            low[0] = min(low[0], torch.cuda.mem_get_info()[0])
            time.sleep(0.003)

    th = threading.Thread(target=poll)
    th.start()
    t0 = time.time()
    try:
        st = traced(lambda: nohuman_amd.build_db([host], d, threads=threads, exclude=exclude), errf)
    finally:
        wall = time.time() - t0
        stop.set()
        th.join()
    trace = open(errf, errors="replace").read()
    b = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in st.items() if k != "taxon_stats"}
    b["wall_s"] = round(wall, 3)
    m = TRACE.search(trace)
    b["count_kernel_s"], b["insert_kernel_s"] = (float(m.group(1)), float(m.group(2))) if m else (None, None)
    mx = TRACE_X.search(trace)
    if mx:
        b["exclude_kernel_s"], b["set_slots"] = float(mx.group(1)), int(mx.group(2))
    b["peak_device_bytes"] = int(before - low[0])
    b["hash_bytes"] = os.path.getsize(os.path.join(d, "hash.k2d"))
    shutil.rmtree(d)
    return b


def median_of(builds, key):
    v = [b[key] for b in builds if b.get(key) is not None]
    return round(statistics.median(v), 4) if v else None


def child(a):
    """the builds without a list, with whatever library NOHUMAN_ENGINE_LIB names (a parent commit's: no `exclude` argument)"""
    os.environ["NOHUMAN_TRACE"] = "1"
    out = []
    for r in range(a.runs + 1):
        d = os.path.join(a.workdir, "parent_db%d" % r)
        errf = os.path.join(a.workdir, "parent_trace%d.txt" % r)
        t0 = time.time()
        st = traced(lambda: build_plain(a.child, d, a.threads), errf)
        wall = time.time() - t0
        m = TRACE.search(open(errf, errors="replace").read())
        out.append({"wall_s": round(wall, 3), "seconds_count": round(st["seconds_count"], 4), "seconds_insert": round(st["seconds_insert"], 4),
                    "count_kernel_s": float(m.group(1)) if m else None, "insert_kernel_s": float(m.group(2)) if m else None,
                    "size": st["size"]})
        shutil.rmtree(d)
    print("CHILD " + json.dumps(out[1:]))


def build_plain(host, d, threads):
    """nh_build_db through ctypes with nothing but what the parent's library knows (_lib.lib() asks for every present symbol)"""
    import ctypes as C
    from nohuman_amd import _lib
    a = _lib.nh_build_args_v3()
    a.struct_size = C.sizeof(_lib.nh_build_args_v3)
    arr = (C.c_char_p * 1)(os.fsencode(host))
    a.n_fasta, a.fasta, a.out_dir, a.threads = 1, arr, os.fsencode(d), threads
    s = _lib.nh_build_stats_v3()
    L = C.CDLL(_lib.LIB_PATH)
    L.nh_last_error.restype = C.c_char_p
    if L.nh_build_db(C.byref(a), C.byref(s)) != 0:
        raise RuntimeError(L.nh_last_error().decode(errors="replace"))
    return {"seconds_count": s.seconds_count, "seconds_insert": s.seconds_insert, "size": s.size}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bases", type=int, default=256_000_000)
    ap.add_argument("--records", type=int, default=8)
    ap.add_argument("--n-runs", type=int, default=6, help="stretches of N in the host")
    ap.add_argument("--seed", type=int, default=20250101)
    ap.add_argument("--share", type=float, default=0.1, help="share of the exclusion input copied from the host")
    ap.add_argument("--stretches", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3, help="measured builds of either kind, after one warm-up each")
    ap.add_argument("--threads", type=int, default=4)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--parent-lib", default=None, help="libnohuman_engine.so of the parent commit, for the builds without the list")
    ap.add_argument("--out", default=None, help="append the result line to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)

    import torch

    import nohuman_amd
    if not torch.cuda.is_available():
        sys.exit("build_exclude_bench: no GPU (there is no CPU path to measure)")
    print("probe:", nohuman_amd.probe(), file=sys.stderr)
    work = a.workdir or tempfile.mkdtemp(prefix="build_exclude_bench")
    os.makedirs(work, exist_ok=True)
    res = {"bases": a.bases, "records": a.records, "seed": a.seed, "share": a.share, "stretches": a.stretches, "threads": a.threads,
           "runs": a.runs}
    try:
        g, cuts = make_genome(a.bases, a.records, a.n_runs, a.seed)
        host, excl = os.path.join(work, "host.fa"), os.path.join(work, "exclude.fa")
        write_fasta(host, g, cuts)
        write_fasta(excl, make_exclusion(g, a.seed + 7, a.share, a.stretches), cuts)
        del g
        os.environ["NOHUMAN_TRACE"] = "1"
        torch.cuda.init()
        plain, listed = [], []
        for r in range(a.runs + 1):
            plain.append(one_build(nohuman_amd, torch, host, os.path.join(work, "p%d" % r), a.threads, None, os.path.join(work, "tp%d.txt" % r)))
        for r in range(a.runs + 1):
            listed.append(one_build(nohuman_amd, torch, host, os.path.join(work, "x%d" % r), a.threads, [excl], os.path.join(work, "tx%d.txt" % r)))
        res["warmup"] = {"plain_wall_s": plain[0]["wall_s"], "listed_wall_s": listed[0]["wall_s"]}
        plain, listed = plain[1:], listed[1:]
        last = listed[-1]
        res["host"] = {k: last[k] for k in ("kmers", "ambiguous_kmers", "distinct_minimizers")}
        res["exclusion"] = {k: last[k] for k in ("exclude_kmers", "exclude_lookups", "excluded_minimizers", "kept_minimizers", "set_slots")}
        res["capacity"] = {"plain": plain[-1]["capacity"], "listed": last["capacity"]}
        res["hash_bytes"] = {"plain": plain[-1]["hash_bytes"], "listed": last["hash_bytes"]}
        keys = ("count_kernel_s", "exclude_kernel_s", "insert_kernel_s", "seconds_count", "seconds_exclude", "seconds_exclude_read",
                "seconds_insert", "seconds_read", "seconds_write", "wall_s", "peak_device_bytes")
        res["plain_median"] = {k: median_of(plain, k) for k in keys if median_of(plain, k) is not None}
        res["listed_median"] = {k: median_of(listed, k) for k in keys if median_of(listed, k) is not None}
        res["plain_runs"] = [[b["count_kernel_s"], b["insert_kernel_s"], b["wall_s"]] for b in plain]
        res["listed_runs"] = [[b["count_kernel_s"], b.get("exclude_kernel_s"), b["insert_kernel_s"], b["wall_s"]] for b in listed]
        lm, pm = res["listed_median"], res["plain_median"]
        if lm.get("exclude_kernel_s"):
            res["exclude_kernel_Gkmers_s"] = round(last["exclude_kmers"] / lm["exclude_kernel_s"] / 1e9, 2)
            res["count_kernel_Gkmers_s"] = round(last["kmers"] / lm["count_kernel_s"] / 1e9, 2)
            res["exclude_over_count"] = round(lm["exclude_kernel_s"] / lm["count_kernel_s"], 3)
        if lm.get("insert_kernel_s") and pm.get("insert_kernel_s"):
            res["insert_kernel_filter_on_over_off"] = round(lm["insert_kernel_s"] / pm["insert_kernel_s"], 3)
        res["wall_listed_over_plain"] = round(lm["wall_s"] / pm["wall_s"], 3)
        if a.parent_lib:
            env = dict(os.environ, NOHUMAN_ENGINE_LIB=os.path.abspath(a.parent_lib))
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", host, "--workdir", work, "--runs", str(a.runs),
                                "--threads", str(a.threads)], env=env, capture_output=True, text=True, timeout=900)
            got = [ln for ln in p.stdout.splitlines() if ln.startswith("CHILD ")]
            if p.returncode != 0 or not got:
                res["parent_error"] = (p.stderr or p.stdout)[-400:]
            else:
                runs = json.loads(got[0][6:])
                res["parent_median"] = {k: median_of(runs, k) for k in ("count_kernel_s", "insert_kernel_s", "seconds_count", "seconds_insert", "wall_s")}
                if res["parent_median"].get("insert_kernel_s"):
                    res["insert_kernel_filter_on_over_parent"] = round(lm["insert_kernel_s"] / res["parent_median"]["insert_kernel_s"], 3)
                res["wall_listed_over_parent"] = round(lm["wall_s"] / res["parent_median"]["wall_s"], 3)
    finally:
        if not a.workdir:
            shutil.rmtree(work, ignore_errors=True)
    line = "BUILD_EXCLUDE " + json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
