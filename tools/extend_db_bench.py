#!/usr/bin/env python3
"""nh_extend_db at genome scale, stage by stage, beside a copy of the table and beside the rebuild it replaces.

A synthetic base (tools/build_db_bench.py's genome: iid ACGT, a few long N runs) is built into a database once.  It is then
extended by a small and by a large synthetic genome, each split over two taxa by a manifest, so that the value field grows from two
to three bits and the re-key and shadow passes run; the small one also as one taxon, where the table is only read.  Per extension:
seconds_load (hash.k2d to the device), seconds_rekey (HIP events round the re-key and shadow kernels) and from the library's trace line
the streaming pass alone, the insert and write stages of nh_build_stats, the wall time, and the counts.

Yardsticks, in the same process: a device-to-device copy of a buffer of the table's size (torch; HIP events, the median of several)
-- the re-key pass reads and writes every cell once, the traffic of a copy -- and the only alternative without nh_extend_db:
nh_build_db of base + addition from their FASTA files at the same capacity.

    python tools/extend_db_bench.py --bases 512000000 --small 5000 --large 50000000 --out profiles/extend_db.txt
"""
import argparse
import hashlib
import json
import os
import re
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from build_db_bench import make_genome, traced, write_fasta  # noqa: E402

TRACE = re.compile(r"re-key ([0-9.]+) s \(the streaming pass alone ([0-9.]+) s\)")
SOURCES = ("nohuman_amd/csrc/nh_extend.hip", "nohuman_amd/csrc/nh_extend.h", "nohuman_amd/csrc/nh_build.hip", "nohuman_amd/csrc/nh_scan.h")


def kernel_source_sha16():
    h = hashlib.sha256()
    for f in SOURCES:
        h.update(open(os.path.join(ROOT, f), "rb").read())
    return h.hexdigest()[:16]


def two_taxa(work, name, bases, seed):
    """a genome of `bases` bases over two FASTA files and their manifest (taxids 20 and 30 under the root)"""
    g, _ = make_genome(bases, 2, 0, seed)
    half = bases // 2
    files = []
    for i, part in enumerate((g[:half], g[half:])):
        p = os.path.join(work, "%s_%d.fa" % (name, i))
        write_fasta(p, part, np.array([0, part.size], dtype=np.int64))
        files.append(p)
    m = os.path.join(work, name + ".tsv")
    with open(m, "w") as f:
        for i, p in enumerate(files):
            f.write("%d\t1\t%s %d\t%s\n" % (20 + 10 * i, name, i, p))
    return files, m


def rounded(st):
    return {k: (round(v, 5) if isinstance(v, float) else v) for k, v in st.items() if k != "taxon_stats"}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bases", type=int, default=512_000_000, help="of the base genome")
    ap.add_argument("--small", type=int, default=5_000)
    ap.add_argument("--large", type=int, default=50_000_000)
    ap.add_argument("--seed", type=int, default=20250101)
    ap.add_argument("--runs", type=int, default=3, help="extensions of each kind; the first is the warm-up")
    ap.add_argument("--threads", type=int, default=4)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--out", default=None, help="append the result line to this file")
    a = ap.parse_args()

    import torch

    import nohuman_amd
    if not torch.cuda.is_available():
        sys.exit("extend_db_bench: no GPU (there is no CPU path to measure)")
    work = a.workdir or tempfile.mkdtemp(prefix="extend_db_bench")
    os.makedirs(work, exist_ok=True)
    res = {"bases": a.bases, "small": a.small, "large": a.large, "seed": a.seed, "threads": a.threads, "kernel_source_sha16": kernel_source_sha16()}
    try:
        g, cuts = make_genome(a.bases, 8, 6, a.seed)
        fa = os.path.join(work, "base.fa")
        write_fasta(fa, g, cuts)
        del g
        base = os.path.join(work, "base")
        t0 = time.time()
        os.environ["NOHUMAN_TRACE"] = "1"
        bst = nohuman_amd.build_db([fa], base, taxid=10, taxon_name="base", threads=a.threads)
        res["base"] = dict(rounded(bst), wall_s=round(time.time() - t0, 3))
        cap = bst["capacity"]
        res["table_bytes"] = 4 * cap

        # the yardstick of the re-key pass: a device-to-device copy of the table's size
        dev = torch.device("cuda:0")
        src = torch.zeros(cap, dtype=torch.int32, device=dev)
        dst = torch.empty_like(src)
        times = []
        for _ in range(9):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e-3)
        del src, dst
        torch.cuda.empty_cache()
        res["d2d_copy_s"] = round(float(np.median(times[2:])), 6)
        res["d2d_copy_GB_s"] = round(2 * 4 * cap / res["d2d_copy_s"] / 1e9, 1)

        for name, bases in (("small", a.small), ("large", a.large)):
            files, manifest = two_taxa(work, name, bases, a.seed + (1 if name == "small" else 2))
            runs = []
            for r in range(a.runs):
                d = os.path.join(work, "ext_%s" % name)
                t0 = time.time()
                errf = os.path.join(work, "trace.txt")
                st = traced(lambda: nohuman_amd.extend_db(base, d, taxa=manifest, threads=a.threads, force=True), errf)
                runs.append(dict(rounded(st), wall_s=round(time.time() - t0, 3)))
                m = TRACE.search(open(errf, errors="replace").read())
                if m:  # (the trace line: k_ext_rekey alone; the rest of seconds_rekey is the shadow pass and the wait between the two)
                    runs[-1]["rekey_pass_s"] = float(m.group(2))
            res[name] = runs
            last = runs[-1]
            res[name + "_rekey_over_copy"] = round(last["seconds_rekey"] / res["d2d_copy_s"], 2)
            if "rekey_pass_s" in last:
                res[name + "_rekey_pass_over_copy"] = round(last["rekey_pass_s"] / res["d2d_copy_s"], 2)
            with nohuman_amd.Engine.open(d) as eng:  # the result opens (content check) and holds what the call says
                assert eng.db_check().non_empty_cells == last["size"]
            shutil.rmtree(d)
            # the rebuild: base + addition from FASTA at the same capacity
            m2 = os.path.join(work, name + "_union.tsv")
            with open(m2, "w") as f:
                f.write("10\t1\tbase\t%s\n" % fa)
                f.write(open(manifest).read())
            d = os.path.join(work, "rebuild_%s" % name)
            t0 = time.time()
            rst = nohuman_amd.build_db(None, d, taxa=m2, capacity=cap, threads=a.threads)
            res[name + "_rebuild"] = dict(rounded(rst), wall_s=round(time.time() - t0, 3))
            # (keys that collide at the narrower width merge or not by the order of arrival: the sizes may differ by a few cells)
            res[name + "_size_minus_rebuild"] = last["size"] - rst["size"]
            shutil.rmtree(d)
            res[name + "_extension_over_rebuild"] = round(last["wall_s"] / res[name + "_rebuild"]["wall_s"], 4)
            if name == "small":  # one taxon: the value field keeps its two bits, the table is read once and not written
                runs = []
                for r in range(a.runs):
                    d = os.path.join(work, "ext_one")
                    t0 = time.time()
                    st = nohuman_amd.extend_db(base, d, files, taxid=20, taxon_name="small", threads=a.threads, force=True)
                    runs.append(dict(rounded(st), wall_s=round(time.time() - t0, 3)))
                shutil.rmtree(d)
                res["small_one_taxon"] = runs
    finally:
        if not a.workdir:
            shutil.rmtree(work, ignore_errors=True)
    line = "EXTEND_DB " + json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
