#!/usr/bin/env python3
"""nh_build_db at genome scale, stage by stage, beside the only insert baseline there is.

A synthetic genome (iid ACGT in a few records, a few long N runs; generated from a seed, no file from outside) is written as FASTA
wrapped at 60 columns and built into a database with nh_build_db (nohuman_amd.build_db): the four stage times of nh_build_stats, and
from the library's trace line the two passes' kernel time alone (HIP events around every batch's launch).  The build runs `--runs`
times; the first run also loads the code objects and is reported apart.

Baseline: the same bases, resident in HBM, cut into contiguous NON-overlapping sequences of piece_kmers + 34 bases and pushed through
nh_synthetic_add_sequences (k_insert_sequences, one wave a sequence) into an nh_open_synthetic table of the same capacity, one copy
of the table (NOHUMAN_TABLE_COPIES=1, so that the call does not also copy the table).  It loses the k-mers that span two of its
sequences (34 in every piece_kmers + 34), so it inserts slightly fewer minimizers: the rates are per inserted cell.  Host clock around
the call, which ends in a device synchronise.

    python tools/build_db_bench.py --bases 512000000 --out profiles/build_db.txt

--mask-low-complexity builds with the masking on (nh_dust.hip): masked_bases, seconds_mask and, from the trace line, the mask
kernel's time over both passes (HIP events) join each build's numbers.  The mask's work does not depend on the content, but what it
masks does: --low-complexity-share F plants homopolymers and microsatellites (periods 2 to 6, 20 to 400 bases each) over about that
share of the genome, which as iid ACGT masks some 0.1 %.

--taxa N --shared F splits the genome over N taxa under the root, a FASTA file each: every file holds bases / N bases, of which the
share F is one stretch that all the files have and the rest the taxon's own.  The files are first built as ONE taxon (all of them
under one taxid: the same bases, the one-taxon insert kernel), then through a manifest; both in this process, `--runs` times each.
From the trace lines: the insert kernel's time of either build, the time of the kernel that counts the cells per node, and the
share of the insertions that found their key under another taxon's value (the LCA path) with the values they replaced.
"""
import argparse
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

TRACE = re.compile(r"kernels alone: count ([0-9.]+) s, insert ([0-9.]+) s")
TRACE_MASK = re.compile(r"mask ([0-9.]+) s for ([0-9]+) masked bases")
TRACE_TAXA = re.compile(r"insertions ([0-9]+), of them ([0-9]+) found .* values replaced ([0-9]+); cells per node ([0-9.]+) s")
PIECE = 1984  # the library's default piece: 16 tiles of 124 k-mers


def make_genome(bases, n_records, n_runs, seed, low_share=0.0):
    """uint8 array of ACGT with n_runs stretches of N (10 kb to 1 Mb), and the records' boundaries; low_share: about that share
    of the bases under planted homopolymers and repeats of period 2 to 6 (drawn after the N runs' generator, so that a share of 0
    gives the genome the tool always made)"""
    rng = np.random.default_rng(seed)
    g = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=bases, dtype=np.uint8)]
    if low_share > 0:
        lrng = np.random.default_rng(seed + 1)
        n = max(1, int(bases * low_share / 210))  # (lengths are uniform in 20 .. 400)
        lens = lrng.integers(20, 401, size=n)
        at = lrng.integers(0, max(1, bases - 400), size=n)
        acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
        for p, ln in zip(at.tolist(), lens.tolist()):
            unit = acgt[lrng.integers(0, 4, size=int(lrng.integers(1, 7)))]
            g[p:p + ln] = np.resize(unit, ln)
    for _ in range(n_runs):
        ln = int(min(bases // 20 + 1, 10 ** rng.uniform(4, 6)))
        p = int(rng.integers(0, bases - ln))
        g[p:p + ln] = ord("N")
    cuts = np.linspace(0, bases, n_records + 1).astype(np.int64)
    return g, cuts


def write_fasta(path, g, cuts, width=60):
    with open(path, "wb") as f:
        for i in range(len(cuts) - 1):
            s = g[cuts[i]:cuts[i + 1]]
            f.write(b">chr%d synthetic\n" % (i + 1))
            full = s.size // width * width
            if full:
                rows = np.empty((full // width, width + 1), dtype=np.uint8)
                rows[:, :width] = s[:full].reshape(-1, width)
                rows[:, width] = ord("\n")
                f.write(rows.tobytes())
            if s.size > full:
                f.write(s[full:].tobytes() + b"\n")
    return os.path.getsize(path)


def write_taxa(work, g, n_taxa, shared):
    """the genome over n_taxa FASTA files of g.size / n_taxa bases each, the first `shared` of every file the same stretch (the
    genome's first bases), and their manifest: leaves under the root -> (the files, the manifest's path)"""
    per = g.size // n_taxa
    n_shared = int(per * shared)
    own = per - n_shared
    files, lines = [], []
    for i in range(n_taxa):
        p = os.path.join(work, "taxon%d.fa" % i)
        part = np.concatenate([g[:n_shared], g[n_shared + i * own:n_shared + (i + 1) * own]])
        write_fasta(p, part, np.linspace(0, part.size, 3).astype(np.int64))
        files.append(p)
        lines.append("%d\t1\ttaxon %d\t%s\n" % (100 + i, i, p))
    manifest = os.path.join(work, "taxa.tsv")
    with open(manifest, "w") as f:
        f.writelines(lines)
    return files, manifest


def traced(fn, errf):
    """fn() with the library's stderr (fd 2) in a file: the trace line"""
    saved = os.dup(2)
    fd = os.open(errf, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    os.dup2(fd, 2)
    os.close(fd)
    try:
        return fn()
    finally:
        os.dup2(saved, 2)
        os.close(saved)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bases", type=int, default=256_000_000)
    ap.add_argument("--records", type=int, default=8)
    ap.add_argument("--n-runs", type=int, default=6, help="stretches of N")
    ap.add_argument("--seed", type=int, default=20250101)
    ap.add_argument("--runs", type=int, default=3, help="builds; the first is the warm-up")
    ap.add_argument("--threads", type=int, default=4)
    ap.add_argument("--workdir", default=None, help="where the FASTA and the databases go (default: a temporary directory)")
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    ap.add_argument("--mask-low-complexity", action="store_true", help="build with low-complexity masking")
    ap.add_argument("--low-complexity-share", type=float, default=0.0, metavar="F",
                    help="plant homopolymers and microsatellites over about this share of the genome")
    ap.add_argument("--no-baseline", action="store_true", help="leave out the k_insert_sequences baseline")
    ap.add_argument("--taxa", type=int, default=0, metavar="N", help="split the genome over N taxa and build it through a manifest too")
    ap.add_argument("--shared", type=float, default=0.0, metavar="FRACTION", help="with --taxa: the share of every taxon's bases that all taxa have")
    a = ap.parse_args()

    import torch

    import nohuman_amd
    if not torch.cuda.is_available():
        sys.exit("build_db_bench: no GPU (there is no CPU path to measure)")
    print("probe:", nohuman_amd.probe(), file=sys.stderr)
    work = a.workdir or tempfile.mkdtemp(prefix="build_db_bench")
    os.makedirs(work, exist_ok=True)
    res = {"bases": a.bases, "records": a.records, "n_runs": a.n_runs, "seed": a.seed, "piece_kmers": PIECE, "threads": a.threads,
           "mask_low_complexity": a.mask_low_complexity, "low_complexity_share": a.low_complexity_share}
    try:
        t0 = time.time()
        g, cuts = make_genome(a.bases, a.records, a.n_runs, a.seed, a.low_complexity_share)
        fa = os.path.join(work, "genome.fa")
        res["fasta_bytes"] = write_fasta(fa, g, cuts)
        res["generate_s"] = round(time.time() - t0, 2)
        os.environ["NOHUMAN_TRACE"] = "1"
        inputs, manifest = [fa], None
        if a.taxa:
            inputs, manifest = write_taxa(work, g, a.taxa, a.shared)
            os.unlink(fa)
            res["taxa"], res["shared"] = a.taxa, a.shared
        builds, taxa_builds = [], []
        for r in range(a.runs * (2 if a.taxa else 1)):
            by_manifest = r >= a.runs
            d = os.path.join(work, "db%d" % r)
            errf = os.path.join(work, "trace%d.txt" % r)
            t0 = time.time()
            kw = {"mask_low_complexity": True} if a.mask_low_complexity else {}
            if by_manifest:
                st = traced(lambda: nohuman_amd.build_db(None, d, taxa=manifest, threads=a.threads, **kw), errf)
            else:
                st = traced(lambda: nohuman_amd.build_db(inputs, d, threads=a.threads, **kw), errf)
            wall = time.time() - t0
            trace = open(errf, errors="replace").read()
            m = TRACE.search(trace)
            b = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in st.items() if k != "taxon_stats"}
            if by_manifest:
                mt = TRACE_TAXA.search(trace)
                b["cells_per_taxon"] = [x["cells"] for x in st["taxon_stats"]]
                if mt:
                    b["insertions"], b["lca_path"], b["values_replaced"] = (int(mt.group(i)) for i in (1, 2, 3))
                    b["value_cells_kernel_s"] = float(mt.group(4))
                    b["lca_share"] = round(b["lca_path"] / max(1, b["insertions"]), 5)
                b["wall_s"] = round(wall, 3)
                b["count_kernel_s"], b["insert_kernel_s"] = (float(m.group(1)), float(m.group(2))) if m else (None, None)
                taxa_builds.append(b)
                shutil.rmtree(d)
                continue
            b["wall_s"] = round(wall, 3)
            b["count_kernel_s"], b["insert_kernel_s"] = (float(m.group(1)), float(m.group(2))) if m else (None, None)
            mm = TRACE_MASK.search(trace)
            if a.mask_low_complexity and mm:
                b["mask_kernel_s"] = float(mm.group(1))
            b["hash_bytes"] = os.path.getsize(os.path.join(d, "hash.k2d"))
            builds.append(b)
            if r + 1 < a.runs:
                shutil.rmtree(d)
        res["builds"] = builds
        if taxa_builds:
            res["taxa_builds"] = taxa_builds
            one, many = builds[-1]["insert_kernel_s"], taxa_builds[-1]["insert_kernel_s"]
            if one and many:
                res["taxa_insert_kernel_ratio"] = round(many / one, 3)
        last = builds[-1]
        cap, size = last["capacity"], last["size"]
        res["load_factor"] = round(size / cap, 4)
        if last["insert_kernel_s"]:
            res["insert_kernel_Mcells_s"] = round(size / last["insert_kernel_s"] / 1e6, 1)
            res["count_kernel_Mkeys_s"] = round(last["distinct_minimizers"] / last["count_kernel_s"] / 1e6, 1)
        res["insert_stage_Mcells_s"] = round(size / last["seconds_insert"] / 1e6, 1)
        res["whole_build_Mbases_s"] = round(a.bases / last["wall_s"] / 1e6, 1)
        if last.get("mask_kernel_s"):  # (both passes: every base goes through the kernel twice)
            res["mask_kernel_Gbases_s"] = round(2 * a.bases / last["mask_kernel_s"] / 1e9, 2)
            res["masked_share"] = round(last["masked_bases"] / a.bases, 5)
        # the database opens (content check) and holds what the build says
        with nohuman_amd.Engine.open(os.path.join(work, "db%d" % (a.runs - 1))) as eng:
            assert eng.db_check().non_empty_cells == size

        if not a.no_baseline and not a.taxa:
            # ---- baseline: k_insert_sequences on the same bases, resident, contiguous sequences of one piece each
            os.environ["NOHUMAN_TABLE_COPIES"] = "1"
            dev = torch.device("cuda:0")
            seg = PIECE + 34
            offs = []
            for i in range(len(cuts) - 1):
                o = np.arange(cuts[i], cuts[i + 1], seg, dtype=np.int64)
                offs.append(o)
            offs = np.concatenate(offs + [np.array([a.bases], dtype=np.int64)])
            # (a record's last sequence ends where the next record starts: boundaries are sequence starts)
            d_bases = torch.empty(a.bases + 64, dtype=torch.uint8, device=dev)
            d_bases[:a.bases] = torch.from_numpy(g).to(dev)
            d_bases[a.bases:] = 0
            d_offs = torch.from_numpy(offs).to(dev)
            base = []
            for r in range(a.runs):
                with nohuman_amd.Engine.synthetic(cap, 0, depth=2, seed=1) as eng:
                    torch.cuda.synchronize()
                    t0 = time.time()
                    eng.add_sequences(d_bases.data_ptr(), d_offs.data_ptr(), offs.size - 1, 2)
                    torch.cuda.synchronize()
                    dt = time.time() - t0
                    base.append({"seconds": round(dt, 4), "size": int(eng.info.size)})
            res["baseline"] = base
            res["baseline_sequences"] = int(offs.size - 1)
            res["baseline_Mcells_s"] = round(base[-1]["size"] / base[-1]["seconds"] / 1e6, 1)
    finally:
        if not a.workdir:
            shutil.rmtree(work, ignore_errors=True)
    line = "BUILD_DB " + json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
