"""What the read lists cost (nh_run_ex's `calls` / `human_ids`): gzip -> gzip runs of pairs with a
"human" fraction p on one GPU, timed in the same process, interleaved:
  none    no list, no -k                  (the run as it was)
  lists   calls table and human ids       (built in HBM, only their bytes fetched)
  k       -k/--kraken-output instead      (per-k-mer taxon lists downloaded, every batch's text fetched, lines made on the host)
Inputs, database and workload are tools/human_out_bench.py's: a synthetic table plus the minimizers of a 4 Mb "human" genome,
human pairs are 150 bp pieces of it with 1 % substitutions; `--distinct` gzip members of `--block` pairs used in rotation up to
--pairs; inputs and outputs in /dev/shm.  One warm-up round, then --reps timed rounds; medians and the spread of each leg.
The list builder's kernel time comes from NOHUMAN_TRACE (HIP events around its launches).  The last round's table is
checked against the -k file of the same round: columns 1-4 equal, line for line.
--repo DIR imports nohuman_amd from another tree (a checkout of the parent commit, built): only the leg `none` runs there --
that is the baseline the cost of the lists is measured against.
    python tools/calls_bench.py [--pairs 4000000] [--p 0.05] [--reps 3] [--legs none,lists,k] [--out profiles/calls_table.txt]
Prints one JSON line and appends it to --out."""
import argparse
import json
import os
import re
import shutil
import statistics
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TRACE = re.compile(r"calls: (\d+) lines, (\d+) bytes; ids: (\d+) lines, (\d+) bytes built on device; (\d+) fetched to host; "
                   r"builder kernels ([0-9.]+) ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4_000_000)
    ap.add_argument("--block", type=int, default=500_000)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--p", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default="none,lists,k")
    ap.add_argument("--capacity", type=int, default=1 << 27)
    ap.add_argument("--load", type=float, default=0.5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repo", default=os.path.dirname(HERE))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    import numpy as np
    from human_out_bench import make_db, make_member, timed
    sys.path.insert(0, os.path.abspath(a.repo))  # (last: the tree named here is the one nohuman_amd comes from)
    from nohuman_amd import Engine, _lib
    base = "/dev/shm" if os.access("/dev/shm", os.W_OK) else None
    tmp = tempfile.mkdtemp(prefix="nh_calls_", dir=base)
    try:
        rng = np.random.default_rng(5)
        genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=4_000_000)].copy()
        db = os.path.join(tmp, "db")
        make_db(db, a.capacity, a.load, genome)
        L = _lib.lib()
        block = min(a.block, a.pairs)
        reps = max(1, a.pairs // block)
        members = [[], []]
        for k in range(min(a.distinct, reps)):
            texts, _nh = make_member(rng, genome, block, a.p, k)
            for m, text in enumerate(texts):
                pl = os.path.join(tmp, "b_%d.fq" % (m + 1))
                open(pl, "wb").write(text)
                assert L.nh_compress_file(pl.encode(), (pl + ".gz").encode(), 2, a.threads) == 0, L.nh_last_error()
                os.remove(pl)
                members[m].append(open(pl + ".gz", "rb").read())
                os.remove(pl + ".gz")
        files = []
        for m in range(2):
            path = os.path.join(tmp, "in_%d.fq.gz" % (m + 1))
            with open(path, "wb") as f:
                for i in range(reps):
                    f.write(members[m][i % len(members[m])])
            files.append(path)
        pairs = block * reps
        res = {"repo": os.path.abspath(a.repo), "p": a.p, "pairs": pairs, "gz_bytes": sum(os.path.getsize(f) for f in files), "legs": {}}
        outs = [os.path.join(tmp, "o_%d.fq.gz" % (m + 1)) for m in range(2)]
        paths = {x: os.path.join(tmp, x) for x in ("calls.tsv", "ids.txt", "k.txt")}
        with Engine.open(db) as eng:
            for rep in range(a.reps + 1):  # rep 0 warms the buffers and the page cache of the outputs
                for leg in a.legs.split(","):
                    kw = dict(in2=files[1], out2=outs[1], threads=a.threads, out_codec=2, codec_threads=a.threads // 2)
                    if leg == "lists":
                        kw.update(calls=paths["calls.tsv"], human_ids=paths["ids.txt"])
                    elif leg == "k":
                        kw.update(kraken_output=paths["k.txt"])
                    st, dt, tr = timed(lambda: eng.run(files[0], outs[0], **kw))
                    if rep == 0:
                        continue
                    r = res["legs"].setdefault(leg, {"wall_s": []})
                    r["wall_s"].append(round(dt, 3))
                    r["classified"] = st.classified
                    t = TRACE.findall(tr)
                    if t:
                        r["calls_lines"], r["calls_bytes"], r["ids_lines"], r["ids_bytes"], r["fetched_bytes"] = (int(x) for x in t[0][:5])
                        r.setdefault("builder_kernel_ms", []).append(float(t[0][5]))
                    r["trace"] = [x.split("] ", 1)[-1] for x in tr.splitlines() if "wall " in x or "gzip reader:" in x]
        for leg, r in res["legs"].items():
            r["median_s"] = statistics.median(r["wall_s"])
            r["spread_s"] = round(max(r["wall_s"]) - min(r["wall_s"]), 3)
            r["mreads_s"] = round(2 * pairs / r["median_s"] / 1e6, 2)
        lg = res["legs"]
        if "lists" in lg and "none" in lg:
            res["lists_vs_none"] = round(lg["lists"]["median_s"] / lg["none"]["median_s"], 3)
        if "lists" in lg and "k" in lg:
            res["k_vs_lists"] = round(lg["k"]["median_s"] / lg["lists"]["median_s"], 3)
            with open(paths["calls.tsv"], "rb") as fc, open(paths["k.txt"], "rb") as fk:
                same = all(c.split(b"\t")[:4] == k.split(b"\t")[:4] for c, k in zip(fc, fk)) and fc.readline() == fk.readline() == b""
            res["columns_1_4_equal_k"] = same
        line = "CALLS " + json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
