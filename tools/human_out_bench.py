"""Split runs against the two runs they replace (nh_run_split): gzip -> gzip pairs with a "human" fraction p,
timed on one GPU, interleaved, per p:
  normal  keep_human=0                 (the non-human reads)
  human   keep_human=1, the -H run     (the human reads: until the split run, formatted on the host)
  split   nh_run_split                 (both, one pass, the human side built in HBM)
The database is synthetic (Engine.synthetic at --load, plus the minimizers of a 4 Mb "human" genome inserted with
nh_synthetic_add_sequences); human reads are 150 bp pieces of that genome with 1 % substitutions, the others iid ACGT.
The inputs are `--distinct` gzip members of `--block` pairs each (the library's block-parallel encoder), Illumina-like
(distinct ids, binned qualities), used in rotation up to --pairs; they and the outputs live in /dev/shm.
    python tools/human_out_bench.py [--pairs 50000000] [--p 0.05,0.9] [--reps 2] [--legs normal,human,split]
Prints one JSON line per p.  The builder's kernel time comes from NOHUMAN_TRACE (HIP events around its launches)."""
import argparse
import json
import os
import re
import shutil
import struct
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

TRACE = re.compile(r"human-out: (\d+) records, (\d+) bytes built on device; (\d+) fetched to host; builder kernels ([0-9.]+) ms")


def make_db(dirname, capacity, load, genome):
    """synthetic table + the genome's minimizers (internal taxon 30), written as a database directory"""
    import torch
    from nohuman_amd import Engine
    eng = Engine.synthetic(capacity, int(capacity * load), depth=30, seed=11)
    g = torch.from_numpy(genome).to("cuda")
    piece = 10_000
    offs = torch.arange(0, len(genome) + 1, piece, dtype=torch.int64)
    if offs[-1].item() != len(genome):
        offs = torch.cat([offs, torch.tensor([len(genome)], dtype=torch.int64)])
    offs = offs.to("cuda")
    eng.add_sequences(g.data_ptr(), offs.data_ptr(), len(offs) - 1, 30)
    torch.cuda.synchronize()
    info = eng.info
    os.makedirs(dirname)
    open(os.path.join(dirname, "opts.k2d"), "wb").write(eng.opts_image())
    open(os.path.join(dirname, "taxo.k2d"), "wb").write(eng.taxonomy_image())
    with open(os.path.join(dirname, "hash.k2d"), "wb") as f:
        f.write(struct.pack("<4Q", info.capacity, info.size, info.key_bits, info.value_bits))
        eng.download_table().tofile(f)
    eng.close()


HDR = b"@SYN:1:HGF2YDSXX:L:TTTT:XXXXX:YYYYY M:N:0:GATTACAG\n"


def make_member(rng, genome, n, p, member, L=150):
    """one member's n pairs of FASTQ text per mate, Illumina-like: per-read distinct ids, iid bases, binned qualities that
    degrade from a per-read position (gzip -6 takes such text to about a quarter, as real reads; constant qualities would
    compress 6:1 and change what both codec kernels do).  Fragment i is human with probability p: both mates are then
    pieces of the genome with 1 % substitutions."""
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    human = rng.random(n) < p
    hi = np.nonzero(human)[0]
    gi = np.arange(n, dtype=np.int64) + member * n
    xs = 10_000 + rng.integers(0, 25_000, size=n)
    texts = []
    for mate in (1, 2):
        reclen = len(HDR) + L + 3 + L + 1
        rec = np.empty((n, reclen), dtype=np.uint8)
        rec[:, :len(HDR)] = np.frombuffer(HDR, dtype=np.uint8)

        def digits(col, val, width):
            for d in range(width):
                rec[:, col + width - 1 - d] = 48 + (val // (10 ** d)) % 10
        digits(HDR.index(b"L:"), 1 + (gi // 12_500_000) % 4, 1)
        digits(HDR.index(b"TTTT"), 1101 + (gi // 50_000) % 1000, 4)
        digits(HDR.index(b"XXXXX"), xs, 5)
        digits(HDR.index(b"YYYYY"), 10_000 + ((gi % 50_000) * 17) // 10, 5)
        rec[:, HDR.index(b" M:") + 1] = 48 + mate
        o = len(HDR)
        seq = acgt[rng.integers(0, 4, size=(n, L))]
        starts = rng.integers(0, len(genome) - L, size=len(hi))
        pieces = genome[starts[:, None] + np.arange(L)[None, :]]
        mut = rng.random(pieces.shape) < 0.01
        pieces[mut] = acgt[rng.integers(0, 4, size=int(mut.sum()))]
        seq[hi] = pieces
        rec[:, o:o + L] = seq
        rec[:, o + L:o + L + 3] = np.frombuffer(b"\n+\n", dtype=np.uint8)
        decay = (L * (0.30 + 0.70 * rng.random((n, 1)) ** 0.4)).astype(np.int64)
        pos = np.arange(L)[None, :]
        r = rng.random((n, L))
        q = np.full((n, L), 70, dtype=np.uint8)
        q[(pos < decay) & (r < 0.06)] = 58
        late = pos >= decay
        q[late & (r < 0.45)] = 58
        q[late & (r >= 0.45) & (r < 0.75)] = 44
        q[late & (r >= 0.92)] = 35
        rec[:, o + L + 3:o + 2 * L + 3] = q
        rec[:, -1] = 10
        texts.append(rec.tobytes())
    return texts, int(human.sum())


def timed(fn):
    err = tempfile.NamedTemporaryFile(prefix="trace_", delete=False)
    err.close()
    saved = os.dup(2)
    fd = os.open(err.name, os.O_WRONLY | os.O_TRUNC)
    os.environ["NOHUMAN_TRACE"] = "1"
    try:
        os.dup2(fd, 2)
        t = time.perf_counter()
        st = fn()
        dt = time.perf_counter() - t
    finally:
        os.dup2(saved, 2)
        os.close(saved)
        os.close(fd)
        os.environ.pop("NOHUMAN_TRACE", None)
    tr = open(err.name).read()
    os.remove(err.name)
    return st, dt, tr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=50_000_000)
    ap.add_argument("--block", type=int, default=500_000)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--p", default="0.05,0.9")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--legs", default="normal,human,split")
    ap.add_argument("--capacity", type=int, default=1 << 27)
    ap.add_argument("--load", type=float, default=0.5)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    from nohuman_amd import Engine, _lib
    base = "/dev/shm" if os.access("/dev/shm", os.W_OK) else None
    tmp = tempfile.mkdtemp(prefix="nh_human_out_", dir=base)
    try:
        rng = np.random.default_rng(5)
        genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=4_000_000)].copy()
        db = os.path.join(tmp, "db")
        make_db(db, a.capacity, a.load, genome)
        L = _lib.lib()
        for p in [float(x) for x in a.p.split(",")]:
            block = min(a.block, a.pairs)
            reps = max(1, a.pairs // block)
            room = shutil.disk_usage(tmp).free
            members = [[], []]  # per mate: the distinct gzip members, used in rotation (A B C D A B ...)
            n_human = []
            for k in range(min(a.distinct, reps)):
                texts, nh = make_member(rng, genome, block, p, k)
                n_human.append(nh)
                for m, text in enumerate(texts):
                    plain = os.path.join(tmp, "b_%d.fq" % (m + 1))
                    open(plain, "wb").write(text)
                    gz1 = plain + ".gz"
                    assert L.nh_compress_file(plain.encode(), gz1.encode(), 2, a.threads) == 0, L.nh_last_error()
                    os.remove(plain)
                    members[m].append(open(gz1, "rb").read())
                    os.remove(gz1)
            # inputs + the outputs (each about the input's size) must fit
            per_rep = sum(len(x) for x in members[0] + members[1]) / len(members[0])
            reps = min(reps, max(1, int(0.5 * room / (per_rep * 4))))
            files = []
            for m in range(2):
                path = os.path.join(tmp, "in_%d.fq.gz" % (m + 1))
                with open(path, "wb") as f:
                    for i in range(reps):
                        f.write(members[m][i % len(members[m])])
                files.append(path)
            n_human = sum(n_human[i % len(n_human)] for i in range(reps))
            pairs = block * reps
            res = {"p": p, "pairs": pairs, "human_pairs": n_human, "distinct_members": len(members[0]),
                   "gz_bytes": sum(os.path.getsize(f) for f in files), "legs": {}}
            outs = {k: os.path.join(tmp, k) for k in ("o1", "o2", "h1", "h2")}
            with Engine.open(db) as eng:
                legs = a.legs.split(",")
                for rep in range(a.reps + 1):  # rep 0 warms the buffers and the page cache of the outputs
                    for leg in legs:
                        for f in outs.values():
                            if os.path.exists(f):
                                os.remove(f)
                        kw = dict(in2=files[1], out2=outs["o2"], threads=a.threads, out_codec=2, codec_threads=a.threads // 2)
                        if leg == "human":
                            kw["keep_human"] = True
                        if leg == "split":
                            kw.update(human_out1=outs["h1"], human_out2=outs["h2"])
                        st, dt, tr = timed(lambda: eng.run(files[0], outs["o1"], **kw))
                        if rep == 0:
                            continue
                        r = res["legs"].setdefault(leg, {"wall_s": []})
                        r["wall_s"].append(round(dt, 3))
                        r["classified"] = st.classified
                        m = TRACE.findall(tr)
                        if m:
                            r["built_records"], r["built_bytes"], r["fetched_bytes"] = (int(x) for x in m[0][:3])
                            r.setdefault("builder_kernel_ms", []).append(float(m[0][3]))
                        # where the wall time went (per-thread stage clocks, the encoders' own lines): kept for the last round
                        r["trace"] = [x.split("] ", 1)[-1] for x in tr.splitlines() if "wall " in x or "gzip encoder" in x
                                      or "gzip reader:" in x]
                for leg, r in res["legs"].items():
                    r["best_s"] = min(r["wall_s"])
                    r["mpairs_s"] = round(pairs / r["best_s"] / 1e6, 2)
                    r["mreads_s"] = round(2 * pairs / r["best_s"] / 1e6, 2)  # (reads: the unit of DESIGN.md 6.3's 36-38)
                if all(k in res["legs"] for k in ("normal", "human", "split")):
                    res["split_vs_sum"] = round(res["legs"]["split"]["best_s"] /
                                                (res["legs"]["normal"]["best_s"] + res["legs"]["human"]["best_s"]), 3)
            for f in files + list(outs.values()):
                if os.path.exists(f):
                    os.remove(f)
            print("HUMAN_OUT " + json.dumps(res), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
