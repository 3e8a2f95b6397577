"""Per-taxon outputs against the classified-out builder they are modelled on (nh_run_taxa): one
process, HIP events only (the NOHUMAN_TRACE event pairs around the builders' launches), no profiler.  The table is the bench's
synthetic one (Engine.synthetic, a chain taxonomy of 30 nodes) with four 1 Mb genomes planted at four nodes of the chain; the
reads are 150 bp pairs, half of them pieces of those genomes with 1 % substitutions (tools/human_out_bench.py's generator),
plain FASTQ in /dev/shm, outputs in --codec.  For the same batches, three runs each, the last reported:
  split      the existing k_hout_* launches (human outputs given): kernel time, files-in -> files-out time
  taxa K     the k_tout_* launches with K = 1, 4, 8 selectors (no human outputs): kernel time
  split+4    the split run with 4 selectors added: files-in -> files-out time against `split`
    python tools/taxon_out_bench.py [--pairs 2000000] [--codec 2]
Prints one JSON line."""
import argparse
import json
import os
import re
import shutil
import struct
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
from human_out_bench import make_member, timed  # noqa: E402

HUMAN = re.compile(r"human-out: (\d+) records, (\d+) bytes built on device; (\d+) fetched to host; builder kernels ([0-9.]+) ms")
TAXON = re.compile(r"taxon-out: (\d+) records, (\d+) bytes built on device; (\d+) fetched to host; kernel ([0-9.]+) ms")
PLANTED = (12, 18, 24, 30)  # internal ids of the chain the four genomes are planted at


def make_db(dirname, capacity, load, genome):
    """synthetic table + the minimizers of the genome's four quarters, each under its own node; returns the chain's external ids"""
    import torch
    from nohuman_amd import Engine
    eng = Engine.synthetic(capacity, int(capacity * load), depth=30, seed=11)
    quarter = len(genome) // 4
    for q, value in enumerate(PLANTED):
        part = genome[q * quarter:(q + 1) * quarter]
        g = torch.from_numpy(part.copy()).to("cuda")
        offs = torch.arange(0, len(part) + 1, 10_000, dtype=torch.int64)
        if offs[-1].item() != len(part):
            offs = torch.cat([offs, torch.tensor([len(part)], dtype=torch.int64)])
        offs = offs.to("cuda")
        eng.add_sequences(g.data_ptr(), offs.data_ptr(), len(offs) - 1, value)
        torch.cuda.synchronize()
    info = eng.info
    ext = [eng.external_id(i) for i in range(int(info.node_count))]
    os.makedirs(dirname)
    open(os.path.join(dirname, "opts.k2d"), "wb").write(eng.opts_image())
    open(os.path.join(dirname, "taxo.k2d"), "wb").write(eng.taxonomy_image())
    with open(os.path.join(dirname, "hash.k2d"), "wb") as f:
        f.write(struct.pack("<4Q", info.capacity, info.size, info.key_bits, info.value_bits))
        eng.download_table().tofile(f)
    eng.close()
    return ext


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2_000_000)
    ap.add_argument("--codec", type=int, default=2)
    ap.add_argument("--capacity", type=int, default=1 << 27)
    ap.add_argument("--load", type=float, default=0.5)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    from nohuman_amd import Engine
    base = "/dev/shm" if os.access("/dev/shm", os.W_OK) else None
    tmp = tempfile.mkdtemp(prefix="nh_taxon_out_", dir=base)
    try:
        rng = np.random.default_rng(5)
        genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=4_000_000)].copy()
        db = os.path.join(tmp, "db")
        ext = make_db(db, a.capacity, a.load, genome)
        block = min(500_000, a.pairs)
        files = [os.path.join(tmp, "in_%d.fq" % (m + 1)) for m in range(2)]
        hitting = 0
        with open(files[0], "wb") as f1, open(files[1], "wb") as f2:
            for k in range(max(1, a.pairs // block)):
                texts, nh = make_member(rng, genome, block, 0.5, k)
                hitting += nh
                f1.write(texts[0])
                f2.write(texts[1])
        pairs = block * max(1, a.pairs // block)
        sel = {1: [ext[1]], 4: [ext[i] for i in PLANTED], 8: [ext[i] for i in (12, 15, 18, 21, 24, 27, 30)] + ["other"]}
        sfx = {0: ".fq", 2: ".fq.gz", 4: ".fq.zst", 5: ".fq.gz"}[a.codec]
        res = {"pairs": pairs, "hitting_pairs": hitting, "codec": a.codec, "legs": {}}
        legs = [("split", True, 0), ("taxa1", False, 1), ("taxa4", False, 4), ("taxa8", False, 8), ("split+4", True, 4)]
        with Engine.open(db) as eng:
            for rep in range(3):  # the last one is reported
                for name, human, K in legs:
                    out = os.path.join(tmp, "out")
                    shutil.rmtree(out, ignore_errors=True)
                    os.makedirs(out)
                    kw = dict(in2=files[1], out2=os.path.join(out, "o2" + sfx), threads=a.threads, out_codec=a.codec, codec_threads=a.threads // 2)
                    if human:
                        kw.update(human_out1=os.path.join(out, "h1" + sfx), human_out2=os.path.join(out, "h2" + sfx))
                    if K:
                        kw["taxon_outs"] = [(s, os.path.join(out, "t%d_1%s" % (i, sfx)), os.path.join(out, "t%d_2%s" % (i, sfx))) for i, s in enumerate(sel[K])]
                    st, dt, tr = timed(lambda: eng.run(files[0], os.path.join(out, "o1" + sfx), **kw))
                    r = {"wall_s": round(dt, 3), "classified": int(st.classified)}
                    m = HUMAN.findall(tr)
                    if m:
                        r["human_records"], r["human_bytes"], r["human_kernel_ms"] = int(m[0][0]), int(m[0][1]), float(m[0][3])
                    m = TAXON.findall(tr)
                    if m:
                        r["taxon_records"], r["taxon_bytes"], r["fetched_bytes"], r["taxon_kernel_ms"] = int(m[0][0]), int(m[0][1]), int(m[0][2]), float(m[0][3])
                        r["fragments"] = list(st.taxon_fragments)
                    res["legs"][name] = r
                    shutil.rmtree(out, ignore_errors=True)
        L = res["legs"]
        for K in (1, 4, 8):
            res["kernel_ratio_K%d" % K] = round(L["taxa%d" % K]["taxon_kernel_ms"] / L["split"]["human_kernel_ms"], 3)
        res["wall_ratio_split+4"] = round(L["split+4"]["wall_s"] / L["split"]["wall_s"], 3)
        print("TAXON_OUT " + json.dumps(res), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
