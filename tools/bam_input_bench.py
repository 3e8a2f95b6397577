"""BAM input (nh_bam.hip, BamReader) on synthetic ONT-like reads (log-normal lengths, 36-character ids) and
150 bp reads (Illumina-like ids, binned qualities); a fifth of the records reverse-strand, one in fifty without qualities:
  kernel   k_bam_fastq alone on the whole file's records in HBM, per NOHUMAN_BAM_SPAN of --spans, in GB/s of FASTQ text written,
           beside a device-to-device copy of as many bytes timed the same way in the same process (the floor)
  e2e      files to files on one GPU: the BAM against the same reads as BGZF-compressed FASTQ read by the host reader
           (NOHUMAN_GZ_READER=host: both sides inflate on the host), gzip output encoded on the GPU; interleaved, the median of
           --reps after a warm-up, and where the wall time of the last repetition went (NOHUMAN_TRACE's stage lines); a third
           leg, the same FASTQ through the gzip reader on the GPU, is there to tell the BAM reader from the hand-over of batches
           born in HBM
  --paired the paired leg alone (profiles/bam_paired.txt): --pairs pairs of 150 bases as ONE collated BAM (every third
           pair stored mate 2 first) against the same reads as TWO BGZF FASTQ files through the host reader, files to files,
           two gzip outputs encoded on the GPU; interleaved, the median and the spread of --reps after a warm-up
    python tools/bam_input_bench.py [--ont-reads 20000] [--short-reads 1500000] [--spans 1024,2048,...] [--reps 3]
    python tools/bam_input_bench.py --paired [--pairs 750000] [--reps 3]
The database is the synthetic one of tools/human_out_bench.py; a tenth of the reads are pieces of its "human" genome."""
import argparse
import json
import os
import shutil
import statistics
import struct
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from human_out_bench import make_db, timed  # noqa: E402

ALPHABET = np.frombuffer(b"=ACMGRSVTWYHKDBN", np.uint8)
CODE = np.zeros(256, np.uint8)
CODE[ALPHABET] = np.arange(16, dtype=np.uint8)
COMP = np.zeros(256, np.uint8)
COMP[np.frombuffer(b"ACGTN", np.uint8)] = np.frombuffer(b"TGCAN", np.uint8)
ACGT = np.frombuffer(b"ACGT", np.uint8)
HEADER = b"BAM\1" + struct.pack("<i", 12) + b"@HD\tVN:1.6\n\0" + struct.pack("<i", 0)


def reads_block(rng, genome, n, L, p_human):
    """n reads of L bases: (letters (n, L), Phred values (n, L), reverse flags, absent-quality flags)"""
    seq = ACGT[rng.integers(0, 4, size=(n, L))]
    hi = np.nonzero(rng.random(n) < p_human)[0]
    starts = rng.integers(0, len(genome) - L, size=len(hi))
    seq[hi] = genome[starts[:, None] + np.arange(L)[None, :]]
    q = np.full((n, L), 37, np.uint8)
    r = rng.random((n, L), dtype=np.float32)
    q[r < 0.25] = 25
    q[r < 0.08] = 11
    q[r < 0.02] = 2
    return seq, q, rng.random(n) < 0.2, rng.random(n) < 0.02


def block_bytes(seq, q, rev, noq, names):
    """the block as BAM records and as the FASTQ they transcode to; names: (n, W) bytes.  -> (bam (n, R), fastq (n, T))"""
    n, L = seq.shape
    W = names.shape[1]
    stored = seq.copy()
    stored[rev] = COMP[seq[rev][:, ::-1]]
    sq = q.copy()
    sq[rev] = q[rev][:, ::-1]
    sq[noq] = 0xFF
    codes = CODE[stored]
    if L & 1:
        codes = np.concatenate([codes, np.zeros((n, 1), np.uint8)], axis=1)
    packed = (codes[:, 0::2] << 4) | codes[:, 1::2]
    body = 32 + W + 1 + packed.shape[1] + L
    fixed = np.frombuffer(struct.pack("<iiiBBHHHIiii", body, -1, -1, W + 1, 0, 4680, 0, 4, L, -1, -1, 0), np.uint8)
    bam = np.zeros((n, 4 + body), np.uint8)
    bam[:, :36] = fixed
    bam[rev, 4 + 14] = 0x14  # (flag: unmapped | reverse -- what a basecaller never writes, and what an aligner does)
    bam[:, 36:36 + W] = names
    o = 36 + W + 1
    bam[:, o:o + packed.shape[1]] = packed
    bam[:, o + packed.shape[1]:] = sq
    fq = np.empty((n, W + 2 * L + 6), np.uint8)
    fq[:, 0] = 64
    fq[:, 1:1 + W] = names
    fq[:, 1 + W] = 10
    fq[:, 2 + W:2 + W + L] = seq
    fq[:, 2 + W + L:5 + W + L] = np.frombuffer(b"\n+\n", np.uint8)
    fq[:, 5 + W + L:5 + W + 2 * L] = np.where(noq[:, None], 34, q + 33)
    fq[:, -1] = 10
    return bam, fq


def names_block(rng, first, n, ont):
    """ids: 36 hexadecimal characters and dashes (ONT), or an Illumina-like id with a running number"""
    if ont:
        hexd = np.frombuffer(b"0123456789abcdef", np.uint8)
        names = hexd[rng.integers(0, 16, size=(n, 36))]
        names[:, [8, 13, 18, 23]] = 45
        return names
    tmpl = b"SYN:1:HGF2YDSXX:1:1101:000000000"
    names = np.tile(np.frombuffer(tmpl, np.uint8), (n, 1))
    idx = np.arange(first, first + n, dtype=np.int64)
    for d in range(9):
        names[:, len(tmpl) - 1 - d] = 48 + (idx // 10 ** d) % 10
    return names


def make_files(rng, genome, tmp, tag, lengths, lib, threads):
    """the reads (groups of one length each) as tag.bam and tag.fq.gz (BGZF); -> paths, counts, the inflated BAM stream, table"""
    bam_parts, fq_parts, table, first = [HEADER], [], [], 0
    bam_at, fq_at = len(HEADER), 0
    for L, n in lengths:
        seq, q, rev, noq = reads_block(rng, genome, n, L, 0.1)
        bam, fq = block_bytes(seq, q, rev, noq, names_block(rng, first, n, tag == "ont"))
        first += n
        t = np.empty((n, 2), np.uint64)
        t[:, 0] = bam_at + np.arange(n, dtype=np.uint64) * np.uint64(bam.shape[1])
        t[:, 1] = fq_at + np.arange(n, dtype=np.uint64) * np.uint64(fq.shape[1])
        table.append(t)
        bam_at += bam.size
        fq_at += fq.size
        bam_parts.append(bam.tobytes())
        fq_parts.append(fq.tobytes())
    stream, text = b"".join(bam_parts), b"".join(fq_parts)
    paths = {}
    for name, data in (("bam", stream), ("fq.gz", text)):
        plain = os.path.join(tmp, tag + ".plain")
        open(plain, "wb").write(data)
        paths[name] = os.path.join(tmp, tag + "." + name)
        assert lib.nh_compress_file(plain.encode(), paths[name].encode(), 5, threads) == 0, lib.nh_last_error()
        os.remove(plain)
    return paths, stream, len(text), np.concatenate(table), sum(L * n for L, n in lengths)


def paired_blocks(rng, genome, n, tags=None):
    """n pairs of 150 bases with one name a pair -> (the records (n, 2, R) in file order: every third pair mate 2 first, the
    two mates' FASTQ (n, T) each); tags: (n, W) bytes appended to every record"""
    names = names_block(rng, 0, n, False)
    bams, fqs = [], []
    for m in (0, 1):
        seq, q, rev, noq = reads_block(rng, genome, n, 150, 0.1)
        bam, fq = block_bytes(seq, q, rev, noq, names)
        bam[:, 4 + 14] = np.where(rev, 0x10, 0) | (0x4D if m == 0 else 0x8D)  # (paired, unmapped, mate unmapped, first / second)
        if tags is not None:
            bam = np.concatenate([bam, tags], axis=1)
            bam[:, :4] = np.frombuffer(struct.pack("<i", bam.shape[1] - 4), np.uint8)
        bams.append(bam)
        fqs.append(fq)
    pair = np.stack(bams, axis=1)
    swap = np.arange(n) % 3 == 2
    pair[swap] = pair[swap][:, ::-1]
    return pair, fqs


def compress(lib, tmp, name, data, threads):
    plain, path = os.path.join(tmp, name + ".plain"), os.path.join(tmp, name)
    open(plain, "wb").write(data)
    assert lib.nh_compress_file(plain.encode(), path.encode(), 5, threads) == 0, lib.nh_last_error()
    os.remove(plain)
    return path


def paired_e2e(eng, rng, genome, tmp, n, lib, threads, reps):
    pair, fqs = paired_blocks(rng, genome, n)
    paths = {"bam": compress(lib, tmp, "pe.bam", HEADER + pair.tobytes(), threads),
             "fq1": compress(lib, tmp, "pe_1.fq.gz", fqs[0].tobytes(), threads), "fq2": compress(lib, tmp, "pe_2.fq.gz", fqs[1].tobytes(), threads)}
    del pair, fqs
    o1, o2 = os.path.join(tmp, "out_1.fq.gz"), os.path.join(tmp, "out_2.fq.gz")
    legs = {"paired_bam": dict(in1=paths["bam"]), "two_bgzf_fastq_host_reader": dict(in1=paths["fq1"], in2=paths["fq2"])}
    res = {k: {"wall_s": []} for k in legs}
    os.environ["NOHUMAN_GZ_READER"] = "host"
    try:
        for r in range(reps + 1):  # rep 0 warms the buffers and the page cache
            for leg, ins in legs.items():
                for o in (o1, o2):
                    if os.path.exists(o):
                        os.remove(o)
                st, dt, tr = timed(lambda: eng.run(out1=o1, out2=o2, threads=threads, out_codec=2, codec_threads=threads // 2, **ins))
                if r == 0:
                    continue
                x = res[leg]
                x["wall_s"].append(round(dt, 3))
                x["pairs"], x["classified"], x["out_bytes"] = st.total_sequences, st.classified, [os.path.getsize(o1), os.path.getsize(o2)]
                x["trace"] = [t.split("] ", 1)[-1] for t in tr.splitlines() if "wall " in t or "BAM reader" in t]
    finally:
        os.environ.pop("NOHUMAN_GZ_READER", None)
    for x in res.values():
        x["median_s"] = statistics.median(x["wall_s"])
        x["spread_s"] = round(max(x["wall_s"]) - min(x["wall_s"]), 3)
    assert len({(x["pairs"], x["classified"], tuple(x["out_bytes"])) for x in res.values()}) == 1, res
    res["bam_over_fastq"] = round(res["paired_bam"]["median_s"] / res["two_bgzf_fastq_host_reader"]["median_s"], 3)
    res["file_bytes"] = {k: os.path.getsize(v) for k, v in paths.items()}
    return res


def kernel_bench(eng, stream, table, text_len, spans, rounds=20):
    import torch
    raw = np.zeros((len(stream) + 3) // 4 * 4 + 8, np.uint8)
    raw[:len(stream)] = np.frombuffer(stream, np.uint8)
    d_bam = torch.from_numpy(raw).cuda()
    d_tab = torch.from_numpy(table.view(np.int64).copy()).cuda()
    d_text = torch.zeros(text_len + 8, dtype=torch.uint8, device="cuda")
    d_copy = torch.zeros(text_len + 8, dtype=torch.uint8, device="cuda")
    d_err = torch.zeros(1, dtype=torch.int32, device="cuda")

    def rate(fn):
        fn()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(rounds):
            fn()
        torch.cuda.synchronize()
        return text_len * rounds / (time.perf_counter() - t) / 1e9

    out = {"text_bytes": text_len, "bam_bytes": len(stream), "records": len(table), "memcpy_d2d_gbs": round(rate(lambda: d_copy.copy_(d_text)), 1)}
    for span in spans:
        os.environ["NOHUMAN_BAM_SPAN"] = str(span)
        out["span_%d_gbs" % span] = round(rate(lambda: eng.bam_to_fastq_device(d_bam.data_ptr(), len(stream), d_tab.data_ptr(), len(table),
                                                                               d_text.data_ptr(), text_len, text_len, d_err.data_ptr())), 1)
    os.environ.pop("NOHUMAN_BAM_SPAN", None)
    assert int(d_err.cpu()[0]) == 0
    out["memcpy_d2d_gbs_after"] = round(rate(lambda: d_copy.copy_(d_text)), 1)
    return out


def e2e_bench(eng, paths, tmp, threads, reps):
    out = os.path.join(tmp, "out.fq.gz")
    # (the third leg is not part of the comparison: the same FASTQ through the gzip reader on the GPU, whose batches are born in
    # HBM like the BAM reader's -- it shows what of a difference is the hand-over of such batches and what the BAM reader itself)
    legs = {"bam": ("bam", "host"), "fq.gz": ("fq.gz", "host"), "fq.gz_gpu_reader": ("fq.gz", "device")}
    res = {k: {"wall_s": []} for k in legs}
    try:
        for rep in range(reps + 1):  # rep 0 warms the buffers and the page cache
            for leg, (src, reader) in legs.items():
                if os.path.exists(out):
                    os.remove(out)
                os.environ["NOHUMAN_GZ_READER"] = reader
                st, dt, tr = timed(lambda: eng.run(paths[src], out, threads=threads, out_codec=2, codec_threads=threads // 2))
                if rep == 0:
                    continue
                r = res[leg]
                r["wall_s"].append(round(dt, 3))
                r["reads"], r["classified"], r["out_bytes"] = st.total_sequences, st.classified, os.path.getsize(out)
                r["trace"] = [x.split("] ", 1)[-1] for x in tr.splitlines() if "wall " in x or "BAM reader" in x]
    finally:
        os.environ.pop("NOHUMAN_GZ_READER", None)
    for r in res.values():
        r["median_s"] = statistics.median(r["wall_s"])
        r["spread_s"] = round(max(r["wall_s"]) - min(r["wall_s"]), 3)
    assert len({(r["reads"], r["classified"]) for r in res.values()}) == 1
    res["bam_over_fastq"] = round(res["bam"]["median_s"] / res["fq.gz"]["median_s"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ont-reads", type=int, default=20000)
    ap.add_argument("--short-reads", type=int, default=1_500_000)
    ap.add_argument("--spans", default="1024,2048,4096,8192,16384,32768,65536")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--capacity", type=int, default=1 << 25)
    ap.add_argument("--paired", action="store_true")
    ap.add_argument("--pairs", type=int, default=750_000)
    a = ap.parse_args()
    from nohuman_amd import Engine, _lib
    base = "/dev/shm" if os.access("/dev/shm", os.W_OK) else None
    tmp = tempfile.mkdtemp(prefix="nh_bam_in_", dir=base)
    try:
        rng = np.random.default_rng(5)
        genome = ACGT[rng.integers(0, 4, size=4_000_000)].copy()
        db = os.path.join(tmp, "db")
        make_db(db, a.capacity, 0.5, genome)
        # ONT-like: log-normal lengths (median 6 kb, a tail to 150 kb), in 64 groups of one length each
        lens = np.clip(rng.lognormal(np.log(6000), 0.9, 64), 300, 150_000).astype(int)
        sets = {"ont": [(int(L), max(1, a.ont_reads // 64)) for L in lens], "short": [(150, a.short_reads)]}
        if a.paired:
            with Engine.open(db) as eng:
                res = {"reads": "150-base pairs", "pairs": a.pairs, "e2e": paired_e2e(eng, rng, genome, tmp, a.pairs, _lib.lib(), a.threads, a.reps)}
            print("BAM_PAIRED_INPUT " + json.dumps(res), flush=True)
            return
        with Engine.open(db) as eng:
            for tag, lengths in sets.items():
                paths, stream, text_len, table, bases = make_files(rng, genome, tmp, tag, lengths, _lib.lib(), a.threads)
                res = {"reads": tag, "records": len(table), "bases": bases, "bam_file_bytes": os.path.getsize(paths["bam"]),
                       "fastq_gz_file_bytes": os.path.getsize(paths["fq.gz"])}
                res["kernel"] = kernel_bench(eng, stream, table, text_len, [int(x) for x in a.spans.split(",")])
                del stream
                res["e2e"] = e2e_bench(eng, paths, tmp, a.threads, a.reps)
                print("BAM_INPUT " + json.dumps(res), flush=True)
                for p in paths.values():
                    os.remove(p)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
