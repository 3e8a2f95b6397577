"""BAM output (nh_bamout.hip, NH_CODEC_BAM) on the two synthetic sets of tools/bam_input_bench.py -- ONT-like
reads (log-normal lengths, 36-character ids), here with tag payloads of a basecaller's size (mv: 1.7 bytes a base of 0 / 1, MM /
ML: a modification call every eighth base, a dozen short tags), and 150 bp reads with an RG tag; a tenth of the reads host:
  kernel   the builder's three launches alone (nh_bam_select_device, which also allocates its scratch and waits for the stream)
           on the whole file's records in HBM, the non-host records selected, per NOHUMAN_BAM_SPAN of --spans, in GB/s of
           record bytes written, beside a device-to-device copy of as many bytes timed the same way in the same process
  e2e      files to files on one GPU: BAM -> BAM with this library against BAM -> BGZF FASTQ of the same reads with the library
           of --parent-lib (a build of the parent commit; without one: this library, and the result says so); a leg is a child
           process that runs a warm-up and --reps runs; the medians, their ratio and the output sizes
  --paired the paired legs alone (profiles/bam_paired.txt) on --pairs pairs of 150 bases with an RG tag, as one collated
           BAM: the builder on pairs (nh_bam_select_pairs_device) beside the single-end builder on the same records in the same
           order (every record with its pair's call), at the default span; a paired BAM -> BAM run against the same file -> two
           BGZF FASTQ files, interleaved in one process, the median and the spread of --reps after a warm-up; and, with
           --parent-lib, the single-end legs (150-base records -> BGZF FASTQ, -> BAM) with this build and with the parent's,
           twice each in turn, with both spreads
    python tools/bam_output_bench.py [--ont-reads 20000] [--short-reads 1500000] [--spans 4096,16384,65536] [--reps 3] [--parent-lib PATH]
    python tools/bam_output_bench.py --paired [--pairs 750000] [--short-reads 1500000] [--reps 3] [--parent-lib PATH]
The database is the synthetic one of tools/human_out_bench.py."""
import argparse
import json
import os
import shutil
import statistics
import struct
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402

from bam_input_bench import ACGT, HEADER, block_bytes, compress, names_block, paired_blocks, reads_block  # noqa: E402


def tag_block(rng, n, L, ont):
    """(n, T) bytes of tags, the same layout for every record of the group"""
    if not ont:
        return np.tile(np.frombuffer(b"RGZlane1\0", np.uint8), (n, 1))
    mv_n, ml_n = int(1.7 * L), max(1, L // 8)
    mm = (b"C+m?," + b",".join(b"%d" % (j % 11) for j in range(ml_n)) + b";\0")
    parts = [np.tile(np.frombuffer(b"qsf\0\0\x90\x41duf\0\0\x20\x41nsi\x10\x27\0\0tsi\x0a\0\0\0chi\x21\0\0\0rni\x05\0\0\0RGZrun_sup@v5.0.0\0"
                                   b"stZ2026-01-01T00:00:00.000+00:00\0mvBc" + struct.pack("<I", mv_n), np.uint8), (n, 1)),
             (rng.random((n, mv_n), dtype=np.float32) < 0.55).astype(np.uint8),
             np.tile(np.frombuffer(b"MMZ" + mm + b"MLBC" + struct.pack("<I", ml_n), np.uint8), (n, 1)),
             rng.integers(0, 256, size=(n, ml_n), dtype=np.uint8)]
    return np.concatenate(parts, axis=1)


def make_bam(rng, genome, tmp, tag, lengths, lib, threads):
    """the reads (groups of one length each) as tag.bam -> (path, the inflated stream, the table of its records, bases)"""
    parts, table, first, at = [HEADER], [], 0, len(HEADER)
    for L, n in lengths:
        seq, q, rev, noq = reads_block(rng, genome, n, L, 0.1)
        bam, _ = block_bytes(seq, q, rev, noq, names_block(rng, first, n, tag == "ont"))
        bam = np.concatenate([bam, tag_block(rng, n, L, tag == "ont")], axis=1)
        bam[:, :4] = np.frombuffer(struct.pack("<i", bam.shape[1] - 4), np.uint8)
        first += n
        t = np.zeros((n, 2), np.uint64)
        t[:, 0] = at + np.arange(n, dtype=np.uint64) * np.uint64(bam.shape[1])
        table.append(t)
        at += bam.size
        parts.append(bam.tobytes())
    stream = b"".join(parts)
    plain, path = os.path.join(tmp, tag + ".plain"), os.path.join(tmp, tag + ".bam")
    open(plain, "wb").write(stream)
    assert lib.nh_compress_file(plain.encode(), path.encode(), 5, threads) == 0, lib.nh_last_error()
    os.remove(plain)
    return path, stream, np.concatenate(table), sum(L * n for L, n in lengths)


def kernel_bench(eng, stream, table, spans, rounds=20):
    import torch
    rng = np.random.default_rng(9)
    raw = np.zeros((len(stream) + 3) // 4 * 4 + 8, np.uint8)
    raw[:len(stream)] = np.frombuffer(stream, np.uint8)
    d_bam = torch.from_numpy(raw).cuda()
    d_tab = torch.from_numpy(table.view(np.int64).copy()).cuda()
    res = np.zeros((len(table), 4), np.uint32)
    res[:, 0] = (rng.random(len(table)) < 0.1) * 30
    d_res = torch.from_numpy(res.view(np.int32).copy()).cuda()
    sizes = np.frombuffer(stream, np.uint8)[table[:, 0].astype(np.int64)[:, None] + np.arange(4)[None, :]].copy().view("<i4")[:, 0] + 4
    total = int(sizes[res[:, 0] == 0].sum())
    d_out = torch.zeros(len(stream) + 64, dtype=torch.uint8, device="cuda")
    d_copy = torch.zeros(total + 8, dtype=torch.uint8, device="cuda")
    d_tot = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_err = torch.zeros(1, dtype=torch.int32, device="cuda")

    def rate(fn):
        fn()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(rounds):
            fn()
        torch.cuda.synchronize()
        return total * rounds / (time.perf_counter() - t) / 1e9

    out = {"selected_bytes": total, "bam_bytes": len(stream), "records": len(table), "mean_record_bytes": round(float(sizes.mean()), 1),
           "memcpy_d2d_gbs": round(rate(lambda: d_copy.copy_(d_out[:total + 8])), 1)}
    for span in spans:
        os.environ["NOHUMAN_BAM_SPAN"] = str(span)
        out["span_%d_gbs" % span] = round(rate(lambda: eng.bam_select_device(d_bam.data_ptr(), len(stream), d_tab.data_ptr(), len(table), d_res.data_ptr(), 0,
                                                                             d_out.data_ptr(), len(stream) + 64, d_tot.data_ptr(), d_err.data_ptr())), 1)
        assert int(d_tot.cpu()[0]) == total and int(d_err.cpu()[0]) == 0
    os.environ.pop("NOHUMAN_BAM_SPAN", None)
    out["memcpy_d2d_gbs_after"] = round(rate(lambda: d_copy.copy_(d_out[:total + 8])), 1)
    return out


def paired_kernel_bench(eng, stream, n, rec_bytes, rounds=20):
    """the builder on the n pairs of the stream (records of rec_bytes each, two a pair) and the single-end builder on the same 2n records"""
    import torch
    rng = np.random.default_rng(9)
    raw = np.zeros((len(stream) + 3) // 4 * 4 + 8, np.uint8)
    raw[:len(stream)] = np.frombuffer(stream, np.uint8)
    d_bam = torch.from_numpy(raw).cuda()
    offs = len(HEADER) + np.arange(2 * n, dtype=np.uint64) * np.uint64(rec_bytes)
    single = np.zeros((2 * n, 2), np.uint64)
    single[:, 0] = offs
    d_pair_tab = torch.from_numpy(offs.view(np.int64).copy()).cuda()  # (two words a pair: its records in file order)
    d_single_tab = torch.from_numpy(single.view(np.int64).copy()).cuda()
    host = rng.random(n) < 0.1
    res_p, res_s = np.zeros((n, 4), np.uint32), np.zeros((2 * n, 4), np.uint32)
    res_p[:, 0] = host * 30
    res_s[:, 0] = np.repeat(host, 2) * 30
    d_res_p, d_res_s = torch.from_numpy(res_p.view(np.int32).copy()).cuda(), torch.from_numpy(res_s.view(np.int32).copy()).cuda()
    total = int((~host).sum()) * 2 * rec_bytes
    d_out = torch.zeros(len(stream) + 64, dtype=torch.uint8, device="cuda")
    d_copy = torch.zeros(total + 8, dtype=torch.uint8, device="cuda")
    d_tot = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_err = torch.zeros(1, dtype=torch.int32, device="cuda")

    def rate(fn):
        fn()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(rounds):
            fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t) / rounds
        return {"ms": round(dt * 1e3, 3), "gbs": round(total / dt / 1e9, 1)}

    out = {"pairs": n, "record_bytes": rec_bytes, "selected_bytes": total, "memcpy_d2d": rate(lambda: d_copy.copy_(d_out[:total + 8]))}
    outs = {}
    for name, fn in (("pairs", lambda: eng.bam_select_pairs_device(d_bam.data_ptr(), len(stream), d_pair_tab.data_ptr(), n, d_res_p.data_ptr(), 0,
                                                                   d_out.data_ptr(), len(stream) + 64, d_tot.data_ptr(), d_err.data_ptr())),
                     ("single_end_same_records", lambda: eng.bam_select_device(d_bam.data_ptr(), len(stream), d_single_tab.data_ptr(), 2 * n, d_res_s.data_ptr(), 0,
                                                                               d_out.data_ptr(), len(stream) + 64, d_tot.data_ptr(), d_err.data_ptr())),
                     ("pairs_again", None), ("single_end_same_records_again", None)):
        fn = fn or outs[name[:-6]][1]
        out["builder_" + name] = rate(fn)
        assert int(d_tot.cpu()[0]) == total and int(d_err.cpu()[0]) == 0
        outs[name] = (d_out[:total].cpu().numpy().tobytes(), fn)
    assert outs["pairs"][0] == outs["single_end_same_records"][0]  # (the same bytes: both records of a pair, in file order)
    return out


def paired_e2e(eng, bam, tmp, threads, reps):
    """a paired BAM -> BAM against the same file -> two BGZF FASTQ files, interleaved"""
    from human_out_bench import timed
    o1, o2 = os.path.join(tmp, "pe_out_1"), os.path.join(tmp, "pe_out_2")
    legs = {"paired_bam_to_bam": dict(out_codec=6), "paired_bam_to_two_bgzf_fastq": dict(out_codec=5, out2=o2)}
    res = {k: {"wall_s": []} for k in legs}
    for r in range(reps + 1):  # rep 0 warms the buffers and the page cache
        for leg, kw in legs.items():
            for o in (o1, o2):
                if os.path.exists(o):
                    os.remove(o)
            st, dt, tr = timed(lambda: eng.run(bam, o1, threads=threads, codec_threads=threads // 2, **kw))
            if r == 0:
                continue
            x = res[leg]
            x["wall_s"].append(round(dt, 3))
            x["pairs"], x["classified"], x["out_bytes"] = st.total_sequences, st.classified, sum(os.path.getsize(o) for o in (o1, o2) if os.path.exists(o))
            x["trace"] = [t.split("] ", 1)[-1] for t in tr.splitlines() if "wall " in t or "bam-out" in t]
    for x in res.values():
        x["median_s"] = statistics.median(x["wall_s"])
        x["spread_s"] = round(max(x["wall_s"]) - min(x["wall_s"]), 3)
    assert len({(x["pairs"], x["classified"]) for x in res.values()}) == 1, res
    res["bam_over_fastq"] = round(res["paired_bam_to_bam"]["median_s"] / res["paired_bam_to_two_bgzf_fastq"]["median_s"], 3)
    return res


def single_end_against_parent(a, tmp, db, bam):
    """the single-end legs with this build and the parent's, twice each in turn: every run's wall time, the medians, the spreads"""
    res = {}
    for turn in range(2):
        for codec, what in ((5, "bam_to_bgzf_fastq"), (6, "bam_to_bam")):
            for lib, who in ((None, "this_build"), (a.parent_lib, "parent")):
                env = dict(os.environ)
                if lib:
                    env["NOHUMAN_ENGINE_LIB"] = os.path.abspath(lib)
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", str(codec), "--tmp", tmp, "--db", db, "--bam", bam, "--reps", str(a.reps),
                                      "--threads", str(a.threads)], env=env, capture_output=True, text=True, timeout=1500)
                assert out.returncode == 0, out.stderr[-3000:]
                leg = json.loads(out.stdout.split("LEG ")[1])
                r = res.setdefault(what, {}).setdefault(who, {"wall_s": []})
                r["wall_s"] += leg["wall_s"]
                r["reads"], r["classified"], r["out_bytes"] = leg["reads"], leg["classified"], leg["out_bytes"]
    for what in res.values():
        for r in what.values():
            r["median_s"] = statistics.median(r["wall_s"])
            r["spread_s"] = round(max(r["wall_s"]) - min(r["wall_s"]), 3)
            r["min_s"], r["max_s"] = min(r["wall_s"]), max(r["wall_s"])
        what["this_over_parent"] = round(what["this_build"]["median_s"] / what["parent"]["median_s"], 3)
        what["inside_parent_spread"] = what["parent"]["min_s"] <= what["this_build"]["median_s"] <= what["parent"]["max_s"]
        assert (what["this_build"]["reads"], what["this_build"]["classified"], what["this_build"]["out_bytes"]) == \
            (what["parent"]["reads"], what["parent"]["classified"], what["parent"]["out_bytes"])
    return res


def paired_main(a, tmp, db, rng, genome, lib):
    from nohuman_amd import Engine
    n = a.pairs
    pair, _ = paired_blocks(rng, genome, n, tags=np.tile(np.frombuffer(b"RGZlane1\0", np.uint8), (n, 1)))
    stream = HEADER + pair.tobytes()
    rec_bytes = pair.shape[2]
    del pair
    bam = compress(lib, tmp, "pe.bam", stream, a.threads)
    res = {"reads": "150-base pairs, RG tag", "pairs": n, "bam_file_bytes": os.path.getsize(bam), "bam_stream_bytes": len(stream)}
    with Engine.open(db) as eng:
        res["kernel"] = paired_kernel_bench(eng, stream, n, rec_bytes)
        del stream
        res["e2e"] = paired_e2e(eng, bam, tmp, a.threads, a.reps)
    print("BAM_PAIRED_OUTPUT " + json.dumps(res), flush=True)
    os.remove(bam)
    if a.parent_lib:
        path, stream, table, _ = make_bam(rng, genome, tmp, "short", [(150, a.short_reads)], lib, a.threads)
        del stream, table
        print("BAM_SINGLE_END_AGAINST_PARENT " + json.dumps({"records": a.short_reads, "parent_lib": a.parent_lib,
                                                              "legs": single_end_against_parent(a, tmp, db, path)}), flush=True)


def leg_main(a):
    """a child process: one leg of the files-to-files comparison with the library NOHUMAN_ENGINE_LIB names"""
    import ctypes
    from human_out_bench import timed
    from nohuman_amd import Engine, _lib
    if os.environ.get("NOHUMAN_ENGINE_LIB"):  # (an older build: the binding asks only for the symbols that build has)
        _lib._preload_hip_runtime()
        old = ctypes.CDLL(_lib.LIB_PATH)
        for name in [s for s in _lib.SYMBOLS if not hasattr(old, s)]:
            del _lib.SYMBOLS[name]
    out = os.path.join(a.tmp, "leg_out")
    res = {"wall_s": []}
    with Engine.open(a.db) as eng:
        for rep in range(a.reps + 1):  # rep 0 warms the buffers and the page cache
            if os.path.exists(out):
                os.remove(out)
            st, dt, tr = timed(lambda: eng.run(a.bam, out, threads=a.threads, out_codec=a.leg, codec_threads=a.threads // 2))
            if rep:
                res["wall_s"].append(round(dt, 3))
        res["reads"], res["classified"], res["out_bytes"] = st.total_sequences, st.classified, os.path.getsize(out)
        res["trace"] = [x.split("] ", 1)[-1] for x in tr.splitlines() if "wall " in x or "bam-out" in x]
    os.remove(out)
    res["median_s"] = statistics.median(res["wall_s"])
    res["spread_s"] = round(max(res["wall_s"]) - min(res["wall_s"]), 3)
    print("LEG " + json.dumps(res), flush=True)


def e2e_bench(a, tmp, db, bam):
    res = {}
    for name, codec, lib in (("bam_to_bam", 6, None), ("bam_to_bgzf_fastq_parent", 5, a.parent_lib)):
        env = dict(os.environ)
        if lib:
            env["NOHUMAN_ENGINE_LIB"] = os.path.abspath(lib)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", str(codec), "--tmp", tmp, "--db", db, "--bam", bam, "--reps", str(a.reps),
                              "--threads", str(a.threads)], env=env, capture_output=True, text=True, timeout=1500)
        assert out.returncode == 0, out.stderr[-3000:]
        res[name] = json.loads(out.stdout.split("LEG ")[1])
        res[name]["library"] = lib or "this build"
    assert (res["bam_to_bam"]["reads"], res["bam_to_bam"]["classified"]) == (res["bam_to_bgzf_fastq_parent"]["reads"], res["bam_to_bgzf_fastq_parent"]["classified"])
    res["bam_over_fastq"] = round(res["bam_to_bam"]["median_s"] / res["bam_to_bgzf_fastq_parent"]["median_s"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ont-reads", type=int, default=20000)
    ap.add_argument("--short-reads", type=int, default=1_500_000)
    ap.add_argument("--spans", default="4096,16384,65536")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--capacity", type=int, default=1 << 25)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--leg", type=int, default=None)  # (a child of e2e_bench: the codec of its runs)
    ap.add_argument("--tmp")
    ap.add_argument("--db")
    ap.add_argument("--bam")
    ap.add_argument("--paired", action="store_true")
    ap.add_argument("--pairs", type=int, default=750_000)
    a = ap.parse_args()
    if a.leg is not None:
        return leg_main(a)
    from human_out_bench import make_db
    from nohuman_amd import Engine, _lib
    base = "/dev/shm" if os.access("/dev/shm", os.W_OK) else None
    tmp = tempfile.mkdtemp(prefix="nh_bam_out_", dir=base)
    try:
        rng = np.random.default_rng(5)
        genome = ACGT[rng.integers(0, 4, size=4_000_000)].copy()
        db = os.path.join(tmp, "db")
        make_db(db, a.capacity, 0.5, genome)
        if a.paired:
            return paired_main(a, tmp, db, rng, genome, _lib.lib())
        lens = np.clip(rng.lognormal(np.log(6000), 0.9, 64), 300, 150_000).astype(int)
        sets = {"ont": [(int(L), max(1, a.ont_reads // 64)) for L in lens], "short": [(150, a.short_reads)]}
        for tag, lengths in sets.items():
            path, stream, table, bases = make_bam(rng, genome, tmp, tag, lengths, _lib.lib(), a.threads)
            res = {"reads": tag, "records": len(table), "bases": bases, "bam_file_bytes": os.path.getsize(path), "bam_stream_bytes": len(stream)}
            with Engine.open(db) as eng:
                res["kernel"] = kernel_bench(eng, stream, table, [int(x) for x in a.spans.split(",")])
            del stream
            res["e2e"] = e2e_bench(a, tmp, db, path)
            print("BAM_OUTPUT " + json.dumps(res), flush=True)
            os.remove(path)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
