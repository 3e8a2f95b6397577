"""What --report-minimizer-data costs (nh_run_mdata; k_mdata_mark and k_mdata_count in nohuman_amd/csrc/nh_mdata.hip; DESIGN.md
section 6.13), on one GPU:
  mark     k_mdata_mark alone on one resident batch -- `--pairs` 150 bp pairs, a fraction --p of them pieces of the genome in the
           table, and `--ont-reads` ONT-like reads, every second one a piece of the genome -- by HIP events around --iters launches
           back to back after --warmup untimed ones (steady state: after the first launch every hit is a repeat, as in a host-heavy
           sample), next to the classify launch on the same batch; and on a cleared bitmap (every hit a first)
  ab       the same in a child process with NOHUMAN_MDATA_ATOMIC=always: no look at the bitmap's word before the atomic OR
  count    k_mdata_count on the sparse bitmap the batch left, on a full bitmap, and with no bitmap (all cells)
  e2e      a gzip -> gzip run of the pairs with and without the flag, interleaved, medians of --reps after one warm-up round
    python tools/mdata_bench.py [--pairs 1000000] [--ont-reads 20000] [--legs mark,ab,count,e2e] [--out profiles/minimizer_data.txt]
Prints one JSON line and appends it to --out."""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TRACE = re.compile(r"minimizer data: (\d+) hit groups on (\d+) distinct minimizers, k_mdata_mark ([0-9.]+) ms, k_mdata_count ([0-9.]+) ms")


def kernel_legs(a, eng, batch, paired, legs):
    import numpy as np
    import torch
    from qmask_bench import time_launches
    text, s, lens, _q, ntext = batch
    d_text = torch.from_numpy(text).cuda()
    d_s = torch.from_numpy(s.view(np.int64)).cuda()
    d_l = torch.from_numpy(lens.view(np.int32)).cuda()
    nseq = len(s)
    nfrag = nseq // (2 if paired else 1)
    nodes = int(eng.info.node_count)
    d_res = torch.zeros(nfrag * 4, dtype=torch.int32, device="cuda")
    d_marks = torch.zeros(eng.minimizer_marks_bytes() // 4, dtype=torch.int32, device="cuda")
    d_groups = torch.zeros(nodes, dtype=torch.int64, device="cuda")
    d_counts = torch.zeros(nodes, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    bases = int(lens.sum())
    long_reads = bases / nfrag > 2000

    def classify():
        eng.classify_records_device(d_text.data_ptr(), ntext, d_s.data_ptr(), d_l.data_ptr(), nfrag, paired, 0.0, d_res.data_ptr(),
                                    stream=stream, long_reads=long_reads)

    def mark():
        eng.minimizer_mark_device(d_text.data_ptr(), ntext, d_s.data_ptr(), d_l.data_ptr(), nfrag, d_marks.data_ptr(), d_groups.data_ptr(),
                                  paired=paired, stream=stream)

    def mark_cleared():
        d_marks.zero_()
        mark()

    def count(marks):
        eng.minimizer_count_device(marks, d_counts.data_ptr(), stream=stream)

    classify()
    torch.cuda.synchronize()
    res = d_res.cpu().numpy().reshape(-1, 4)
    r = {"fragments": nfrag, "bases": bases, "classified_fraction": round(float((res[:, 0] != 0).mean()), 4), "hit_groups": int(res[:, 3].sum())}
    if "mark" in legs:
        r["mark_ms"] = round(time_launches(torch, mark, a.warmup, a.iters), 4)
        assert int(d_groups.sum()) == r["hit_groups"] * (a.warmup + a.iters), "k_mdata_mark counted %d hit groups" % int(d_groups.sum())
        r["classify_ms"] = round(time_launches(torch, classify, a.warmup, a.iters), 4)
        r["mark_vs_classify"] = round(r["mark_ms"] / r["classify_ms"], 2)
        clear_ms = time_launches(torch, d_marks.zero_, a.warmup, a.iters)
        r["mark_first_hits_ms"] = round(time_launches(torch, mark_cleared, a.warmup, a.iters) - clear_ms, 4)
        mark()
    if "count" in legs:
        mark()
        torch.cuda.synchronize()
        d_counts.zero_()
        count(d_marks.data_ptr())
        torch.cuda.synchronize()
        r["distinct"] = int(d_counts.sum())
        r["bitmap_bytes"] = d_marks.numel() * 4
        r["count_sparse_ms"] = round(time_launches(torch, lambda: count(d_marks.data_ptr()), a.warmup, a.iters), 4)
        d_full = torch.full_like(d_marks, -1)
        r["count_full_ms"] = round(time_launches(torch, lambda: count(d_full.data_ptr()), a.warmup, a.iters), 4)
        r["count_all_cells_ms"] = round(time_launches(torch, lambda: count(0), a.warmup, a.iters), 4)
    return r


def ont_with_hits(rng, genome, n):
    """tools/qmask_bench.py's ONT-like batch, every second read a piece of the genome"""
    from qmask_bench import ont_batch
    text, s, lens, q, ntext = ont_batch(rng, n)
    for i in range(0, n, 2):
        ln = int(lens[i])
        if ln < genome.size:
            at = int(rng.integers(0, genome.size - ln))
            text[int(s[i]):int(s[i]) + ln] = genome[at:at + ln]
    return text, s, lens, q, ntext


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--ont-reads", type=int, default=20_000)
    ap.add_argument("--p", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default="mark,ab,count,e2e")
    ap.add_argument("--capacity", type=int, default=1 << 27)
    ap.add_argument("--load", type=float, default=0.5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    legs = a.legs.split(",")
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    import numpy as np
    from human_out_bench import make_db, make_member, timed
    from qmask_bench import pairs_batch
    from nohuman_amd import Engine, _lib
    base = "/dev/shm" if os.access("/dev/shm", os.W_OK) else None
    tmp = tempfile.mkdtemp(prefix="nh_mdata_", dir=base)
    try:
        rng = np.random.default_rng(5)
        genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=4_000_000)].copy()
        db = os.path.join(tmp, "db")
        make_db(db, a.capacity, a.load, genome)
        texts, _nh = make_member(rng, genome, a.pairs, a.p, 0)
        res = {"pairs": a.pairs, "p": a.p, "warmup": a.warmup, "iters": a.iters, "atomic": os.environ.get("NOHUMAN_MDATA_ATOMIC", "test-first")}
        with Engine.open(db) as eng:
            klegs = [x for x in legs if x in ("mark", "count")]
            if klegs:
                res["pairs_150"] = kernel_legs(a, eng, pairs_batch(texts, a.pairs), True, klegs)
                res["ont"] = kernel_legs(a, eng, ont_with_hits(rng, genome, a.ont_reads), False, klegs)
            if "e2e" in legs:
                L = _lib.lib()
                files = []
                for m, text in enumerate(texts):
                    pl = os.path.join(tmp, "in_%d.fq" % (m + 1))
                    open(pl, "wb").write(text)
                    assert L.nh_compress_file(pl.encode(), (pl + ".gz").encode(), 2, a.threads) == 0, L.nh_last_error()
                    os.remove(pl)
                    files.append(pl + ".gz")
                outs = [os.path.join(tmp, "o_%d.fq.gz" % (m + 1)) for m in range(2)]
                e2e = {}
                for rep in range(a.reps + 1):  # rep 0 warms the buffers and the page cache of the outputs
                    for leg in ("none", "mdata"):
                        extra = dict(minimizer_table=os.path.join(tmp, "m.tsv")) if leg == "mdata" else {}
                        kw = dict(in2=files[1], out2=outs[1], threads=a.threads, out_codec=2, codec_threads=a.threads // 2, **extra)
                        st, dt, tr = timed(lambda: eng.run(files[0], outs[0], **kw))
                        if rep == 0:
                            continue
                        r = e2e.setdefault(leg, {"wall_s": []})
                        r["wall_s"].append(round(dt, 3))
                        r["classified"] = st.classified
                        t = TRACE.findall(tr)
                        if t:
                            r["hit_groups"], r["distinct"] = int(t[0][0]), int(t[0][1])
                            r.setdefault("mark_kernel_ms", []).append(float(t[0][2]))
                            r.setdefault("count_kernel_ms", []).append(float(t[0][3]))
                for r in e2e.values():
                    r["median_s"] = statistics.median(r["wall_s"])
                    r["spread_s"] = round(max(r["wall_s"]) - min(r["wall_s"]), 3)
                res["mdata_vs_none"] = round(e2e["mdata"]["median_s"] / e2e["none"]["median_s"], 3)
                res["table"] = open(os.path.join(tmp, "m.tsv")).read()
                res["e2e"] = e2e
        if "ab" in legs:  # the knob is read once a process: a fresh child
            env = dict(os.environ, NOHUMAN_MDATA_ATOMIC="always")
            cmd = [sys.executable, os.path.abspath(__file__), "--legs", "mark", "--pairs", str(a.pairs), "--ont-reads", str(a.ont_reads),
                   "--p", str(a.p), "--warmup", str(a.warmup), "--iters", str(a.iters), "--capacity", str(a.capacity), "--load", str(a.load)]
            out = subprocess.run(cmd, env=env, capture_output=True, text=True)
            assert out.returncode == 0, out.stderr[-2000:]
            res["always_atomic"] = json.loads(out.stdout.split("MDATA ")[1])
        line = "MDATA " + json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
