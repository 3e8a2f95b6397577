"""What --read-stats costs (nh_run_rstats, k_rstats in nohuman_amd/csrc/nh_rstats.hip), on one GPU:
  kernel   k_rstats alone on one resident batch -- `--pairs` 150 bp pairs and `--ont-reads` ONT-like reads, the batches of
           tools/qmask_bench.py -- with the calls the classifier gave that batch, by HIP events around --iters launches back to
           back after --warmup launches that are not timed (steady state); GB/s counts sequence + qualities read; the same with
           the grid capped at --caps workgroups
  qmask    k_qmask (Q 20) on the same batch, timed the same way: it also reads about 2 bytes per base (and writes one)
  classify the classify launch (nh_classify_records_device) on the same batch: the kernel k_rstats stands behind
  e2e      a gzip -> gzip run of the pairs with and without the option, interleaved, medians of --reps after one warm-up round
    python tools/rstats_bench.py [--pairs 1000000] [--ont-reads 20000] [--legs kernel,qmask,classify,e2e] [--out profiles/rstats.txt]
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
TRACE = re.compile(r"rstats: (\d+) bases, kernel ([0-9.]+) ms")


def kernel_legs(a, eng, batch, paired, legs):
    import numpy as np
    import torch
    from qmask_bench import time_launches
    text, s, lens, q, ntext = batch
    d_text = torch.from_numpy(text).cuda()
    d_out = torch.empty_like(d_text)
    d_s = torch.from_numpy(s.view(np.int64)).cuda()
    d_l = torch.from_numpy(lens.view(np.int32)).cuda()
    d_q = torch.from_numpy(q.view(np.int64)).cuda()
    nseq = len(s)
    nfrag = nseq // (2 if paired else 1)
    d_res = torch.zeros(nfrag * 4, dtype=torch.int32, device="cuda")
    acc = np.zeros((4, 102), dtype=np.uint64)
    acc[:, 2] = 2 ** 64 - 1
    d_acc = torch.from_numpy(acc.view(np.int64)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    bases = int(lens.sum())
    long_reads = bases / nfrag > 2000

    def classify():
        eng.classify_records_device(d_text.data_ptr(), ntext, d_s.data_ptr(), d_l.data_ptr(), nfrag, paired, 0.0, d_res.data_ptr(),
                                    stream=stream, long_reads=long_reads)

    def rstats(cap=0):
        eng.read_stats_device(d_text.data_ptr(), ntext, d_s.data_ptr(), d_l.data_ptr(), d_q.data_ptr(), d_res.data_ptr(), nfrag,
                              d_acc.data_ptr(), paired=paired, max_workgroups=cap, stream=stream)

    classify()  # the calls k_rstats sorts the reads by
    torch.cuda.synchronize()
    r = {"sequences": nseq, "bases": bases, "text_bytes": ntext,
         "human_fraction": round(float((d_res.cpu().numpy().reshape(-1, 4)[:, 0] != 0).mean()), 4)}
    if "kernel" in legs:
        ms = time_launches(torch, rstats, a.warmup, a.iters)
        r["rstats_ms"] = round(ms, 4)
        r["rstats_gb_s"] = round(2 * bases / ms / 1e6, 1)
        got = d_acc.cpu().numpy().view(np.uint64).reshape(4, 102)
        assert int(got[:, 1].sum()) == bases * (a.warmup + a.iters), "k_rstats counted %d bases" % int(got[:, 1].sum())
        r["rstats_ms_by_cap"] = {str(c): round(time_launches(torch, lambda: rstats(c), a.warmup, a.iters), 4) for c in a.caps}
    if "qmask" in legs:
        ms = time_launches(torch, lambda: eng.quality_mask_device(d_text.data_ptr(), ntext, d_s.data_ptr(), d_l.data_ptr(), d_q.data_ptr(), nseq,
                                                                  20, d_out.data_ptr(), 0, stream), a.warmup, a.iters)
        r["qmask_ms"] = round(ms, 4)
        if "rstats_ms" in r:
            r["rstats_vs_qmask"] = round(r["rstats_ms"] / ms, 2)
    if "classify" in legs:
        r["classify_ms"] = round(time_launches(torch, classify, a.warmup, a.iters), 4)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--ont-reads", type=int, default=20_000)
    ap.add_argument("--p", type=float, default=0.05)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--caps", type=lambda v: [int(x) for x in v.split(",")], default=[256, 768, 1280, 2560, 4096])
    ap.add_argument("--legs", default="kernel,qmask,classify,e2e")
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
    from qmask_bench import ont_batch, pairs_batch
    from nohuman_amd import Engine, ReadStats, _lib
    base = "/dev/shm" if os.access("/dev/shm", os.W_OK) else None
    tmp = tempfile.mkdtemp(prefix="nh_rstats_", dir=base)
    try:
        rng = np.random.default_rng(5)
        genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=4_000_000)].copy()
        db = os.path.join(tmp, "db")
        make_db(db, a.capacity, a.load, genome)
        texts, _nh = make_member(rng, genome, a.pairs, a.p, 0)
        res = {"pairs": a.pairs, "warmup": a.warmup, "iters": a.iters}
        with Engine.open(db) as eng:
            klegs = [x for x in legs if x in ("kernel", "qmask", "classify")]
            if klegs:
                res["pairs_150"] = kernel_legs(a, eng, pairs_batch(texts, a.pairs), True, klegs)
                res["ont"] = kernel_legs(a, eng, ont_batch(rng, a.ont_reads), False, klegs)
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
                    for leg in ("none", "rstats"):
                        extra = dict(read_stats=ReadStats(os.path.join(tmp, "stats.tsv"))) if leg == "rstats" else {}
                        kw = dict(in2=files[1], out2=outs[1], threads=a.threads, out_codec=2, codec_threads=a.threads // 2, **extra)
                        st, dt, tr = timed(lambda: eng.run(files[0], outs[0], **kw))
                        if rep == 0:
                            continue
                        r = e2e.setdefault(leg, {"wall_s": []})
                        r["wall_s"].append(round(dt, 3))
                        r["classified"] = st.classified
                        t = TRACE.findall(tr)
                        if t:
                            r["bases"] = int(t[0][0])
                            r.setdefault("rstats_kernel_ms", []).append(float(t[0][1]))
                for r in e2e.values():
                    r["median_s"] = statistics.median(r["wall_s"])
                    r["spread_s"] = round(max(r["wall_s"]) - min(r["wall_s"]), 3)
                res["rstats_vs_none"] = round(e2e["rstats"]["median_s"] / e2e["none"]["median_s"], 3)
                res["table"] = open(os.path.join(tmp, "stats.tsv")).read()
                res["e2e"] = e2e
        line = "RSTATS " + json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
