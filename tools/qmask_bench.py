"""What --minimum-base-quality costs (nh_run_minq, k_qmask in nohuman_amd/csrc/nh_qmask.hip), on one GPU:
  kernel   k_qmask alone on one resident batch -- `--pairs` 150 bp pairs (tools/human_out_bench.py's Illumina-like text, both
           mates' text in one buffer as nh_run lays it out), and `--ont-reads` ONT-like reads (lengths log-normal around 8 kb,
           qualities of 3 .. 40 in stretches) -- by HIP events around --iters launches back to back after --warmup launches that
           are not timed (steady state: the chip's first tens of milliseconds under load are a transient); the masked bytes per
           second count sequence + qualities read and sequence written
  classify the classify launch (nh_classify_records_device) on the same batch, timed the same way -- the kernel the pre-pass
           stands in front of; with --repo <parent checkout> the library of that tree is the one timed
  e2e      a gzip -> gzip run of the pairs with and without Q, interleaved, medians of --reps after one warm-up round
    python tools/qmask_bench.py [--pairs 1000000] [--ont-reads 20000] [--q 20] [--legs kernel,classify,e2e] [--out profiles/qmask.txt]
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
TRACE = re.compile(r"qmask: Q (\d+), (\d+) of (\d+) bases masked, kernel ([0-9.]+) ms")


def pairs_batch(texts, n, L=150):
    """both mates' FASTQ text (records of one length) as one batch text: (text, starts, lens, qual starts), mates interleaved"""
    import numpy as np
    len1 = len(texts[0])
    base2 = (len1 + 8 + 255) & ~255
    text = np.zeros(base2 + len(texts[1]) + 8, dtype=np.uint8)
    text[:len1] = np.frombuffer(texts[0], dtype=np.uint8)
    text[base2:base2 + len(texts[1])] = np.frombuffer(texts[1], dtype=np.uint8)
    reclen = len1 // n
    hdr = reclen - (L + 3 + L + 1)
    s = np.empty(2 * n, dtype=np.uint64)
    s[0::2] = np.arange(n, dtype=np.uint64) * reclen + hdr
    s[1::2] = s[0::2] + base2
    return text, s, np.full(2 * n, L, dtype=np.uint32), s + np.uint64(L + 3), base2 + len(texts[1])


def ont_batch(rng, n):
    import numpy as np
    lens = np.clip(rng.lognormal(9.0, 0.6, size=n), 200, 300_000).astype(np.int64)
    rec = 4 + lens + 3 + lens + 1  # "@rX\n" + seq + "\n+\n" + qual + "\n"
    off = np.concatenate([[0], np.cumsum(rec)])
    text = np.full(int(off[-1]) + 8, 0x0A, dtype=np.uint8)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    total = int(lens.sum())
    bases = acgt[rng.integers(0, 4, size=total)]
    # qualities in stretches of 50: a level of 3 .. 40 each, +-2 of noise
    level = np.repeat(rng.integers(3, 41, size=total // 50 + 1), 50)[:total]
    quals = (33 + np.clip(level + rng.integers(-2, 3, size=total), 0, 60)).astype(np.uint8)
    s = (off[:-1] + 4).astype(np.uint64)
    q = (off[:-1] + 4 + lens + 3).astype(np.uint64)
    at = 0
    for i in range(n):
        ln = int(lens[i])
        text[int(off[i]):int(off[i]) + 3] = np.frombuffer(b"@rX", dtype=np.uint8)
        text[int(s[i]):int(s[i]) + ln] = bases[at:at + ln]
        text[int(s[i]) + ln + 1] = 0x2B
        text[int(q[i]):int(q[i]) + ln] = quals[at:at + ln]
        at += ln
    return text, s, lens.astype(np.uint32), q, int(off[-1])


def time_launches(torch, fn, warmup, iters):
    """milliseconds per launch: events around `iters` launches back to back, after `warmup` untimed ones"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def kernel_legs(a, eng, name, batch, paired, legs):
    import numpy as np
    import torch
    text, s, lens, q, ntext = batch
    d_text = torch.from_numpy(text).cuda()
    d_out = torch.empty_like(d_text)
    d_s = torch.from_numpy(s.view(np.int64)).cuda()
    d_l = torch.from_numpy(lens.view(np.int32)).cuda()
    d_q = torch.from_numpy(q.view(np.int64)).cuda()
    d_m = torch.zeros(1, dtype=torch.int64, device="cuda")
    nseq = len(s)
    nfrag = nseq // (2 if paired else 1)
    d_res = torch.zeros(nfrag * 4, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    bases = int(lens.sum())
    r = {"sequences": nseq, "bases": bases, "text_bytes": ntext}
    if "kernel" in legs:
        ms = time_launches(torch, lambda: eng.quality_mask_device(d_text.data_ptr(), ntext, d_s.data_ptr(), d_l.data_ptr(), d_q.data_ptr(), nseq,
                                                                  a.q, d_out.data_ptr(), d_m.data_ptr(), stream), a.warmup, a.iters)
        r["qmask_ms"] = round(ms, 4)
        r["qmask_gb_s"] = round(3 * bases / ms / 1e6, 1)
        r["masked_fraction"] = round(int(d_m.cpu()[0]) / (a.warmup + a.iters) / bases, 4)
    if "classify" in legs:
        long_reads = bases / nfrag > 2000
        for what, buf in (("classify_ms", d_text), ("classify_masked_ms", d_out)):
            if buf is d_out and "kernel" not in legs:
                continue
            ms = time_launches(torch, lambda: eng.classify_records_device(buf.data_ptr(), ntext, d_s.data_ptr(), d_l.data_ptr(), nfrag, paired, 0.0,
                                                                          d_res.data_ptr(), stream=stream, long_reads=long_reads), a.warmup, a.iters)
            r[what] = round(ms, 4)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--ont-reads", type=int, default=20_000)
    ap.add_argument("--q", type=int, default=20)
    ap.add_argument("--p", type=float, default=0.05)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default="kernel,classify,e2e")
    ap.add_argument("--capacity", type=int, default=1 << 27)
    ap.add_argument("--load", type=float, default=0.5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repo", default=os.path.dirname(HERE))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    legs = a.legs.split(",")
    sys.path.insert(0, HERE)
    import numpy as np
    from human_out_bench import make_db, make_member, timed
    sys.path.insert(0, os.path.abspath(a.repo))  # (last: the tree named here is the one nohuman_amd comes from)
    from nohuman_amd import Engine, _lib
    base = "/dev/shm" if os.access("/dev/shm", os.W_OK) else None
    tmp = tempfile.mkdtemp(prefix="nh_qmask_", dir=base)
    try:
        rng = np.random.default_rng(5)
        genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=4_000_000)].copy()
        db = os.path.join(tmp, "db")
        make_db(db, a.capacity, a.load, genome)
        texts, _nh = make_member(rng, genome, a.pairs, a.p, 0)
        res = {"repo": os.path.abspath(a.repo), "q": a.q, "pairs": a.pairs, "warmup": a.warmup, "iters": a.iters}
        with Engine.open(db) as eng:
            has_qmask = hasattr(eng, "quality_mask_device")
            klegs = [x for x in legs if x in ("kernel", "classify") and (x != "kernel" or has_qmask)]
            if klegs:
                res["pairs_150"] = kernel_legs(a, eng, "pairs", pairs_batch(texts, a.pairs), True, klegs)
                res["ont"] = kernel_legs(a, eng, "ont", ont_batch(rng, a.ont_reads), False, klegs)
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
                runs = {"none": {}}
                if has_qmask:
                    runs["minq"] = dict(min_base_quality=a.q)
                e2e = {}
                for rep in range(a.reps + 1):  # rep 0 warms the buffers and the page cache of the outputs
                    for leg, extra in runs.items():
                        kw = dict(in2=files[1], out2=outs[1], threads=a.threads, out_codec=2, codec_threads=a.threads // 2, **extra)
                        st, dt, tr = timed(lambda: eng.run(files[0], outs[0], **kw))
                        if rep == 0:
                            continue
                        r = e2e.setdefault(leg, {"wall_s": []})
                        r["wall_s"].append(round(dt, 3))
                        r["classified"] = st.classified
                        t = TRACE.findall(tr)
                        if t:
                            r["masked_bases"], r["bases"] = int(t[0][1]), int(t[0][2])
                            r.setdefault("qmask_kernel_ms", []).append(float(t[0][3]))
                for r in e2e.values():
                    r["median_s"] = statistics.median(r["wall_s"])
                    r["spread_s"] = round(max(r["wall_s"]) - min(r["wall_s"]), 3)
                if "minq" in e2e:
                    res["minq_vs_none"] = round(e2e["minq"]["median_s"] / e2e["none"]["median_s"], 3)
                res["e2e"] = e2e
        line = "QMASK " + json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
