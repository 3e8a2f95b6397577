"""What --dust-reads costs (nh_run_dust, k_rdust in nohuman_amd/csrc/nh_dust.hip), on one GPU:
  kernel   nh_dust_reads_device alone on one resident batch -- `--pairs` 150 bp pairs (tools/qmask_bench.py's batch: both mates'
           text in one buffer as nh_run lays it out) and `--ont-reads` ONT-like reads -- wall time of --iters calls after
           --warmup calls that are not timed (the entry waits for its stream, so a call is the three launches and the
           allocation of its scratch); Gbases/s = the batch's bases per call.  Beside it k_dust on AS MANY BASES in the same
           process, through nh_dust_mask: the same sequences, back to back in one host buffer, as its segments.  nh_dust_mask
           also allocates and copies the buffer both ways, so k_dust's time is taken as the DIFFERENCE between a call with all
           segments and a call on the same buffer with one segment of 7 bases (medians of --reps): the tile table's upload and
           the kernel.  ratio = k_rdust's Gbases/s over k_dust's.
  e2e      a gzip -> gzip run of the pairs with and without the flag, interleaved, medians of --reps after one warm-up round;
           with --repo <parent checkout> the library of that tree runs the leg without the flag (it has no flag to run)
    python tools/read_dust_bench.py [--pairs 1000000] [--ont-reads 20000] [--legs kernel,e2e] [--out profiles/read_dust.txt]
Prints one JSON line and appends it to --out."""
import argparse
import ctypes as C
import json
import os
import re
import shutil
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
TRACE = re.compile(r"dust-reads: (\d+) of (\d+) bases masked, kernel ([0-9.]+) ms")


def kernel_leg(a, eng, L, batch):
    import numpy as np
    import torch
    text, s, lens, _q, ntext = batch
    d_text = torch.from_numpy(text).cuda()
    d_out = d_text.clone()
    d_s = torch.from_numpy(s.view(np.int64)).cuda()
    d_l = torch.from_numpy(lens.view(np.int32)).cuda()
    d_m = torch.zeros(1, dtype=torch.int64, device="cuda")
    nseq, bases = len(s), int(lens.sum())
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        eng.dust_reads_device(d_text.data_ptr(), ntext, d_s.data_ptr(), d_l.data_ptr(), nseq, d_out.data_ptr(), d_m.data_ptr(), stream)

    for _ in range(a.warmup):
        call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        call()
    ms = (time.perf_counter() - t0) * 1e3 / a.iters
    r = {"sequences": nseq, "bases": bases, "text_bytes": ntext, "rdust_ms": round(ms, 4), "rdust_gbases_s": round(bases / ms / 1e6, 2),
         "masked_fraction": round(int(d_m.cpu()[0]) / (a.warmup + a.iters) / bases, 5)}
    # k_dust on as many bases: the sequences back to back in one host buffer, each a segment of nh_dust_mask
    starts = np.concatenate([[0], np.cumsum(lens.astype(np.uint64))]).astype(np.uint64)
    flat = np.empty(bases, dtype=np.uint8)
    order = np.argsort(s, kind="stable")
    at = 0
    for i in order:  # (a copy loop on the host: not timed)
        n = int(lens[i])
        flat[at:at + n] = text[int(s[i]):int(s[i]) + n]
        at += n
    seg_s = np.ascontiguousarray(starts[:-1])
    seg_l = np.ascontiguousarray(lens[order].astype(np.uint64))
    one_s, one_l = np.array([0], dtype=np.uint64), np.array([7], dtype=np.uint64)
    masked = C.c_uint64(0)
    P = lambda x: x.ctypes.data_as(C.c_void_p)
    U = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint64))

    def dust_mask(ss, ll):
        buf = flat.copy()
        t = time.perf_counter()
        assert L.nh_dust_mask(a.device, P(buf), bases, U(ss), U(ll), len(ss), C.byref(masked)) == 0, L.nh_last_error()
        return (time.perf_counter() - t) * 1e3

    full, base = [], []
    for rep in range(a.reps + 1):
        f, b = dust_mask(seg_s, seg_l), dust_mask(one_s, one_l)
        if rep:
            full.append(f), base.append(b)
    kd = statistics.median(full) - statistics.median(base)
    r.update(dust_mask_ms=[round(x, 3) for x in full], dust_mask_one_segment_ms=[round(x, 3) for x in base], k_dust_ms=round(kd, 4),
             k_dust_gbases_s=round(bases / kd / 1e6, 2) if kd > 0 else None, ratio=round(kd / ms, 3) if kd > 0 else None)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--ont-reads", type=int, default=20_000)
    ap.add_argument("--p", type=float, default=0.05)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default="kernel,e2e")
    ap.add_argument("--capacity", type=int, default=1 << 27)
    ap.add_argument("--load", type=float, default=0.5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--repo", default=os.path.dirname(HERE))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    legs = a.legs.split(",")
    sys.path.insert(0, HERE)
    import numpy as np
    from human_out_bench import make_db, make_member, timed
    from qmask_bench import ont_batch, pairs_batch
    sys.path.insert(0, os.path.abspath(a.repo))  # (last: the tree named here is the one nohuman_amd comes from)
    from nohuman_amd import Engine, _lib
    base = "/dev/shm" if os.access("/dev/shm", os.W_OK) else None
    tmp = tempfile.mkdtemp(prefix="nh_rdust_", dir=base)
    try:
        rng = np.random.default_rng(5)
        genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=4_000_000)].copy()
        db = os.path.join(tmp, "db")
        make_db(db, a.capacity, a.load, genome)
        texts, _nh = make_member(rng, genome, a.pairs, a.p, 0)
        res = {"repo": os.path.abspath(a.repo), "pairs": a.pairs, "warmup": a.warmup, "iters": a.iters, "reps": a.reps}
        with Engine.open(db) as eng:
            has = hasattr(eng, "dust_reads_device")
            L = _lib.lib()
            if "kernel" in legs and has:
                res["pairs_150"] = kernel_leg(a, eng, L, pairs_batch(texts, a.pairs))
                res["ont"] = kernel_leg(a, eng, L, ont_batch(rng, a.ont_reads))
            if "e2e" in legs:
                files = []
                for m, text in enumerate(texts):
                    pl = os.path.join(tmp, "in_%d.fq" % (m + 1))
                    open(pl, "wb").write(text)
                    assert L.nh_compress_file(pl.encode(), (pl + ".gz").encode(), 2, a.threads) == 0, L.nh_last_error()
                    os.remove(pl)
                    files.append(pl + ".gz")
                outs = [os.path.join(tmp, "o_%d.fq.gz" % (m + 1)) for m in range(2)]
                runs = {"none": {}}
                if has:
                    runs["dust"] = dict(dust_reads=True)
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
                            r["masked_bases"], r["bases"] = int(t[0][0]), int(t[0][1])
                            r.setdefault("rdust_kernel_ms", []).append(float(t[0][2]))
                for r in e2e.values():
                    r["median_s"] = statistics.median(r["wall_s"])
                    r["spread_s"] = round(max(r["wall_s"]) - min(r["wall_s"]), 3)
                if "dust" in e2e:
                    res["dust_vs_none"] = round(e2e["dust"]["median_s"] / e2e["none"]["median_s"], 3)
                res["e2e"] = e2e
        line = "READ_DUST " + json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
