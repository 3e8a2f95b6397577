"""What --host-bases-only costs (nh_run_hostbases; k_cover_close in nohuman_amd/csrc/nh_cover.hip, the bitmap form of k_mask_copy and
k_mask_fill in nh_mask.hip), on one GPU:
  kernel   on one resident batch -- `--pairs` 150 bp pairs, a fraction --p of them pieces of the genome in the table, and
           `--ont-reads` ONT-like reads (tools/mdata_bench.py's: every second one a piece of the genome) -- nh_cover_close_device
           on the bitmap nh_host_cover_device left, for every --gaps: the wall time of a call on a fresh copy of the bitmap and the
           synchronize behind it, less the copy's own time, the median of --iters calls after --warmup (the entry waits for its
           stream itself).  closed_bases: what the kernel counted.
  e2e      a gzip -> gzip paired run of the pairs, four legs on this library -- a masked run (mask), a masked run with the host
           intervals' file (mask_bed: it pays for the mark pass already), the mode at gap 0 (hb0) and at gap 34 (hb34) -- and, with
           --parent-lib (a libnohuman_engine.so built from the parent commit), mask and mask_bed on that library: every leg a child
           process of its own that opens the database once and repeats the run, the legs in turn, forwards and backwards: medians
           and spreads of --reps after one warm-up run.  mask_builder_ms: the mask builder's kernel time from the run's trace line
           (events on the slots' streams), cover_ms: the mark pass (and the report's builders, the closing) likewise.
    python tools/host_bases_bench.py [--pairs 1000000] [--ont-reads 20000] [--legs kernel,e2e] [--parent-lib tools/old_engine_parent.so]
                                     [--out profiles/host_bases.txt]
Prints one JSON line and appends it to --out."""
import argparse
import ctypes as C
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
MASK = re.compile(r"mask: \d+ records masked, \d+ written, \d+ bytes built on device; \d+ fetched to host; builder kernels ([0-9.]+) ms")
COVER = re.compile(r"host-intervals: [^\n]*kernels ([0-9.]+) ms")
HB = re.compile(r"host-bases-only: (\d+) of (\d+) host bases masked, (\d+) by closing; gap \d+, cover kernels ([0-9.]+) ms")


def wall_ms(torch, fn, warmup, iters):
    ts = []
    for i in range(warmup + iters):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts)


def kernel_legs(a, eng, batch, gaps):
    import numpy as np
    import torch
    text, s, lens, _q, ntext = batch
    d_text = torch.from_numpy(text).cuda()
    d_s = torch.from_numpy(s.view(np.int64)).cuda()
    d_l = torch.from_numpy(lens.view(np.int32)).cuda()
    nseq = len(s)
    d_cover = torch.zeros((ntext + 31) // 32 + 1, dtype=torch.int32, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    eng.host_cover_device(d_text.data_ptr(), ntext, d_s.data_ptr(), d_l.data_ptr(), nseq, d_cover.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    d_saved = d_cover.clone()
    r = {"sequences": nseq, "bases": int(lens.sum()), "text_bytes": ntext}
    r["copy_ms"] = round(wall_ms(torch, lambda: d_cover.copy_(d_saved), a.warmup, a.iters), 4)
    r["covered_bases"] = int(np.unpackbits(d_saved.cpu().numpy().view(np.uint8)).sum())
    for gap in gaps:
        def close():
            d_cover.copy_(d_saved)
            eng.cover_close_device(d_cover.data_ptr(), ntext, d_s.data_ptr(), d_l.data_ptr(), nseq, gap, d_n.data_ptr(), stream=stream)
        d_n.zero_()
        close()
        torch.cuda.synchronize()
        r["gap_%d" % gap] = {"closed_bases": int(d_n.cpu()[0]), "close_ms": round(wall_ms(torch, close, a.warmup, a.iters) - r["copy_ms"], 4)}
    return r


def child(a):
    """one leg of e2e: the library a.lib, the database opened once, the run a.reps + 1 times; a.child: mask, mask_bed, hb0 or hb34"""
    sys.path.insert(0, os.path.dirname(HERE))
    from nohuman_amd import _lib
    L = C.CDLL(a.lib)
    L.nh_last_error.restype = C.c_char_p
    h = C.c_void_p()
    assert L.nh_open(a.db.encode(), 0, C.byref(h)) == 0, L.nh_last_error()
    ra = _lib.nh_run_args()
    ra.in1, ra.in2 = a.in1.encode(), a.in2.encode()
    ra.out1, ra.out2 = (a.out + "_1.fq.gz").encode(), (a.out + "_2.fq.gz").encode()
    ra.threads, ra.n_devices, ra.out_codec, ra.codec_threads = a.threads, 1, 2, max(a.threads // 2, 1)
    st = _lib.nh_stats()
    x = _lib.nh_run_extras()
    x.struct_size, x.mask = C.sizeof(_lib.nh_run_extras), 1
    hi = _lib.nh_host_intervals(C.sizeof(_lib.nh_host_intervals), 0, (a.out + ".bed").encode(), 0, 0, 0)
    hb = _lib.nh_host_bases(C.sizeof(_lib.nh_host_bases), 1, 34 if a.child == "hb34" else 0, 0, 0, 0, 0)
    os.environ["NOHUMAN_TRACE"] = "1"
    walls = []
    for rep in range(a.reps + 1):  # rep 0 warms the buffers and the page cache of the outputs
        t = time.perf_counter()
        if a.child.startswith("hb"):
            rc = L.nh_run_engine_hostbases(h, C.byref(ra), C.byref(x), 0, None, None, None, 0, None, None, None, None, C.byref(hb), C.byref(st))
        elif a.child == "mask_bed":
            rc = L.nh_run_engine_intervals(h, C.byref(ra), C.byref(x), 0, None, None, None, 0, None, None, None, C.byref(hi), C.byref(st))
        else:
            rc = L.nh_run_engine_mask(h, C.byref(ra), None, None, C.byref(st))
        dt = time.perf_counter() - t
        assert rc == 0, L.nh_last_error()
        if rep:
            walls.append(round(dt, 3))
    L.nh_close(h)
    out = {"wall_s": walls, "classified": st.classified}
    if a.child.startswith("hb"):
        out.update(host_bases=hb.host_bases, masked_bases=hb.masked_bases, closed_bases=hb.closed_bases)
    print("LEG " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--ont-reads", type=int, default=20_000)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--gaps", default="34,4096")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default="kernel,e2e")
    ap.add_argument("--capacity", type=int, default=1 << 27)
    ap.add_argument("--load", type=float, default=0.5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    for name in ("--child", "--lib", "--db", "--in1", "--in2"):  # (a leg of e2e in its own process)
        ap.add_argument(name, default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    legs = a.legs.split(",")
    gaps = [int(g) for g in a.gaps.split(",")]
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    import numpy as np
    from human_out_bench import make_db, make_member
    from mdata_bench import ont_with_hits
    from qmask_bench import pairs_batch
    from nohuman_amd import Engine, _lib
    base = "/dev/shm" if os.access("/dev/shm", os.W_OK) else None
    tmp = tempfile.mkdtemp(prefix="nh_hbases_", dir=base)
    try:
        rng = np.random.default_rng(5)
        genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=4_000_000)].copy()
        db = os.path.join(tmp, "db")
        make_db(db, a.capacity, a.load, genome)
        texts, _nh = make_member(rng, genome, a.pairs, a.p, 0)
        res = {"pairs": a.pairs, "p": a.p, "warmup": a.warmup, "iters": a.iters, "reps": a.reps}
        files = []
        with Engine.open(db) as eng:
            if "kernel" in legs:
                res["pairs_150"] = kernel_legs(a, eng, pairs_batch(texts, a.pairs), gaps)
                res["ont"] = kernel_legs(a, eng, ont_with_hits(rng, genome, a.ont_reads), gaps)
            print("kernel legs done", file=sys.stderr, flush=True)
            if "e2e" in legs:
                L = _lib.lib()
                for m, text in enumerate(texts):
                    pl = os.path.join(tmp, "in_%d.fq" % (m + 1))
                    open(pl, "wb").write(text)
                    assert L.nh_compress_file(pl.encode(), (pl + ".gz").encode(), 2, a.threads) == 0, L.nh_last_error()
                    os.remove(pl)
                    files.append(pl + ".gz")
        del texts
        if "e2e" in legs:
            plan = [(leg, leg, _lib.LIB_PATH) for leg in ("mask", "mask_bed", "hb0", "hb34")]
            if a.parent_lib:
                plan = [("parent_" + leg, leg, os.path.abspath(a.parent_lib)) for leg in ("mask", "mask_bed")] + plan
            e2e = {}
            for name, leg, lib in plan + plan[::-1]:  # forwards and backwards: a drift of the box shows as a difference between the two
                cmd = [sys.executable, os.path.abspath(__file__), "--child", leg, "--lib", lib, "--db", db, "--in1", files[0], "--in2", files[1],
                       "--out", os.path.join(tmp, "o_" + name), "--reps", str(a.reps), "--threads", str(a.threads)]
                out = subprocess.run(cmd, capture_output=True, text=True)
                assert out.returncode == 0, out.stderr[-2000:]
                got = json.loads(out.stdout.split("LEG ")[1])
                print("leg %s: %s" % (name, got["wall_s"]), file=sys.stderr, flush=True)
                r = e2e.setdefault(name, {"wall_s": []})
                r["wall_s"] += got.pop("wall_s")
                r.update(got)
                r.setdefault("mask_builder_ms", []).extend(float(x) for x in MASK.findall(out.stderr)[1:])
                cov = [x[3] for x in HB.findall(out.stderr)] or COVER.findall(out.stderr)
                if cov:
                    r.setdefault("cover_ms", []).extend(float(x) for x in cov[1:])
            for r in e2e.values():
                r["median_s"] = statistics.median(r["wall_s"])
                r["spread_s"] = round(max(r["wall_s"]) - min(r["wall_s"]), 3)
                if r["mask_builder_ms"]:
                    r["mask_builder_median_ms"] = statistics.median(r["mask_builder_ms"])
            ref = "parent_" if a.parent_lib else ""
            res["hb34_vs_mask_bed"] = round(e2e["hb34"]["median_s"] / e2e[ref + "mask_bed"]["median_s"], 4)
            res["hb0_vs_mask"] = round(e2e["hb0"]["median_s"] / e2e[ref + "mask"]["median_s"], 4)
            if a.parent_lib:
                res["mask_vs_parent"] = round(e2e["mask"]["median_s"] / e2e["parent_mask"]["median_s"], 4)
            res["e2e"] = e2e
        line = "HOST_BASES " + json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
