"""What --host-intervals costs (nh_run_intervals; k_cover_mark, k_cover_ivl_*, k_cover_line_* in nohuman_amd/csrc/nh_cover.hip; DESIGN.md
section 6.19), on one GPU:
  kernel   on one resident batch -- `--pairs` 150 bp pairs, a fraction --p of them pieces of the genome in the table, and
           `--ont-reads` ONT-like reads (tools/mdata_bench.py's: every second one a piece of the genome) -- four things timed the
           same way, in the same process, on the same buffers: the classify launch, k_mdata_mark (the same scan and the same probe),
           nh_host_cover_device (the piece scan's three launches and k_cover_mark; the entry allocates 8 bytes a sequence of
           scratch and waits for its stream) and nh_cover_intervals_device on the bitmap it left (three launches; 4 bytes a
           sequence).  Each is the wall time of a call followed by a device synchronize, the median of --iters calls after --warmup:
           the two device entries wait for the stream themselves, so events around launches back to back would not compare.
           clear_ms: zeroing the bitmap, which a run does once a batch.  The line builder has no entry of its own: its time is
           part of the run's trace line (e2e: kernels_ms = mark + intervals + lines, by events on the slots' streams).
  e2e      a gzip -> gzip paired run of the pairs with and without the flag and -- with --parent-lib, a libnohuman_engine.so
           built from the parent commit -- the run on that library: every leg a child process of its own that opens the database
           once and repeats the run, the legs in turn, forwards and backwards: medians and spreads of --reps after one warm-up run
    python tools/host_intervals_bench.py [--pairs 1000000] [--ont-reads 20000] [--legs kernel,e2e] [--parent-lib tools/old_engine_parent.so]
                                         [--out profiles/host_intervals.txt]
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
TRACE = re.compile(r"host-intervals: (\d+) intervals in (\d+) fragments, (\d+) bases covered, (\d+) bytes built on device; kernels ([0-9.]+) ms")


def wall_ms(torch, fn, warmup, iters):
    """milliseconds a call and the synchronize behind it: the median of `iters` after `warmup`"""
    ts = []
    for i in range(warmup + iters):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts)


def kernel_legs(a, eng, batch, paired):
    import numpy as np
    import torch
    text, s, lens, _q, ntext = batch
    d_text = torch.from_numpy(text).cuda()
    d_s = torch.from_numpy(s.view(np.int64)).cuda()
    d_l = torch.from_numpy(lens.view(np.int32)).cuda()
    nseq = len(s)
    nfrag = nseq // (2 if paired else 1)
    nodes = int(eng.info.node_count)
    bases = int(lens.sum())
    d_res = torch.zeros(nfrag * 4, dtype=torch.int32, device="cuda")
    d_marks = torch.zeros(eng.minimizer_marks_bytes() // 4, dtype=torch.int32, device="cuda")
    d_groups = torch.zeros(nodes, dtype=torch.int64, device="cuda")
    d_cover = torch.zeros((ntext + 31) // 32 + 1, dtype=torch.int32, device="cuda")
    cap = int(((lens.astype(np.int64) + 1) // 36).sum())
    d_rec = torch.zeros(3 * cap + 3, dtype=torch.int32, device="cuda")
    d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_err = torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    long_reads = bases / nfrag > 2000

    def classify():
        eng.classify_records_device(d_text.data_ptr(), ntext, d_s.data_ptr(), d_l.data_ptr(), nfrag, paired, 0.0, d_res.data_ptr(),
                                    stream=stream, long_reads=long_reads)

    def mdata_mark():
        eng.minimizer_mark_device(d_text.data_ptr(), ntext, d_s.data_ptr(), d_l.data_ptr(), nfrag, d_marks.data_ptr(), d_groups.data_ptr(),
                                  paired=paired, stream=stream)

    def cover_mark():
        eng.host_cover_device(d_text.data_ptr(), ntext, d_s.data_ptr(), d_l.data_ptr(), nseq, d_cover.data_ptr(), stream=stream)

    def cover_mark_cleared():
        d_cover.zero_()
        cover_mark()

    def intervals():
        eng.cover_intervals_device(d_cover.data_ptr(), ntext, d_s.data_ptr(), d_l.data_ptr(), nseq, d_rec.data_ptr(), cap, d_total.data_ptr(),
                                   d_err.data_ptr(), stream=stream)

    r = {"sequences": nseq, "bases": bases, "text_bytes": ntext}
    r["classify_ms"] = round(wall_ms(torch, classify, a.warmup, a.iters), 4)
    r["classified_fraction"] = round(float((d_res.cpu().numpy().reshape(-1, 4)[:, 0] != 0).mean()), 4)
    r["mdata_mark_ms"] = round(wall_ms(torch, mdata_mark, a.warmup, a.iters), 4)
    r["cover_mark_ms"] = round(wall_ms(torch, cover_mark, a.warmup, a.iters), 4)  # (steady state: every bit is set already)
    r["clear_ms"] = round(wall_ms(torch, d_cover.zero_, a.warmup, a.iters), 4)
    r["cover_mark_first_ms"] = round(wall_ms(torch, cover_mark_cleared, a.warmup, a.iters) - r["clear_ms"], 4)
    r["intervals_ms"] = round(wall_ms(torch, intervals, a.warmup, a.iters), 4)
    r["intervals"] = int(d_total.cpu()[0])
    r["covered_fraction"] = round(float(np.unpackbits(d_cover.cpu().numpy().view(np.uint8)).sum()) / bases, 4)
    assert int(d_err.cpu()[0]) == 0
    r["cover_vs_mdata_mark"] = round(r["cover_mark_first_ms"] / r["mdata_mark_ms"], 3)
    r["cover_vs_classify"] = round(r["cover_mark_first_ms"] / r["classify_ms"], 3)
    return r


def child(a):
    """one leg of e2e: the library a.lib, the database opened once, the run a.reps + 1 times; a.child: "flag" or "none" """
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
    hi = _lib.nh_host_intervals(C.sizeof(_lib.nh_host_intervals), 0, (a.out + ".bed").encode(), 0, 0, 0)
    os.environ["NOHUMAN_TRACE"] = "1"
    walls = []
    for rep in range(a.reps + 1):  # rep 0 warms the buffers and the page cache of the outputs
        t = time.perf_counter()
        if a.child == "flag":
            rc = L.nh_run_engine_intervals(h, C.byref(ra), None, 0, None, None, None, 0, None, None, None, C.byref(hi), C.byref(st))
        else:
            rc = L.nh_run_engine(h, C.byref(ra), C.byref(st))
        dt = time.perf_counter() - t
        assert rc == 0, L.nh_last_error()
        if rep:
            walls.append(round(dt, 3))
    L.nh_close(h)
    out = {"wall_s": walls, "classified": st.classified}
    if a.child == "flag":
        out.update(fragments=hi.fragments, intervals=hi.intervals, covered_bases=hi.covered_bases, bed_bytes=os.path.getsize(a.out + ".bed"))
    print("LEG " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--ont-reads", type=int, default=20_000)
    ap.add_argument("--p", type=float, default=0.1)
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
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    import numpy as np
    from human_out_bench import make_db, make_member
    from mdata_bench import ont_with_hits
    from qmask_bench import pairs_batch
    from nohuman_amd import Engine, _lib
    base = "/dev/shm" if os.access("/dev/shm", os.W_OK) else None
    tmp = tempfile.mkdtemp(prefix="nh_cover_", dir=base)
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
                res["pairs_150"] = kernel_legs(a, eng, pairs_batch(texts, a.pairs), True)
                res["ont"] = kernel_legs(a, eng, ont_with_hits(rng, genome, a.ont_reads), False)
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
            plan = [("none", _lib.LIB_PATH), ("flag", _lib.LIB_PATH)]
            if a.parent_lib:
                plan.insert(0, ("parent", os.path.abspath(a.parent_lib)))
            e2e = {}
            for leg, lib in plan + plan[::-1]:  # forwards and backwards: a drift of the box shows as a difference between the two
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "flag" if leg == "flag" else "none", "--lib", lib, "--db", db,
                       "--in1", files[0], "--in2", files[1], "--out", os.path.join(tmp, "o_" + leg), "--reps", str(a.reps), "--threads", str(a.threads)]
                out = subprocess.run(cmd, capture_output=True, text=True)
                assert out.returncode == 0, out.stderr[-2000:]
                got = json.loads(out.stdout.split("LEG ")[1])
                r = e2e.setdefault(leg, {"wall_s": []})
                r["wall_s"] += got.pop("wall_s")
                r.update(got)
                t = TRACE.findall(out.stderr)
                if t:
                    r.setdefault("kernels_ms", []).extend(float(x[4]) for x in t[1:])
            for r in e2e.values():
                r["median_s"] = statistics.median(r["wall_s"])
                r["spread_s"] = round(max(r["wall_s"]) - min(r["wall_s"]), 3)
            res["flag_vs_none"] = round(e2e["flag"]["median_s"] / e2e["none"]["median_s"], 4)
            if a.parent_lib:
                res["none_vs_parent"] = round(e2e["none"]["median_s"] / e2e["parent"]["median_s"], 4)
            res["e2e"] = e2e
        line = "HOST_INTERVALS " + json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
