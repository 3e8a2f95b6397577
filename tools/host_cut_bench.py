"""What --host-cut costs (nh_run_hostcut; nohuman_amd/csrc/nh_cut.hip), on one GPU, beside the mode it is the
alternative to, --host-bases-only:
  kernel   single-end runs, plain -> plain, of three inputs -- `--reads` reads of 150 bases, a fraction --p of them pieces of the
           genome in the table; `--ont-reads` ONT-like reads (tools/mdata_bench.py's: every second one a piece of the genome); the
           same ONT-like reads with, in every other second one, a 300-base piece of the genome every 4000 bases (the read the mode is for:
           long pieces between short host stretches) -- in ONE child process that opens the database once and runs the two modes at
           gap 34 in turn: the builders' kernel times from the runs' trace lines (device events around the builder's launches on the
           slots' streams, summed over the batches; the first run of each mode is the warm-up), their medians and the ratio
           cut / hostbases.  The batches are the same in both modes: the same reader, the same cuts.
  e2e      a gzip -> gzip run of the 150-base reads: this library with --host-cut --host-gap 34 against --parent-lib (a
           libnohuman_engine.so built from the parent commit; without it: this library) with --host-bases-only --host-gap 34, both
           loaded into one child process, each with the database opened once, the runs in turn: the median of --reps each after one
           warm-up run, the parent's spread (max - min), and whether the new median lies no more than that spread above the parent's.
    python tools/host_cut_bench.py [--reads 1000000] [--ont-reads 20000] [--legs kernel,e2e] [--parent-lib tools/old_engine_parent.so]
                                   [--out profiles/host_cut.txt]
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
HB = re.compile(r"host-bases-only: (\d+) of (\d+) host bases masked, (\d+) by closing; gap \d+, cover kernels ([0-9.]+) ms, mask builder kernels ([0-9.]+) ms")
CUT = re.compile(r"host-cut: (\d+) host bases: (\d+) in (\d+) pieces, (\d+) cut \((\d+) by closing\), (\d+) in short runs; (\d+) reads dropped; (\d+) items; "
                 r"gap \d+, min piece \d+, cover kernels ([0-9.]+) ms, cut builder kernels ([0-9.]+) ms")


def run_args(_lib, in1, out1, threads, codec):
    ra = _lib.nh_run_args()
    ra.in1, ra.out1 = in1.encode(), out1.encode()
    ra.threads, ra.n_devices, ra.out_codec, ra.codec_threads = threads, 1, codec, max(threads // 2, 1)
    return ra


def child_kernel(a):
    """the two modes in turn on this library, a.reps + 1 times each; the trace lines go to stderr, in the order of the runs"""
    sys.path.insert(0, os.path.dirname(HERE))
    from nohuman_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    assert L.nh_open(a.db.encode(), 0, C.byref(h)) == 0, L.nh_last_error()
    ra = run_args(_lib, a.in1, a.out + ".fq", a.threads, 0)
    st = _lib.nh_stats()
    x = _lib.nh_run_extras()
    x.struct_size, x.mask = C.sizeof(_lib.nh_run_extras), 1
    os.environ["NOHUMAN_TRACE"] = "1"
    sizes = {}
    for rep in range(a.reps + 1):
        hb = _lib.nh_host_bases(C.sizeof(_lib.nh_host_bases), 1, 34, 0, 0, 0, 0)
        rc = L.nh_run_engine_hostbases(h, C.byref(ra), C.byref(x), 0, None, None, None, 0, None, None, None, None, C.byref(hb), C.byref(st))
        assert rc == 0, L.nh_last_error()
        sizes["hostbases_bytes"] = os.path.getsize(a.out + ".fq")
        hc = _lib.nh_host_cut(C.sizeof(_lib.nh_host_cut), 1, 34, a.min_piece)
        rc = L.nh_run_engine_hostcut(h, C.byref(ra), C.byref(x), 0, None, None, None, 0, None, None, None, None, None, C.byref(hc), C.byref(st))
        assert rc == 0, L.nh_last_error()
        sizes["cut_bytes"] = os.path.getsize(a.out + ".fq")
    L.nh_close(h)
    print("LEG " + json.dumps(sizes), flush=True)


def child_e2e(a):
    """the parent's library with --host-bases-only and this one with --host-cut, loaded side by side, the runs in turn"""
    sys.path.insert(0, os.path.dirname(HERE))
    from nohuman_amd import _lib
    new = _lib.lib()
    old = C.CDLL(a.lib)
    old.nh_last_error.restype = C.c_char_p
    st = _lib.nh_stats()
    x = _lib.nh_run_extras()
    x.struct_size, x.mask = C.sizeof(_lib.nh_run_extras), 1
    hs = []
    for L in (old, new):
        h = C.c_void_p()
        assert L.nh_open(a.db.encode(), 0, C.byref(h)) == 0, L.nh_last_error()
        hs.append(h)
    walls = {"parent_hostbases": [], "hostcut": []}
    for rep in range(a.reps + 1):  # rep 0 warms the buffers and the page cache of the outputs
        hb = _lib.nh_host_bases(C.sizeof(_lib.nh_host_bases), 1, 34, 0, 0, 0, 0)
        ra = run_args(_lib, a.in1, a.out + "_hb.fq.gz", a.threads, 2)
        t = time.perf_counter()
        rc = old.nh_run_engine_hostbases(hs[0], C.byref(ra), C.byref(x), 0, None, None, None, 0, None, None, None, None, C.byref(hb), C.byref(st))
        dt = time.perf_counter() - t
        assert rc == 0, old.nh_last_error()
        if rep:
            walls["parent_hostbases"].append(round(dt, 3))
        hc = _lib.nh_host_cut(C.sizeof(_lib.nh_host_cut), 1, 34, a.min_piece)
        ra = run_args(_lib, a.in1, a.out + "_cut.fq.gz", a.threads, 2)
        t = time.perf_counter()
        rc = new.nh_run_engine_hostcut(hs[1], C.byref(ra), C.byref(x), 0, None, None, None, 0, None, None, None, None, None, C.byref(hc), C.byref(st))
        dt = time.perf_counter() - t
        assert rc == 0, new.nh_last_error()
        if rep:
            walls["hostcut"].append(round(dt, 3))
    counts = {k: int(getattr(hc, k)) for k in ("host_bases", "pieces", "piece_bases", "cut_bases", "short_bases", "dropped_reads", "closed_bases")}
    old.nh_close(hs[0])
    new.nh_close(hs[1])
    print("LEG " + json.dumps({"wall_s": walls, "counts": counts, "masked_bases": int(hb.masked_bases)}), flush=True)


def chimeric(rng, genome, batch, stretch=300, every=4000):
    """the ONT-like batch with, in every second read -- the random ones, between the reads that are pieces of the genome whole --, a
    piece of the genome of `stretch` bases every `every` bases"""
    text, s, lens, q, ntext = batch
    text = text.copy()
    for i in range(1, len(s), 2):
        for at in range(every // 2, int(lens[i]) - stretch, every):
            g = int(rng.integers(0, genome.size - stretch))
            text[int(s[i]) + at:int(s[i]) + at + stretch] = genome[g:g + stretch]
    return text, s, lens, q, ntext


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--ont-reads", type=int, default=20_000)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--min-piece", type=int, default=35)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--legs", default="kernel,e2e")
    ap.add_argument("--capacity", type=int, default=1 << 27)
    ap.add_argument("--load", type=float, default=0.5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    for name in ("--child", "--lib", "--db", "--in1"):  # (a leg in its own process)
        ap.add_argument(name, default=None)
    a = ap.parse_args()
    if a.child:
        return child_kernel(a) if a.child == "kernel" else child_e2e(a)
    legs = a.legs.split(",")
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    import numpy as np
    from human_out_bench import make_db, make_member
    from mdata_bench import ont_with_hits
    from nohuman_amd import _lib
    base = "/dev/shm" if os.access("/dev/shm", os.W_OK) else None
    tmp = tempfile.mkdtemp(prefix="nh_hcut_", dir=base)
    try:
        rng = np.random.default_rng(5)
        genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=4_000_000)].copy()
        db = os.path.join(tmp, "db")
        make_db(db, a.capacity, a.load, genome)
        texts, _nh = make_member(rng, genome, a.reads, a.p, 0)
        inputs = {"reads_150": os.path.join(tmp, "reads.fq")}
        open(inputs["reads_150"], "wb").write(texts[0])
        del texts
        res = {"reads": a.reads, "p": a.p, "ont_reads": a.ont_reads, "min_piece": a.min_piece, "reps": a.reps}

        def run_child(leg, in1, lib, name):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", leg, "--lib", lib, "--db", db, "--in1", in1, "--out", os.path.join(tmp, "o_" + name),
                   "--reps", str(a.reps), "--threads", str(a.threads), "--min-piece", str(a.min_piece)]
            out = subprocess.run(cmd, capture_output=True, text=True)
            assert out.returncode == 0, out.stderr[-3000:]
            return json.loads(out.stdout.split("LEG ")[1]), out.stderr

        if "kernel" in legs:
            ont = ont_with_hits(rng, genome, a.ont_reads)
            for name, batch in (("ont", ont), ("ont_chimeric", chimeric(rng, genome, ont))):
                inputs[name] = os.path.join(tmp, name + ".fq")
                batch[0][:batch[4]].tofile(inputs[name])
            del ont
            for name in ("reads_150", "ont", "ont_chimeric"):
                sizes, err = run_child("kernel", inputs[name], _lib.LIB_PATH, name)
                hb, cut = HB.findall(err), CUT.findall(err)
                assert len(hb) == len(cut) == a.reps + 1, err[-3000:]
                mask_ms, cut_ms = [float(x[4]) for x in hb[1:]], [float(x[9]) for x in cut[1:]]
                r = dict(sizes, input_bytes=os.path.getsize(inputs[name]), host_bases=int(cut[-1][0]), piece_bases=int(cut[-1][1]), pieces=int(cut[-1][2]),
                         cut_bases=int(cut[-1][3]), closed_bases=int(cut[-1][4]), short_bases=int(cut[-1][5]), dropped_reads=int(cut[-1][6]),
                         items=int(cut[-1][7]), masked_bases=int(hb[-1][0]), cover_ms=statistics.median(float(x[8]) for x in cut[1:]),
                         mask_builder_ms=mask_ms, cut_builder_ms=cut_ms)
                r["mask_builder_median_ms"], r["cut_builder_median_ms"] = statistics.median(mask_ms), statistics.median(cut_ms)
                r["cut_vs_hostbases"] = round(r["cut_builder_median_ms"] / r["mask_builder_median_ms"], 3)
                res[name] = r
                print("kernel leg %s: mask builder %.3f ms, cut builder %.3f ms" % (name, r["mask_builder_median_ms"], r["cut_builder_median_ms"]),
                      file=sys.stderr, flush=True)
        if "e2e" in legs:
            L = _lib.lib()
            gz = inputs["reads_150"] + ".gz"
            assert L.nh_compress_file(inputs["reads_150"].encode(), gz.encode(), 2, a.threads) == 0, L.nh_last_error()
            lib = os.path.abspath(a.parent_lib) if a.parent_lib else _lib.LIB_PATH
            got, _err = run_child("e2e", gz, lib, "e2e")
            w = got["wall_s"]
            e2e = {"parent_lib": bool(a.parent_lib), "wall_s": w, "counts": got["counts"], "masked_bases": got["masked_bases"]}
            e2e["parent_median_s"], e2e["cut_median_s"] = statistics.median(w["parent_hostbases"]), statistics.median(w["hostcut"])
            e2e["parent_spread_s"] = round(max(w["parent_hostbases"]) - min(w["parent_hostbases"]), 3)
            e2e["accepted"] = e2e["cut_median_s"] <= e2e["parent_median_s"] + e2e["parent_spread_s"]
            res["e2e"] = e2e
        line = "HOST_CUT " + json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
