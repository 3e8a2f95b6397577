"""What a host selection costs (--host-taxid / --keep-taxid, nh_run_host; k_host_filter in nohuman_amd/csrc/nh_host.hip; DESIGN.md
section 6.14), on one GPU:
  kernel   k_host_filter alone on the results of one resident batch of --sizes 150 bp pairs (a fraction --p of them pieces of the
           genome in the table), out of place with counters as the run launches it, by HIP events around --iters launches back to
           back after --warmup untimed ones (the warm-up alone runs past the first 40 ms), --rounds times: median and spread; the
           same without counters (what the atomics on the two shared words cost); next to the classify launch on the same batch
  e2e      a gzip -> gzip paired run of the first size with --host-taxid 9606 against the same run without it, and -- with
           --parent-lib, a libnohuman_engine.so built from the parent commit -- against the run on that library: every leg a child
           process of its own (a library is loaded once a process) that opens the database once and repeats the run, the legs in
           turn, forwards and backwards: medians and spreads of --reps after one warm-up run
    python tools/host_filter_bench.py [--sizes 1000000,2500000] [--legs kernel,e2e] [--parent-lib tools/old_engine_parent.so]
                                      [--out profiles/host_taxid.txt]
Prints one JSON line and appends it to --out."""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))


def kernel_leg(a, eng, batch, rng):
    import numpy as np
    import torch
    from qmask_bench import time_launches
    from nohuman_amd import engine
    text, s, lens, _q, ntext = batch
    d_text = torch.from_numpy(text).cuda()
    d_s = torch.from_numpy(s.view(np.int64)).cuda()
    d_l = torch.from_numpy(lens.view(np.int32)).cuda()
    nfrag = len(s) // 2
    d_res = torch.zeros(nfrag * 4, dtype=torch.int32, device="cuda")
    d_out = torch.zeros(nfrag * 4, dtype=torch.int32, device="cuda")
    d_cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    table = np.frombuffer(engine.host_table(eng.taxonomy_image(), [9606]), dtype=np.uint8)
    d_tab = torch.from_numpy(table.copy()).cuda()
    stream = torch.cuda.current_stream().cuda_stream

    def classify():
        eng.classify_records_device(d_text.data_ptr(), ntext, d_s.data_ptr(), d_l.data_ptr(), nfrag, True, 0.0, d_res.data_ptr(), stream=stream)

    def host_filter():
        eng.host_filter_device(d_res.data_ptr(), d_out.data_ptr(), nfrag, d_tab.data_ptr(), len(table), d_cnt.data_ptr(), stream=stream)

    def host_filter_uncounted():
        eng.host_filter_device(d_res.data_ptr(), d_out.data_ptr(), nfrag, d_tab.data_ptr(), len(table), 0, stream=stream)

    classify()
    torch.cuda.synchronize()
    res = d_res.cpu().numpy().reshape(-1, 4).copy()
    # the classifier leaves two kinds of call here (0 and the genome's taxon): spread the classified ones over the chain's nodes so
    # that the look-up touches the whole table and a part of the fragments is spared
    classified = res[:, 0] != 0
    res[classified, 0] = rng.integers(1, len(table), size=int(classified.sum())).astype(np.int32)
    d_res.copy_(torch.from_numpy(res.reshape(-1)))
    host_filter()
    torch.cuda.synchronize()
    host, spared = (int(x) for x in d_cnt.cpu())
    assert host == int((table[res[:, 0].view(np.uint32)] != 0).sum()) and host + spared == int(classified.sum())
    ms = [time_launches(torch, host_filter, a.warmup, a.iters) for _ in range(a.rounds)]
    ums = [time_launches(torch, host_filter_uncounted, a.warmup, a.iters) for _ in range(a.rounds)]
    r = {"fragments": nfrag, "classified_fraction": round(float(classified.mean()), 4), "host": host, "spared": spared,
         "host_filter_us": [round(1000 * x, 2) for x in ms], "host_filter_median_us": round(1000 * statistics.median(ms), 2),
         "host_filter_spread_us": round(1000 * (max(ms) - min(ms)), 2)}
    r["without_counters_median_us"] = round(1000 * statistics.median(ums), 2)
    r["without_counters_spread_us"] = round(1000 * (max(ums) - min(ums)), 2)
    r["bytes_moved"] = 32 * nfrag
    r["GBps"] = round(r["bytes_moved"] / (statistics.median(ms) * 1e6), 1)
    classify()  # (the true results again: the classifier's own time does not depend on them, its counters' checker might)
    cms = [time_launches(torch, classify, 5, 20) for _ in range(a.rounds)]
    r["classify_median_ms"] = round(statistics.median(cms), 3)
    r["classify_spread_ms"] = round(max(cms) - min(cms), 3)
    r["host_filter_vs_classify"] = round(statistics.median(ms) / statistics.median(cms), 5)
    return r


def child(a):
    """one leg of e2e: --reps + 1 runs on one open engine of the library named by --lib, through ctypes alone (a library of the
    parent commit has no entry for the selection and cannot be bound by nohuman_amd._lib)"""
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
    hf = _lib.nh_host_filter()
    ids = (C.c_uint64 * 1)(9606)
    hf.struct_size, hf.n_host, hf.host_taxids = C.sizeof(hf), 1, ids
    walls = []
    for rep in range(a.reps + 1):  # rep 0 warms the buffers and the page cache of the outputs
        t = time.perf_counter()
        if a.child == "host":
            rc = L.nh_run_engine_host(h, C.byref(ra), None, 0, None, None, None, 0, None, C.byref(hf), C.byref(st))
        else:
            rc = L.nh_run_engine(h, C.byref(ra), C.byref(st))
        dt = time.perf_counter() - t
        assert rc == 0, L.nh_last_error()
        if rep:
            walls.append(round(dt, 3))
    L.nh_close(h)
    sizes = [os.path.getsize(p.decode()) for p in (ra.out1, ra.out2)]
    print("LEG " + json.dumps({"wall_s": walls, "classified": st.classified, "host": hf.host_fragments, "spared": hf.spared_fragments,
                               "out_bytes": sizes}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,2500000")
    ap.add_argument("--p", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=4000)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
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
    sizes = [int(x) for x in a.sizes.split(",")]
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    import numpy as np
    from human_out_bench import make_db, make_member
    from qmask_bench import pairs_batch
    from nohuman_amd import Engine, _lib
    base = "/dev/shm" if os.access("/dev/shm", os.W_OK) else None
    tmp = tempfile.mkdtemp(prefix="nh_host_", dir=base)
    try:
        rng = np.random.default_rng(5)
        genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=4_000_000)].copy()
        db = os.path.join(tmp, "db")
        make_db(db, a.capacity, a.load, genome)
        res = {"sizes": sizes, "p": a.p, "warmup": a.warmup, "iters": a.iters, "rounds": a.rounds}
        files = []
        with Engine.open(db) as eng:
            for i, n in enumerate(sizes):
                texts, _nh = make_member(rng, genome, n, a.p, 0)
                if "kernel" in legs:
                    res["pairs_%d" % n] = kernel_leg(a, eng, pairs_batch(texts, n), rng)
                if "e2e" in legs and i == 0:
                    L = _lib.lib()
                    for m, text in enumerate(texts):
                        pl = os.path.join(tmp, "in_%d.fq" % (m + 1))
                        open(pl, "wb").write(text)
                        assert L.nh_compress_file(pl.encode(), (pl + ".gz").encode(), 2, a.threads) == 0, L.nh_last_error()
                        os.remove(pl)
                        files.append(pl + ".gz")
                del texts
        if "e2e" in legs:
            plan = [("none", _lib.LIB_PATH), ("host", _lib.LIB_PATH)]
            if a.parent_lib:
                plan.insert(0, ("parent", os.path.abspath(a.parent_lib)))
            e2e = {}
            for leg, lib in plan + plan[::-1]:  # forwards and backwards: a drift of the box shows as a difference between the two
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "host" if leg == "host" else "none", "--lib", lib, "--db", db,
                       "--in1", files[0], "--in2", files[1], "--out", os.path.join(tmp, "o_" + leg), "--reps", str(a.reps), "--threads", str(a.threads)]
                out = subprocess.run(cmd, capture_output=True, text=True)
                assert out.returncode == 0, out.stderr[-2000:]
                got = json.loads(out.stdout.split("LEG ")[1])
                r = e2e.setdefault(leg, {"wall_s": []})
                r["wall_s"] += got.pop("wall_s")
                r.update(got)
            for r in e2e.values():
                r["median_s"] = statistics.median(r["wall_s"])
                r["spread_s"] = round(max(r["wall_s"]) - min(r["wall_s"]), 3)
            res["host_vs_none"] = round(e2e["host"]["median_s"] / e2e["none"]["median_s"], 4)
            if a.parent_lib:
                res["host_vs_parent"] = round(e2e["host"]["median_s"] / e2e["parent"]["median_s"], 4)
                res["none_vs_parent"] = round(e2e["none"]["median_s"] / e2e["parent"]["median_s"], 4)
            res["e2e"] = e2e
        line = "HOSTFILTER " + json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
