"""Masked runs against normal runs (nh_run_mask): pairs with a "human" fraction p, timed on one GPU in
the same process, interleaved, per p:
  gz.normal     gzip -> gzip, keep_human=0                 (the non-human reads)
  gz.mask       gzip -> gzip, nh_run_mask                  (every read, the human ones' bases as N, built in HBM)
  gz.mask.host  gzip -> gzip, nh_run_mask, NOHUMAN_GZ_READER=host (the reader choice of a masked run, measured)
  plain.normal  gzip -> plain, keep_human=0
  plain.mask    gzip -> plain, nh_run_mask
Inputs, database and workload are tools/human_out_bench.py's: a synthetic table plus the minimizers of a 4 Mb "human" genome,
human pairs are 150 bp pieces of it with 1 % substitutions; `--distinct` gzip members of `--block` pairs used in rotation up to
--pairs; inputs and outputs in /dev/shm.  One warm-up round, then --reps timed rounds; medians.  The builder's kernel time and
rate come from NOHUMAN_TRACE (HIP events around its launches).
The outputs are checked: the plain masked output, with its masked records restored from the input, equals the input text
(every record has the same length here, so the check runs on arrays), and the gzip masked output has the plain one's fields
(sha256 of the decompressed text).
    python tools/mask_bench.py [--pairs 50000000] [--p 0.05,0.5] [--reps 3] [--out profiles/mask_e2e.txt]
Prints one JSON line per p and appends it to --out."""
import argparse
import hashlib
import json
import os
import re
import shutil
import statistics
import sys
import tempfile
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402

from human_out_bench import HDR, make_db, make_member, timed  # noqa: E402

TRACE = re.compile(r"mask: (\d+) records masked, (\d+) written, (\d+) bytes built on device; (\d+) fetched to host; "
                   r"builder kernels ([0-9.]+) ms \(([0-9.]+) GB/s")
LEGS = {  # name: (out_codec, mask, env)
    "gz.normal": (2, False, {}),
    "gz.mask": (2, True, {}),
    "gz.mask.host": (2, True, {"NOHUMAN_GZ_READER": "host"}),
    "plain.normal": (0, False, {}),
    "plain.mask": (0, True, {}),
}


def check_plain(path, members, reps, L=150):
    """the masked plain output against the input text: rows whose sequence is all N restored from the input, then the whole
    text hashed against the input's.  -> (masked rows, equal, sha256 of the output as written)"""
    reclen = len(HDR) + 2 * L + 4  # (HDR ends in its newline)
    s0 = len(HDR)
    h_raw, h_out, h_in = hashlib.sha256(), hashlib.sha256(), hashlib.sha256()
    masked = 0
    off = 0
    for i in range(reps):
        inp = np.frombuffer(members[i % len(members)], dtype=np.uint8).reshape(-1, reclen)
        out = np.fromfile(path, dtype=np.uint8, count=inp.size, offset=off).reshape(-1, reclen).copy()
        off += inp.size
        h_raw.update(out.tobytes())
        rows = (out[:, s0:s0 + L] == ord("N")).all(axis=1)
        masked += int(rows.sum())
        out[rows, s0:s0 + L] = inp[rows, s0:s0 + L]
        h_out.update(out.tobytes())
        h_in.update(inp.tobytes())
    return masked, h_out.digest() == h_in.digest() and off == os.path.getsize(path), h_raw.digest()


def gunzip_sha256(path):
    """sha256 of a gzip file's decompressed text (every member)"""
    h = hashlib.sha256()
    with open(path, "rb") as f:
        d = zlib.decompressobj(31)
        while True:
            chunk = f.read(64 << 20)
            if not chunk:
                break
            while chunk:
                h.update(d.decompress(chunk))
                if d.eof:  # the next member
                    chunk = d.unused_data
                    d = zlib.decompressobj(31)
                else:
                    chunk = b""
        h.update(d.flush())
    return h.digest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=50_000_000)
    ap.add_argument("--block", type=int, default=500_000)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--p", default="0.05,0.5")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--capacity", type=int, default=1 << 27)
    ap.add_argument("--load", type=float, default=0.5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from nohuman_amd import Engine, _lib
    base = "/dev/shm" if os.access("/dev/shm", os.W_OK) else None
    tmp = tempfile.mkdtemp(prefix="nh_mask_", dir=base)
    try:
        rng = np.random.default_rng(5)
        genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=4_000_000)].copy()
        db = os.path.join(tmp, "db")
        make_db(db, a.capacity, a.load, genome)
        L = _lib.lib()
        for p in [float(x) for x in a.p.split(",")]:
            block = min(a.block, a.pairs)
            reps = max(1, a.pairs // block)
            room = shutil.disk_usage(tmp).free
            plain = [[], []]  # per mate: the distinct members' text (the check), and their gzip form
            members = [[], []]
            n_human = []
            for k in range(min(a.distinct, reps)):
                texts, nh = make_member(rng, genome, block, p, k)
                n_human.append(nh)
                for m, text in enumerate(texts):
                    pl = os.path.join(tmp, "b_%d.fq" % (m + 1))
                    open(pl, "wb").write(text)
                    assert L.nh_compress_file(pl.encode(), (pl + ".gz").encode(), 2, a.threads) == 0, L.nh_last_error()
                    os.remove(pl)
                    members[m].append(open(pl + ".gz", "rb").read())
                    os.remove(pl + ".gz")
                    plain[m].append(text)
            # inputs + the plain outputs (the input's size) of one leg must fit
            per_rep = sum(len(x) for x in members[0] + members[1]) / len(members[0])
            per_rep_plain = sum(len(x) for x in plain[0] + plain[1]) / len(plain[0])
            reps = min(reps, max(1, int(0.7 * room / (3 * per_rep + per_rep_plain))))
            files = []
            for m in range(2):
                path = os.path.join(tmp, "in_%d.fq.gz" % (m + 1))
                with open(path, "wb") as f:
                    for i in range(reps):
                        f.write(members[m][i % len(members[m])])
                files.append(path)
            n_human = sum(n_human[i % len(n_human)] for i in range(reps))
            pairs = block * reps
            res = {"p": p, "pairs": pairs, "human_pairs": n_human, "distinct_members": len(members[0]),
                   "gz_bytes": sum(os.path.getsize(f) for f in files), "legs": {}}
            legs = a.legs.split(",")
            with Engine.open(db) as eng:
                for rep in range(a.reps + 1):  # rep 0 warms the buffers and the page cache of the outputs
                    for leg in legs:
                        codec, mask, env = LEGS[leg]
                        ext = ".fq.gz" if codec == 2 else ".fq"
                        outs = [os.path.join(tmp, "%s_%d%s" % (leg, m + 1, ext)) for m in range(2)]
                        for f in os.listdir(tmp):  # (room: every plain output goes, and every gzip one but gz.mask's)
                            if f.startswith((leg + "_", "plain.")) or (f.startswith("gz.") and not f.startswith("gz.mask_")):
                                os.remove(os.path.join(tmp, f))
                        kw = dict(in2=files[1], out2=outs[1], threads=a.threads, out_codec=codec, codec_threads=a.threads // 2,
                                  mask=mask)
                        os.environ.update(env)
                        try:
                            st, dt, tr = timed(lambda: eng.run(files[0], outs[0], **kw))
                        finally:
                            for k in env:
                                os.environ.pop(k, None)
                        if rep == a.reps and leg == "plain.mask":  # the last round's masked outputs: checked
                            chk = [check_plain(outs[m], plain[m], reps) for m in range(2)]
                            res["check_plain"] = {"masked_rows": [c[0] for c in chk], "restored_equals_input": all(c[1] for c in chk),
                                                  "masked_rows_are_the_classified": all(c[0] == st.classified for c in chk)}
                            gz = [os.path.join(tmp, "gz.mask_%d.fq.gz" % (m + 1)) for m in range(2)]
                            if all(os.path.exists(g) for g in gz):
                                res["check_gzip_equals_plain"] = all(gunzip_sha256(gz[m]) == chk[m][2] for m in range(2))
                        if rep == 0:
                            continue
                        r = res["legs"].setdefault(leg, {"wall_s": []})
                        r["wall_s"].append(round(dt, 3))
                        r["classified"] = st.classified
                        t = TRACE.findall(tr)
                        if t:
                            r["masked"], r["written"], r["built_bytes"], r["fetched_bytes"] = (int(x) for x in t[0][:4])
                            r.setdefault("builder_kernel_ms", []).append(float(t[0][4]))
                            r.setdefault("builder_gb_s", []).append(float(t[0][5]))
                        r["trace"] = [x.split("] ", 1)[-1] for x in tr.splitlines() if "wall " in x or "gzip encoder" in x
                                      or "gzip reader:" in x]
                for leg, r in res["legs"].items():
                    r["median_s"] = statistics.median(r["wall_s"])
                    r["mreads_s"] = round(2 * pairs / r["median_s"] / 1e6, 2)
                lg = res["legs"]
                for fmt in ("gz", "plain"):
                    if fmt + ".mask" in lg and fmt + ".normal" in lg:
                        res[fmt + "_mask_vs_normal"] = round(lg[fmt + ".mask"]["median_s"] / lg[fmt + ".normal"]["median_s"], 3)
                if "gz.mask.host" in lg and "gz.mask" in lg:
                    res["gz_mask_host_reader_vs_default"] = round(lg["gz.mask.host"]["median_s"] / lg["gz.mask"]["median_s"], 3)
            for f in os.listdir(tmp):
                if f != "db":
                    os.remove(os.path.join(tmp, f))
            line = "MASK " + json.dumps(res)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
