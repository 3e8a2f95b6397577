"""The encoder's BGZF mode against its gzip mode, and against the gzip mode of another BUILD of the library (the parent
commit's), in one process and in interleaved passes (boxes and processes differ by a few percent; only numbers of one call
compare).  Every leg sends the same text through nh_gzip_gpu_file / nh_bgzf_gpu_file to a file in /dev/shm and reports the kernel
time the library measures (HIP events around a chunk's kernels: deflate, offsets, pack) and the file's size.
usage: bgzf_encoder_bench.py [--mb 1000] [--passes 5] [--only LEG] name=path.so [name=path.so ...]
  e.g.  bgzf_encoder_bench.py new=nohuman_amd/libnohuman_engine.so parent=tools/ab_engine_parent.so
  --only LEG (e.g. new:bgzf): that leg alone, for a kernel trace of it (rocprofv3 --kernel-trace --stats -- python tools/bgzf_encoder_bench.py ...)
A build without nh_bgzf_gpu_file runs its gzip leg only."""
import ctypes as C
import gzip
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nohuman_amd import _lib  # noqa: E402

argv = sys.argv[1:]


def opt(name, default):
    if name in argv:
        i = argv.index(name)
        v = argv[i + 1]
        del argv[i:i + 2]
        return type(default)(v)
    return default


mb, passes, only = opt("--mb", 1000), opt("--passes", 5), opt("--only", "")
libs = [a.split("=", 1) for a in argv]
if not libs:
    raise SystemExit(__doc__)
_lib._preload_hip_runtime()


def fastq_unit(n_reads, seed):
    """bench-like reads: 150 bases, binned qualities that fall off towards the end, Illumina-style names"""
    rng = np.random.default_rng(seed)
    L = 150
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n_reads, L))]
    q = np.where(rng.random((n_reads, L)) < 0.06, ord(":"), ord("F")).astype(np.uint8)
    cut = (L * (0.3 + 0.7 * rng.random(n_reads) ** 0.4)).astype(int)
    tail = rng.choice(np.frombuffer(b"F:,#", np.uint8), (n_reads, L))
    q = np.where(np.arange(L)[None, :] >= cut[:, None], tail, q)
    out = []
    for i in range(n_reads):
        out.append(b"@NH1:7:HGF2YDSXX:1:%d:%d:%d 1:N:0:GATTACAG\n%s\n+\n%s\n"
                   % (1101 + i // 5000, 10000 + int(rng.integers(0, 25000)), 10000 + (i * 17) // 10, seq[i].tobytes(), q[i].tobytes()))
    return b"".join(out)


unit = fastq_unit(60000, 3)
data = (unit * (mb * 1_000_000 // len(unit) + 1))[:mb * 1_000_000]
buf = np.frombuffer(data, np.uint8)
legs = []
for name, path in libs:
    L = C.CDLL(os.path.abspath(path))
    L.nh_last_error.restype = C.c_char_p
    for mode in ("gzip", "bgzf"):
        fn = getattr(L, "nh_%s_gpu_file" % mode, None)
        if fn is None:
            continue
        fn.argtypes = [C.c_int32, C.c_void_p, C.c_uint64, C.c_char_p, C.POINTER(C.c_uint64)]
        if not only or only == "%s:%s" % (name, mode):
            legs.append(("%s:%s" % (name, mode), L, fn))
out = "/dev/shm/bgzf_encoder_bench_%d.gz" % os.getpid()


def one(leg):
    _, L, fn = leg
    st = (C.c_uint64 * 2)()
    t0 = time.perf_counter()
    rc = fn(0, buf.ctypes.data, len(data), out.encode(), st)
    dt = time.perf_counter() - t0
    if rc != 0:
        raise RuntimeError(L.nh_last_error().decode())
    return st[1] / 1e6, st[0], dt


try:
    for leg in legs:  # warm-up, and the content check
        one(leg)
        with gzip.open(out, "rb") as f:
            n = 0
            while True:
                b = f.read(1 << 24)
                if not b:
                    break
                assert b == data[n:n + len(b)], leg[0]
                n += len(b)
        assert n == len(data), leg[0]
    rows = {leg[0]: [] for leg in legs}
    size = {}
    for p in range(passes):
        for leg in (legs if p % 2 == 0 else legs[::-1]):
            k, sz, dt = one(leg)
            rows[leg[0]].append((k, dt))
            size[leg[0]] = sz
finally:
    if os.path.exists(out):
        os.unlink(out)
print("%d bytes of FASTQ text (a unit of %d bytes, repeated), %d passes, every file inflated back to the text once" % (len(data), len(unit), passes))
base = None
for name, r in rows.items():
    ks = sorted(k for k, _ in r)
    med = ks[len(ks) // 2]
    base = base or med
    print("  %-12s kernel s %s   median %.4f = %.2f GB/s of text (%+.2f %% vs %s)   file %d bytes (%.4f : 1)   whole call, median %.3f s" % (
        name, " ".join("%.4f" % k for k, _ in r), med, len(data) / med / 1e9, 100.0 * (base / med - 1.0), next(iter(rows)),
        size[name], len(data) / size[name], sorted(d for _, d in r)[len(r) // 2]))
