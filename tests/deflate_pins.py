"""The pin set of the GPU gzip / BGZF encoder and the comparison with its host model (a helper of the tests, not a test).

The encoder's file is a pure function of (text, ways, region bytes, chunk bytes, price choice, mode), and nh_gzip_model_file
(nohuman_amd/csrc/nh_deflate_model.h) computes that function on a CPU from the kernel's own lane-level code.  pin_set() is the list
of named texts at which an encoder can be wrong and still round-trip: sizes around the hash context, the step, the longest match and
the region; runs and repeats of every critical length started at lanes 0, 62 and 63; distances around the window; one hash bucket
under more candidates than it has ways; counts that force the length limits, ties, one-symbol codes; texts that make the price
pilot choose either set.  assert_equals_model() is the one comparison: bytes equal, or a message that says where they part.
tests/test_deflate_model.py checks on a CPU that the set separates the encoder's variants at all."""
import ctypes as C
import functools
import os
import tempfile
import zlib

import numpy as np

from nohuman_amd import _lib

BGZF_REGION = 65280
SIZES = (0, 1, 2, 3, 4, 5, 63, 64, 65, 257, 258, 259, 260, 4095, 4096, 4097, 65279, 65280, 65281, 65535, 65536, 65537)
LENGTHS = (3, 4, 5, 31, 32, 33, 257, 258, 259, 258 + 64)
PERIODS = (1, 2, 3, 4, 5, 63, 64, 65)
# The encoder's variants the pin set is run under (tests/test_gpu_deflate_pin.py: a fresh process each, the knobs are read once):
# (name, the knobs, BGZF?).  All six k_deflate instantiations, the small regions with both forced price sets and the pilot, and the
# pageable staging buffers.
VARIANTS = tuple(
    [("ways%d_%s" % (w, "bgzf" if b else "gzip"), {"NOHUMAN_GZIP_WAYS": str(w)}, b) for b in (False, True) for w in (4, 6, 8)]
    + [("ways%d_region4096_%s" % (w, "pilot" if p is None else "prices" + p),
        dict({"NOHUMAN_GZIP_WAYS": str(w), "NOHUMAN_GZIP_REGION": "4096"}, **({} if p is None else {"NOHUMAN_GZIP_PRICES": p})), False)
       for w in (4, 8) for p in ("0", "1", None)]
    + [("pageable_staging", {"NOHUMAN_NO_PINNED": "1"}, False)])
STAT_NAMES = ("file_bytes", "regions", "price_set", "dynamic_blocks", "stored_blocks", "repaired15", "repaired7", "longest_match",
              "longest_dist", "extended", "tokens", "matches")


# ---- the model --------------------------------------------------------------------------------------------------------------
def encoder_options(env=None, bgzf=False):
    """the options the encoder reads from its environment (nh_deflate.hip: gzip_ways, region_bytes, chunk_bytes_now, pilot)"""
    env = os.environ if env is None else env

    def atol(name, default):
        s = env.get(name)
        if s is None:
            return default
        digits = ""
        s = s.strip()
        for i, ch in enumerate(s):
            if ch.isdigit() or (i == 0 and ch in "+-"):
                digits += ch
            else:
                break
        return int(digits) if digits.strip("+-") else 0

    w = atol("NOHUMAN_GZIP_WAYS", 4)
    mb = atol("NOHUMAN_GZIP_CHUNK_MB", 128)
    r = atol("NOHUMAN_GZIP_REGION", 65536)
    p = env.get("NOHUMAN_GZIP_PRICES", "")
    return dict(ways=w if w in (6, 8) else 4, region=r, chunk=min(max(mb, 64), 512) << 20, prices=int(p[0]) if p[:1] in ("0", "1") else -1,
                bgzf=bgzf)


def model(data, ways=4, region=65536, chunk=128 << 20, prices=-1, bgzf=False, threads=0):
    """-> (file bytes, stats dict, bytes of every region's deflate stream)"""
    region_len = BGZF_REGION if bgzf else min(max(region, 4096), 65536) & ~63
    chunk_len = chunk - chunk % region_len if bgzf else chunk
    cap = sum(-(-min(chunk_len, len(data) - at) // region_len) for at in range(0, len(data), chunk_len))
    sizes = (C.c_uint32 * max(1, cap))()
    opts = _lib.nh_gzip_model_opts(ways=ways, region_bytes=max(0, min(region, 0xFFFFFFFF)), chunk_bytes=chunk, prices=prices, bgzf=int(bgzf),
                                   threads=threads, region_sizes=sizes, region_sizes_cap=cap)
    stats = (C.c_uint64 * 12)()
    fd, path = tempfile.mkstemp(suffix=".model.gz")
    os.close(fd)
    try:
        rc = _lib.lib().nh_gzip_model_file(data, len(data), os.fsencode(path), C.byref(opts), stats)
        assert rc == 0, _lib.lib().nh_last_error().decode()
        with open(path, "rb") as f:
            raw = f.read()
    finally:
        os.unlink(path)
    st = dict(zip(STAT_NAMES, (int(v) for v in stats)))
    assert st["file_bytes"] == len(raw) and st["regions"] == cap
    return raw, st, [int(v) for v in sizes[:cap]]


def _inflates_to(stream, want):
    """the deflate stream at the head of `stream` (more may follow it) starts with the text `want`"""
    try:
        return zlib.decompressobj(-15).decompress(stream, max(1, len(want))) == want
    except zlib.error:
        return False


def assert_equals_model(raw, data, name, variant="", **opts):
    """the encoder's file `raw` for the text `data` == the model's, byte for byte.  On a mismatch the message names the input, the
    variant, the region, the first differing offset inside its stream and whether the two streams inflate to the same text."""
    want, st, sizes = model(data, **opts)
    if raw == want:
        return st
    m = min(len(raw), len(want))
    diff = np.flatnonzero(np.frombuffer(raw, dtype=np.uint8, count=m) != np.frombuffer(want, dtype=np.uint8, count=m))
    at = int(diff[0]) if len(diff) else m
    bgzf = opts.get("bgzf", False)
    region_len = BGZF_REGION if bgzf else min(max(opts.get("region", 65536), 4096), 65536) & ~63
    chunk = opts.get("chunk", 128 << 20)
    chunk -= chunk % region_len if bgzf else 0
    where = "the framing behind the last region"
    pos = 0 if bgzf else 10
    texts = []
    for c0 in range(0, len(data), chunk):
        c1 = min(len(data), c0 + chunk)
        texts += [(a, min(c1, a + region_len)) for a in range(c0, c1, region_len)]
    for r, size in enumerate(sizes):
        lo = pos + (18 if bgzf else 0)
        hi = lo + size + (8 if bgzf else 0)
        if at < hi:
            t0, t1 = texts[r]
            part = "member header" if at < lo else "stream" if at < lo + size else "member trailer"
            same = _inflates_to(want[lo:lo + size], data[t0:t1]) and _inflates_to(raw[lo:], data[t0:t1])
            where = ("region %d of %d (text bytes %d..%d), %s, offset %d of the model's %d stream bytes; both streams inflate to the "
                     "region's text: %s" % (r, len(sizes), t0, t1, part, at - lo, size, "yes" if same else "NO"))
            break
        pos = hi
    raise AssertionError("GPU encoder != host model on input %r, variant %r %r: files of %d / %d bytes part at byte %d: %s"
                         % (name, variant, opts, len(raw), len(want), at, where))


# ---- the texts ----------------------------------------------------------------------------------------------------------------
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _rand(rng, n, k=256):
    return rng.integers(0, k, n, dtype=np.uint8).tobytes()


def fastq_text(n_reads, seed):
    """the suite's short-read text (tests/test_gpu_deflate.py has the same generator)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_reads):
        seq = "".join("ACGT"[c] for c in rng.integers(0, 4, 150))
        q = np.where(rng.random(150) < 0.06, ord(":"), ord("F")).astype(np.uint8)
        cut = int(150 * (0.3 + 0.7 * rng.random() ** 0.4))
        q[cut:] = rng.choice(np.frombuffer(b"F:,#", dtype=np.uint8), 150 - cut)
        out.append("@NH1:7:HGF2YDSXX:1:%d:%d:%d 1:N:0:GATTACAG\n%s\n+\n%s\n"
                   % (1101 + i // 5000, 10000 + int(rng.integers(0, 25000)), 10000 + (i * 17) // 10, seq, q.tobytes().decode()))
    return "".join(out).encode()


def _sized(kind, n):
    if kind == "fastq":
        text = fastq_text(n // 300 + 1, n)
        return (text * (n // len(text) + 1))[:n]
    if kind == "random":
        return _rand(np.random.default_rng(n), n)
    return b"G" * n


def _repeats(lane):
    """every length x period: a unit of `period` bytes, then `length` more bytes of its repetition starting at `lane` of a step (a
    match of that length at that distance, begun where the lazy rule looks at the next step or cannot), then a byte that ends it.
    Steps are 64 positions from the region's start and regions are multiples of 64, so the offset in the text decides the lane."""
    rng = _rng("repeats%d" % lane)
    out = bytearray()
    for length in LENGTHS:
        for period in PERIODS:
            out += _rand(rng, 70)
            out += _rand(rng, (lane - len(out) - period) % 64)  # the repetition starts at `lane`
            unit = bytearray(_rand(rng, period))
            if period > 1 and unit[0] == unit[-1]:
                unit[-1] ^= 0x55
            out += unit
            assert len(out) % 64 == lane
            out += (bytes(unit) * (length // period + 1))[:length]
            out.append(unit[length % period] ^ 0xFF)  # the match ends here
    return bytes(out)


def _cut_by_region_end():
    """a 258-byte match that would cross the end of a region: cut at 4096 (the small regions) and at 65536"""
    rng = _rng("cut")
    out = bytearray(_rand(rng, 65536 + 4096))
    for end in (4096, 65536):
        unit = _rand(rng, 300)
        out[end - 700:end - 400] = unit
        out[end - 200:end + 100] = unit   # 200 bytes of it before the end, 100 behind
    return bytes(out)


def _distance(d):
    """200 random bytes seen again d bytes on, inside one 64 KiB region; the bytes between are one run, which lives in a single
    hash bucket and leaves the unit's entries where they are"""
    rng = _rng("distance")
    unit = _rand(rng, 200)
    return b"\0" * 128 + unit + b"\0" * (d - 200) + unit + b"\0" * 333


def _distance_across_regions():
    unit = _rand(_rng("across"), 200)
    return b"\0" * (65536 - 300) + unit + b"\0" * 200 + unit + b"\0" * 333   # the second copy lies in region 1: no candidate


def _bucket_pressure():
    """Twelve earlier positions with the same 5-byte context, one per step, each followed by a different number of the query's next
    bytes: the slot (step % ways) decides which survive, so 4, 6 and 8 ways find matches of different lengths (the candidate that
    agrees for 30 bytes is kept by 8 ways only, the one for 25 by 6 and 8, the one for 20 by all)."""
    rng = _rng("bucket")
    agree = [5, 6, 7, 8, 9, 30, 10, 25, 11, 12, 20, 13]   # by step; the query comes in step 12
    out = bytearray()
    for rep in range(24):
        ctx, tail = _rand(rng, 5), _rand(rng, 40)
        out += _rand(rng, (10 - len(out)) % 64)
        for k in agree:
            cell = bytearray(ctx + tail[:k] + bytes([tail[k] ^ 0xFF]))
            out += cell + _rand(rng, 64 - len(cell))
        out += ctx + tail + _rand(rng, 64 - 45)
    return bytes(out)


def _steep_counts():
    """Eighteen symbols with counts 1, 2, 3, 5, 9, ... (a factor of 1.75): an unrestricted code of more than 15 bits, so the limit has
    to be repaired.  The five most frequent are A C G T N, which set 1 prices at 2 bits -- no match among them pays, and the counts of
    the one block the text makes (31594 bytes, at the default region) stay as steep as written."""
    rng = _rng("steep")
    syms = list(range(97, 97 + 13)) + [ord(c) for c in "NTGCA"]
    return bytes(rng.permutation(np.concatenate([np.full(max(1, round(1.75 ** i)), s, dtype=np.uint8) for i, s in enumerate(syms)])))


def _all_values_equally_often():
    rng = _rng("ties")
    return b"".join(bytes(rng.permutation(256).astype(np.uint8)) for _ in range(100))


def _de_bruijn(k, n):
    """every n-gram over k symbols exactly once: a text that shrinks (few symbols) and holds no match"""
    a = [0] * k * n
    seq = []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return bytes(65 + s for s in seq)


def _skewed_code_lengths():
    """3000 bytes over a skewed alphabet (a draw of the kind the suite's mixtures make, picked with the model): one dynamic block whose
    header uses a few code lengths very often and many once -- a code-length code deeper than 7 bits before the repair"""
    rng = np.random.default_rng(11)
    p = np.cumsum(rng.random(256) ** 4)
    return np.searchsorted(p / p[-1], rng.random(3000)).astype(np.uint8).tobytes()


def reads_with_qualities(kind, n, seed):
    """FASTQ whose qualities decide which starting price set is smaller (tests/test_gpu_deflate.py has the same generator)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        L = 150
        seq = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), L))
        if kind == "forty":
            base = 38 - np.linspace(0, 12, L) * rng.random()
            q = np.clip(base + rng.normal(0, 3, L) + np.cumsum(rng.normal(0, 0.6, L)), 2, 41).astype(np.uint8) + 33
        elif kind == "spread":
            q = np.clip(rng.normal(20, 7, L), 1, 50).astype(np.uint8) + 33
        else:
            bins = np.array([2, 6, 15, 22, 27, 33, 37, 40], dtype=np.uint8)
            idx = np.clip((7 - np.linspace(0, 3, L) * rng.random() + rng.normal(0, 0.8, L)).round(), 0, 7).astype(int)
            q = bins[idx] + 33
        out.append(b"@SRR1234567.%d %d/1\n%s\n+\n%s\n" % (i + 1, i + 1, seq, q.tobytes()))
    return b"".join(out)


def _pilot_tie(region):
    """sixteen regions without A C G T N -- the two price sets give the same sizes there, a tie, and set 1 goes on -- then reads,
    whose regions start from the chosen set's prices"""
    lines = b"".join(b"%d\t%d\n" % (i, i * i) for i in range(16 * region // 12 + 1))
    return lines[:16 * region] + fastq_text(region // 300 + 30, region)[:region + 5000]


@functools.lru_cache(maxsize=None)
def pin_set():
    """-> ((name, text), ...), built once per process and never changed"""
    from tests.test_gpu_deflate import _mixture   # (the suite's random mixtures, as they are)
    pins = []
    for n in SIZES:
        for kind in ("fastq", "random", "run"):
            pins.append(("size_%d_%s" % (n, kind), _sized(kind, n)))
    for lane in (0, 62, 63):
        pins.append(("repeats_from_lane_%d" % lane, _repeats(lane)))
    pins.append(("match_cut_by_region_end", _cut_by_region_end()))
    for d in (32767, 32768, 32769):
        pins.append(("distance_%d" % d, _distance(d)))
    pins.append(("distance_across_regions", _distance_across_regions()))
    pins.append(("bucket_pressure", _bucket_pressure()))
    pins.append(("steep_counts", _steep_counts()))
    pins.append(("all_values_equally_often", _all_values_equally_often()))
    pins.append(("one_distinct_byte", b"A" * 40000))
    pins.append(("no_match", _de_bruijn(16, 3)))
    pins.append(("almost_only_matches", _rand(_rng("unit"), 37) * 1000))
    pins.append(("skewed_code_lengths", _skewed_code_lengths()))
    for kind in ("bins", "forty", "spread"):
        text = reads_with_qualities(kind, 250, 31)
        for regions in (15, 16, 17):   # the pilot looks at 16 regions: one fewer, exactly, one more (at NOHUMAN_GZIP_REGION=4096)
            pins.append(("pilot_%s_%d_regions" % (kind, regions), text[:4096 * regions - 7]))
    pins.append(("pilot_tie_small_regions", _pilot_tie(4096)))
    pins.append(("pilot_tie", _pilot_tie(65536)))   # (1.1 MB: sixteen regions of the default size take that much)
    for seed in range(4):
        pins.append(("mixture_%d" % seed, _mixture(seed)))
    assert len(dict(pins)) == len(pins)
    return tuple(pins)
