"""Hash images that aim at the classifier's probe loops (nh_kernels.hip: probe_queue, probe_queue_quad, the double-hashing
loop, the BIG second pass), a model of CompactHashTable::Get that says what every look-up does on such an image, and the
cases of tests/test_gpu_probe_variants.py.  tests/test_table_forge.py asserts on the CPU what every table and read set here
promises.  Host code, numpy only; everything is made once a process (functools.lru_cache) from committed seeds and never
changed.

  random_cells   `capacity` random cells, a fraction `fill` of them occupied: tiny and full tables
  comb           filler everywhere but for one stop every `period` cells: look-ups run from their home to the next stop, so
                 run lengths are uniform, from every position in a 128-byte line, and the last stretch wraps round the end
  probe_runs     per look-up: cells examined before the stop, home mod 32, cells to the table's end, wrapped, hit, and for
                 double hashing the length of the step's cycle and whether the look-up came back to its first cell
"""
from __future__ import annotations

import functools
import math
import struct

import numpy as np

from oracle import minidb
from tests import build_db_util as u
from tests import synth

VB_RANDOM = 26  # value bits of the random tables: 6 key bits, unrelated minimizers match by chance all the time
VB_COMB = 8     # value bits of the comb tables: 24 key bits, so a key that no minimizer has exists

RUN_DTYPE = np.dtype([("run", "<i8"), ("res32", "<i8"), ("to_end", "<i8"), ("wrapped", "?"), ("hit", "?"),
                      ("cycle", "<i8"), ("returned", "?"), ("step", "<i8")])


def fmix64(x) -> np.ndarray:
    """kv_store.h MurmurHash3 finalizer over an array of 64-bit values"""
    x = np.array(x, dtype=np.uint64, copy=True).reshape(-1)
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xFF51AFD7ED558CCD)
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xC4CEB9FE1A85EC53)
    x ^= x >> np.uint64(33)
    return x


def image(cells: np.ndarray, value_bits: int) -> bytes:
    """hash.k2d image of `cells`: capacity, size (cells with a value), key bits, value bits, the cells"""
    cells = np.ascontiguousarray(cells, dtype=np.uint32)
    size = int(np.count_nonzero(cells & np.uint32((1 << value_bits) - 1)))
    return struct.pack("<4Q", cells.size, size, 32 - value_bits, value_bits) + cells.tobytes()


def cells_of(hashb: bytes):
    """(cells, value_bits) of a hash image"""
    cap, _, _, vb = struct.unpack_from("<4Q", hashb, 0)
    return np.frombuffer(hashb, dtype=np.uint32, count=cap, offset=32), int(vb)


def random_cells(rng, capacity, fill, value_bits, n_values) -> bytes:
    """hash image of `capacity` random cells (values 1 .. n_values), a fraction `fill` of them occupied"""
    cells = np.zeros(capacity, dtype=np.uint32)
    occ = rng.random(capacity) < fill if fill < 1.0 else np.ones(capacity, bool)
    keys = rng.integers(0, 1 << (32 - value_bits), size=capacity, dtype=np.uint32)
    vals = rng.integers(1, n_values + 1, size=capacity, dtype=np.uint32)
    cells[occ] = ((keys[occ] << np.uint32(value_bits)) | vals[occ]).astype(np.uint32)
    return image(cells, value_bits)


def _looked_up(db, minimizers):
    """the minimizers that make a look-up (the min-hash cut drops the others before the table is touched)"""
    m = np.asarray(minimizers, dtype=np.uint64).reshape(-1)
    if db.min_hash:
        m = m[fmix64(m) >= np.uint64(db.min_hash)]
    return m


def comb_stops(capacity, period):
    """cells of the comb's stops: one every `period` cells, placed so that half a period of cells lies behind the last of
    them: the stretch before the first stop begins there and wraps round the table's end"""
    return np.arange((capacity - 1 - period // 2) % period, capacity, period)


def comb(db, minimizers, capacity, period, value_bits=VB_COMB, n_values=9) -> bytes:
    """A table that is all filler (a non-zero value under a compacted key that none of `minimizers` has) except for one stop
    every `period` cells.  Stops alternate between a cell with the key of a minimizer whose home lies in the stretch before
    it -- the one most often looked up there -- and an empty cell.  A look-up runs from its home to the next stop; if that
    stop holds another minimizer's key it runs on to the empty stop behind it: hits and misses at the end of runs of
    0 .. 2 * period - 1 cells.  The FIRST stop is planted for a minimizer whose home lies behind the last stop and before the
    table's end, so a hit is found after a wrap (a ValueError if `minimizers` has none there).  `minimizers`: one entry a
    look-up, repeats and all."""
    uniq, counts = np.unique(_looked_up(db, minimizers), return_counts=True)
    hc = fmix64(uniq)
    home = (hc % np.uint64(capacity)).astype(np.int64)
    key = (hc >> np.uint64(32 + value_bits)).astype(np.int64)
    used = set(key.tolist())
    filler = next(k for k in range(1 << (32 - value_bits)) if k not in used)
    stops = comb_stops(capacity, period)
    if stops.size < 2:
        raise ValueError("a comb needs two stops at least: one of them empty")
    cells = ((filler << value_bits) | (1 + np.arange(capacity) % n_values)).astype(np.uint32)
    for i, s in enumerate(stops):
        cells[s] = 0
        if i % 2:
            continue
        inside = (home > stops[i - 1]) & (home <= s) if i else home > stops[-1]
        if not inside.any():
            if i == 0:
                raise ValueError("no minimizer has its home behind the last stop: no hit after a wrap")
            continue  # (an empty stop more)
        j = np.nonzero(inside)[0]
        j = int(j[np.argmax(counts[j])])
        cells[s] = (int(key[j]) << value_bits) | (1 + (i // 2) % n_values)
    return image(cells, value_bits)


def probe_runs(db, minimizers, linear=True) -> np.ndarray:
    """CompactHashTable::Get (compact_hash.cc) for every look-up of `minimizers` on the table of `db` (k2_literal.DB), as
    a record of RUN_DTYPE each: run = cells examined before the one that stopped the look-up (every cell seen, if none
    did); res32 = home mod 32; to_end = cells from the home to the table's end; wrapped = the look-up went on past the
    table's end; hit; and for double hashing cycle = capacity / gcd(step mod capacity, capacity), step = step mod capacity,
    returned = the look-up ended by coming back to its first cell (linear probing: after a whole table without a stop)."""
    m = _looked_up(db, minimizers)
    uniq, inv = np.unique(m, return_inverse=True)
    cells = np.asarray(db.cells, dtype=np.uint32)
    cap, vb = int(db.capacity), int(db.value_bits)
    assert cells.size == cap
    empty = (cells & np.uint32((1 << vb) - 1)) == 0
    keys = (cells >> np.uint32(vb)).astype(np.int64)
    hc = fmix64(uniq)
    out = np.zeros(uniq.size, dtype=RUN_DTYPE)
    for i, h in enumerate(hc.tolist()):
        home = h % cap
        step = 1 % cap if linear else ((h >> 8) | 1) % cap
        cycle = cap // math.gcd(step, cap)  # (gcd(0, cap) = cap: a step of 0 sees one cell)
        order = (home + step * np.arange(cycle, dtype=np.int64)) % cap
        stop = empty[order] | (keys[order] == (h >> (32 + vb)))
        n = int(np.argmax(stop)) if stop.any() else cycle
        r = out[i]
        r["run"], r["res32"], r["to_end"], r["cycle"], r["step"] = n, home % 32, cap - home, cycle, step
        r["returned"] = not stop.any()
        r["hit"] = bool(stop.any() and not empty[order[n]])
        seen = order[:min(n + 1, cycle)]
        r["wrapped"] = bool(r["returned"] or (seen[1:] < seen[:-1]).any())
    return out[inv]


# run lengths (cells examined before the stop) that every comb must show, where the period allows them: around one 16-byte
# load (4 cells), around the 16 cells of a wide round, around a 128-byte line (32 cells)
RUN_LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33)
LONG_RUN = 40


def comb_gaps(runs, period):
    """The classes of look-up that a comb of `period` is there for and that `runs` (probe_runs) does not show; [] is what
    tests/test_table_forge.py asserts.  Run lengths: those of RUN_LENGTHS below the period, which a look-up that stops at the
    first stop it meets can have; and one of LONG_RUN cells or more where a run can be that long at all: a look-up passes a
    stop that holds another minimizer's key and ends at the empty stop behind it, so runs reach 2 * period - 1 cells
    (3 * period - 1 across the table's end, where two planted stops may follow each other): 14 cells on a comb of period 5,
    73 and more on the others."""
    have = set(np.unique(runs["run"]).tolist())
    gaps = ["run length %d" % n for n in RUN_LENGTHS if n < period and n not in have]
    if 2 * period - 1 >= LONG_RUN and not (runs["run"] >= LONG_RUN).any():
        gaps.append("a run of %d cells or more" % LONG_RUN)
    residues = set(np.unique(runs["res32"]).tolist())
    gaps += ["home at cell %d of a line" % r for r in range(32) if r not in residues]
    for r in (29, 30, 31):
        if not ((runs["res32"] == r) & (runs["run"] >= 4)).any():
            gaps.append("a run of 4 cells or more from cell %d of a line" % r)
    if not ((runs["to_end"] < 16) & (runs["run"] > runs["to_end"])).any():
        gaps.append("a run longer than the cells left before the table's end, fewer than 16 of them")
    if not (runs["wrapped"] & runs["hit"]).any():
        gaps.append("a hit after a wrap")
    if not (runs["wrapped"] & ~runs["hit"]).any():
        gaps.append("a miss after a wrap")
    if runs["hit"].mean() < 0.2:
        gaps.append("hits in a fifth of the look-ups (%.3f)" % runs["hit"].mean())
    if runs["returned"].any():
        gaps.append("every look-up ends at a stop")
    return gaps


# ---- reads ---------------------------------------------------------------------------------------------------------------
def tandem_pool(rng, units, length):
    """one sequence of `length` bases per entry of `units`: a random unit of that many bases, repeated.  Reads cut from
    them share a handful of minimizers, so the minimizers a comb plants are looked up again and again."""
    return [(synth.random_seq(rng, n) * (length // n + 1))[:length] for n in units]


def pool_reads(rng, pool, lengths, cold=0.15):
    """a read of each length: cut from a sequence of `pool` (either strand), or, a fraction `cold` of them, random"""
    reads = []
    for ln in lengths:
        ln = int(ln)
        if rng.random() < cold:
            reads.append(synth.random_seq(rng, ln))
            continue
        src = pool[int(rng.integers(0, len(pool)))]
        st = int(rng.integers(0, len(src) - ln))
        s = src[st:st + ln]
        reads.append(synth.revcomp(s) if rng.random() < 0.5 else s)
    return reads


def pairs_of(reads):
    """the reads as pairs: (0, 1), (2, 3) ..."""
    return list(zip(reads[0::2], reads[1::2]))


def lookup_minimizers(odb, reads, paired=False):
    """the minimizer of every look-up ClassifySequence makes for `reads` (one a run of equal minimizers, a mate starts
    afresh; the min-hash cut is left to the caller), by the scanner of oracle/k2_oracle.c"""
    out = []
    for frag in reads:
        for seq in (frag if paired else (frag,)):
            mins, amb = odb.scan(seq)
            mins = mins[amb == 0]
            if mins.size:
                out.append(mins[np.concatenate(([True], mins[1:] != mins[:-1]))])
    return np.concatenate(out) if out else np.zeros(0, np.uint64)


# ---- the cases of tests/test_gpu_probe_variants.py -------------------------------------------------------------------------
RANDOM_CAPS = (1, 2, 3, 5, 15, 16, 17, 31, 32, 33, 100, 257)
COMPOSITE_CAPS = (96, 255, 256)  # double hashing only: steps that share a factor with the capacity
FILLS = (0.5, 0.95, 1.0)
COMBS = ((5, 331), (37, 1000), (70, 4099), (131, 2003))  # (period, capacity)
SHAPES = ["cells%d" % c for c in RANDOM_CAPS] + ["comb%d_%d" % pc for pc in COMBS]
DOUBLE_SHAPES = SHAPES + ["cells%d" % c for c in COMPOSITE_CAPS]

GEOMS = {"default": {}, "k31l31": dict(k=31, l=31), "k40l25": dict(k=40, l=25, spaced_mask=0),
         "revcom0": dict(revcom_version=0), "minhash": dict(min_hash=1 << 62)}
PER_LANE = ("k31l31", "k40l25", "revcom0", "minhash")

TQ = 124                     # k-mers per tile at k=35, l=31
SEG_KMERS = 32 * TQ          # k-mers per segment of a cut read
SPLIT_MIN_TILES = 48         # reads of more tiles than this are cut (nh_device.h)
SEG_CAP = 64                 # NOHUMAN_SEG_CAP of the segment cases: room for every segment of their reads

# read classes: name -> (lengths drawn from [lo, hi), how many, lengths added by hand)
CLASSES = {
    "generic": (159, 421, 296, (159, 160, 316, 317)),              # more than one tile each: the generic kernel
    "short": (35, 159, 296, (35, 36, 157, 158)),                   # one tile each: k_classify_short
    "mixed": (20, 560, 290, (0, 1, 30, 34, 35, 39, 40, 158, 159, 531)),  # from below k to four tiles
    "segments": (1000, 3001, 40, (6100, 6500, 7200, 8100, 9000, 12500)),  # the last six are cut: 2 .. 4 segments
}
# seeds of the read sets: chosen so that all four combs built from a set show every class of comb_gaps
# (test_table_forge.py asserts it)
SEEDS = {("default", "generic"): 2, ("default", "short"): 19, ("default", "segments"): 2, ("default", "mixed"): 2,
         ("k31l31", "mixed"): 1, ("k40l25", "mixed"): 1, ("revcom0", "mixed"): 2, ("minhash", "mixed"): 2}
# bases of the pool's repeated units: some twenty distinct minimizers in all under each geometry's window of k - l + 1 l-mers
# (a comb of 15 stops plants 8 of them, and these must make a fifth of all look-ups)
POOL_UNITS = {"default": (17, 19, 23), "revcom0": (17, 19, 23), "minhash": (17, 19, 23), "k31l31": (5, 7, 9),
              "k40l25": (53, 59, 61)}
COLD = 0.1  # share of random reads: the look-ups that cover every run length and every position in a line


def opts_of(geom):
    return minidb.opts_bytes(**GEOMS[geom])


@functools.lru_cache(maxsize=None)
def toy_taxo():
    return synth.toy_db()[1]


@functools.lru_cache(maxsize=None)
def reads_of(cls, geom="default"):
    lo, hi, n, extra = CLASSES[cls]
    rng = np.random.default_rng(SEEDS[geom, cls])
    pool = tandem_pool(rng, POOL_UNITS[geom], max(hi, max(extra)) + 64)
    lengths = list(rng.integers(lo, hi, size=n)) + list(extra)
    reads = pool_reads(rng, pool, lengths, COLD)
    order = rng.permutation(len(reads))
    return tuple(reads[int(i)] for i in order)


def scanner(geom, taxo=None):
    """an oracle of the geometry with a table of one empty cell: for its scanner"""
    from oracle import oracle as orc
    odb = orc.OracleDB(opts_of(geom), taxo or toy_taxo(), image(np.zeros(1, np.uint32), VB_COMB))
    odb.set(ambiguity_rule=u.rule())
    return odb


@functools.lru_cache(maxsize=None)
def minimizers_of(geom, cls):
    """one entry a look-up of the class's reads, single-end (the pairs are the same sequences, two a fragment)"""
    odb = scanner(geom)
    try:
        return lookup_minimizers(odb, reads_of(cls, geom))
    finally:
        odb.close()


class _Geom:
    def __init__(self, geom):
        self.min_hash = GEOMS[geom].get("min_hash", 0)


@functools.lru_cache(maxsize=None)
def table(shape, fill, geom="default", cls="generic", n_values=9):
    """the hash image of a shape: cells<capacity> at `fill` (the same for every geometry and class), or comb<period>_<capacity>
    built from the look-ups of the class's reads under the geometry (`fill` is ignored)"""
    if shape.startswith("cells"):
        cap = int(shape[5:])
        rng = np.random.default_rng(1000 * cap + int(fill * 100) + 7 * n_values)
        return random_cells(rng, cap, fill, VB_RANDOM, n_values)
    period, cap = (int(x) for x in shape[4:].split("_"))
    return comb(_Geom(geom), minimizers_of(geom, cls), cap, period, VB_COMB, n_values)


def tables(shape, geom="default", cls="generic"):
    """[(name, image)]: the three fills of a cells shape, or the one comb"""
    if shape.startswith("cells"):
        return [("%s fill %.2f" % (shape, f), table(shape, f)) for f in FILLS]
    return [(shape, table(shape, 0.0, geom, cls))]


def cut_reads(reads, k=35, tq=TQ):
    """(reads that k_prep_items cuts, segments they make): more than SPLIT_MIN_TILES tiles, 32 tiles a segment"""
    n_cut = n_seg = 0
    for r in reads:
        nt = (max(len(r) - k + 1, 0) + tq - 1) // tq
        if nt > SPLIT_MIN_TILES:
            n_cut += 1
            n_seg += (nt + 31) // 32
    return n_cut, n_seg


# ---- many taxa: the second pass ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def many_taxonomy():
    """the tree of test_more_than_64_distinct_taxa_take_the_second_pass: 150 leaves under 10 genera under the root"""
    edges = {1: 0}
    for g in range(10):
        edges[100 + g] = 1
    for i in range(150):
        edges[1000 + i] = 100 + i % 10
    return minidb.Taxonomy(edges)


MANY_TABLES = (("cells1000", 0.95), ("cells257", 1.0))


def many_table(shape, fill):
    """random cells with values over every node of many_taxonomy()"""
    return table(shape, fill, n_values=many_taxonomy().node_count - 1)


@functools.lru_cache(maxsize=None)
def many_reads(long_reads=False):
    """random reads: 40 of 600 .. 1500 bases (some 160 to 500 look-ups, most of them chance hits: more than 64 distinct
    taxa), 60 of 35 .. 300 that stay below; long_reads: 6 more that are cut, with more than 30 distinct taxa a segment"""
    rng = np.random.default_rng(15)
    lens = list(rng.integers(600, 1501, size=40)) + list(rng.integers(35, 301, size=60))
    if long_reads:
        lens += [6100, 6600, 7300, 8200, 9100, 12400]
    reads = [synth.random_seq(rng, int(n)) for n in lens]
    order = rng.permutation(len(reads))
    return tuple(reads[int(i)] for i in order)


# ---- which tables go under which path: shared by the GPU file and by the CPU checks of tests/test_table_forge.py ----------
LINEAR_CASES = (("default", "generic"), ("default", "short"), ("default", "segments")) + tuple((g, "mixed") for g in PER_LANE)
DOUBLE_GEOMS = ("default", "k31l31")  # double hashing, class "mixed"
# second pass: (path, geometry, linear probing, paired too, long_reads)
MANY_CASES = (("generic", "default", True, True, False), ("segments", "default", True, False, True),
              ("per_lane", "k31l31", True, True, False), ("double", "default", False, True, False))
