"""What the tests of nh_build_db share: FASTA writers, the Python model of a one-taxon build (oracle/minidb.py) and readers of a
database directory.  The model's genomes stay small (tens of kilobases): kmer_minimizers is pure Python."""
from __future__ import annotations

import gzip
import math
import os
import struct

import numpy as np

from oracle import k2_literal as lit
from oracle import minidb
from tests import synth

DB_FILES = ("hash.k2d", "opts.k2d", "taxo.k2d")
VALUE_BITS = 2  # three nodes: null, root, the taxon


def rule() -> int:
    """the ambiguity rule in force as a plain index (0 = last l-mer, 1 = queue): the engine's default unless
    NOHUMAN_OPT_AMBIGUITY_RULE overrides it, as the library reads it"""
    v = os.environ.get("NOHUMAN_OPT_AMBIGUITY_RULE")
    if v is None:
        return 1
    try:
        return int(int(v.strip() or 0) != 0)
    except ValueError:
        return 0


def fasta_text(records, width=60, crlf=False) -> bytes:
    """records: (id, sequence bytes); width 0: one line a sequence"""
    nl = b"\r\n" if crlf else b"\n"
    out = bytearray()
    for name, seq in records:
        out += b">" + name + nl
        if width:
            for i in range(0, len(seq), width):
                out += seq[i:i + width] + nl
        elif seq:
            out += seq + nl
    return bytes(out)


def write_fasta(path, records, width=60, crlf=False, gz=False) -> str:
    text = fasta_text(records, width, crlf)
    with open(path, "wb") as f:
        f.write(gzip.compress(text, 6) if gz else text)
    return str(path)


def taxonomy(taxid=9606, name="Homo sapiens"):
    return minidb.Taxonomy({1: 0, taxid: 1}, {1: "root", taxid: name})


def _shim(capacity=1):
    return lit.DB(minidb.DEFAULT_K, minidb.DEFAULT_L, minidb.default_spaced_mask(), minidb.DEFAULT_TOGGLE, 1, 0, 1, capacity, 0,
                  32 - VALUE_BITS, VALUE_BITS, [], [0, 0, 1], [0, 1, 9606], ambiguity_rule=rule())


def minimizers(seqs):
    """(distinct minimizers of the non-ambiguous k-mers, k-mers, ambiguous k-mers) of the sequences under the rule in force"""
    db = _shim()
    out, kmers, amb = set(), 0, 0
    for s in seqs:
        for a, m in lit.kmer_minimizers(db, s):
            kmers += 1
            if a:
                amb += 1
            else:
                out.add(m)
    return out, kmers, amb


def default_capacity(n_distinct, load_factor=0.7) -> int:
    return int(math.ceil(n_distinct / load_factor))


def model_hash(seqs, capacity, taxid=9606):
    """minidb.build_hash of the sequences under one taxon -> (hash.k2d bytes, size)"""
    return minidb.build_hash(taxonomy(taxid), [(taxid, s) for s in seqs], capacity, ambiguity_rule=rule())


def cells_of(hash_bytes):
    cap, size, kb, vb = struct.unpack_from("<4Q", hash_bytes, 0)
    cells = np.frombuffer(hash_bytes, dtype="<u4", offset=32)
    assert cells.size == cap
    return (cap, size, kb, vb), cells


def read_db(d):
    """a database directory -> ((capacity, size, key_bits, value_bits), cells, opts bytes, taxo bytes)"""
    with open(os.path.join(d, "hash.k2d"), "rb") as f:
        hdr, cells = cells_of(f.read())
    with open(os.path.join(d, "opts.k2d"), "rb") as f:
        ob = f.read()
    with open(os.path.join(d, "taxo.k2d"), "rb") as f:
        tb = f.read()
    return hdr, cells, ob, tb


def same_table(a, b):
    """two (header, cells): equal headers, the same occupied positions, the same sorted cell words.  Which key sits in which
    occupied cell depends on the order of insertion (as in kraken2's threaded build), so layouts are not compared."""
    (ha, ca), (hb, cb) = a, b
    assert ha == hb, (ha, hb)
    assert np.array_equal(ca != 0, cb != 0), "occupied positions differ"
    assert np.array_equal(np.sort(ca), np.sort(cb)), "sorted cells differ"


def order_free(seqs, capacity, mins=None):
    """asserts that the sorted cells of this input do not depend on the order of insertion -- forward against reversed records,
    and the condition behind it: no two distinct minimizers share a compacted key (then no order can merge two of them, and the
    occupied positions of linear probing never depend on the order) -- and returns (hash bytes, size, distinct minimizers)"""
    fwd, size = model_hash(seqs, capacity)
    rev, size_r = model_hash(list(reversed(seqs)), capacity)
    assert size == size_r and np.array_equal(np.sort(cells_of(fwd)[1]), np.sort(cells_of(rev)[1]))
    if mins is None:
        mins, _, _ = minimizers(seqs)
    keys = {lit.fmix64(m) >> (32 + VALUE_BITS) for m in mins}
    assert len(keys) == len(mins) == size, "two minimizers share a compacted key: choose another seed.  (An input that shares " \
        "keys on purpose has no order-free table to compare with: hold it to build_forge.valid_table instead.)"
    return fwd, size, mins


def genome(seed, n_seq=8, length=2500):
    """about 20 kb of iid ACGT in n_seq records, with lowercase stretches, a few single N and one N run"""
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n_seq):
        s = bytearray(synth.random_seq(rng, length + int(rng.integers(0, 100))))
        lo = int(rng.integers(0, length - 300))
        s[lo:lo + 200] = bytes(s[lo:lo + 200]).lower()
        for p in rng.integers(0, length, size=2):
            s[int(p)] = ord("N")
        if i == 3:
            s[1000:1090] = b"N" * 90
        recs.append((b"chr%d some description" % (i + 1), bytes(s)))
    return recs


def border_records(P, seed=11):
    """inputs made to break a cut into pieces of P k-mers (piece p = bases [p P, p P + P + 34))"""
    rng = np.random.default_rng(seed)
    rs = lambda n: synth.random_seq(rng, n)  # noqa: E731
    recs = [(b"len%d" % n, rs(n)) for n in (0, 34, 35, 36, P + 33, P + 34, P + 35, 2 * P + 34)]
    # single N: one at every offset -36 .. +36 around some piece border (borders every P bases; every second one is used)
    s = bytearray(rs(2 * P * 75))
    for j, off in enumerate(range(-36, 37)):
        s[2 * P * (j + 1) + off] = ord("N")
    recs.append((b"single_n", bytes(s)))
    recs.append((b"n_run", rs(P + 50) + b"N" * (3 * P + 10) + rs(2 * P + 7)))
    recs.append((b"all_n", b"N" * (2 * P + 40)))
    low = bytearray(rs(3 * P + 60))
    low[P - 20:P + 50] = bytes(low[P - 20:P + 50]).lower()
    low[2 * P + 30:] = bytes(low[2 * P + 30:]).lower()
    recs.append((b"lower", bytes(low)))
    return recs


def fast_minimizers(seqs):
    """the distinct minimizers of larger inputs, by the C oracle's scanner (oracle/k2_oracle.c) under the rule in force -> sorted
    uint64 array"""
    from oracle import oracle as orc
    ob, tb, hb, _, _ = synth.toy_db()  # (any database of the default geometry: only the scanner is used)
    odb = orc.OracleDB(ob, tb, hb)
    odb.set(ambiguity_rule=rule())
    parts = []
    for s in seqs:
        mins, amb = odb.scan(s)
        parts.append(mins[amb == 0])
    return np.unique(np.concatenate(parts)) if parts else np.zeros(0, np.uint64)


def fmix64_np(k):
    k = k.astype(np.uint64).copy()
    k ^= k >> np.uint64(33)
    k *= np.uint64(0xff51afd7ed558ccd)
    k ^= k >> np.uint64(33)
    k *= np.uint64(0xc4ceb9fe1a85ec53)
    k ^= k >> np.uint64(33)
    return k


def longest_run(cells) -> int:
    """the longest stretch of occupied cells, cyclic"""
    occ = np.concatenate([cells != 0, cells != 0]).astype(np.int8)
    edges = np.flatnonzero(np.diff(np.concatenate([[0], occ, [0]])))
    return int(min((edges[1::2] - edges[::2]).max(initial=0), cells.size))


def assert_order_free_fast(mins, capacity, apart=1024):
    """the condition of order_free for larger inputs: minimizers that share a compacted key have home cells at least `apart`
    cells from each other; with every run of occupied cells shorter than that (longest_run of the table built) no probe path
    holds two of them"""
    hc = fmix64_np(mins)
    ck = hc >> np.uint64(32 + VALUE_BITS)
    home = (hc % np.uint64(capacity)).astype(np.int64)
    order = np.argsort(ck, kind="stable")
    ck, home = ck[order], home[order]
    same = np.nonzero(ck[1:] == ck[:-1])[0]
    for i in same:
        d = abs(int(home[i + 1]) - int(home[i]))
        assert min(d, capacity - d) >= apart, "two minimizers share a compacted key and a probe path: choose another seed"
    return len(same)
