"""What the tests of a build of several taxa (nh_build_args.taxa_file) share: manifest writers, the inputs of the GPU tests with
their Python model (oracle/minidb.py: build_hash stores a minimizer of two taxa as their lowest common ancestor), readers of
taxo.k2d and raw ctypes calls.  The inputs are made once a process (functools.lru_cache) and never changed."""
from __future__ import annotations

import ctypes as C
import functools
import os
import struct

import numpy as np

from oracle import minidb
from tests import build_db_util as u
from tests import build_forge as bf
from tests import synth

NO_DEVICE = 1 << 20  # a device id no machine has
# external ids of the tree of the GPU tests: A and B under the inner node G under the root, C under the root
A, B, C_, G = 10, 20, 30, 100
TREE_LINES = ((G, 1, "group G"), (A, G, "taxon A"), (B, G, "taxon B"), (C_, 1, "taxon C"))
# seeds of the genomes: chosen so that no two distinct minimizers of a case share a compacted key (test_build_taxa_model.py
# asserts it for every case, on the CPU)
TREE_SEEDS = {A: 501, B: 502, C_: 503, G: 504, "stretches": 505}
RACE_SEED = 4001
BORDER_SEED = 2001
WIDE_SEED = 3004


def manifest_text(lines, crlf=False) -> bytes:
    """lines: (taxid, parent taxid, name, paths...) tuples, or bytes / str taken as they are"""
    nl = "\r\n" if crlf else "\n"
    out = []
    for ln in lines:
        if isinstance(ln, bytes):
            ln = ln.decode()
        out.append(ln if isinstance(ln, str) else "\t".join(str(f) for f in ln))
    return (nl.join(out) + nl).encode()


def write_manifest(path, lines, crlf=False) -> str:
    with open(path, "wb") as f:
        f.write(manifest_text(lines, crlf))
    return str(path)


def taxonomy_of(lines) -> minidb.Taxonomy:
    """the model's taxonomy of manifest lines (taxid, parent, name, ...): the root is implicit"""
    edges, names = {1: 0}, {1: "root"}
    for taxid, parent, name, *_ in lines:
        edges[taxid] = parent
        names[taxid] = name
    return minidb.Taxonomy(edges, names)


def model(tax, pairs, capacity):
    """minidb.build_hash of (external taxid, sequence) pairs under the ambiguity rule in force -> (hash.k2d bytes, size)"""
    return minidb.build_hash(tax, pairs, capacity, ambiguity_rule=u.rule())


def interleaved(pairs):
    """the pairs with the taxa taking turns: the first of every taxon, then the second of every taxon, ..."""
    by = {}
    for t, s in pairs:
        by.setdefault(t, []).append(s)
    out, i = [], 0
    while any(i < len(v) for v in by.values()):
        out += [(t, v[i]) for t, v in by.items() if i < len(v)]
        i += 1
    assert sorted(out) == sorted(pairs)
    return out


def assert_order_free(tax, pairs, capacity, forward=None):
    """the model's table of the pairs forward, reversed and interleaved: the same occupied positions and sorted cells; and the
    condition behind it, no two distinct minimizers with one compacted key at the database's key_bits.  forward: the model's
    (hash bytes, size) of the pairs as they are, where it is there already -> (hash bytes, size)"""
    vb = minidb.value_bits_for(tax.node_count)
    fwd, size = forward if forward is not None else model(tax, pairs, capacity)
    for other in (list(reversed(pairs)), interleaved(pairs)):
        blob, size_o = model(tax, other, capacity)
        assert size_o == size
        u.same_table(u.cells_of(fwd), u.cells_of(blob))
    mins = u.fast_minimizers([s for _, s in pairs])
    keys = np.unique(u.fmix64_np(mins) >> np.uint64(32 + vb))
    assert len(keys) == len(mins) == size, "two minimizers share a compacted key at %d key bits: choose another seed" % (32 - vb)
    return fwd, size


def value_counts(cells, vb, node_count):
    """cells of a table per value, as a list by internal id"""
    occ = cells[cells != 0]
    return np.bincount((occ & np.uint32((1 << vb) - 1)).astype(np.int64), minlength=node_count).tolist()


def parse_taxo(tb):
    """taxo.k2d -> a list of nodes (parent, first child, child count, external id, name)"""
    assert tb[:8] == b"K2TAXDAT"
    n, name_len, rank_len = struct.unpack_from("<3Q", tb, 8)
    names = tb[32 + 56 * n:32 + 56 * n + name_len]
    ranks = tb[32 + 56 * n + name_len:]
    assert len(ranks) == rank_len and ranks == b"no rank\0"
    out = []
    for i in range(n):
        parent, first, count, name_off, rank_off, ext, god = struct.unpack_from("<7Q", tb, 32 + 56 * i)
        assert rank_off == 0 and god == 0
        out.append((parent, first, count, ext, names[name_off:names.index(b"\0", name_off)].decode()))
    return out


def model_nodes(tax):
    """what parse_taxo gives for the model's taxonomy (the sentinel's name is the root's in the library's file)"""
    out = parse_taxo(tax.to_bytes())
    return [out[0][:4] + ("root",)] + out[1:]


def per_taxon(pairs, tax):
    """sequences, bases and k-mers per internal id of the (taxid, sequence) pairs"""
    out = [[0, 0, 0] for _ in range(tax.node_count)]
    for t, s in pairs:
        o = out[tax.internal[t]]
        o[0] += 1
        o[1] += len(s)
        o[2] += max(0, len(s) - 34)
    return [tuple(o) for o in out]


def write_case(tmp, lines, records, name="taxa.tsv", width=60):
    """one FASTA per taxon with records (relative paths in the manifest) -> the manifest's path"""
    out = []
    for taxid, parent, tname in lines:
        recs = records.get(taxid)
        if recs is None:
            out.append((taxid, parent, tname))
        else:
            u.write_fasta(os.path.join(str(tmp), "t%d.fa" % taxid), recs, width=width)
            out.append((taxid, parent, tname, "t%d.fa" % taxid))
    return write_manifest(os.path.join(str(tmp), name), out)


def pairs_of(tax, records):
    """(taxid, sequence) in the order the library reads them: by internal id, a file's records in order"""
    return [(t, s) for t in tax.external[2:] for _, s in records.get(t, [])]


def _planted(recs, i, at, stretch):
    n, s = recs[i]
    recs[i] = (n, s[:at] + stretch + s[at:])


@functools.lru_cache(maxsize=None)
def tree_case():
    """A, B under G under the root, C under the root; four 20 kb genomes; B shares a 3 kb stretch with A, C another with A and B,
    G (which carries sequences itself) a 1 kb stretch with A"""
    rng = np.random.default_rng(TREE_SEEDS["stretches"])
    ab, abc, ag = (synth.random_seq(rng, n) for n in (3000, 3000, 1000))
    records = {t: [(b"t%d_" % t + n, s) for n, s in u.genome(TREE_SEEDS[t])] for t in (A, B, C_, G)}
    _planted(records[A], 1, 700, ab), _planted(records[B], 2, 1200, ab)
    _planted(records[A], 4, 300, abc), _planted(records[B], 5, 2000, abc), _planted(records[C_], 0, 1500, abc)
    _planted(records[A], 6, 100, ag), _planted(records[G], 3, 400, ag)
    tax = taxonomy_of(TREE_LINES)
    assert tax.external == [0, 1, C_, G, A, B] and tax.node_count == 6 and minidb.value_bits_for(6) == 3
    pairs = pairs_of(tax, records)
    mins = u.fast_minimizers([s for _, s in pairs])
    cap = u.default_capacity(len(mins))
    blob, size = model(tax, pairs, cap)
    return dict(lines=TREE_LINES, tax=tax, records=records, pairs=pairs, mins=mins, cap=cap, model=blob, size=size,
                stretches=dict(ab=ab, abc=abc, ag=ag))


def race_records():
    """the one 20 kb genome that the race tests put under several taxa"""
    return u.genome(RACE_SEED)


@functools.lru_cache(maxsize=None)
def border_case():
    """the tree again, small: two records a taxon, a record shorter than 35 bases at the end of one taxon's file and at the start
    of the next one's, B with a stretch of A, C with a stretch of both"""
    rng = np.random.default_rng(BORDER_SEED)
    g = u.genome(BORDER_SEED)
    ab, abc = synth.random_seq(rng, 400), synth.random_seq(rng, 300)
    short = lambda i: (b"short%d" % i, synth.random_seq(rng, 20 + i))  # noqa: E731
    records = {
        C_: [g[0], (b"c2", g[1][1][:900] + abc + g[1][1][900:]), short(0)],
        G: [short(1), g[2], short(2)],
        A: [short(3), (b"a1", g[3][1][:500] + ab + g[3][1][500:]), (b"a2", abc + g[4][1]), short(4)],
        B: [short(5), (b"b1", g[5][1] + ab), (b"b2", g[6][1][:77] + abc + g[6][1][77:])],
    }
    tax = taxonomy_of(TREE_LINES)
    pairs = pairs_of(tax, records)
    mins = u.fast_minimizers([s for _, s in pairs])
    cap = u.default_capacity(len(mins))
    blob, size = model(tax, pairs, cap)
    return dict(lines=TREE_LINES, tax=tax, records=records, pairs=pairs, mins=mins, cap=cap, model=blob, size=size)


@functools.lru_cache(maxsize=None)
def wide_case(n=300):
    """n leaf taxa under the root, one 100-base record each; every tenth record shares its first 50 bases with its neighbour"""
    rng = np.random.default_rng(WIDE_SEED)
    lines = tuple((1000 + i, 1, "leaf %d" % i) for i in range(n))
    seqs = [synth.random_seq(rng, 100) for _ in range(n)]
    for i in range(0, n - 1, 10):
        seqs[i + 1] = seqs[i][:50] + seqs[i + 1][50:]
    records = {1000 + i: [(b"r%d" % i, seqs[i])] for i in range(n)}
    tax = taxonomy_of(lines)
    pairs = pairs_of(tax, records)
    mins = u.fast_minimizers([s for _, s in pairs])
    cap = u.default_capacity(len(mins))
    blob, size = model(tax, pairs, cap)
    return dict(lines=lines, tax=tax, records=records, pairs=pairs, mins=mins, cap=cap, model=blob, size=size)


def shared_key_case(capacity, seed=7):
    """build_forge.shared_key_records dealt to two taxa under the root so that the minimizers of one key take turns between the
    taxa (the others alternate as they come) -> (lines, taxonomy, [(taxid, name, record)] in file order, minimizers)"""
    from oracle import k2_literal as lit
    recs, mins = bf.shared_key_records(capacity, np.random.default_rng(seed))
    lines = ((7, 1, "seven"), (8, 1, "eight"))
    tax = taxonomy_of(lines)
    assert tax.node_count == 4 and minidb.value_bits_for(4) == u.VALUE_BITS
    keys = [lit.fmix64(m) >> bf.KEY_SHIFT for m in mins]
    seen, dealt = {}, []
    for i, ((n, s), k) in enumerate(zip(recs, keys)):
        j = seen.get(k, 0)
        seen[k] = j + 1
        dealt.append(((7, 8)[(j if keys.count(k) > 1 else i) % 2], n, s))
    for k in set(keys):
        if keys.count(k) > 1:
            assert {x for (x, _, _), kk in zip(dealt, keys) if kk == k} == {7, 8}
    return lines, tax, dealt, mins


def raw_args(taxa=None, out_dir=None, paths=(), struct_size=None, **kw):
    """nh_build_args of the present layout, every field settable; keeps what it points to alive -> (args, stats, keep)"""
    from nohuman_amd import _lib
    a = _lib.nh_build_args_v3()
    a.struct_size = C.sizeof(_lib.nh_build_args_v3) if struct_size is None else struct_size
    arr = (C.c_char_p * max(len(paths), 1))(*[os.fsencode(p) for p in paths])
    a.n_fasta = len(paths)
    if paths:
        a.fasta = arr
    a.taxa_file = None if taxa is None else os.fsencode(taxa)
    a.out_dir = None if out_dir is None else os.fsencode(out_dir)
    a.device = NO_DEVICE
    per = (_lib.nh_build_taxon_stats * 4096)()
    a.taxon_stats, a.taxon_stats_cap = per, 4096
    for k, v in kw.items():
        setattr(a, k, v)
    return a, _lib.nh_build_stats_v3(), (arr, per)


def raw_call(fn, *args, **kw):
    """nh_build_db or nh_build_check through ctypes -> (return code, message, stats, per-node array)"""
    from nohuman_amd import _lib
    a, s, (arr, per) = raw_args(*args, **kw)
    rc = getattr(_lib.lib(), fn)(C.byref(a), C.byref(s))
    return rc, _lib.lib().nh_last_error().decode(errors="replace"), s, per

