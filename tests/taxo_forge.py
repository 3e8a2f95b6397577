"""Large and deep taxonomies for the tests of everything that scales with the tree: generators of {external child: external
parent} maps with the manifest lines of build_taxa_util.write_case, a lowest common ancestor that compares no ids (lca_by_sets:
the reference of minidb.Taxonomy.lca and of the kernels, which all let "the larger id walk up"), and the inputs of the GPU cases
of test_gpu_build_db_deep.py, test_gpu_taxa_lists.py and test_gpu_taxon_out_deep.py.  tests/test_taxo_forge.py asserts on the CPU
what every one of these inputs promises.  Everything is made once a process (functools.lru_cache) from committed seeds and never
changed."""
from __future__ import annotations

import functools

import numpy as np

from oracle import minidb
from tests import build_db_util as u
from tests import build_taxa_util as t
from tests import synth

ROOT = 1
# seeds: chosen so that no two distinct minimizers of a case share a compacted key at the database's key_bits
# (test_taxo_forge.py asserts it for every case)
DEEP_SEED, RACE_SEED, SHUFFLED_SEED, TOP_SEED = 6101, 6204, 6301, 6401
FLAT_SEED, CHAIN_SEED, POOL_SEED = 1, 6501, 6601


def C(i):
    """external id of the caterpillar's chain node i (1 = the root's child)"""
    return 1000 + i


def L(i):
    """external id of the leaf under chain node i"""
    return 5000 + i


def lines_of(parent, order=None):
    """manifest lines (taxid, parent, name) of a parent map, in its own order or in `order`"""
    return tuple((c, parent[c], "taxon %d" % c) for c in (parent if order is None else order))


def caterpillar(depth):
    """a chain C_1 .. C_depth under the root and a leaf L_i under every C_i -> (parent map, manifest lines)"""
    parent = {}
    for i in range(1, depth + 1):
        parent[C(i)] = C(i - 1) if i > 1 else ROOT
        parent[L(i)] = C(i)
    return parent, lines_of(parent)


def random_tree(n, seed):
    """n taxa, each under one of the nodes made before it (the root among them); the external ids 2 .. n + 1 are dealt at random,
    so a child's id may be smaller than its parent's and only the BFS rule decides the internal ids; the manifest lines are in
    a random order too -> (parent map, manifest lines)"""
    rng = np.random.default_rng(seed)
    par = [0] + [int(rng.integers(0, k)) for k in range(1, n + 1)]  # node 0 is the root
    ext = [ROOT] + (rng.permutation(n) + 2).tolist()
    parent = {ext[k]: ext[par[k]] for k in range(1, n + 1)}
    return parent, lines_of(parent, [ext[int(k) + 1] for k in rng.permutation(n)])


def heap(n):
    """taxon i (external id 10 + i) under taxon (i - 1) // 2, taxon 0 under the root -> (parent map, manifest lines)"""
    parent = {10 + i: ROOT if i == 0 else 10 + (i - 1) // 2 for i in range(n)}
    return parent, lines_of(parent)


def ancestor_sets(parent):
    """{external id: the set of the node and all its ancestors} for every node of the map and the root"""
    out = {ROOT: frozenset([ROOT])}

    def of(x):
        chain = []
        while x not in out:
            chain.append(x)
            x = parent[x]
        for c in reversed(chain):
            out[c] = out[parent[c]] | {c}
        return out

    for x in parent:
        of(x)
    return out


def lca_by_sets(parent, taxa, anc=None):
    """the lowest common ancestor of a set of external ids from their ancestor sets: the common ancestor with the most ancestors
    of its own.  No id is compared with another.  anc: ancestor_sets(parent) where it is there already"""
    anc = anc if anc is not None else ancestor_sets(parent)
    taxa = list(taxa)
    common = frozenset.intersection(*[anc[x] for x in taxa])
    (best,) = [c for c in common if len(anc[c]) == len(common)]  # the common ancestors are a chain from the root
    return best


def edges_of(parent):
    """the parent map as minidb.Taxonomy and taxout_model take it: with the root"""
    out = {ROOT: 0}
    out.update(parent)
    return out


@functools.lru_cache(maxsize=None)
def _scanner():
    from oracle import oracle as orc
    ob, tb, hb, _, _ = synth.toy_db()  # (any database of the default geometry: only the scanner is used)
    odb = orc.OracleDB(ob, tb, hb)
    odb.set(ambiguity_rule=u.rule())
    return odb


def minimizers_of(seqs):
    """the distinct minimizers of the sequences' non-ambiguous k-mers (the C oracle's scanner) -> a set of ints"""
    out = set()
    for s in seqs:
        mins, amb = _scanner().scan(s)
        out.update(mins[amb == 0].tolist())
    return out


def owners(c):
    """{minimizer: the set of external taxids whose sequences hold it} of a case"""
    out = {}
    for taxid, recs in c["records"].items():
        for m in minimizers_of([s for _, s in recs]):
            out.setdefault(m, set()).add(taxid)
    return out


def expected_values(c):
    """{minimizer: external id of lca_by_sets of its owners}"""
    anc = ancestor_sets(c["parent"])
    return {m: lca_by_sets(c["parent"], o, anc) for m, o in owners(c).items()}


def expected_cells(c):
    """the sorted occupied cells of the case's table, from expected_values alone (no minidb.Taxonomy.lca, no build_hash)"""
    tax = c["tax"]
    vb = minidb.value_bits_for(tax.node_count)
    ev = expected_values(c)
    mins = np.array(sorted(ev), dtype=np.uint64)
    keys = (u.fmix64_np(mins) >> np.uint64(32 + vb)).astype(np.uint32)
    vals = np.array([tax.internal[ev[m]] for m in sorted(ev)], dtype=np.uint32)
    return np.sort((keys << np.uint32(vb)) | vals)


def assert_cells_are_the_lcas(cells, c):
    """every occupied cell of a table of the case against lca_by_sets of the taxa whose sequences hold its minimizer"""
    got, want = np.sort(cells[cells != 0]), expected_cells(c)
    assert got.size == want.size, (got.size, want.size)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "cells %s, lca_by_sets has %s" % (got[bad[:8]], want[bad[:8]])


def _case(parent, lines, records, **more):
    tax = t.taxonomy_of(lines)
    pairs = t.pairs_of(tax, records)
    mins = u.fast_minimizers([s for _, s in pairs])
    cap = u.default_capacity(len(mins))
    blob, size = t.model(tax, pairs, cap)
    return dict(more, parent=parent, lines=lines, tax=tax, records=records, pairs=pairs, mins=mins, cap=cap, model=blob, size=size)


# ---- build: the deep tree

DEEP = 60
# stretches of 60 bases and the taxa that share each: leaves with leaves, a leaf with an ancestor that carries sequences itself, a
# leaf with a chain node below its own, one triple
DEEP_LEAF_PAIRS = ((1, 60), (12, 30), (2, 3), (7, 50), (15, 16), (20, 45), (25, 26), (28, 59), (33, 34), (35, 52), (38, 39), (42, 58),
                   (44, 47), (48, 49), (51, 55), (53, 54), (56, 57), (4, 22), (6, 9), (10, 41), (13, 27), (17, 31), (18, 19), (23, 37))
DEEP_GROUPS = tuple((L(i), L(j)) for i, j in DEEP_LEAF_PAIRS) + (
    (L(30), C(10)), (L(60), C(5)), (L(11), C(10)),  # the ancestor is a party
    (L(3), C(40)), (L(14), C(20)), (L(44), C(45)),  # the chain node lies below the leaf's
    (L(8), L(21), C(35)))
DEEP_NO_READS = L(32)  # a leaf with a record that the read pool never draws from


@functools.lru_cache(maxsize=None)
def deep_case():
    """caterpillar(60): a record of 150 bases of its own for every leaf and every fifth chain node, the stretches of DEEP_GROUPS
    planted between pieces of at least 37 own bases.  spans: per taxon the (start, end, group index or None) of its record"""
    parent, lines = caterpillar(DEEP)
    rng = np.random.default_rng(DEEP_SEED)
    taxa = [L(i) for i in range(1, DEEP + 1)] + [C(j) for j in range(5, DEEP + 1, 5)]
    own = {x: synth.random_seq(rng, 150) for x in taxa}
    stretches = [synth.random_seq(rng, 60) for _ in DEEP_GROUPS]
    records, spans = {}, {}
    for x in taxa:
        mine = [g for g, parties in enumerate(DEEP_GROUPS) if x in parties]
        assert len(mine) <= 3
        cuts = [150 * k // (len(mine) + 1) for k in range(len(mine) + 2)]
        seq, sp = b"", []
        for k in range(len(mine) + 1):
            piece = own[x][cuts[k]:cuts[k + 1]]
            assert len(piece) >= 37
            sp.append((len(seq), len(seq) + len(piece), None))
            seq += piece
            if k < len(mine):
                sp.append((len(seq), len(seq) + 60, mine[k]))
                seq += stretches[mine[k]]
        records[x] = [(b"t%d" % x, seq)]
        spans[x] = sp
    return _case(parent, lines, records, spans=spans, stretches=stretches, taxa=taxa)


# ---- build: many taxa meet in one cell

RACE_DEPTH, RACE_RECORDS = 16, 40


@functools.lru_cache(maxsize=None)
def race_case():
    """caterpillar(16), 32 taxa: a 5 kb sequence cut into 40 records of 125 bases, record j in the FASTA of every taxon of a
    random subset S_j (2 to 32 taxa, the first all 32).  subsets: the S_j; by_record: the minimizers of record j"""
    parent, lines = caterpillar(RACE_DEPTH)
    rng = np.random.default_rng(RACE_SEED)
    taxa = list(parent)
    assert len(taxa) == 32
    genome = synth.random_seq(rng, 125 * RACE_RECORDS)
    recs = [(b"r%d" % j, genome[125 * j:125 * j + 125]) for j in range(RACE_RECORDS)]
    subsets = [tuple(taxa)]
    for j in range(1, RACE_RECORDS):
        # two in three are large and meet near the root; every third is small and drawn below chain node j // 3, so that the
        # expected values reach down the chain
        size = int(rng.integers(10, 33)) if j % 3 else int(rng.integers(2, 5))
        among = taxa if j % 3 else [C(i) for i in range(j // 3 + 1, RACE_DEPTH + 1)] + [L(i) for i in range(j // 3, RACE_DEPTH + 1)]
        subsets.append(tuple(int(x) for x in rng.choice(among, size=size, replace=False)))
    records = {x: [recs[j] for j in range(RACE_RECORDS) if x in subsets[j]] for x in taxa}
    records = {x: r for x, r in records.items() if r}
    return _case(parent, lines, records, subsets=subsets, by_record=[minimizers_of([s]) for _, s in recs])


# ---- build: external ids that say nothing about the tree

@functools.lru_cache(maxsize=None)
def shuffled_case():
    """random_tree(1000): 40 taxa with a record of 100 bases each, 10 stretches of 50 bases shared by two or three of them"""
    parent, lines = random_tree(1000, SHUFFLED_SEED)
    rng = np.random.default_rng(SHUFFLED_SEED + 1)
    taxa = [int(x) for x in rng.choice(sorted(parent), size=40, replace=False)]
    seqs = {x: synth.random_seq(rng, 100) for x in taxa}
    groups = []
    for g in range(10):
        parties = [int(x) for x in rng.choice(taxa, size=2 + g % 2, replace=False)]
        stretch = synth.random_seq(rng, 50)
        for x in parties:
            seqs[x] = seqs[x][:50] + stretch + seqs[x][50:]
        groups.append(tuple(parties))
    records = {x: [(b"s%d" % x, s)] for x, s in seqs.items()}
    return _case(parent, lines, records, groups=groups)


# ---- build: the top of the range

@functools.lru_cache(maxsize=None)
def top_case(n):
    """heap(n), n = 4094 or 4095: records of 60 bases of their own for 12 taxa -- the three last ones (the largest internal ids),
    the last one's parent, taxon 0 --, two more shared by the last taxon and taxon 0, two by the last two taxa"""
    parent, lines = heap(n)
    rng = np.random.default_rng(TOP_SEED + n)
    last = n - 1
    idx = [last, last - 1, last - 2, (last - 1) // 2, 0, 1, 2, 5, 100, 1000, 2047, 3000]
    assert len(set(idx)) == 12
    records = {10 + i: [(b"own%d" % i, synth.random_seq(rng, 60))] for i in idx}
    for k, parties in enumerate(((last, 0), (last, 0), (last, last - 1), (last, last - 1))):
        s = synth.random_seq(rng, 60)
        for i in parties:
            records[10 + i].append((b"shared%d" % k, s))
    return _case(parent, lines, records, last=10 + last, shared=((10 + last, 10), (10 + last, 10 + last - 1)))


BUILD_CASES = {"deep": deep_case, "race": race_case, "shuffled": shuffled_case, "top4094": lambda: top_case(4094),
               "top4095": lambda: top_case(4095)}


# ---- classify: the taxon lists

FLAT_LEAVES, FLAT_SEG, FLAT_CAPACITY = 2100, 45, 60013


def oracle_of(db):
    from oracle import oracle as orc
    odb = orc.OracleDB(db["opts"], db["taxo"], db["hash"])
    odb.set(ambiguity_rule=u.rule())
    return odb


@functools.lru_cache(maxsize=None)
def flat_db():
    """2100 leaves under the root, a segment of 45 bases each, built by minidb (value_bits 12)"""
    rng = np.random.default_rng(FLAT_SEED)
    leaves = [100 + i for i in range(FLAT_LEAVES)]
    tax = minidb.Taxonomy(edges_of({e: ROOT for e in leaves}))
    segs = [synth.random_seq(rng, FLAT_SEG) for _ in leaves]
    hashb, _ = minidb.build_hash(tax, list(zip(leaves, segs)), FLAT_CAPACITY, ambiguity_rule=u.rule())
    assert minidb.value_bits_for(tax.node_count) == 12
    return dict(opts=minidb.opts_bytes(), taxo=tax.to_bytes(), hash=hashb, tax=tax, segs=segs, leaves=leaves)


def flat_read(lo, hi=None):
    """the segments [lo, hi) joined; flat_read(N): the first N"""
    if hi is None:
        lo, hi = 0, lo
    return b"".join(flat_db()["segs"][lo:hi])


@functools.lru_cache(maxsize=None)
def flat_short_reads():
    """200 reads of 100 bases over the first 40 segments' neighbourhoods, a fifth of them random"""
    rng = np.random.default_rng(FLAT_SEED + 1)
    src = {i: flat_read(2 * i, 2 * i + 3) for i in range(20)}
    return synth.sample_reads(rng, src, 200, length=100, frac_random=0.2)


def distinct_taxa(taxa):
    """the distinct taxa among per-k-mer taxa (no hit, ambiguous and the mates' border left out)"""
    from oracle import oracle as orc
    return set(int(x) for x in np.unique(taxa)) - {0, orc.AMBIG, orc.BORDER}


CHAIN_DEPTH = 200


@functools.lru_cache(maxsize=None)
def chain_db():
    """caterpillar(200): a segment of 120 bases on every leaf and every fourth chain node; 40 long reads that visit 70 to 140 of
    these nodes and 200 short reads, single-end and as pairs"""
    parent, _ = caterpillar(CHAIN_DEPTH)
    rng = np.random.default_rng(CHAIN_SEED)
    tax = minidb.Taxonomy(edges_of(parent))
    nodes = [L(i) for i in range(1, CHAIN_DEPTH + 1)] + [C(j) for j in range(4, CHAIN_DEPTH + 1, 4)]
    segs = {e: synth.random_seq(rng, 120) for e in nodes}
    hashb, _ = minidb.build_hash(tax, sorted(segs.items()), 40009, ambiguity_rule=u.rule())

    def long_read():
        pick = rng.choice(nodes, size=int(rng.integers(70, 141)), replace=False)
        return b"".join(segs[int(e)][10:110] for e in pick)

    long_se = [long_read() for _ in range(40)]
    long_pe = [(long_read(), long_read()) for _ in range(40)]
    few = {e: segs[e] for e in nodes[:20] + nodes[-20:]}
    short_se = synth.sample_reads(rng, few, 200, length=100, frac_random=0.2)
    short_pe = synth.sample_reads(rng, few, 200, length=100, frac_random=0.2, paired=True)
    return dict(opts=minidb.opts_bytes(), taxo=tax.to_bytes(), hash=hashb, tax=tax, parent=parent, segs=segs,
                reads={False: long_se + short_se, True: long_pe + short_pe}, n_long=40)


# ---- per-taxon outputs: reads of the deep database

def _window(rng, seq, lo, hi, inside):
    """a window of the record: inside [lo, hi) where `inside`, else 55 to 70 bases that hold 35 bases of [lo, hi) in a row"""
    if inside:
        n = int(rng.integers(52, hi - lo + 1))
        at = int(rng.integers(lo, hi - n + 1))
        return seq[at:at + n]
    n = int(rng.integers(55, 71))
    p = int(rng.integers(lo, hi - 35 + 1))
    at = max(0, min(p - int(rng.integers(0, n - 35 + 1)), len(seq) - n))
    return seq[at:at + n]


@functools.lru_cache(maxsize=None)
def deep_reads():
    """about 1500 reads (and a mate for each, drawn in the same way from the same place) cut from the records of deep_case(): 16
    for every taxon that hold at least 35 bases in a row of what only this taxon has, 10 inside every shared stretch; none from
    the record of DEEP_NO_READS -> [(id, read, mate, the external taxid lca_by_sets gives for the taxa whose records hold it)]"""
    c = deep_case()
    rng = np.random.default_rng(POOL_SEED)
    anc = ancestor_sets(c["parent"])
    out = []
    assert all(y != DEEP_NO_READS for g in DEEP_GROUPS for y in g)
    for x in c["taxa"]:
        if x == DEEP_NO_READS:
            continue
        (_, seq), = c["records"][x]
        own = [(lo, hi) for lo, hi, g in c["spans"][x] if g is None]
        for i in range(16):
            lo, hi = own[i % len(own)]
            out.append((b"o%d_%d" % (x, i), _window(rng, seq, lo, hi, False), _window(rng, seq, lo, hi, False), x))
    for g, parties in enumerate(DEEP_GROUPS):
        s = c["stretches"][g]
        want = lca_by_sets(c["parent"], parties, anc)
        for i in range(10):
            out.append((b"s%d_%d" % (g, i), _window(rng, s, 0, 60, True), _window(rng, s, 0, 60, True), want))
    return [out[int(i)] for i in rng.permutation(len(out))]


def holders(c, read):
    """the external taxids whose records hold the read"""
    return {x for x, s in c["pairs"] if read in s}


# selector lists of the per-taxon outputs on the deep database
DEEP_SEL_NESTED = [C(5), C(10), C(20), C(40), L(10), L(41), DEEP_NO_READS, "other"]
DEEP_SEL_EIGHT = [C(5), C(10), C(20), C(40), L(10), L(41), C(30), L(2)]
DEEP_SEL_BOTTOM = [C(60)]
