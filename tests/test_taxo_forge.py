"""tests/taxo_forge.py on the CPU: the generators, minidb.Taxonomy.lca against lca_by_sets on every tree the GPU cases use, and
what every input of test_gpu_build_db_deep.py, test_gpu_taxa_lists.py and test_gpu_taxon_out_deep.py promises: seeds without two
minimizers of one compacted key, the nodes the expected values cover, exact counts of distinct taxa per read, the calls of the
read pool."""
import itertools

import numpy as np
import pytest

from oracle import minidb
from oracle import oracle as orc
from tests import build_db_util as u
from tests import build_taxa_util as t
from tests import synth
from tests import taxo_forge as tf
from tests import taxout_model as tm

TREES = {
    "toy": lambda: {c: p for c, p in synth.TOY_EDGES.items() if p},
    "caterpillar16": lambda: tf.caterpillar(16)[0],
    "caterpillar60": lambda: tf.caterpillar(60)[0],
    "caterpillar200": lambda: tf.caterpillar(200)[0],
    "random1000": lambda: tf.random_tree(1000, tf.SHUFFLED_SEED)[0],
    "flat2100": lambda: {100 + i: 1 for i in range(tf.FLAT_LEAVES)},
    "heap4094": lambda: tf.heap(4094)[0],
    "heap4095": lambda: tf.heap(4095)[0],
}


# ---- the generators

def test_caterpillar():
    parent, lines = tf.caterpillar(60)
    assert len(parent) == 120 and len(lines) == 120 and parent[tf.C(1)] == 1
    anc = tf.ancestor_sets(parent)
    assert len(anc[tf.L(60)]) == 62 and len(anc[tf.C(60)]) == 61 and anc[tf.L(1)] == {1, tf.C(1), tf.L(1)}
    tax = t.taxonomy_of(lines)
    assert tax.node_count == 122
    assert all(tax.parent[i] < i for i in range(2, tax.node_count))  # the BFS rule: what "the larger id walks up" stands on


def test_random_tree():
    parent, lines = tf.random_tree(1000, tf.SHUFFLED_SEED)
    assert sorted(parent) == list(range(2, 1002)) and [ln[0] for ln in lines] != sorted(parent)
    assert (parent, lines) == tf.random_tree(1000, tf.SHUFFLED_SEED)
    smaller = sum(1 for c, p in parent.items() if c < p)
    assert 300 < smaller < 700  # the external ids say nothing about the tree
    tax = t.taxonomy_of(lines)
    assert all(tax.parent[i] < i for i in range(2, tax.node_count))
    assert max(len(a) for a in tf.ancestor_sets(parent).values()) >= 10  # (deeper than anything the toy trees have)
    assert sum(1 for ln in lines[1:] if ln[1] != 1 and [x[0] for x in lines].index(ln[1]) > lines.index(ln)) > 100  # children first


def test_heap_is_the_tree_of_the_manifest_tests():
    for n in (4094, 4095):
        parent, lines = tf.heap(n)
        assert lines == tuple((10 + i, 1 if i == 0 else 10 + (i - 1) // 2, "taxon %d" % (10 + i)) for i in range(n))
        assert len(tf.ancestor_sets(parent)[10 + n - 1]) == 13  # the root, taxon 0 and eleven more
    assert minidb.value_bits_for(4094 + 2) == 12 and minidb.value_bits_for(4095 + 2) == 13


def test_lca_by_sets_by_hand():
    parent = {c: p for c, p in synth.TOY_EDGES.items() if p}
    for taxa, want in (((111, 112), 11), ((111, 12), 10), ((111, 21), 1), ((111, 11), 11), ((111,), 111), ((111, 112, 12), 10),
                       ((21, 9606, 20), 20), ((1, 111), 1)):
        assert tf.lca_by_sets(parent, taxa) == want, taxa
        assert tf.lca_by_sets(parent, reversed(taxa)) == want


@pytest.mark.parametrize("name", sorted(TREES))
def test_minidb_lca_is_lca_by_sets(name):
    """all pairs of nodes; a random sample of 20 000 pairs for the two trees of more than 4000 nodes"""
    parent = TREES[name]()
    tax = minidb.Taxonomy(tf.edges_of(parent))
    anc = tf.ancestor_sets(parent)
    nodes = sorted(anc)
    if len(nodes) <= 2200:
        pairs = itertools.combinations_with_replacement(nodes, 2)
    else:
        rng = np.random.default_rng(len(nodes))
        pairs = [(nodes[int(a)], nodes[int(b)]) for a, b in rng.integers(0, len(nodes), size=(20000, 2))]
    internal, external, lca = tax.internal, tax.external, tax.lca
    n = 0
    for a, b in pairs:
        want = tf.lca_by_sets(parent, (a, b), anc)
        assert external[lca(internal[a], internal[b])] == want == external[lca(internal[b], internal[a])], (a, b)
        n += 1
    assert n >= min(20000, len(nodes) * (len(nodes) + 1) // 2)


# ---- the build cases

@pytest.mark.parametrize("name", sorted(tf.BUILD_CASES))
def test_build_case_has_no_shared_key_and_its_model_holds_the_lcas(name):
    c = tf.BUILD_CASES[name]()
    t.assert_order_free(c["tax"], c["pairs"], c["cap"], forward=(c["model"], c["size"]))
    tf.assert_cells_are_the_lcas(u.cells_of(c["model"])[1], c)
    assert c["size"] == len(c["mins"]) == len(tf.owners(c))


def _merged(c):
    """(owners, expected value) of the minimizers that more than one taxon holds"""
    own, ev = tf.owners(c), tf.expected_values(c)
    return [(o, ev[m]) for m, o in own.items() if len(o) > 1]


def test_deep_case():
    c = tf.deep_case()
    assert c["tax"].node_count == 122 and minidb.value_bits_for(122) == 7
    assert len(c["pairs"]) == 72 and all(150 <= len(s) <= 330 for _, s in c["pairs"])
    merged = _merged(c)
    values = {v for _, v in merged}
    assert len(values) >= 20 and tf.C(1) in values, sorted(values)
    assert any(v in o for o, v in merged)                       # the ancestor is a party itself
    assert any(len(o) == 3 for o, _ in merged)                  # the triple
    assert any(v not in o and tf.C(40) in o for o, v in merged)  # a chain node below the leaf's
    # the cuts of batch = 997 put more than one taxon into a batch and carry sequences over
    assert sum(len(s) for _, s in c["pairs"]) > 10 * 997


def test_race_case():
    c = tf.race_case()
    assert c["tax"].node_count == 34
    subsets = c["subsets"]
    assert len(subsets) == 40 and set(subsets[0]) == set(c["parent"]) and all(2 <= len(s) <= 32 == len(c["parent"]) for s in subsets)
    assert all(len(set(s)) == len(s) for s in subsets)
    assert sum((len(s) - 34 + 63) // 64 for _, s in c["pairs"]) > 1000  # pieces of 64 k-mers, a wave each
    assert max(len(s) for s in subsets[1:]) > 25 and sum(1 for s in subsets if len(s) > 3) > 20
    ev = tf.expected_values(c)
    seen = set()
    for j, mins in enumerate(c["by_record"]):
        assert mins and not (mins & seen)
        seen |= mins
        want = tf.lca_by_sets(c["parent"], subsets[j])
        assert {ev[m] for m in mins} == {want}, j
    assert seen == set(ev)
    assert len(set(ev.values())) >= 8, sorted(set(ev.values()))


def test_shuffled_case():
    c = tf.shuffled_case()
    assert c["tax"].node_count == 1002 and minidb.value_bits_for(1002) == 10
    assert len(c["records"]) == 40 and len(c["groups"]) == 10
    merged = _merged(c)
    assert len({frozenset(o) for o, _ in merged}) >= 10 and any(len(o) == 3 for o, _ in merged)
    assert sum(1 for o, v in merged if v not in o and v != 1) >= 3  # inner nodes without sequences of their own


@pytest.mark.parametrize("n,bits", [(4094, (20, 12)), (4095, (19, 13))])
def test_top_case(n, bits):
    c = tf.top_case(n)
    tax = c["tax"]
    vb = minidb.value_bits_for(tax.node_count)
    assert (32 - vb, vb) == bits and tax.node_count == n + 2
    last = c["last"]
    assert tax.internal[last] == tax.node_count - 1 == (4095 if n == 4094 else 4096)  # the last entry of a table of 2^12; the first id of 13 bits
    assert [tax.internal[x] for x in (last - 1, last - 2)] == [tax.node_count - 2, tax.node_count - 3]
    for x in (last, last - 1, last - 2, c["parent"][last], 10):
        assert x in c["records"]
    assert len(c["records"]) == 12 and all(len(s) == 60 for _, s in c["pairs"])
    merged = _merged(c)
    assert {frozenset(o) for o, _ in merged} == {frozenset(s) for s in c["shared"]}
    assert {v for o, v in merged if 10 in o} == {10}
    steps, x = 0, tax.internal[last]
    while x != tax.internal[10]:
        x, steps = tax.parent[x], steps + 1
    assert steps == 11  # the walk from the largest id up to taxon 0
    counts = t.value_counts(u.cells_of(c["model"])[1], vb, tax.node_count)
    assert counts[-1] > 0 and counts[tax.internal[10]] > 0


# ---- the taxon lists

FLAT_N = (63, 64, 65, 66, 2047, 2048, 2049)


def test_flat_reads_hit_exactly_n_distinct_taxa():
    db = tf.flat_db()
    odb = tf.oracle_of(db)
    assert db["tax"].node_count == 2102
    for n in FLAT_N + (2100,):
        read = tf.flat_read(n)
        assert len(read) == 45 * n
        _, _, taxa, _ = odb.classify(*orc.pack_reads([read], False), False, 0.0, want_taxa=True)
        d = tf.distinct_taxa(taxa)
        assert len(d) == n and 1 not in d and d == {db["tax"].internal[e] for e in db["leaves"][:n]}, n
        if n > 2000:  # as a pair: no read of the pair is long enough for the split items alone
            pair = (tf.flat_read(0, 1024), tf.flat_read(1024, n))
            _, _, taxa, _ = odb.classify(*orc.pack_reads([pair], True), True, 0.0, want_taxa=True)
            assert len(tf.distinct_taxa(taxa)) == n
    assert len(tf.flat_read(2047)) > 2000  # alone it is a batch of long reads: the library takes the split items
    short = tf.flat_short_reads()
    exp, _ = odb.classify(*orc.pack_reads(short, False), False, 0.0)
    assert len(short) == 200 and 100 < int((exp["call"] != 0).sum()) < 200


def test_chain_reads():
    db = tf.chain_db()
    odb = tf.oracle_of(db)
    tax = db["tax"]
    assert tax.node_count == 402
    inner = {tax.internal[tf.C(i)] for i in range(1, tf.CHAIN_DEPTH + 1)}
    for paired in (False, True):
        reads = db["reads"][paired]
        assert len(reads) == 240
        bases, offs = orc.pack_reads(reads, paired)
        exp, _, taxa, toff = odb.classify(bases, offs, paired, 0.0, want_taxa=True)
        for i in range(db["n_long"]):
            assert len(tf.distinct_taxa(taxa[int(toff[i]):int(toff[i + 1])])) > 64, i
        exp3, _ = odb.classify(bases, offs, paired, 0.3)
        calls = {int(x) for x in exp3["call"][:db["n_long"]]}
        assert calls & inner, calls
        assert len({int(x) for x in exp["call"][:db["n_long"]]}) > 5


# ---- the reads of the per-taxon outputs on the deep database

def _deep_oracle():
    c = tf.deep_case()
    return tf.oracle_of(dict(opts=minidb.opts_bytes(), taxo=c["tax"].to_bytes(), hash=c["model"]))


def test_deep_reads_are_called_where_lca_by_sets_says():
    c = tf.deep_case()
    reads = tf.deep_reads()
    assert 1400 <= len(reads) <= 1600 and len({n for n, _, _, _ in reads}) == len(reads)
    odb = _deep_oracle()
    ext = c["tax"].external
    anc = tf.ancestor_sets(c["parent"])
    for n, r, m, want in reads:
        assert tf.lca_by_sets(c["parent"], tf.holders(c, r), anc) == want == tf.lca_by_sets(c["parent"], tf.holders(c, m), anc), n
    assert not any(tf.DEEP_NO_READS in tf.holders(c, r) | tf.holders(c, m) for _, r, m, _ in reads)
    exp, _ = odb.classify(*orc.pack_reads([r for _, r, _, _ in reads], False), False, 0.0)
    assert [ext[int(x)] for x in exp["call"]] == [w for _, _, _, w in reads]
    exp, _ = odb.classify(*orc.pack_reads([(r, m) for _, r, m, _ in reads], True), True, 0.0)
    assert [ext[int(x)] for x in exp["call"]] == [w for _, _, _, w in reads]


def test_deep_selectors():
    c = tf.deep_case()
    calls = [w for _, _, _, w in tf.deep_reads()]
    parent = tf.edges_of(c["parent"])
    for sel in (tf.DEEP_SEL_NESTED, tf.DEEP_SEL_EIGHT):
        assert len(sel) == 8 and len(set(sel)) == 8
    got = tm.route_calls(calls, parent, tf.DEEP_SEL_NESTED)
    counts = [len(g) for g in got]
    assert counts[6] == 0 and all(n > 0 for i, n in enumerate(counts) if i != 6) and sum(counts) == len(calls), counts
    at12 = [i for i, w in enumerate(calls) if w == tf.C(12)]
    assert at12 and set(at12) <= set(got[1])  # a read called at C_12 lands in C_10's file
    anc = tf.ancestor_sets(c["parent"])
    assert anc[tf.L(41)] > anc[tf.C(40)] > anc[tf.C(20)] > anc[tf.C(10)] > anc[tf.C(5)]  # four selectors deep, and a fifth
    counts8 = [len(g) for g in tm.route_calls(calls, parent, tf.DEEP_SEL_EIGHT)]
    assert all(counts8) and sum(counts8) < len(calls), counts8
    (bottom,) = tm.route_calls(calls, parent, tf.DEEP_SEL_BOTTOM)
    assert 0 < len(bottom) < 60
