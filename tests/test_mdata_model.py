"""tests/mdata_model.py against brute force on the toy database, its invariants, and a hand-made case with the numbers written
out.  CPU only."""
import numpy as np
import pytest

from oracle import k2_literal as lit
from oracle import minidb
from tests import mdata_model as mm
from tests import synth


@pytest.fixture(scope="module")
def toy_lit(toy):
    ob, tb, hb, _, _ = toy
    return lit.DB.from_images(ob, tb, hb)


def _fragments(toy, n=120, paired=False, seed=3):
    rng = np.random.default_rng(seed)
    reads = synth.sample_reads(rng, toy[3], n, paired=paired, len_jitter=40)
    return [tuple(r) if paired else (r,) for r in reads]


def _brute(db, fragments):
    """no run logic: every non-ambiguous k-mer's minimizer looked up by a walk of the table written here"""
    vmask = (1 << db.value_bits) - 1
    where = {}  # minimizer -> (value, cell) or None
    cells, groups = set(), np.zeros(len(db.parent), dtype=np.uint64)
    for mates in fragments:
        prev = None
        for seq in mates:
            if db.reset_per_mate:
                prev = None
            for amb, m in lit.kmer_minimizers(db, seq):
                if amb:
                    continue
                if m not in where:
                    hc = lit.fmix64(m)
                    hit = None
                    for d in range(db.capacity):
                        c = (hc + d) % db.capacity
                        if db.cells[c] & vmask == 0:
                            break
                        if db.cells[c] >> db.value_bits == hc >> (32 + db.value_bits):
                            hit = (db.cells[c] & vmask, c)
                            break
                    where[m] = hit
                if where[m] is not None:
                    cells.add(where[m][1])
                    if m != prev:
                        groups[where[m][0]] += np.uint64(1)
                prev = m
    return groups, cells


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("reset", [True, False])
def test_model_against_brute_force(toy, toy_lit, paired, reset):
    toy_lit.reset_per_mate = reset
    try:
        frags = _fragments(toy, paired=paired)
        groups, marked, per_fragment = mm.scan(toy_lit, frags)
        want_groups, want_cells = _brute(toy_lit, frags)
        assert marked == want_cells and np.array_equal(groups, want_groups)
        # the classifier's own hit groups, fragment by fragment
        assert per_fragment == [lit.classify_fragment(toy_lit, list(f), 0.0)[3] for f in frags]
        assert int(groups.sum()) > 500 and len(marked) > 300
    finally:
        toy_lit.reset_per_mate = True


def test_the_c_scanner_gives_the_same_numbers(toy, toy_lit, toy_oracle):
    """mm.c_scanner, which the run tests use for thousands of reads, against lit.kmer_minimizers, under both ambiguity rules"""
    frags = _fragments(toy, 60, paired=True, seed=8)
    try:
        for rule in (0, 1):
            toy_lit.ambiguity_rule = rule
            toy_oracle.set(ambiguity_rule=rule)
            slow, fast = mm.scan(toy_lit, frags), mm.scan(toy_lit, frags, mm.c_scanner(toy_oracle))
            assert np.array_equal(slow[0], fast[0]) and slow[1] == fast[1] and slow[2] == fast[2]
            assert any(b"N" in m for f in frags for m in f)
    finally:
        toy_lit.ambiguity_rule = lit.DB.ambiguity_rule
        toy_oracle.set(ambiguity_rule=lit.DB.ambiguity_rule)


def test_invariants(toy, toy_lit):
    frags = _fragments(toy, 200, paired=True, seed=4)
    calls = [lit.classify_fragment(toy_lit, list(f), 0.0)[0] for f in frags]
    num = mm.numbers(toy_lit, frags, calls)
    assert int(num["minimizers_own"].sum()) == sum(num["per_fragment"])
    assert (num["distinct_own"] <= np.minimum(num["minimizers_own"], num["db_cells_own"])).all()
    assert int(num["db_cells_own"].sum()) == toy_lit.size
    for q in ("reads", "minimizers", "distinct", "db_cells"):
        assert int(num[q + "_clade"][1]) == int(num[q + "_own"].sum())  # the root's clade is everything
    assert int(num["distinct_own"].sum()) == len(num["marked"])
    words = mm.bitmap(toy_lit, num["marked"])
    assert words.size == (4001 + 31) // 32 and int(sum(bin(int(w)).count("1") for w in words)) == len(num["marked"])
    assert int(words[-1]) >> (4001 - 32 * (words.size - 1)) == 0


# ---- a hand-made case: two taxa under the root; B's genome starts with the first 50 bases of A's
A_SEQ = b"GATTACAGGCTTAACCGTGCATGGAACCTTAGCGATCGGATACCATGCAAGTCCGATTGACCAGTAGGCATCAGTTCAAGG"
B_OWN = b"TTGACCGGATAACTGGCCATTAGACCGTTAGCAACGGTCAT"


@pytest.fixture(scope="module")
def hand():
    tax = minidb.Taxonomy({1: 0, 5: 1, 6: 1}, {1: "root", 5: "taxon A", 6: "taxon B"})
    genomes = [(5, A_SEQ), (6, A_SEQ[:50] + B_OWN)]
    hashb, size = minidb.build_hash(tax, genomes, 101, ambiguity_rule=1)
    db = lit.DB.from_images(minidb.opts_bytes(), tax.to_bytes(), hashb)
    db.ambiguity_rule = 1
    return db, tax, size


def test_hand_made_case(hand):
    db, tax, size = hand
    frags = [(A_SEQ,), (A_SEQ,), (A_SEQ[:50] + B_OWN,), (A_SEQ[:45],), (b"ACGT" * 20,), (A_SEQ[:40] + b"N" + A_SEQ[41:],)]
    calls = [lit.classify_fragment(db, list(f), 0.0)[0] for f in frags]
    num = mm.numbers(db, frags, calls)
    got = {f: [int(x) for x in num[f]] for f in mm.FIELDS}
    # nodes: 0 the sentinel, 1 root, 2 taxon A (5), 3 taxon B (6).  The shared 50 bases' minimizers sit under the root.
    assert size == sum(got["db_cells_own"]) == got["db_cells_clade"][1]
    want = HAND_NUMBERS
    assert got == want, got
    assert num["per_fragment"] == HAND_GROUPS and calls == HAND_CALLS
    names = mm.names_of(tax.to_bytes())
    assert mm.table(db, names, num) == HAND_TABLE
    assert mm.report(db, names, num, len(frags)) == HAND_REPORT
    assert mm.drop_minimizer_columns(HAND_REPORT) == mm.report(db, names, num, len(frags), minimizer_data=False)


# The first 50 bases of A_SEQ hold 16 k-mers with 7 distinct minimizers: both genomes have them, so their 7 cells hold the root.
# A's other 31 k-mers have 11 minimizers, B's 41 have 14: 32 cells.  A_SEQ read whole is 7 + 11 = 18 hit groups (no minimizer comes
# back once it has left), B's genome 7 + 14 = 21, the first 45 bases 5 (of the root's), a read without a hit 0, and A_SEQ with an N
# at base 40 keeps 4 of the root's groups in front of the N and A's last 3 behind it.
HAND_GROUPS = [18, 18, 21, 5, 0, 7]
HAND_CALLS = [2, 2, 3, 1, 0, 2]
HAND_NUMBERS = {
    "reads_clade": [0, 5, 3, 1], "reads_own": [0, 1, 3, 1],
    "minimizers_clade": [0, 69, 25, 14], "minimizers_own": [0, 7 + 7 + 7 + 5 + 4, 11 + 11 + 3, 14],
    "distinct_clade": [0, 32, 11, 14], "distinct_own": [0, 7, 11, 14],
    "db_cells_clade": [0, 32, 11, 14], "db_cells_own": [0, 7, 11, 14],
}
HAND_TABLE = mm.HEADER + "1\troot\t5\t1\t69\t30\t32\t7\t32\t7\t100.0000\n" \
    "5\ttaxon A\t3\t3\t25\t25\t11\t11\t11\t11\t100.0000\n6\ttaxon B\t1\t1\t14\t14\t14\t14\t14\t14\t100.0000\n"
HAND_REPORT = " 16.67\t1\t1\t0\t0\tU\t0\tunclassified\n 83.33\t5\t1\t69\t32\tR\t1\troot\n" \
    " 50.00\t3\t3\t25\t11\tR1\t5\t  taxon A\n 16.67\t1\t1\t14\t14\tR1\t6\t  taxon B\n"
