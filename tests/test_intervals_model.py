"""tests/intervals_model.py, the specification of --host-intervals, against the oracle's own hit list: the bases the model calls
covered are the bases covered by the k-mers whose entry in oracle/k2_literal.classify_fragment's per-k-mer taxa is neither 0 nor
the ambiguous marker -- on the goldens' reads and the toy database, under both ambiguity rules, with reset_per_mate 0 and 1 (the
intervals depend on neither the call nor the carry across mates).  No GPU, nothing of the library."""
import os

import numpy as np
import pytest

from oracle import k2_literal as lit
from tests import intervals_model as im
from tests import synth
from tests.fastq_util import read_fastq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def gold_db():
    rd = lambda n: open(os.path.join(GOLD, "toy_db", n), "rb").read()
    return lit.DB.from_images(rd("opts.k2d"), rd("taxo.k2d"), rd("hash.k2d"))


def gold_fragments(paired):
    if not paired:
        return [(r[2],) for r in read_fastq(os.path.join(GOLD, "reads_se.fq"))]
    a, b = (read_fastq(os.path.join(GOLD, "reads_pe_%d.fq" % m)) for m in (1, 2))
    return [(x[2], y[2]) for x, y in zip(a, b)]


def split_taxa(db, taxa, mates):
    """the fragment's hit list cut into its mates' (the border entry dropped)"""
    out, at = [], 0
    for i, seq in enumerate(mates):
        nk = max(0, len(seq) - db.k + 1)
        out.append(taxa[at:at + nk])
        at += nk + (1 if len(mates) == 2 and i == 0 else 0)
    assert at == len(taxa)
    return out


@pytest.mark.parametrize("reset", [0, 1])
@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("paired", [False, True])
def test_cover_is_the_oracles_hit_list(paired, rule, reset):
    db = gold_db()
    db.ambiguity_rule, db.reset_per_mate = rule, bool(reset)
    frags = gold_fragments(paired)
    assert len(frags) >= 50
    n_cov = n_n = 0
    for mates in frags:
        taxa = lit.classify_fragment(db, mates, 0.0)[4]
        for seq, hits in zip(mates, split_taxa(db, taxa, mates)):
            want = im.from_hits(hits, db.k, len(seq))
            got = im.covered(db, seq)
            assert np.array_equal(got, want)
            assert im.kmer_facts(db, seq) == lit.kmer_minimizers(db, seq)
            n_cov += int(got.sum())
            n_n += any(c not in b"ACGTacgt" for c in seq) and bool(got.any())
    assert n_cov > 1000 and n_n > 0  # (host reads, and host reads with an ambiguous base, are among them)


def test_intervals_and_the_n_rule():
    """a host stretch gives one interval; lower case is a base; an ambiguous base splits the stretch only where no unambiguous
    k-mer contains it.  Under rule 1, kraken2's (mmscanner.h is_ambiguous()), an N costs the k - 1 k-mers that hold it in their
    last k - 1 bases: the k-mer that BEGINS with it is looked up, so a single N stays covered and two split the stretch into
    [.., p) and [p + 1, ..); under rule 0 (the last l bases) it takes k - l + 1 = 5"""
    ob, tb, hb, genomes, _tax = synth.toy_db()
    db = lit.DB.from_images(ob, tb, hb)
    g = genomes[9606][900:1100]
    rng = np.random.default_rng(5)
    read = synth.random_seq(rng, 60) + g + synth.random_seq(rng, 60)
    iv = im.intervals(db, read)
    assert len(iv) == 1 and iv[0][0] <= 60 and iv[0][1] >= 260 and iv[0][1] - iv[0][0] < 200 + 2 * 34  # (a flank may share a minimizer)
    assert im.intervals(db, read.lower()) == iv
    p = 60 + 100
    with_n = lambda n: im.intervals(db, read[:p] + b"N" * n + read[p + n:])
    assert db.ambiguity_rule == 1 and with_n(1) == iv
    assert with_n(2) == [(iv[0][0], p), (p + 1, iv[0][1])] and with_n(5) == [(iv[0][0], p), (p + 4, iv[0][1])]
    db.ambiguity_rule = 0
    assert with_n(1) == iv and with_n(5) == [(iv[0][0], p), (p + 1, iv[0][1])]
    db.ambiguity_rule = 1
    assert im.intervals(db, synth.random_seq(rng, 300)) == [] and im.intervals(db, g[:34]) == []
    # host k-mers i < j with j <= i + k share an interval: two flags 35 apart touch, 36 apart do not
    flags = [False] * 100
    flags[10] = flags[45] = True
    assert im.runs(im.cover_of(flags, 35, 134)) == [(10, 80)]
    flags[45], flags[46] = False, True
    assert im.runs(im.cover_of(flags, 35, 134)) == [(10, 45), (46, 81)]


def test_host_table_and_minimum_hash():
    ob, tb, hb, genomes, tax = synth.toy_db()
    db = lit.DB.from_images(ob, tb, hb)
    seq = genomes[9606][:1200]
    human = db.external.index(9606)
    host_of = [0] * len(db.external)
    host_of[human] = 1
    taxa = lit.classify_fragment(db, (seq,), 0.0)[4]
    want = im.cover_of([t not in (0, lit.AMBIG) and host_of[t] for t in taxa], db.k, len(seq))
    got = im.covered(db, seq, host_of)
    assert np.array_equal(got, want) and 0 < got.sum() < im.covered(db, seq).sum()
    ob2, tb2, hb2, genomes2, _ = synth.toy_db(min_hash=1 << 62)
    db2 = lit.DB.from_images(ob2, tb2, hb2)
    assert db2.min_hash == 1 << 62
    seq2 = genomes2[9606][:1200]
    taxa2 = lit.classify_fragment(db2, (seq2,), 0.0)[4]
    assert np.array_equal(im.covered(db2, seq2), im.from_hits(taxa2, db2.k, len(seq2)))
    assert im.covered(db2, seq2).sum() < im.covered(db, seq).sum()


def test_bed_lines_and_counts():
    ob, tb, hb, genomes, _tax = synth.toy_db()
    db = lit.DB.from_images(ob, tb, hb)
    rng = np.random.default_rng(9)
    g = genomes[9606]
    r1 = synth.random_seq(rng, 50) + g[100:200] + b"NN" + g[202:260]
    r2 = synth.random_seq(rng, 120)
    human = db.external.index(9606)
    text, counts = im.bed(db, [b"@a/1 x", b"@b/1", b"@/1"], [(r1, r2), (r2, r2), (g[300:400], r2)], [human, 0, 0], db.external)
    lines = text.split(b"\n")[:-1]
    assert [ln.split(b"\t")[0] for ln in lines] == [b"a", b"a", b"/1"]
    assert [ln.split(b"\t")[3:] for ln in lines] == [[b"1", b"9606"], [b"1", b"9606"], [b"1", b"0"]]
    assert lines[0].split(b"\t")[2] == b"150" and lines[1].split(b"\t")[1:3] == [b"151", b"210"]
    assert counts[0] == 2 and counts[1] == 3 and counts[2] == sum(int(ln.split(b"\t")[2]) - int(ln.split(b"\t")[1]) for ln in lines)
    # single-end: the id keeps its /1
    text, _c = im.bed(db, [b"@a/1 x"], [(r1,)], [0], db.external)
    assert text.startswith(b"a/1\t")
    # the bitmap and the records of a text with two sequences back to back
    covs = [im.covered(db, g[100:200]), im.covered(db, g[200:300])]
    recs = [(3, 100), (103, 100)]
    words = im.cover_words(210, recs, covs)
    assert words.size == 7 and int(sum(bin(int(w)).count("1") for w in words)) == 200
    assert im.records_of(recs, covs) == [(0, 0, 100), (1, 0, 100)]
